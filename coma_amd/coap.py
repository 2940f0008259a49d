"""COAP on MI355X: the learned occupancy body model behind the reference's collision loss (imports/coap/coap.py, modules.py), as
src/generation/optimize_depth.py uses it -- encode a posed body once, query points against it, the collision term and its derivative
with respect to the displacement d along the camera's front vector.

The ARCHITECTURE is pinned against the code the reference vendors, with seeded weights (tests/golden/make_golden_coap.py); the
trained checkpoint is a download that has never been executed here.  Rule set: include/coma_hip.h, "COAP"; kernels:
coma_amd/csrc/coap.hip; no CPU fallback for anything the device does.

Host side, here: the partition of the body into parts (Partitioner.partition_body without trimesh), the checkpoint loader, the
packing of the weights into the device layout, and the surface sample table.  pytorch3d's sample_points_from_meshes is not available
and not reproduced: the table is drawn here with its method (area-weighted faces, barycentric weights (1 - sqrt u, sqrt u (1 - v),
sqrt u v)) from a seeded NumPy generator, ONCE per encoded body -- the reference re-draws every epoch -- and the point set is
therefore not the reference's.  The gradient through the encoder (src/application/optimize.py --use_collision) is not built.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib

MERGE_BODY_PARTS = {"smpl": sorted([15, 10, 11, 3, 13, 14, 22, 23], reverse=True), "smplx": sorted([15, 10, 11, 3, 13, 14, 9], reverse=True)}
LATENT, HIDDEN = 128, 128
ENCODER_BLOCKS = ("block_0", "block_1", "block_3", "block_4")
MAX_PARTS, MAX_JOINTS, MAX_SAMPLES = 32, 64, 4096


# ---- host: partition, checkpoint, packing, samples ----
def partition(v_template, faces, lbs_weights, parents, model_type="smplx"):
    """Partitioner.partition_body and joint_mapper: dict(tight_faces i32 [K,Ft,3], extended_faces i32 [K,Fe,3] (padded with -1),
    tight_vert_selector i64 [K,S] (padded with the row's first id), joint_mapper bool [mK]).  A vertex belongs to the joint of its
    largest skinning weight after the merges (SMPL-X: jaw into head, fingers into wrists, eyes dropped, then MERGE_BODY_PARTS into
    their parents); a face to the most frequent part of its three vertices; a part's extended faces add its parent's and its
    children's.  Raises ValueError when a part owns no vertex."""
    faces = np.asarray(faces).astype(np.int64)
    label = np.asarray(lbs_weights).argmax(axis=1)
    tree = np.asarray(parents).astype(np.int64).copy()
    merge = MERGE_BODY_PARTS.get(model_type, [])
    if model_type == "smplx":
        label[label == 22] = tree[22]
        label[(label >= 25) & (label < 40)] = tree[28]
        label[(label >= 40) & (label < 55)] = tree[43]
        label[label >= 22] = 100
        n_parts = 22
    elif model_type == "smpl":
        n_parts = 24
    else:
        n_parts = tree.shape[0]
    tree = tree[:n_parts]
    valid = list(range(n_parts))
    for ind in merge:
        label[label == ind] = tree[ind]
        valid[ind] = tree[ind]
        tree[tree == ind] = tree[ind]
    face_label = np.array([np.bincount(label[f]).argmax() for f in faces])
    tight, extended, selector = [], [], []
    for part in range(n_parts):
        if part in merge:
            continue
        near = [valid[part]] + ([valid[tree[part]]] if tree[part] != -1 else []) + [valid[ch] for ch in range(n_parts) if tree[ch] == part]
        tight.append(faces[face_label == valid[part]])
        extended.append(faces[np.isin(face_label, near)])
        selector.append(np.nonzero(label == valid[part])[0])
    if any(len(s) == 0 for s in selector):
        raise ValueError("coap.partition: a body part owns no vertex")

    def padded(rows):
        out = np.full((len(rows), max(len(r) for r in rows), 3), -1, np.int32)
        for i, r in enumerate(rows):
            out[i, :len(r)] = r
        return out

    width = max(len(s) for s in selector)
    sel = np.stack([np.concatenate([s, np.full(width - len(s), s[0])]) for s in selector]).astype(np.int64)
    mapper = np.ones(len(selector) + len(merge), bool)
    mapper[merge] = False
    return dict(tight_faces=padded(tight), extended_faces=padded(extended), tight_vert_selector=sel, joint_mapper=mapper)


def layer_shapes(K):
    """name -> (out, in) of every Linear of encoder, query_encoder and decoder, in the reference's key layout."""
    d_in = 4 + K + LATENT
    s = {"encoder.fc_pos": (2 * HIDDEN, 3), "encoder.fc_c": (LATENT, HIDDEN)}
    for b in ENCODER_BLOCKS:
        s[f"encoder.{b}.fc_0"], s[f"encoder.{b}.fc_1"], s[f"encoder.{b}.shortcut"] = (HIDDEN, 2 * HIDDEN), (HIDDEN, HIDDEN), (HIDDEN, 2 * HIDDEN)
    for i, shape in enumerate(((256, d_in), (256 - d_in, 256), (256, 256), (128, 256))):
        s[f"query_encoder.lin{i}"] = shape
    for i, shape in enumerate(((256, 131), (256, 256), (125, 256), (256, 256), (256, 256), (256, 256), (1, 256))):
        s[f"decoder.lin{i}"] = shape
    return s


def load_coap_state(path_or_dict, K=None):
    """A checkpoint {"state_dict": ...} (or the state dict itself, or a path torch.load reads) in the reference's key layout -> dict
    of f32 NumPy arrays holding exactly the Linear weights and biases of the three networks; buffers (partition tensors, k_one_hot)
    are dropped.  K defaults to what query_encoder.lin0 implies.  Raises ValueError on a missing key or a wrong shape."""
    state = path_or_dict
    if not isinstance(state, dict):
        state = torch.load(state, map_location="cpu")
    state = state.get("state_dict", state)
    host = lambda a: (a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)).astype(np.float32)
    if "query_encoder.lin0.weight" not in state:
        raise ValueError("coap: the checkpoint holds no query_encoder.lin0.weight (not a COAP state dict)")
    implied = int(host(state["query_encoder.lin0.weight"]).shape[1]) - 4 - LATENT
    K = implied if K is None else int(K)
    out = {}
    for name, (o, n) in layer_shapes(K).items():
        for key, shape in ((name + ".weight", (o, n)), (name + ".bias", (o,))):
            if key.endswith("shortcut.bias"):
                continue
            if key not in state:
                raise ValueError(f"coap: the checkpoint lacks {key}")
            a = host(state[key])
            if a.shape != shape:
                raise ValueError(f"coap: {key} has shape {a.shape}, {shape} expected for K={K}")
            out[key] = np.ascontiguousarray(a)
    return out


def _fragments(Wt, nb, g):
    """[in, out] -> the device's fragment order [nb][g][64 lanes][4]: lane l of step s holds W[8 s + 4 (l // 32) + e][32 b + l % 32]."""
    P = np.zeros((8 * g, 32 * nb), np.float32)
    P[:Wt.shape[0], :Wt.shape[1]] = Wt
    return np.ascontiguousarray(P.reshape(g, 2, 4, nb, 32).transpose(3, 0, 1, 4, 2)).reshape(-1)


def pack_weights(state, K):
    """The f32 vector coma_coap_encode_f32 / coma_coap_query_f32 read (layout: include/coma_hip.h, "COAP", weights)."""
    w = lambda k: np.asarray(state[k], np.float32)
    T = lambda k: w(k + ".weight").T
    n1 = 124 - K
    nb1, g2 = (n1 + 31) // 32, (n1 + 3 + 7) // 8
    r2 = np.float32(1.0) / np.sqrt(np.float32(2.0))
    out = [_fragments(T("encoder.fc_pos"), 8, 1), w("encoder.fc_pos.bias")]
    for i, b in enumerate(ENCODER_BLOCKS):
        p = f"encoder.{b}."
        rows, g = (256, 32) if i == 0 else (128, 16)
        out += [_fragments(T(p + "fc_0")[:rows], 4, g), _fragments(T(p + "shortcut")[:rows], 4, g), _fragments(T(p + "fc_1"), 4, 16),
                w(p + "fc_0.bias"), w(p + "fc_1.bias")]
        if i:
            out += [T(p + "fc_0")[128:].reshape(-1), T(p + "shortcut")[128:].reshape(-1)]
    out += [T("encoder.fc_c").reshape(-1), w("encoder.fc_c.bias")]
    for name, at, scale in (("query_encoder.lin0", 0, np.float32(1.0)), ("query_encoder.lin2", n1, r2)):
        Wt = T(name) * scale
        out += [Wt[at + 3], Wt[at + 4:at + 4 + K].reshape(-1), Wt[at + 4 + K:].reshape(-1), w(name + ".bias")]

    def bias(name, n):
        b = np.zeros(n, np.float32)
        if name:
            b[:len(w(name))] = w(name)
        return b
    layers = ((T("query_encoder.lin0")[:3], 8, 1, None), (T("query_encoder.lin1"), nb1, 32, "query_encoder.lin1.bias"),
              (T("query_encoder.lin2")[:n1 + 3] * r2, 8, g2, None), (T("query_encoder.lin3"), 4, 32, "query_encoder.lin3.bias"),
              (T("decoder.lin0"), 8, 17, "decoder.lin0.bias"), (T("decoder.lin1"), 8, 32, "decoder.lin1.bias"),
              (T("decoder.lin2"), 4, 32, "decoder.lin2.bias"), (T("decoder.lin3") * r2, 8, 32, "decoder.lin3.bias"),
              (T("decoder.lin4"), 8, 32, "decoder.lin4.bias"), (T("decoder.lin5"), 8, 32, "decoder.lin5.bias"))
    for Wt, nb, g, b in layers:
        out += [_fragments(Wt, nb, g), bias(b, 32 * nb)]
    out += [w("decoder.lin6.weight").reshape(-1), bias("decoder.lin6.bias", 4)]
    return np.ascontiguousarray(np.concatenate([np.asarray(a, np.float32).reshape(-1) for a in out]))


def weights_layout(K):
    """name -> (offset, floats) of every field of the packed vector, the mirror of coap_layout() in coma_amd/csrc/coap.hip; "total"
    -> its length.  Fragment fields: e_pos_w, e_fc0_i, e_sc_i, e_fc1_i, w_i; the others are plain."""
    n1 = 124 - K
    nb1, g2 = (n1 + 31) // 32, (n1 + 3 + 7) // 8
    out, at = {}, 0

    def take(name, n):
        nonlocal at
        out[name] = (at, n)
        at += n
    take("e_pos_w", 8 * 1 * 256), take("e_pos_b", 256)
    for i in range(4):
        g = 32 if i == 0 else 16
        take(f"e_fc0_{i}", 4 * g * 256), take(f"e_sc_{i}", 4 * g * 256), take(f"e_fc1_{i}", 4 * 16 * 256), take(f"e_b0_{i}", 128), take(f"e_b1_{i}", 128)
        if i:
            take(f"e_fc0p_{i}", 128 * 128), take(f"e_scp_{i}", 128 * 128)
    take("e_fcc_w", 128 * 128), take("e_fcc_b", 128)
    for i in (0, 2):
        take(f"q{i}_in", 256), take(f"q{i}_hot", K * 256), take(f"q{i}_lat", 128 * 256), take(f"q{i}_b", 256)
    for i, (nb, g) in enumerate(((8, 1), (nb1, 32), (8, g2), (4, 32), (8, 17), (8, 32), (4, 32), (8, 32), (8, 32), (8, 32))):
        take(f"w_{i}", nb * g * 256), take(f"b_{i}", nb * 32)
    take("w6", 256), take("b6", 4)
    out["total"] = at
    return out


def draw_samples(rng, vertices, part, n_samples):
    """(ids i32 [K,n,3], bary f32 [K,n,3]): n // 2 entries on each part's tight faces, the rest on its extended faces, faces picked
    by area of the posed mesh, weights (1 - sqrt u, sqrt u (1 - v), sqrt u v).  rng: a numpy RandomState / Generator with
    choice() and random_sample() / random()."""
    v = np.asarray(vertices, np.float64)
    uniform = rng.random_sample if hasattr(rng, "random_sample") else rng.random
    K, n_tight = len(part["tight_faces"]), n_samples // 2
    ids, bary = np.zeros((K, n_samples, 3), np.int32), np.zeros((K, n_samples, 3), np.float32)
    for k in range(K):
        at = 0
        for table, n in ((part["tight_faces"][k], n_tight), (part["extended_faces"][k], n_samples - n_tight)):
            f = table[table[:, 0] >= 0]
            if len(f) == 0:
                raise ValueError(f"coap.draw_samples: part {k} has no face to sample")
            area = 0.5 * np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1)
            pick = rng.choice(len(f), size=n, p=area / area.sum())
            su, t = np.sqrt(uniform(n)), uniform(n)
            ids[k, at:at + n] = f[pick]
            bary[k, at:at + n] = np.stack([1 - su, su * (1 - t), su * t], 1)
            at += n
    return ids, bary


# ---- device ----
class DeviceCOAP:
    """COAPBodyModel's encode_body / query / collision_loss / detach_cache / sample_scene_points on the device.

    body: a coma_amd.body_model.DeviceSMPLX (its model arrays are read) or a dict / object with v_template [V,3], faces [F,3],
    lbs_weights [V,J] and parents [J].  state: what load_coap_state returns (or accepts).  Building the object touches no device:
    the weights go up with the first encode_body."""

    def __init__(self, body, state, n_samples=1000, seed=0, model_type="smplx", device="cuda"):
        self.device = _lib.need_device(device, "DeviceCOAP", resolve=False)
        get = (lambda k: body[k]) if isinstance(body, dict) else (lambda k: getattr(body, k))
        host = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        kept = getattr(body, "host", None)          # DeviceSMPLX keeps host copies of its model arrays, and the faces beside them
        if isinstance(kept, dict) and "v_template" in kept:
            get = lambda k: body.faces if k == "faces" else kept[{"lbs_weights": "weights"}.get(k, k)]
        self.part = partition(host(get("v_template")), host(get("faces")), host(get("lbs_weights")), host(get("parents")), model_type)
        self.K, self.mK = len(self.part["tight_faces"]), len(self.part["joint_mapper"])
        if not (1 <= self.K <= MAX_PARTS and self.mK <= MAX_JOINTS):
            raise _lib.ComaHipError(f"DeviceCOAP: K={self.K} outside [1, {MAX_PARTS}] or mK={self.mK} above {MAX_JOINTS}")
        if not 2 <= int(n_samples) <= MAX_SAMPLES:
            raise _lib.ComaHipError(f"DeviceCOAP: n_samples={n_samples} outside [2, {MAX_SAMPLES}]")
        self.state = load_coap_state(state, self.K)
        self.packed = pack_weights(self.state, self.K)
        self.n_samples, self.rng = int(n_samples), np.random.RandomState(seed)
        parents = np.asarray(host(get("parents"))).astype(np.int64)[:self.mK]
        self._parents = (C.c_int32 * self.mK)(*[int(max(p, 0)) for p in parents])
        self._mapper = (C.c_uint8 * self.mK)(*[int(b) for b in self.part["joint_mapper"]])
        self.level_set, self.weights, self.code, self._selector, self._ws = 0.5, None, None, None, {}

    # -- buffers --
    def _upload(self):
        if self.weights is None:
            self.device = _lib.need_device(self.device, "DeviceCOAP")
            self.weights = torch.as_tensor(self.packed, device=self.device)
            need = int(_lib.lib().coma_coap_weights_floats(self.K))
            if need != self.weights.numel():
                raise _lib.ComaHipError(f"DeviceCOAP: packed {self.weights.numel()} floats, the library expects {need}")
            self._selector = torch.as_tensor(self.part["tight_vert_selector"].astype(np.int32), device=self.device)

    def _scratch(self, key, nbytes):
        t = self._ws.get(key)
        if t is None or t.numel() < nbytes:
            t = self._ws[key] = torch.empty([max(int(nbytes), 16)], dtype=torch.uint8, device=self.device)
        return t

    def _f32(self, a, shape):
        t = a if torch.is_tensor(a) else torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=np.float32)))
        return t.to(device=self.device, dtype=torch.float32).reshape(shape).contiguous()

    @staticmethod
    def _fields(smpl_output):
        if isinstance(smpl_output, dict):
            return smpl_output["full_pose"], smpl_output["joints"], smpl_output["vertices"]
        return smpl_output.full_pose, smpl_output.joints, smpl_output.vertices

    # -- the reference's calls --
    def encode_body(self, smpl_output, samples=None):
        """full_pose [.., 3 J], joints [.., >= mK, 3], vertices [.., V, 3] of ONE body (a leading batch dimension of 1 is dropped).
        samples: (ids i32 [K,n,3], bary f32 [K,n,3]), drawn from the object's seeded generator when None.  Returns the code block."""
        self._upload()
        L = _lib.lib()
        pose, joints, verts = self._fields(smpl_output)
        pose, joints, verts = self._f32(pose, [-1]), self._f32(joints, [-1, 3]), self._f32(verts, [-1, 3])
        if pose.numel() < 3 * self.mK or joints.shape[0] < self.mK:
            raise _lib.ComaHipError(f"DeviceCOAP.encode_body: full_pose / joints shorter than the {self.mK} joints of the partition")
        ids, bary = samples if samples is not None else draw_samples(self.rng, verts.cpu().numpy(), self.part, self.n_samples)
        ids = torch.as_tensor(np.ascontiguousarray(np.asarray(ids, dtype=np.int32)), device=self.device)
        bary = self._f32(bary, list(ids.shape))
        n = int(ids.shape[1])
        code = torch.zeros([int(L.coma_coap_code_bytes(self.K))], dtype=torch.uint8, device=self.device)
        ws = self._scratch("encode", L.coma_coap_encode_workspace_bytes(self.K, n))
        with _lib.on_device(self.device) as stream:
            rc = L.coma_coap_encode_f32(_lib.ptr(self.weights), self.weights.numel(), _lib.ptr(pose), _lib.ptr(joints), _lib.ptr(verts), int(verts.shape[0]),
                                        self._parents, self._mapper, self.mK, self.K, _lib.ptr(self._selector, torch.int32), int(self._selector.shape[1]),
                                        _lib.ptr(ids, torch.int32), _lib.ptr(bary), n, _lib.ptr(code), _lib.ptr(ws), ws.numel(), stream)
            if rc == 0:
                rc = L.coma_coap_status(_lib.ptr(code), stream)
        _lib.check(rc, "coma_coap_encode_f32")
        self.code = code
        return code

    def detach_cache(self):
        self.code = None

    def _attach(self, smpl_output):
        if smpl_output is not None and self.code is None:
            self.encode_body(smpl_output)
        if self.code is None:
            raise _lib.ComaHipError("DeviceCOAP: no encoded body (call encode_body, or pass smpl_output)")

    def _shift(self, d, front):
        dd = None if d is None else (d if torch.is_tensor(d) else torch.tensor([float(d)], dtype=torch.float64)).to(device=self.device, dtype=torch.float64).reshape(1)
        fr = None if front is None else _lib.vec3(np.asarray(front.detach().cpu().numpy() if torch.is_tensor(front) else front, dtype=np.float64).reshape(3))
        return dd, fr

    def query(self, points, smpl_output=None, d=None, front=None, derivative=False):
        """points [.., T, 3] -> occupancy f32 [T] (device); with derivative also d occ / d d along -front, as a second tensor.
        d (a number or a one-element f64 device tensor) and front: the body taken as moved by d front."""
        self._attach(smpl_output)
        L = _lib.lib()
        p = self._f32(points, [-1, 3])
        T = int(p.shape[0])
        occ = torch.empty([T], dtype=torch.float32, device=self.device)
        docc = torch.empty([T], dtype=torch.float32, device=self.device) if derivative else None
        dd, fr = self._shift(d, front)
        ws = self._scratch("query", L.coma_coap_query_workspace_bytes(self.K, T))
        with _lib.on_device(self.device) as stream:
            rc = L.coma_coap_query_f32(_lib.ptr(self.weights), self.weights.numel(), _lib.ptr(self.code), self.K, _lib.ptr(p), T, _lib.ptr(dd), fr,
                                       1 if derivative else 0, _lib.ptr(occ), _lib.ptr(docc), _lib.ptr(ws), ws.numel(), stream)
        _lib.check(rc, "coma_coap_query_f32")
        return (occ, docc) if derivative else occ

    def collision_term(self, points, d=None, front=(0.0, 0.0, 1.0), filter_threshold=0.01):
        """The epoch's term: (result f64 [2] = {loss, d loss / d d}, kept i64 [1]) on the device."""
        self._attach(None)
        L = _lib.lib()
        p = self._f32(points, [-1, 3])
        T = int(p.shape[0])
        result = torch.zeros([2], dtype=torch.float64, device=self.device)
        kept = torch.zeros([1], dtype=torch.int64, device=self.device)
        dd, fr = self._shift(d, front)
        ws = self._scratch("query", L.coma_coap_query_workspace_bytes(self.K, T))
        with _lib.on_device(self.device) as stream:
            rc = L.coma_coap_collision_f32(_lib.ptr(self.weights), self.weights.numel(), _lib.ptr(self.code), self.K, _lib.ptr(p), T, _lib.ptr(dd), fr,
                                           float(filter_threshold), _lib.ptr(result), _lib.ptr(kept), _lib.ptr(ws), ws.numel(), stream)
        _lib.check(rc, "coma_coap_collision_f32")
        return result, kept

    def collision_loss(self, point_cloud, smpl_output=None, ret_collision_mask=False):
        """sum relu(occ - 0.5) over the points, f32 [1] on the device (and the mask occ > 0.5 when asked)."""
        occ = self.query(point_cloud, smpl_output)
        loss = torch.relu(occ - self.level_set)
        return (loss.sum().reshape(1), loss > 0) if ret_collision_mask else loss.sum().reshape(1)

    @torch.no_grad()
    def sample_scene_points(self, smpl_output, scene_vertices, scene_normals=None, n_upsample=2, max_queries=10000, generator=None):
        """optimize_depth.py:104-132: the scene vertices inside the posed vertices' box whose occupancy exceeds 0.01, with offset
        copies along the normals when given, at most max_queries of them; None when nothing is left.  [1, N, 3] f32."""
        _, _, verts = self._fields(smpl_output)
        v = self._f32(verts, [-1, 3])
        pts = self._f32(scene_vertices, [-1, 3])
        inds = ((pts >= v.min(0).values) & (pts <= v.max(0).values)).all(-1)
        if not bool(inds.any()):
            return None
        cand = pts[inds]
        hit = self.query(cand, smpl_output) > 0.01
        self.detach_cache()
        if not bool(hit.any()):
            return None
        out = cand[hit]
        if scene_normals is not None and out.shape[0] > 0:
            norms = self._f32(scene_normals, [-1, 3])[inds][hit]
            offsets = 0.5 * torch.normal(0.05, 0.05, size=(out.shape[0] * n_upsample, 1), device=self.device, generator=generator).abs()
            out = torch.cat((out, out.repeat(n_upsample, 1) - offsets * norms.repeat(n_upsample, 1)), dim=0)
        if out.shape[0] > max_queries:
            out = out[torch.randperm(out.shape[0], device=self.device, generator=generator)[:max_queries]]
        return out.float().reshape(1, -1, 3)
