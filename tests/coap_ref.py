"""The project's own restatement of COAP, the learned occupancy body model behind the reference's collision loss (rule set:
include/coma_hip.h, "COAP"): NumPy in f64.  Each function names the lines of the reference's imports/coap/coap.py (C:) or
imports/coap/modules.py (M:) it restates.  Pinned against the reference's own COAPBodyModel executed in f64 with the seeded state dict
(tests/golden/coap_golden.npz, R64) by tests/test_coap_host.py.

The surface sampler (pytorch3d's sample_points_from_meshes) is not restated: samples are an INPUT, a table per part of n_samples // 2
entries on the tight faces and the rest on the extended faces, each a face's three vertex ids and three barycentric weights.
draw_samples draws such a table with pytorch3d's method (area-weighted faces, weights (1 - sqrt u, sqrt u (1 - v), sqrt u v)).

Deviation: where more than max_queries = 10 000 points survive the epoch's filter the reference keeps a random 10 000
(src/generation/optimize_depth.py:129-130); here every survivor counts."""
import os

import numpy as np

from tests import smplx_ref as S

SMPLX_PARENTS = (-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 15, 15, 15,
                 20, 25, 26, 20, 28, 29, 20, 31, 32, 20, 34, 35, 20, 37, 38, 21, 40, 41, 21, 43, 44, 21, 46, 47, 21, 49, 50, 21, 52, 53)
MERGE_BODY_PARTS = {"smpl": sorted([15, 10, 11, 3, 13, 14, 22, 23], reverse=True),        # C:163-189
                    "smplx": sorted([15, 10, 11, 3, 13, 14, 9], reverse=True)}
BBOX_PADDING, LEVEL_SET, BETA, SOFTPLUS_THRESHOLD = 1.125, 0.5, 100.0, 20.0              # C:603, C:621, M:111, torch's Softplus
LATENT, HIDDEN = 128, 128
ENCODER_BLOCKS = ("block_0", "block_1", "block_3", "block_4")                             # M:20-25 with use_block2 False


# ---- partition (C:435-541, C:246-248) ----
def partition(v_template, faces, lbs_weights, parents, model_type="smplx"):
    """dict(tight_faces i32 [K,Ft,3], extended_faces i32 [K,Fe,3] (padded with -1), tight_vert_selector i64 [K,S] (padded with the
    row's first id), joint_mapper bool [mK]).  A face's label is the most frequent label of its own three vertices, which is what
    the reference's walk through edges_unique / faces_unique_edges yields."""
    faces = np.asarray(faces).astype(np.int64)
    max_part = np.asarray(lbs_weights).argmax(axis=1)
    kintree = np.asarray(parents).astype(np.int64).copy()
    merge = MERGE_BODY_PARTS.get(model_type, [])
    if model_type == "smplx":
        max_part[max_part == 22] = kintree[22]
        max_part[(max_part >= 25) & (max_part < 40)] = kintree[28]
        max_part[(max_part >= 40) & (max_part < 55)] = kintree[43]
        max_part[max_part >= 22] = 100
        n_parts = 22
    elif model_type == "smpl":
        n_parts = 24
    else:
        n_parts = kintree.shape[0]
    kintree = kintree[:n_parts]
    valid = list(range(n_parts))
    for ind in merge:
        max_part[max_part == ind] = kintree[ind]
        valid[ind] = kintree[ind]
        kintree[kintree == ind] = kintree[ind]
    face_labels = np.array([np.bincount(max_part[f]).argmax() for f in faces])
    tight, extended, selector = [], [], []
    for b in range(n_parts):
        if b in merge:
            continue
        lab = valid[b]
        ext = face_labels == lab
        if kintree[b] != -1:
            ext = ext | (face_labels == valid[kintree[b]])
        for ch in range(n_parts):
            if kintree[ch] == b:
                ext = ext | (face_labels == valid[ch])
        tight.append(faces[face_labels == lab])
        extended.append(faces[ext])
        selector.append(np.nonzero(max_part == lab)[0])

    def pad(rows):
        out = np.full((len(rows), max(len(r) for r in rows), 3), -1, np.int32)
        for i, r in enumerate(rows):
            out[i, :len(r)] = r
        return out

    if any(len(s) == 0 for s in selector):
        raise ValueError("a body part has no vertex (the reference indexes [0] of its vertex set)")
    sel = np.stack([np.concatenate([s, np.full(max(map(len, selector)) - len(s), s[0])]) for s in selector]).astype(np.int64)
    mapper = np.ones(len(selector) + len(merge), bool)
    mapper[merge] = False
    return dict(tight_faces=pad(tight), extended_faces=pad(extended), tight_vert_selector=sel, joint_mapper=mapper)


# ---- transforms and boxes ----
def abs_transforms(full_pose, joints, parents, joint_mapper):
    """C:562-588: [K,3,4] (rotation | origin): the Rodrigues chain over the first mK joints, then joint_mapper."""
    mK = len(joint_mapper)
    R = S.rodrigues(np.asarray(full_pose, np.float64).reshape(-1, 3))
    chain = [R[0]]
    for i in range(1, mK):
        chain.append(chain[parents[i]] @ R[i])
    A = np.concatenate([np.stack(chain), np.asarray(joints, np.float64).reshape(-1, 3)[:mK, :, None]], 2)
    return A[np.asarray(joint_mapper)]


def bone_trans(A):
    """C:634-637: [K,3,4], the inverse of (R | j) as the reference takes it, by a general matrix inverse: (R^-1 | -R^-1 j).  R is a
    product of Rodrigues matrices whose axis r / |r + 1e-8| is not quite a unit vector, so R^-1 differs from R^T by about 1e-8; the
    device takes the analytic rigid inverse R^T, a difference far below its f32 bound."""
    Ri = np.linalg.inv(A[:, :, :3])
    return np.concatenate([Ri, -np.einsum("krc,kc->kr", Ri, A[:, :, 3])[:, :, None]], 2)


def bbox_bounds(vertices, B, tight_vert_selector):
    """C:410-432: (min [K,3], max [K,3]) of each part's own vertices in its local frame."""
    pv = np.asarray(vertices, np.float64)[tight_vert_selector]                       # [K,S,3]
    local = np.einsum("krc,ksc->ksr", B[:, :, :3], pv) + B[:, None, :, 3]
    return local.min(1), local.max(1)


# ---- surface samples (an input; C:544-560 calls pytorch3d) ----
def draw_samples(rng, vertices, part, n_samples):
    """(ids i32 [K,n,3], bary f64 [K,n,3]) drawn with pytorch3d's method from `rng` (a numpy RandomState)."""
    v = np.asarray(vertices, np.float64)
    K = len(part["tight_faces"])
    n_tight = n_samples // 2
    ids, bary = np.zeros((K, n_samples, 3), np.int32), np.zeros((K, n_samples, 3))
    for k in range(K):
        at = 0
        for table, n in ((part["tight_faces"][k], n_tight), (part["extended_faces"][k], n_samples - n_tight)):
            f = table[table[:, 0] >= 0]
            if len(f) == 0:
                raise ValueError(f"part {k} has no face to sample")
            area = 0.5 * np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1)
            pick = rng.choice(len(f), size=n, p=area / area.sum())
            su, w = np.sqrt(rng.rand(n)), rng.rand(n)
            ids[k, at:at + n] = f[pick]
            bary[k, at:at + n] = np.stack([1 - su, su * (1 - w), su * w], 1)
            at += n
    return ids, bary


def sample_points(vertices, ids, bary):
    """v0 + b1 (v1 - v0) + b2 (v2 - v0): the first weight is implied, so that the weights sum to one exactly (stored f32 weights do
    not) and a translation of the body moves every sample with it -- which the derivative's design rests on."""
    v, b = np.asarray(vertices, np.float64)[ids], np.asarray(bary, np.float64)
    return v[:, :, 0] + b[:, :, 1, None] * (v[:, :, 1] - v[:, :, 0]) + b[:, :, 2, None] * (v[:, :, 2] - v[:, :, 0])


# ---- the encoder (M:7-105) ----
def _lin(w, name, x):
    y = x @ np.asarray(w[name + ".weight"], np.float64).T
    return y + np.asarray(w[name + ".bias"], np.float64) if name + ".bias" in w else y


def pointnet(w, p, prefix="encoder."):
    """M:34-61 without block_2: p [K,n,3] -> [K,128]."""
    relu = lambda a: np.maximum(a, 0.0)
    net = _lin(w, prefix + "fc_pos", p)
    for i, blk in enumerate(ENCODER_BLOCKS):
        b = prefix + blk
        dx = _lin(w, b + ".fc_1", relu(_lin(w, b + ".fc_0", relu(net))))          # M:96-105
        net = _lin(w, b + ".shortcut", net) + dx
        if i < 3:
            net = np.concatenate([net, np.broadcast_to(net.max(1, keepdims=True), net.shape)], 2)
    return _lin(w, prefix + "fc_c", relu(net.max(1)))


def encode(w, part, parents, full_pose, joints, vertices, ids, bary):
    """C:639-668: dict(A, bone_trans [K,3,4], bbox_min/max, centre, size (padded), latent [K,128], vmin/vmax of the posed vertices)."""
    A = abs_transforms(full_pose, joints, parents, part["joint_mapper"])
    B = bone_trans(A)
    lo, hi = bbox_bounds(vertices, B, part["tight_vert_selector"])
    pts = sample_points(vertices, ids, bary)
    local = np.einsum("krc,knc->knr", B[:, :, :3], pts) + B[:, None, :, 3]
    v = np.asarray(vertices, np.float64)
    return dict(A=A, bone_trans=B, bbox_min=lo, bbox_max=hi, centre=(lo + hi) * 0.5, size=np.abs(hi - lo) * BBOX_PADDING,
                latent=pointnet(w, local), vmin=v.min(0), vmax=v.max(0), local_samples=local)


# ---- the query (C:688-730, M:108-165) ----
def softplus(y):
    z = BETA * y
    return np.where(z > SOFTPLUS_THRESHOLD, y, np.log1p(np.exp(np.minimum(z, SOFTPLUS_THRESHOLD))) / BETA)


def softplus_slope(y):
    z = BETA * y
    return np.where(z > SOFTPLUS_THRESHOLD, 1.0, 1.0 / (1.0 + np.exp(-np.clip(z, -700.0, SOFTPLUS_THRESHOLD))))


def implicit_net(w, prefix, n_layers, skip_in, x, dx=None):
    """M:149-165 and its tangent: y' = W x', then x' * softplus'(y) at each activation."""
    inp, dinp = x, dx
    for layer in range(n_layers):
        if layer in skip_in:
            x = np.concatenate([x, inp], -1) / np.sqrt(2)
            if dx is not None:
                dx = np.concatenate([dx, dinp], -1) / np.sqrt(2)
        W = np.asarray(w[f"{prefix}lin{layer}.weight"], np.float64)
        x = x @ W.T + np.asarray(w[f"{prefix}lin{layer}.bias"], np.float64)
        if dx is not None:
            dx = dx @ W.T
        if layer < n_layers - 1:
            if dx is not None:
                dx = dx * softplus_slope(x)
            x = softplus(x)
    return x, dx


def query(w, code, points, direction=None, inside=None):
    """dict(occupancy [T], part_occupancy [K,T], inside bool [K,T], local [K,T,3]) and, with a world `direction`, docc [T]: the
    derivative of the occupancy along it (the winning part's tangent pass; zero where no part contains the point).  `inside`
    overrides the box decisions (the device's own, at points too close to a face of a box to call)."""
    B, K = code["bone_trans"], len(code["bone_trans"])
    p = np.asarray(points, np.float64).reshape(-1, 3)
    T = len(p)
    q = np.einsum("krc,tc->ktr", B[:, :, :3], p) + B[:, None, :, 3]
    own = (np.abs(q - code["centre"][:, None]) < code["size"][:, None] * 0.5).all(-1)          # C:706, strict
    if inside is not None:
        own = np.asarray(inside, bool)
    z = np.concatenate([q, own[:, :, None].astype(np.float64), np.broadcast_to(np.eye(K)[:, None], (K, T, K)),
                        np.broadcast_to(code["latent"][:, None], (K, T, LATENT))], -1)
    dz = dq = None
    if direction is not None:
        dq = np.broadcast_to(np.einsum("krc,c->kr", B[:, :, :3], np.asarray(direction, np.float64))[:, None], (K, T, 3))
        dz = np.concatenate([dq, np.zeros((K, T, z.shape[-1] - 3))], -1)
    f, df = implicit_net(w, "query_encoder.", 4, (2,), z, dz)
    x, dx = implicit_net(w, "decoder.", 7, (3,), np.concatenate([q, f], -1), None if dq is None else np.concatenate([dq, df], -1))
    sig = 1.0 / (1.0 + np.exp(x[..., 0]))                                                     # sigmoid(-x)
    part_occ = sig * own
    out = dict(occupancy=part_occ.max(0), part_occupancy=part_occ, inside=own, local=q)
    if direction is not None:
        dpart = -sig * (1.0 - sig) * dx[..., 0] * own
        win = part_occ.argmax(0)
        out["docc"] = np.where(own.any(0), dpart[win, np.arange(T)], 0.0)
        out["part_docc"] = dpart
    return out


def collision(w, code, points, d, f, filter_threshold=0.01, decisions=None):
    """The epoch's term (optimize_depth.py:104-132, 752-753; C:732-742) with the body shifted by d f: dict(loss, dloss (d loss / d d),
    kept bool [T], occupancy, docc).  `decisions` (dict of bool arrays: inside [K,T], prefilter [T], kept [T], above [T]) overrides
    the discrete outcomes where given."""
    p, f = np.asarray(points, np.float64).reshape(-1, 3), np.asarray(f, np.float64)
    dec = decisions or {}
    r = query(w, code, p - d * f, direction=-f, inside=dec.get("inside"))
    pre = ((p >= code["vmin"] + d * f) & (p <= code["vmax"] + d * f)).all(-1)
    pre = dec.get("prefilter", pre)
    kept = dec.get("kept", pre & (r["occupancy"] > filter_threshold))
    above = dec.get("above", r["occupancy"] > LEVEL_SET)
    return dict(loss=float(np.sum(np.where(kept & above, r["occupancy"] - LEVEL_SET, 0.0))), dloss=float(np.sum(np.where(kept & above, r["docc"], 0.0))),
                kept=kept, prefilter=pre, above=above, occupancy=r["occupancy"], docc=r["docc"], inside=r["inside"])


# ---- seeded model, weights and cases ----
def layer_shapes(K):
    """name -> (out, in) of every Linear of the three networks, in the reference's key layout."""
    d_in = 4 + K + LATENT
    s = {"encoder.fc_pos": (2 * HIDDEN, 3), "encoder.fc_c": (LATENT, HIDDEN)}
    for b in ENCODER_BLOCKS:
        s[f"encoder.{b}.fc_0"], s[f"encoder.{b}.fc_1"], s[f"encoder.{b}.shortcut"] = (HIDDEN, 2 * HIDDEN), (HIDDEN, HIDDEN), (HIDDEN, 2 * HIDDEN)
    for i, (o, n) in enumerate(((256, d_in), (256 - d_in, 256), (256, 256), (128, 256))):
        s[f"query_encoder.lin{i}"] = (o, n)
    for i, (o, n) in enumerate(((256, 131), (256, 256), (125, 256), (256, 256), (256, 256), (256, 256), (1, 256))):
        s[f"decoder.lin{i}"] = (o, n)
    return s


LAST_SCALE = 10.0         # the decoder's last layer, so that occupancies spread over (0, 0.01), (0.01, 0.5), (0.5, 1): the generator checks


def seeded_weights(K, seed=7000):
    rng = np.random.RandomState(seed)
    w = {}
    for name, (o, n) in layer_shapes(K).items():
        w[name + ".weight"] = (rng.normal(size=(o, n)) * np.sqrt(2.0 / n)).astype(np.float32)
        if not name.endswith("shortcut"):
            w[name + ".bias"] = (rng.normal(size=o) * 0.1).astype(np.float32)
    w["decoder.lin6.weight"] = (w["decoder.lin6.weight"] * LAST_SCALE).astype(np.float32)
    return w


MODEL_V, MODEL_F = 330, 660


def seeded_model(seed=7100):
    """A file-style SMPL-X-layout model (55 joints on SMPL-X's own tree, MODEL_V vertices gathered round their joints so that every
    part owns vertices and faces): tests/smplx_ref.synthetic_model with geometry, skinning weights, tree and faces replaced."""
    J = 55
    m = S.synthetic_model(MODEL_V, J, 20, 45, "chain", seed=seed, n_faces=MODEL_F, n_landmarks=51)
    rng = np.random.RandomState(seed + 1)
    parents = np.array(SMPLX_PARENTS)
    centre = np.zeros((J, 3))
    for j in range(1, J):
        centre[j] = centre[parents[j]] + rng.normal(size=3) * (0.12 if j < 22 else 0.03)
    own = np.concatenate([np.arange(MODEL_V // J * J) % J, rng.randint(0, 22, MODEL_V - MODEL_V // J * J)])
    v = centre[own] + rng.normal(size=(MODEL_V, 3)) * 0.04
    W = rng.rand(MODEL_V, J) * 0.02
    W[np.arange(MODEL_V), own] += 1.0
    W[np.arange(MODEL_V), np.maximum(parents[own], 0)] += 0.3
    Jr = np.zeros((J, MODEL_V))
    Jr[own, np.arange(MODEL_V)] = 1.0
    faces = np.zeros((MODEL_F, 3), np.int64)
    for i in range(MODEL_F):
        j = i % J
        mine = np.nonzero(own == j)[0]
        a, b = rng.choice(mine, 2, replace=False)
        pool = np.setdiff1d(np.nonzero((own == j) | (own == max(parents[j], 0)))[0], [a, b])
        faces[i] = (a, b, rng.choice(pool))
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    m.update(v_template=f32(v), weights=f32(W / W.sum(1, keepdims=True)), J_regressor=f32(Jr / Jr.sum(1, keepdims=True)), f=faces,
             kintree_table=np.stack([np.where(parents < 0, 2 ** 32 - 1, parents), np.arange(J)]).astype(np.int64),
             posedirs=f32(m["posedirs"] * 0.1), shapedirs=f32(m["shapedirs"] * 0.1))
    return m


#        name      n_samples  T     pose scale
CASES = (("small",  64,       1000, 0.3),
         ("ragged", 1000,     1000, 0.5))
CASE_NAMES = tuple(c[0] for c in CASES)
DISPLACEMENTS = (0.0, 0.04, -0.07)
FILTER_THRESHOLD = 0.01
QUANTITIES = ("bone_trans", "bbox_min", "bbox_max", "latent", "part_occupancy", "occupancy", "docc", "loss", "dloss")

_cache = {}


def model_arrays():
    """dict(v_template, faces, lbs_weights, parents, fm (tests/smplx_ref flat model), part, weights) of the seeded model."""
    if "model" not in _cache:
        m = seeded_model()
        fm = S.flat_model(m)
        part = partition(m["v_template"], m["f"], m["weights"], fm["parents"], "smplx")
        _cache["model"] = dict(file=m, fm=fm, v_template=m["v_template"], faces=m["f"], lbs_weights=m["weights"], parents=fm["parents"], part=part,
                               weights=seeded_weights(len(part["tight_faces"])))
    return _cache["model"]


def case_inputs(name):
    """The seeded inputs of a golden case, f32 where the device takes f32: full_pose [165], joints [55,3], vertices [V,3] (the seeded
    model posed by tests/smplx_ref.forward), the sample table (ids, bary), points [T,3], front [3]."""
    if name in _cache:
        return _cache[name]
    i = CASE_NAMES.index(name)
    _, n_samples, T, scale = CASES[i]
    M = model_arrays()
    rng = np.random.RandomState(7200 + i)
    fm = M["fm"]
    theta = rng.normal(size=S.n_theta(fm)) * scale
    fwd = S.forward(fm, rng.normal(size=fm["shapedirs"].shape[-1]), theta, rng.uniform(-0.5, 0.5, 3))
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    vertices, joints, full_pose = f32(fwd["vertices"]), f32(fwd["joints"]), f32(fwd["full_pose"])
    ids, bary = draw_samples(rng, vertices, M["part"], n_samples)
    near = vertices[rng.randint(0, len(vertices), T)] + rng.normal(size=(T, 3)) * 0.05
    far = near + np.sign(rng.normal(size=(T, 3))) * 10.0
    points = np.where((np.arange(T) % 10 == 9)[:, None], far, near)
    front = rng.normal(size=3)
    out = dict(full_pose=full_pose, joints=joints, vertices=vertices, ids=ids, bary=f32(bary), points=f32(points),
               front=f32(front / np.linalg.norm(front)), n_samples=n_samples)
    _cache[name] = out
    return out


def case_code(name):
    M, c = model_arrays(), case_inputs(name)
    key = name + "__code"
    if key not in _cache:
        _cache[key] = encode(M["weights"], M["part"], M["parents"], c["full_pose"], c["joints"], c["vertices"], c["ids"], c["bary"])
    return _cache[key]


rel_dev = S.rel_dev

TRAJECTORY = dict(case="small", E=20, lr=0.01, w_multiview=1e-3, w_collision=0.4, d0=0.0)


def trajectory_inputs():
    """The depth optimisation the fixture records: the multiview inputs of the depth-optimisation fixture's "converge" case (its front
    vector moves the body of COAP case "small" as well) and that case's points."""
    from tests.test_depth_opt_host import _golden_case
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depth_opt_golden.npz"), allow_pickle=False)
    c = _golden_case(g, "converge")
    return dict(views=c["views"], joints0=c["joints0"], front=c["front"], cand_view=c["cand_view"], cand_xy=c["cand_xy"])


def optimize(term, views, joints0, front, cand_view, cand_xy, d0, lr, w_multiview, w_collision, E):
    """dict(d, traj f64 [E+1], Ctraj f64 [E,2], losses f64 [E,2]) of coma_depth_optimize_coap_f64: tests/shift_ref.optimize with the
    collision term term(d) -> (loss, d loss / d d) in place of the column profile."""
    from tests import shift_ref as SR
    views, joints0, cand_xy = (np.asarray(a, dtype=np.float64) for a in (views, joints0, cand_xy))
    lr, w_mv, w_col = np.float64(lr), np.float64(w_multiview), np.float64(w_collision)
    traj, Ctraj, losses = np.zeros(E + 1), np.zeros((E, 2)), np.zeros((E, 2))
    d, m, v, p1, p2 = np.float64(d0), np.float64(0.0), np.float64(0.0), np.float64(1.0), np.float64(1.0)
    b1, b2 = np.float64(SR.BETA1), np.float64(SR.BETA2)
    traj[0] = d
    for e in range(E):
        loss, g_mv = SR.multiview(d, views, joints0, front, cand_view, cand_xy)
        if w_collision != 0.0:
            Ctraj[e] = term(float(d))
        losses[e] = [loss, Ctraj[e, 0]]
        g = w_mv * np.float64(g_mv) + w_col * np.float64(Ctraj[e, 1])
        m = b1 * m + (np.float64(1.0) - b1) * g
        v = b2 * v + (np.float64(1.0) - b2) * g * g
        p1, p2 = p1 * b1, p2 * b2
        d = d - (lr / (np.float64(1.0) - p1)) * m / (np.sqrt(v) / np.sqrt(np.float64(1.0) - p2) + np.float64(SR.EPS))
        traj[e + 1] = d
    return dict(d=float(traj[-1]), traj=traj, Ctraj=Ctraj, losses=losses)


def restated_term(name, front, decisions=None):
    """term(d) of a golden case's body and points under the restatement, for optimize()."""
    M, c, code = model_arrays(), case_inputs(name), case_code(name)

    def term(d):
        r = collision(M["weights"], code, c["points"], d, front, FILTER_THRESHOLD, None if decisions is None else decisions(d))
        return r["loss"], r["dloss"]
    return term


def undecided(r, code, g, points=None, d=0.0, f=None):
    """bool [T]: the points whose discrete outcomes a comparison in f32 cannot be held to -- within four times the reference's own
    f32 error (g: the fixture, or a dict with its e_ref_* keys) of a face of a part's box, of occ = FILTER_THRESHOLD or LEVEL_SET, or
    (with `points`, for the epoch's term) of a face of the posed vertices' box.  r: query()'s result for the same points.
    A local coordinate is R p + t, so an element error E of bone_trans moves it by at most E (|p|_1 + 1)."""
    B = code["bone_trans"]
    E = 4.0 * float(g["e_ref_bone_trans"]) * np.abs(B).max()
    p1 = np.abs(np.einsum("krc,ktr->tc", B[:1, :, :3], r["local"][:1] - B[:1, None, :, 3])).sum(-1)      # |p|_1 back from part 0's frame
    box = 4.0 * max(float(g["e_ref_bbox_min"]) * np.abs(code["bbox_min"]).max(), float(g["e_ref_bbox_max"]) * np.abs(code["bbox_max"]).max()) * BBOX_PADDING
    gap = np.abs(np.abs(r["local"] - code["centre"][:, None]) - code["size"][:, None] * 0.5)            # [K,T,3]
    near = (gap <= (E * (p1 + 1.0) + box)[None, :, None]).any(-1).any(0)
    b = 4.0 * float(g["e_ref_occupancy"]) * max(np.abs(r["occupancy"]).max(), 1e-300)
    for thr in (FILTER_THRESHOLD, LEVEL_SET):
        near |= np.abs(r["occupancy"] - thr) <= b
    if points is not None:
        p, f = np.asarray(points, np.float64), np.asarray(f, np.float64)
        tol = 4.0 * np.finfo(np.float32).eps * max(np.abs(code["vmin"]).max(), np.abs(code["vmax"]).max(), np.abs(p).max())
        near |= (np.minimum(np.abs(p - (code["vmin"] + d * f)), np.abs(p - (code["vmax"] + d * f))) <= tol).any(-1)
    return near


def load_golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coap_golden.npz"), allow_pickle=False)
