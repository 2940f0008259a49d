#!/usr/bin/env python
"""Generate tests/golden/coap_golden.npz: COAP, the learned occupancy body model behind the reference's collision loss, from the code
the reference vendors, on the CPU.

Run where a checkout of the reference is available (COMA_REFERENCE, default: a directory `reference` beside this repository):
    python tests/golden/make_golden_coap.py

The reference's OWN code is executed; nothing of it is copied, the fixture holds results only (model, weights and inputs are
regenerated from the seeds of tests/coap_ref.py).  imports/coap/modules.py and coap.py are loaded by file path as a package of their
own, the vendored `smplx` is put on sys.path as make_golden_smplx.py does, and stand-in modules are registered for what is absent:
  * trimesh: a minimal Trimesh exposing faces, edges_unique and faces_unique_edges computed from the faces;
  * skimage (only extract_mesh uses it; nothing here calls that);
  * pytorch3d.structures.Meshes and pytorch3d.ops.sample_points_from_meshes: a stand-in that returns the points of the case's sample
    table (as torch operations on the mesh's vertices, so that autograd runs through them as it does through pytorch3d's sampler).
The reference's COAPBodyModel is built on a seeded SMPL-X-layout model made by the vendored smplx.create from a temporary model file,
the seeded state dict is loaded, and every case of tests/coap_ref.CASES is run once with every tensor in f32 (R32) and once in f64
(R64).  Recorded: the partition tensors, bone_trans, the boxes, latent_code, part_occupancy and occupancy of the case's points,
d occupancy / d d of every point at d = 0 by forward-mode AD through the WHOLE model, collision_loss and its mask, and d loss / d d by CPU autograd through the WHOLE model (vertices = V0 + d f, joints = J0 + d f) at
every d of coap_ref.DISPLACEMENTS, over the points that the epoch's filter (optimize_depth.py:104-132) keeps.
Conditions (a case that misses one is refused): every part owns vertices; the f64 autograd derivative and the restatement's tangent
formula agree to 1e-9 relative -- the premise of evaluating the term's derivative without a backward pass through the encoder; among
the points inside at least one box a tenth each have an R64 occupancy below 0.01, between 0.01 and 0.5, above 0.5; every value finite;
at most 2 % of a case's points lie within 4 e_ref of a threshold or of a box face (so a device test may exclude them), and R32 decides
every other point as R64 does.
A 20-epoch depth optimisation (coap_ref.TRAJECTORY: both terms on, the multiview inputs of depth_opt_golden's "converge" case) is
recorded with the reference's term in f32 and in f64; e_ref_traj and e_ref_Ctraj are its R32-versus-R64 gaps.
e_ref_* = max|R32 - R64| / max|R64| per quantity, the largest over the cases: the reference's own f32 error; no case may inflate a pool
by more than 10x."""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.environ.get("COMA_REFERENCE") or os.path.join(os.path.dirname(ROOT), "reference")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(REF, "imports", "hand4whole", "common", "utils_hand4whole", "smplx"))

import smplx  # noqa: E402  (the vendored package)

from tests import coap_ref as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "coap_golden.npz")


class _Trimesh:
    def __init__(self, vertices, faces, process=False):
        self.vertices, self.faces = np.asarray(vertices), np.asarray(faces)
        e = np.sort(self.faces[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2), axis=1)
        self.edges_unique, inverse = np.unique(e, axis=0, return_inverse=True)
        self.faces_unique_edges = inverse.reshape(-1, 3)


class _Meshes:
    def __init__(self, verts, faces):
        self.verts, self.faces = verts, faces


_table = {}          # the current case's sample table, and how far into it the sampler's calls have read


def _sample_points_from_meshes(meshes, n):
    ids, bary, at = _table["ids"], _table["bary"], _table["at"]
    _table["at"] = (at + n) % ids.shape[1]
    K = ids.shape[0]
    v = meshes.verts.reshape(-1, K, meshes.verts.shape[-2], 3)[0]                     # B = 1: [K,V,3]
    i = torch.as_tensor(ids[:, at:at + n].astype(np.int64))
    picked = torch.stack([v[k][i[k]] for k in range(K)])                                # [K,n,3,3]
    b = torch.as_tensor(bary[:, at:at + n]).to(v.dtype)[..., None]                      # the first weight is implied (coap_ref.sample_points)
    return picked[:, :, 0] + b[:, :, 1] * (picked[:, :, 1] - picked[:, :, 0]) + b[:, :, 2] * (picked[:, :, 2] - picked[:, :, 0])


def _stand_ins():
    tm = types.ModuleType("trimesh")
    tm.Trimesh = _Trimesh
    sk = types.ModuleType("skimage")
    sk.measure = types.ModuleType("skimage.measure")
    p3, p3s, p3o = types.ModuleType("pytorch3d"), types.ModuleType("pytorch3d.structures"), types.ModuleType("pytorch3d.ops")
    p3s.Meshes, p3o.sample_points_from_meshes = _Meshes, _sample_points_from_meshes
    for name, mod in (("trimesh", tm), ("skimage", sk), ("skimage.measure", sk.measure), ("pytorch3d", p3), ("pytorch3d.structures", p3s),
                      ("pytorch3d.ops", p3o)):
        sys.modules.setdefault(name, mod)


def _load_coap():
    pkg = types.ModuleType("reference_coap")
    pkg.__path__ = [os.path.join(REF, "imports", "coap")]
    sys.modules["reference_coap"] = pkg
    for name in ("modules", "coap"):
        spec = importlib.util.spec_from_file_location(f"reference_coap.{name}", os.path.join(REF, "imports", "coap", name + ".py"))
        module = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = module
        spec.loader.exec_module(module)
    return sys.modules["reference_coap.coap"]


def build(coap, directory, dtype):
    body = smplx.create(model_path=directory, model_type="smplx", num_pca_comps=45, dtype=dtype)
    model = coap.COAPBodyModel(body)
    K = model.partitioner.num_parts
    state = {k: torch.as_tensor(v) for k, v in R.seeded_weights(K).items()}
    missing, unexpected = model.load_state_dict(state, strict=False)
    assert not unexpected and all(not k.startswith(("encoder.", "query_encoder.", "decoder.")) for k in missing), (missing, unexpected)
    return model.to(dtype).eval()


def run(model, name, dtype):
    c = R.case_inputs(name)
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)
    model.n_samples = c["n_samples"]
    _table.update(ids=c["ids"], bary=c["bary"], at=0)
    V0, J0, pose, f, pts = t(c["vertices"])[None], t(c["joints"])[None], t(c["full_pose"])[None], t(c["front"]), t(c["points"])[None]
    out = {}
    with torch.no_grad():
        model.detach_cache()
        so = types.SimpleNamespace(full_pose=pose, joints=J0, vertices=V0)
        occ, mid = model.query(pts, so, ret_intermediate=True)
        code = model.impl_code
        out.update(bone_trans=code["bone_trans"][0, :, :3].numpy(), bbox_min=code["bbox_min"][0, :, 0].numpy(), bbox_max=code["bbox_max"][0, :, 0].numpy(),
                   latent=code["latent_code"][0].numpy(), part_occupancy=mid["part_occupancy"][0].numpy(), occupancy=occ[0].numpy())
    import torch.autograd.forward_ad as fwAD
    with fwAD.dual_level():             # d occupancy / d d of every point at d = 0: forward-mode AD through the whole model
        d = fwAD.make_dual(torch.tensor(0.0, dtype=dtype), torch.tensor(1.0, dtype=dtype))
        model.detach_cache()
        _table["at"] = 0
        occ = model.query(pts, types.SimpleNamespace(full_pose=pose, joints=J0 + d * f, vertices=V0 + d * f))
        tangent = fwAD.unpack_dual(occ).tangent
        out["docc"] = (torch.zeros_like(occ) if tangent is None else tangent)[0].detach().numpy()
        model.detach_cache()
    loss, dloss, masks, kepts = [], [], [], []
    for d0 in R.DISPLACEMENTS:
        d = torch.tensor(d0, dtype=dtype, requires_grad=True)
        model.detach_cache()
        _table["at"] = 0
        so = types.SimpleNamespace(full_pose=pose, joints=J0 + d * f, vertices=V0 + d * f)
        with torch.no_grad():           # the epoch's filter (optimize_depth.py:104-120)
            inds = ((pts[0] >= so.vertices.min(1).values) & (pts[0] <= so.vertices.max(1).values)).all(-1)
            kept = inds.clone()
            kept[inds] = (model.query(pts[:, inds], so) > R.FILTER_THRESHOLD).reshape(-1)
            model.detach_cache()
            _table["at"] = 0
        value, mask = model.collision_loss(pts[:, kept], so)
        if kept.any():
            value.sum().backward()
        full = torch.zeros(pts.shape[1], dtype=torch.bool)
        full[kept] = mask[0]
        loss.append(float(value.sum())), dloss.append(0.0 if d.grad is None else float(d.grad)), masks.append(full.numpy()), kepts.append(kept.numpy())
    out.update(loss=np.array(loss), dloss=np.array(dloss), mask=np.stack(masks), kept=np.stack(kepts))
    return out


def reference_term(model, name, front, dtype):
    """term(d) -> (collision_loss, d loss / d d by autograd through the whole model) of the reference, for coap_ref.optimize."""
    c = R.case_inputs(name)
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)
    V0, J0, pose, f, pts = t(c["vertices"])[None], t(c["joints"])[None], t(c["full_pose"])[None], t(front), t(c["points"])[None]

    def term(d0):
        model.n_samples = c["n_samples"]
        _table.update(ids=c["ids"], bary=c["bary"], at=0)
        d = torch.tensor(d0, dtype=dtype, requires_grad=True)
        model.detach_cache()
        so = types.SimpleNamespace(full_pose=pose, joints=J0 + d * f, vertices=V0 + d * f)
        with torch.no_grad():
            inds = ((pts[0] >= so.vertices.min(1).values) & (pts[0] <= so.vertices.max(1).values)).all(-1)
            kept = inds.clone()
            kept[inds] = (model.query(pts[:, inds], so) > R.FILTER_THRESHOLD).reshape(-1)
            model.detach_cache()
            _table["at"] = 0
        value, _ = model.collision_loss(pts[:, kept], so)
        value.sum().backward()
        return float(value.sum().detach()), float(d.grad)
    return term


def main():
    _stand_ins()
    coap = _load_coap()
    M = R.model_arrays()
    store, errs = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "smplx"))
        np.savez(os.path.join(tmp, "smplx", "SMPLX_NEUTRAL.npz"), **M["file"])
        m32, m64 = build(coap, tmp, torch.float32), build(coap, tmp, torch.float64)
    P = m64.partitioner
    for key, ref in (("tight_faces", P.tight_face_tensor), ("extended_faces", P.extended_face_tensor), ("tight_vert_selector", P.tight_vert_selector),
                     ("joint_mapper", P.joint_mapper)):
        store[f"partition__{key}"] = ref.numpy()
    assert all((np.asarray(M["lbs_weights"]).argmax(1) >= 0).tolist())
    for name in R.CASE_NAMES:
        r32, r64 = run(m32, name, torch.float32), run(m64, name, torch.float64)
        c, code = R.case_inputs(name), R.case_code(name)
        for q in R.QUANTITIES:
            assert np.all(np.isfinite(r64[q])) and np.all(np.isfinite(r32[q])), (name, q)
            store[f"{name}__r64_{q}"], store[f"{name}__r32_{q}"] = r64[q].astype(np.float64), r32[q].astype(np.float32)
        store[f"{name}__r64_mask"], store[f"{name}__r64_kept"] = r64["mask"], r64["kept"]
        errs[name] = {q: R.rel_dev(r32[q], r64[q]) for q in R.QUANTITIES}
        # the premise: the whole model's autograd derivative is the tangent pass of the two query networks
        mine = R.query(M["weights"], code, c["points"], direction=-c["front"].astype(np.float64))
        assert R.rel_dev(mine["docc"], r64["docc"]) <= 1e-9, f"{name}: the tangent pass misses the per-point derivative: {R.rel_dev(mine['docc'], r64['docc']):.3e}"
        for i, d in enumerate(R.DISPLACEMENTS):
            mine = R.collision(M["weights"], code, c["points"], d, c["front"], R.FILTER_THRESHOLD)
            gap = abs(mine["dloss"] - r64["dloss"][i]) / max(abs(r64["dloss"][i]), 1e-300)
            print(f"{name:8s} d={d:+.2f}  loss {r64['loss'][i]:.6f}  dloss autograd {r64['dloss'][i]:+.9e}  tangent {mine['dloss']:+.9e}  rel {gap:.1e}  "
                  f"kept {int(r64['kept'][i].sum())}  above {int(r64['mask'][i].sum())}")
            assert r64["kept"][i].sum() > 0 and r64["mask"][i].sum() > 0, f"{name}: nothing collides at d={d}"
            assert gap <= 1e-9, f"{name}: the tangent formula misses the autograd derivative at d={d}: {gap:.3e}"
        inside = R.query(M["weights"], code, c["points"])["inside"].any(0)
        o = r64["occupancy"][inside]
        share = [float(np.mean(o < 0.01)), float(np.mean((o >= 0.01) & (o <= 0.5))), float(np.mean(o > 0.5))]
        print(f"{name:8s} " + "  ".join(f"{q} {v:.3e}" for q, v in errs[name].items()) + f"  inside {int(inside.sum())}  shares {share}")
        assert min(share) >= 0.1, f"{name}: occupancies do not spread ({share}): rescale coap_ref.LAST_SCALE"
    for q in R.QUANTITIES:
        ranked = sorted(e[q] for e in errs.values())
        assert ranked[-1] <= 10 * max(ranked[-2], 1e-300), f"one case inflates e_ref_{q}: {ranked[-1]:.3e} against {ranked[-2]:.3e}"
        store[f"e_ref_{q}"] = np.float64(ranked[-1])
        print(f"e_ref_{q} = {ranked[-1]:.3e}")
    # the cap on points a device test may exclude, and R32's own decisions elsewhere
    for name in R.CASE_NAMES:
        c, code = R.case_inputs(name), R.case_code(name)
        r = R.query(M["weights"], code, c["points"])
        near = R.undecided(r, code, store)
        frac = float(near.mean())
        o32, o64 = store[f"{name}__r32_occupancy"], store[f"{name}__r64_occupancy"]
        for thr in (R.FILTER_THRESHOLD, R.LEVEL_SET):
            assert np.array_equal((o32 > thr)[~near], (o64 > thr)[~near]), f"{name}: R32 decides occ > {thr} otherwise away from the threshold"
        assert np.array_equal((store[f"{name}__r32_part_occupancy"] > 0)[:, ~near], (store[f"{name}__r64_part_occupancy"] > 0)[:, ~near]), name
        print(f"{name:8s} undecided points {int(near.sum())} of {len(near)} ({frac:.2%})")
        assert frac <= 0.02, f"{name}: {frac:.2%} of the points lie within 4 e_ref of a threshold"
    # the depth optimisation: the reference's term in f32 and in f64 under the same f64 Adam; the gap is the trajectory's own f32 error
    tr, ti = R.TRAJECTORY, R.trajectory_inputs()
    runs = {}
    for tag, model, dtype in (("r32", m32, torch.float32), ("r64", m64, torch.float64)):
        runs[tag] = R.optimize(reference_term(model, tr["case"], ti["front"], dtype), ti["views"], ti["joints0"], ti["front"], ti["cand_view"], ti["cand_xy"],
                               tr["d0"], tr["lr"], tr["w_multiview"], tr["w_collision"], tr["E"])
        for q in ("traj", "Ctraj", "losses"):
            assert np.all(np.isfinite(runs[tag][q])), (tag, q)
            store[f"trajectory__{tag}_{q}"] = runs[tag][q]
    mine = R.optimize(R.restated_term(tr["case"], ti["front"]), ti["views"], ti["joints0"], ti["front"], ti["cand_view"], ti["cand_xy"], tr["d0"], tr["lr"],
                      tr["w_multiview"], tr["w_collision"], tr["E"])
    assert R.rel_dev(mine["traj"], runs["r64"]["traj"]) <= 1e-9 and R.rel_dev(mine["Ctraj"], runs["r64"]["Ctraj"]) <= 1e-9, "the restated trajectory"
    for q in ("traj", "Ctraj"):
        store[f"e_ref_{q}"] = np.float64(R.rel_dev(runs["r32"][q], runs["r64"][q]))
        print(f"e_ref_{q} = {store[f'e_ref_{q}']:.3e}   (d {runs['r64']['traj'][0]:+.4f} -> {runs['r64']['traj'][-1]:+.4f}, "
              f"loss {runs['r64']['Ctraj'][0, 0]:.4f} -> {runs['r64']['Ctraj'][-1, 0]:.4f})")
    assert runs["r64"]["Ctraj"][:, 0].min() > 0.0 and store["e_ref_traj"] > 0.0
    np.savez_compressed(OUT, **store)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
