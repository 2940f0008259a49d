#!/usr/bin/env python3
"""Digests of the fitting kernels' outputs: one `name sha256` line per output tensor, seeded, for comparing two BUILDS of the library
bit for bit (the kernels of csrc/smplx.hip, vposer.hip, app_objective.hip, app_fit.hip, mesh_volume.hip, depth_opt.hip and reduce.hip use fixed
summation shapes, so equal code gives equal bits).  Run it once per build in separate processes and diff the outputs:

    COMA_HIP_LIB=/path/to/other/libcoma_hip.so python scripts/fit_digests.py > a.txt
    python scripts/fit_digests.py > b.txt && diff a.txt b.txt

Inputs are the seeded cases of tests/*_ref.py, the committed tests/golden/ fixtures and seeded synthetic meshes; the cases are the
smallest that still reach every shared helper (more than one workgroup, sizes that are no multiple of a tile, both hand paths).
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
POSE_KEYS = ("global_orient", "body_pose", "jaw_pose", "leye_pose", "reye_pose", "left_hand_pose", "right_hand_pose")


def emit(name, x):
    import torch
    a = np.ascontiguousarray(x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x))
    assert a.size, name
    print(f"{name} {hashlib.sha256(str((a.dtype.str, a.shape)).encode() + a.tobytes()).hexdigest()}", flush=True)


def smplx():
    """Shape stage, forward and backward: V not a multiple of 128, J < 64, n_pca > 0 / n_pca = 0, and hand_dim = 0 (tiny_model)."""
    import torch
    from coma_amd.body_model import DeviceSMPLX
    from tests import smplx_ref as S
    t = lambda x, shape: torch.as_tensor(np.asarray(x, dtype=np.float32)).reshape(shape).to(DEV)
    for name in ("moderate", "no_pca", "tiny_model", "smpl_like"):
        model, fm = S.case_model(name)
        inp = S.case_inputs(name)
        body = DeviceSMPLX(model, n_pca=max(fm["n_pca"], 1), use_pca=bool(fm["n_pca"]), device=DEV, extra_joint_vertex_ids=[0, fm["V"] - 1])
        assert body.hand_dim == fm["hd"] and (name != "tiny_model" or body.hand_dim == 0)
        kw, at = {}, 0
        for key, n in zip(POSE_KEYS, (3, body.num_body, 3, 3, 3, body.hand_size, body.hand_size)):
            kw[key] = t(inp["theta"][at:at + n], (1, n)).requires_grad_(True)
            at += n
        assert at == len(inp["theta"])
        kw["transl"] = t(inp["transl"], (1, 3)).requires_grad_(True)
        coef = t(inp["coefficients"], (1, -1))
        kw["betas"], kw["expression"] = coef[:, :body.num_betas], (coef[:, body.num_betas:] if body.num_expression_coeffs else None)
        out = body(**kw, return_verts=True, return_full_pose=True)
        (out.vertices[0] * t(inp["g"], (-1, 3))).sum().backward()
        state, n3 = body._shape_state.cpu().numpy(), 24 * fm["V"]          # f64 v_shaped [V,3], then j_rest [J,3] at the next multiple of 16
        emit(f"smplx.{name}.v_shaped", state[:n3].view(np.float64))
        emit(f"smplx.{name}.j_rest", state[(n3 + 15) // 16 * 16:][:24 * fm["J"]].view(np.float64))
        for q in ("vertices", "joints", "full_pose"):
            emit(f"smplx.{name}.{q}", getattr(out, q))
        emit(f"smplx.{name}.grad_theta", torch.cat([kw[k].grad.reshape(-1) for k in POSE_KEYS]))
        emit(f"smplx.{name}.grad_transl", kw["transl"].grad)


def smplx_full():
    """The full backward (differentiable joints, full_pose and shape): the loss over all three outputs with two vertex picks and the
    landmarks carrying gradient, on the same cases; digests of the gradients to the pose, transl and the coefficients."""
    import torch
    from coma_amd.body_model import DeviceSMPLX
    from tests import smplx_grad_ref as GR
    from tests import smplx_ref as S
    t = lambda x, shape: torch.as_tensor(np.asarray(x, dtype=np.float32)).reshape(shape).to(DEV)
    for name in ("moderate", "no_pca", "tiny_model", "smpl_like"):
        model, fm = S.case_model(name)
        inp = S.case_inputs(name)
        gJ, gP = GR.case_upstream(name)
        body = DeviceSMPLX(model, n_pca=max(fm["n_pca"], 1), use_pca=bool(fm["n_pca"]), device=DEV, extra_joint_vertex_ids=[0, fm["V"] - 1],
                           differentiable=("joints", "full_pose", "shape"))
        kw, at = {}, 0
        for key, n in zip(POSE_KEYS, (3, body.num_body, 3, 3, 3, body.hand_size, body.hand_size)):
            kw[key] = t(inp["theta"][at:at + n], (1, n)).requires_grad_(True)
            at += n
        kw["transl"] = t(inp["transl"], (1, 3)).requires_grad_(True)
        kw["betas"] = t(inp["coefficients"][:body.num_betas], (1, -1)).requires_grad_(True)
        kw["expression"] = t(inp["coefficients"][body.num_betas:], (1, -1)).requires_grad_(True) if body.num_expression_coeffs else None
        out = body(**kw, return_verts=True, return_full_pose=True)
        gE = np.random.RandomState(5).normal(size=(body.num_extra, 3))           # the extra joints' upstream gradient
        ((out.vertices[0] * t(inp["g"], (-1, 3))).sum() + (out.joints[0] * t(np.concatenate([gJ, gE]), (-1, 3))).sum()
         + (out.full_pose[0] * t(gP, (-1,))).sum()).backward()
        emit(f"smplx_full.{name}.grad_theta", torch.cat([kw[k].grad.reshape(-1) for k in POSE_KEYS]))
        emit(f"smplx_full.{name}.grad_transl", kw["transl"].grad)
        emit(f"smplx_full.{name}.grad_betas", kw["betas"].grad)
        if kw["expression"] is not None:
            emit(f"smplx_full.{name}.grad_expression", kw["expression"].grad)


def smplx_batch():
    """One batched object at batch_size = kChunk + 1 (two sweeps over posedirs, the second with one body; an odd body count for the
    skinning pairs) on the `moderate` model: the three outputs and, from a loss over all of them, the gradients to the pose and transl."""
    import torch
    from coma_amd.body_model import DeviceSMPLX
    from tests import smplx_batch_ref as B
    from tests import smplx_ref as S
    N = B.C_CHUNK + 1
    model, fm = S.case_model("moderate")
    inp = S.case_inputs("moderate")
    rng = np.random.RandomState(7)
    t = lambda x: torch.as_tensor(np.asarray(x, dtype=np.float32)).to(DEV)
    body = DeviceSMPLX(model, n_pca=fm["n_pca"], device=DEV, extra_joint_vertex_ids=[0, fm["V"] - 1], differentiable=("joints", "full_pose"),
                       batch_size=N)
    theta = t(inp["theta"] + 0.2 * rng.normal(size=(N, len(inp["theta"])))).requires_grad_(True)
    transl = t(inp["transl"] + rng.normal(size=(N, 3))).requires_grad_(True)
    coef = t(inp["coefficients"]).reshape(1, -1)
    sizes = (3, body.num_body, 3, 3, 3, body.hand_size, body.hand_size)
    out = body(betas=coef[:, :body.num_betas], expression=coef[:, body.num_betas:] if body.num_expression_coeffs else None, transl=transl, return_full_pose=True,
               **dict(zip(POSE_KEYS, torch.split(theta, sizes, 1))))
    ((out.vertices * t(rng.normal(size=out.vertices.shape))).sum() + (out.joints * t(rng.normal(size=out.joints.shape))).sum()
     + (out.full_pose * t(rng.normal(size=out.full_pose.shape))).sum()).backward()
    for q in ("vertices", "joints", "full_pose"):
        emit(f"smplx_batch.{q}", getattr(out, q))
    emit("smplx_batch.grad_theta", theta.grad)
    emit("smplx_batch.grad_transl", transl.grad)


def vposer():
    """Decode, decode-backward, encode at N = 1 and N = 3 (and the odd sizes H = 80, D = 7, NJ = 5); the angle prior and its backward."""
    import torch
    from coma_amd.pose_prior import DeviceAnglePrior, DeviceVPoser
    from tests import vposer_ref as V
    prior = DeviceAnglePrior(device=DEV)
    for name in ("branches", "batch3", "odd", "cos_negative"):
        c, inp = V.case_shape(name), V.case_inputs(name)
        vp = DeviceVPoser(V.case_weights(name), c["H"], c["D"], [1, c["NJ"], 3], device=DEV)
        z = torch.as_tensor(inp["z"]).to(DEV).requires_grad_(True)
        aa = vp.decode(z, output_type="aa")
        aa.backward(torch.as_tensor(inp["g"]).to(DEV).reshape(aa.shape))
        emit(f"vposer.{name}.aa", aa)
        emit(f"vposer.{name}.grad_z", z.grad)
        emit(f"vposer.{name}.matrot", vp.decode(z.detach(), output_type="matrot"))
        emit(f"vposer.{name}.branch", vp.branches(z.detach()))
        enc = vp.encode(torch.as_tensor(inp["pose"]).to(DEV))
        emit(f"vposer.{name}.mean", enc.mean)
        emit(f"vposer.{name}.scale", enc.scale)
        pose = torch.as_tensor(inp["prior_pose"]).to(DEV).requires_grad_(True)
        out = prior(pose)
        out.backward(torch.as_tensor(inp["prior_g"]).to(DEV))
        emit(f"prior.{name}.out", out)
        emit(f"prior.{name}.grad_pose", pose.grad)


def app_objective():
    """k = 0, k = 1, k no multiple of 64 in one and in several workgroups (k = 333 > 256), on a mesh of more than 256 vertices."""
    import torch
    from coma_amd.app import ComaObjective
    from tests import app_ref as A
    mesh = A.grid_mesh(20, seed=31)
    for k in (0, 1, 37, 333):
        c = A.make_case(mesh, max(k, 1), seed=40 + k)
        sel, targets = c["sel"][:k], c["obj_verts"][c["objects"]][:k]
        obj = ComaObjective(c["faces"], c["gt"], c["obj_normals"][c["ref_index"]], sel, targets, c["p"], c["sub_p"], c["eps"], device=DEV)
        terms, g_o, g_c = obj.evaluate(torch.as_tensor(c["verts"]).to(DEV))
        emit(f"app.k{k}.terms", terms)
        emit(f"app.k{k}.grad_orientation", g_o)
        emit(f"app.k{k}.grad_contact", g_c)


def app_objective_batch():
    """N = 9 bodies (more than 8) of the k = 333 case above in one coma_app_objective_batch_f32 call, and the last body once as a row
    of the batch and once through the single-body call: those two digests are equal."""
    import torch
    from coma_amd.app import ComaObjective
    from tests import app_batch_ref as AB
    from tests import app_ref as A
    c = A.make_case(A.grid_mesh(20, seed=31), 333, seed=40 + 333)
    obj = ComaObjective(c["faces"], c["gt"], c["obj_normals"][c["ref_index"]], c["sel"], c["obj_verts"][c["objects"]], c["p"], c["sub_p"], c["eps"], device=DEV)
    verts = torch.as_tensor(AB.batch_vertices(c, 9, seed=47)).to(DEV)
    for name, batched, single in zip(("terms", "grad_orientation", "grad_contact"), obj.evaluate(verts), obj.evaluate(verts[8])):
        emit(f"app_batch.k333.{name}", batched)
        emit(f"app_batch.k333.body8.{name}", batched[8])
        emit(f"app_batch.k333.single8.{name}", single)


def app_fit():
    """The fitting app's whole loop (coma_app_fit_f32) on the golden cases: 45 and 6 hand components, and no selected vertices."""
    from coma_amd.app import ComaObjective, DeviceFit
    from coma_amd.body_model import DeviceSMPLX
    from coma_amd.pose_prior import DeviceAnglePrior, DeviceVPoser
    from tests import fit_ref as R
    from tests import vposer_ref as V
    golden = R.load_golden()
    c = V.case_shape(R.DECODER)
    for name in R.CASE_NAMES:
        model, _, w, n_pca, _, _ = R.case_models(name)
        o = R.golden_objective(*golden, name)
        fit = DeviceFit(DeviceSMPLX(model, n_pca=n_pca, device=DEV, extra_joint_vertex_ids=[]), DeviceVPoser(w, c["H"], c["D"], [1, c["NJ"], 3], device=DEV),
                        DeviceAnglePrior(DEV), ComaObjective(o["faces"], o["gt"], o["obj_normal"], o["sel"], o["targets"], o["p"], o["sub_p"], o["eps"], device=DEV))
        got = fit.run(num_iters=R.ITERS, betas=[R.DEFAULT_BETAS], record=True, **R.WEIGHTS)
        emit(f"app_fit.{name}.traj", got["parameters"])
        emit(f"app_fit.{name}.losses", got["loss_terms"])
        emit(f"app_fit.{name}.vertices", got["vertices"])


def bumpy_sphere(n_lat, n_lon, seed, centre, radius):
    """A closed, outward-facing latitude-longitude sphere with a seeded radial bump per vertex: F = 2 n_lon (n_lat - 1) faces."""
    rng = np.random.default_rng(seed)
    th = np.pi * np.arange(1, n_lat) / n_lat
    ph = 2 * np.pi * np.arange(n_lon) / n_lon
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones(n_lon))], -1).reshape(-1, 3)
    unit = np.concatenate([[[0.0, 0.0, 1.0]], ring, [[0.0, 0.0, -1.0]]])
    verts = np.asarray(centre) + unit * (radius * (1.0 + 0.05 * rng.uniform(-1, 1, size=(len(unit), 1))))
    at = lambda i, j: 1 + i * n_lon + j % n_lon
    south = 1 + (n_lat - 1) * n_lon
    faces = []
    for j in range(n_lon):
        faces.append((0, at(0, j), at(0, j + 1)))
        faces.append((south, at(n_lat - 2, j + 1), at(n_lat - 2, j)))
        for i in range(n_lat - 2):
            faces += [(at(i, j), at(i + 1, j), at(i + 1, j + 1)), (at(i, j), at(i + 1, j + 1), at(i, j + 1))]
    return verts, np.asarray(faces, dtype=np.int32)


def volumes_and_depth():
    """Mesh volume, intersection columns, the shift profile and the depth optimisation on two closed meshes, one with 256 < F <
    256 x 256 faces (several partials of one pass) and one with F > 256 x 256 (every workgroup strides, 256 partials)."""
    from coma_amd import depth_opt as D, metrics as M
    from tests.test_depth_opt_host import _golden_case
    small = bumpy_sphere(13, 24, 51, (0.45, 0.5, 0.45), 0.3)
    large = bumpy_sphere(130, 256, 52, (0.55, 0.5, 0.6), 0.32)
    assert 256 < len(small[1]) < 256 * 256 < len(large[1])
    res = 48
    for name, m in (("small", small), ("large", large)):
        emit(f"volume.{name}", np.float64(M.mesh_volume(m[0], m[1], device=DEV)))
    sums, col = M.intersection_columns(small[0], small[1], large[0], large[1], 0.0, 0.0, float(res), res, res, want_columns=True, device=DEV)
    assert sums[0] > 0
    emit("columns.sums", sums)
    emit("columns.col_ab", col)
    cols = D.prepare_columns(small[0], small[1], large[0], large[1], 0.0, 0.0, float(res), res, res, device=DEV)
    emit("shift.lengths", np.asarray([cols.L_A, cols.L_B, cols.crossings], dtype=np.int64))
    emit("shift.profile", D.shift_profile(cols, np.linspace(-0.4, 0.4, 17)))
    g = np.load(os.path.join(ROOT, "tests", "golden", "depth_opt_golden.npz"), allow_pickle=False)
    c = _golden_case(g, "converge")
    for tag, columns, w_mv, w_col, E in (("both", cols, 1e-3, 0.4, 6), ("multiview", None, 1e-3, 0.0, 3), ("one_epoch", cols, 0.0, 0.4, 1)):
        got = D.optimize_displacement(columns, c["views"], c["joints0"], c["front"], c["cand_view"], c["cand_xy"], 0.0, 0.01, w_mv, w_col, E, device=DEV)
        for q in ("traj", "Ltraj", "losses"):
            emit(f"depth.{tag}.{q}", got[q])


def row_reductions():
    """Entropy, masked max (both directions) and row argmax of csrc/reduce.hip; the row counts are no multiple of 4 (rows per workgroup)."""
    import torch
    from coma_amd import _lib, consumer
    L = _lib.lib()
    rng = np.random.default_rng(61)
    H, O, N = 7, 9, 100
    f32, u8 = torch.float32, torch.uint8
    prob = torch.as_tensor(rng.random((H * O, N), dtype=np.float32) ** 4).to(DEV)
    score = torch.empty([H * O], dtype=f32, device=DEV)
    _lib.check(L.coma_entropy_f32(_lib.ptr(prob, f32), H * O, N, 1e-8, 20.0, _lib.ptr(score), _lib.stream_ptr(DEV)), "coma_entropy_f32")
    emit("reduce.entropy.prob", prob)
    emit("reduce.entropy.score", score)
    cnt = torch.as_tensor(rng.integers(0, 6, size=(H, O)).astype(np.float32)).to(DEV)
    pairs, col_any, row_any = (torch.empty(s, dtype=u8, device=DEV) for s in ([H, O], [O], [H]))
    _lib.check(L.coma_significant_pairs_u8(_lib.ptr(cnt, f32), 3.0, H, O, _lib.ptr(pairs), _lib.ptr(col_any), _lib.ptr(row_any), _lib.stream_ptr(DEV)),
               "coma_significant_pairs_u8")
    cm = torch.as_tensor(rng.random((H, O), dtype=np.float32)).to(DEV)
    for which, n in ((0, H), (1, O)):
        out = torch.empty([n], dtype=f32, device=DEV)
        _lib.check(L.coma_masked_max_f32(_lib.ptr(cm, f32), _lib.ptr(col_any), _lib.ptr(row_any), H, O, which, _lib.ptr(out), _lib.stream_ptr(DEV)),
                   "coma_masked_max_f32")
        emit(f"reduce.masked_max.{which}", out)
    x = torch.as_tensor(rng.integers(0, 50, size=(13, 150)).astype(np.float32)).to(DEV)      # ties: the first maximum wins
    idx, val = consumer.row_argmax(x, 130, row_stride=150, col_offset=7, want_max=True)
    emit("reduce.argmax.idx", idx)
    emit("reduce.argmax.val", val)


def main():
    import torch
    from coma_amd import _lib
    assert torch.cuda.is_available(), "the digests are of device results"
    print(f"# library: {_lib.LIB_PATH}", file=sys.stderr)
    for part in (smplx, smplx_full, smplx_batch, vposer, app_objective, app_objective_batch, app_fit, volumes_and_depth, row_reductions):
        part()
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
