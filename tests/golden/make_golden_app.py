#!/usr/bin/env python3
"""Generate tests/golden/app_objective_golden.npz: the optimisation app's ComA objective, from the REAL reference on the CPU.

Run where a checkout of the reference is available (COMA_REFERENCE, default: a directory `reference` beside this repository):
    python tests/golden/make_golden_app.py

The objective sits inside the reference's optimize_smpl (src/application/optimize.py), which needs smplx / COAP / VPoser.  As for the
consumer vectors of make_golden.py, the lines that matter are read from the reference file at generation time and executed: the three
functions of file lines 69-164 (canonicalize_a_wrt_b_to_p, compute_vertex_normals, chamfer_distance) and the loss lines 274-289 and
295-296, with a two-method stand-in for pytorch3d's Meshes, the reference's own normalize_vectors_torch, both weights 1, under CPU
autograd -- once in f32 as the reference runs (R32) and once with every tensor in f64 (R64).  Nothing of the reference is copied:
the fixture holds inputs and recorded results.

Stored besides the cases: e_ref_* = max|R32 - R64| / max|R64| pooled (the maximum) over the cases -- for the two contact quantities over
the cases with k <= 25 only, where torch.cdist computes distances directly (above 25 it switches to its matrix-product form, whose f32
error is not an error of the formula) -- and e_reg_*, the same pool without the one ill-conditioned case (`near`, 1 + b.p just above
eps, where the reference's f32 loses the digits of 1 + b.p).  Tests hold the device to 4 * e_ref everywhere, and to 4 * e_reg on every
case but `near`.  Also stored: a 20-iteration Adam trajectory of src/application/optimize.py's loop over the restatement
tests/app_ref.py with a rigid stand-in body, in f64, and its deviation from the same loop in f32.
"""
import importlib.util
import json
import os
import sys
import textwrap

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("COMA_REFERENCE") or os.path.join(os.path.dirname(ROOT), "reference")
sys.path.insert(0, ROOT)

from tests import app_ref  # noqa: E402

TRAJ_ITERS = 20
TRAJ_ARGS = dict(lr=1e-2, body_pose_weight=10000.0, bending_prior_weight=31700.0, pprior_weight=1e-6, orientation_weight=10.0,
                 contact_weight=5.0, scale_factor=0.84)


def reference_pieces():
    with open(os.path.join(REF, "src", "application", "optimize.py")) as fh:
        lines = fh.read().split("\n")
    funcs = lines[68:164]                                        # file lines 69-164
    assert funcs[0].startswith("def canonicalize_a_wrt_b_to_p(") and funcs[-1].strip() == "return chamfer_dist", (funcs[0], funcs[-1])
    head = lines[273:289]                                        # 274-289
    assert head[0].lstrip().startswith("human_mesh = Meshes(") and head[-1].lstrip().startswith("relative_normal_for_reference_object_index ="), head
    tail = lines[294:296]                                        # 295-296
    assert tail[0].lstrip().startswith("orientation_loss =") and tail[1].lstrip().startswith("contact_loss = chamfer_distance("), tail
    spec = importlib.util.spec_from_file_location("reference_transformations", os.path.join(REF, "utils", "transformations.py"))
    tr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tr)
    space = dict(torch=torch, np=np, normalize_vectors_torch=tr.normalize_vectors_torch)
    exec("\n".join(funcs), space)
    return space, textwrap.dedent("\n".join(head + tail))


class Meshes:
    """What the executed lines need of pytorch3d.structures.Meshes: one mesh, packed."""

    def __init__(self, verts, faces):
        self.v, self.f = verts, faces

    def verts_packed(self):
        return self.v.reshape(-1, 3)

    def faces_packed(self):
        return self.f.reshape(-1, 3)


def run_reference(space, loss_src, case, dtype):
    c = lambda x: torch.as_tensor(np.asarray(x, dtype=np.float32)).to(dtype)
    vertices = c(case["verts"])[None].requires_grad_(True)
    ns = dict(space)
    ns.update(Meshes=Meshes, vertices=vertices, faces=torch.as_tensor(case["faces"]), eps=float(case["eps"]), obj_normals=c(case["obj_normals"]),
              principle_vec=c(case["p"]), sub_principle_vec=c(case["sub_p"]), reference_object_vertex_index=int(case["ref_index"]),
              relative_orientation_GT=c(case["gt"]), orientation_weight=1, contact_weight=1, selected_human_indices=(case["sel"],),
              corresponding_object_indices=case["objects"], obj_verts=c(case["obj_verts"]))
    exec(loss_src, ns)
    g_o, = torch.autograd.grad(ns["orientation_loss"], vertices, retain_graph=True)
    g_c, = torch.autograd.grad(ns["contact_loss"], vertices)
    return dict(terms=np.array([ns["orientation_loss"].item(), ns["contact_loss"].item()]), grad_orientation=g_o[0].numpy(), grad_contact=g_c[0].numpy())


def trajectory(case, dtype):
    from src.application.optimize import fit
    template = torch.as_tensor(case["verts"]).to(dtype)
    body = app_ref.RigidBody(template, case["faces"])

    def loss(vertices):
        t_o, t_c = app_ref.objective(vertices.reshape(-1, 3), case["faces"], case["gt"], case["obj_normals"][case["ref_index"]], case["p"], case["sub_p"],
                                     case["eps"], case["sel"], case["obj_verts"][case["objects"]])
        return TRAJ_ARGS["orientation_weight"] * t_o + TRAJ_ARGS["contact_weight"] * t_c
    out = fit(loss, body, app_ref.NullPoseDecoder(dtype), app_ref.null_angle_prior, lr=TRAJ_ARGS["lr"], body_pose_weight=TRAJ_ARGS["body_pose_weight"],
              bending_prior_weight=TRAJ_ARGS["bending_prior_weight"], pprior_weight=TRAJ_ARGS["pprior_weight"], scale_factor=TRAJ_ARGS["scale_factor"],
              num_iters=TRAJ_ITERS, device="cpu", dtype=dtype, record=True)
    return np.asarray(out["trajectory"], dtype=np.float64), np.asarray(out["losses"], dtype=np.float64)


def main():
    space, loss_src = reference_pieces()
    small, large = app_ref.grid_mesh(12, seed=11), app_ref.grid_mesh(40, seed=12)
    assert len(small[0]) == 145 and len(large[0]) == 1601
    cases = {}
    for k in (1, 7, 20, 25, 60):
        cases[f"small_k{k}"] = app_ref.make_case(small, k, seed=100 + k)
    for k in (300, 1000):
        cases[f"large_k{k}"] = app_ref.make_case(large, k, seed=200 + k)
    # b = -p exactly.  With one eps in the normalisations and in the branch test, 1 + b.p is about 2 eps there, so the reference
    # does NOT take its replacer branch at eps = 1e-6; `opposite_replacer` reaches it with eps = 0.7
    cases["opposite"] = app_ref.make_case(small, 20, seed=301, b=(0, 0, -1))
    cases["opposite_replacer"] = app_ref.make_case(small, 20, seed=302, b=(0, 0, -1), eps=0.7)
    cases["near"] = app_ref.make_case(small, 20, seed=303, b=(1.5e-3, -0.8e-3, -1.0))          # 1 + b.p about 3.4e-6: just above eps
    # p, sub_p off the axes (the b_cross quirk shows only there); chosen so that p^.s^ is exactly 0 in f32 too (the reference asserts it)
    cases["tilted"] = app_ref.make_case(small, 20, seed=304, p=(1, 1, 1), sub_p=(1, -1, 0))
    traj_case = app_ref.make_case(small, 20, seed=305)
    # no argmin can flip between precisions: every row's two smallest distances differ by more than app_ref.GAP (make_case draws until so)
    assert all(app_ref.gaps_ok(c) for c in list(cases.values()) + [traj_case])

    out, meta = {}, {}
    pool = {name: [] for name in ("term_orientation", "term_contact", "grad_orientation", "grad_contact")}
    for name, case in cases.items():
        r32, r64 = run_reference(space, loss_src, case, torch.float32), run_reference(space, loss_src, case, torch.float64)
        assert not any(np.isnan(v).any() for v in r32.values()), f"{name}: R32 holds a NaN"
        assert not any(np.isnan(v).any() for v in r64.values()), f"{name}: R64 holds a NaN"
        mine = app_ref.evaluate(case["verts"], case["faces"], case["gt"], case["obj_normals"][case["ref_index"]], case["p"], case["sub_p"], case["eps"],
                                case["sel"], case["obj_verts"][case["objects"]])
        b_hat = case["obj_normals"][case["ref_index"]].astype(np.float64)
        b_hat, p_hat = b_hat / (np.linalg.norm(b_hat) + case["eps"]), case["p"].astype(np.float64) / (np.linalg.norm(case["p"].astype(np.float64)) + case["eps"])
        opc = 1 + float(b_hat @ p_hat)
        dev = dict(term_orientation=app_ref.rel_dev(r32["terms"][0], r64["terms"][0]), term_contact=app_ref.rel_dev(r32["terms"][1], r64["terms"][1]),
                   grad_orientation=app_ref.rel_dev(r32["grad_orientation"], r64["grad_orientation"]),
                   grad_contact=app_ref.rel_dev(r32["grad_contact"], r64["grad_contact"]))
        pin = max(app_ref.rel_dev(mine["terms"][0], r64["terms"][0]), app_ref.rel_dev(mine["terms"][1], r64["terms"][1]),
                  app_ref.rel_dev(mine["grad_orientation"], r64["grad_orientation"]), app_ref.rel_dev(mine["grad_contact"], r64["grad_contact"]))
        k = len(case["sel"])
        print(f"{name:18s} V={len(case['verts'])} k={k} 1+b.p={opc:.3e} replacer={opc < case['eps']}  R32 vs R64: " +
              " ".join(f"{q_}={v:.2e}" for q_, v in dev.items()) + f"  restatement vs R64: {pin:.2e}")
        for q_, v in dev.items():
            if q_.endswith("contact") and k > 25:
                continue
            pool[q_].append((name, v))
        mesh = "small" if case["verts"] is small[0] else "large"
        meta[name] = dict(mesh=mesh, k=k, eps=case["eps"], ref_index=case["ref_index"], one_plus_b_dot_p=opc, replacer=bool(opc < case["eps"]))
        for key in ("gt", "obj_verts", "obj_normals", "p", "sub_p", "sel", "objects"):
            out[f"{name}__{key}"] = case[key]
        for key, v in r64.items():
            out[f"{name}__r64_{key}"] = np.asarray(v, dtype=np.float64)
        for key, v in r32.items():
            out[f"{name}__r32_{key}"] = np.asarray(v, dtype=np.float32)
    for mesh, (verts, faces) in (("small", small), ("large", large)):
        out[f"mesh_{mesh}__verts"], out[f"mesh_{mesh}__faces"] = verts, faces.astype(np.int32)
    for q_, vals in pool.items():
        out[f"e_ref_{q_}"] = np.float64(max(v for _, v in vals))
        out[f"e_reg_{q_}"] = np.float64(max(v for n, v in vals if n != "near"))
        print(f"e_ref_{q_} = {float(out[f'e_ref_{q_}']):.3e}   e_reg_{q_} = {float(out[f'e_reg_{q_}']):.3e}")

    t64, l64 = trajectory(traj_case, torch.float64)
    t32, _ = trajectory(traj_case, torch.float32)
    for key in ("gt", "obj_verts", "obj_normals", "p", "sub_p", "sel", "objects"):
        out[f"traj__{key}"] = traj_case[key]
    meta["traj"] = dict(mesh="small", k=20, eps=traj_case["eps"], ref_index=traj_case["ref_index"], iters=TRAJ_ITERS, **TRAJ_ARGS)
    out["traj__r64_trajectory"], out["traj__r64_losses"] = t64, l64
    out["traj__e_ref"] = np.float64(np.max(np.abs(t32 - t64)))
    print(f"trajectory: {TRAJ_ITERS} iterations, max|f32 - f64| = {float(out['traj__e_ref']):.3e}, loss {l64[0]:.6f} -> {l64[-1]:.6f}")
    out["meta_json"] = np.array(json.dumps(meta))
    pth = os.path.join(HERE, "app_objective_golden.npz")
    np.savez_compressed(pth, **out)
    print(f"wrote {pth} ({os.path.getsize(pth) / 1e3:.0f} kB, {len(out)} arrays)")


if __name__ == "__main__":
    main()
