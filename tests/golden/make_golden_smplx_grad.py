#!/usr/bin/env python
"""Generate tests/golden/smplx_grad_golden.npz: the SMPL-X body model's gradients through vertices, joints and the assembled pose,
to the pose, transl and the shape / expression coefficients, from the third-party package the reference vendors, on the CPU.

Run where a checkout of the reference is available (COMA_REFERENCE, default: a directory `reference` beside this repository):
    python tests/golden/make_golden_smplx_grad.py

As make_golden_smplx.py: the vendored package's directory is put on sys.path and the package's OWN code is executed under CPU
autograd; nothing of it is copied, the fixture holds arrays only.
  * Every case of tests/smplx_ref.CASES: the package's `lbs.lbs` on the seeded synthetic model and inputs with the coefficients, the
    packed pose parameters and transl as leaves, once in f32 (R32) and once in f64 (R64), for four losses (smplx_grad_ref.LOSSES):
    sum(vertices g) + sum(joints gJ) + sum(full_pose gP) and each of the three terms alone.  g is the forward fixture's, gJ and gP
    are smplx_grad_ref.case_upstream's.  lbs returns the J posed joints only: these cases have no extra joints.
  * One case through the package's SMPLX CLASS (as make_golden_smplx.py builds it), every call argument a leaf, betas and expression
    included, the same four losses over ALL vertices, the 55 + 21 + 51 joints and full_pose.
Stored per case and loss: the R64 gradients grad_pose [NT], grad_transl [3], grad_coef [NB] (betas then expression).
e_ref_{grad_pose,grad_transl,grad_coef} = max|R32 - R64| / max|R64|, the largest over all cases and losses: the package's own f32
error; e_reg_* is the same pool without smplx_ref.ILL_CONDITIONED (`small_angle`), exactly as the forward fixture defines them.  The
generator prints every figure and checks that no further case stands out.
"""
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.environ.get("COMA_REFERENCE") or os.path.join(os.path.dirname(ROOT), "reference")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(REF, "imports", "hand4whole", "common", "utils_hand4whole", "smplx"))

import smplx  # noqa: E402  (the vendored package)
from smplx import lbs as package_lbs  # noqa: E402

from tests import smplx_grad_ref as GR  # noqa: E402
from tests import smplx_ref as S  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "smplx_grad_golden.npz")
POSE_ORDER = ("global_orient", "body_pose", "jaw_pose", "leye_pose", "reye_pose", "left_hand_pose", "right_hand_pose")


def _loss(loss, vertices, joints, full_pose, g, gJ, gP):
    ug, ugJ, ugP = GR.upstream(loss, g, gJ, gP)
    total = 0.0
    if ug is not None:
        total = total + (vertices * ug).sum()
    if ugJ is not None:
        total = total + (joints * ugJ).sum()
    if ugP is not None:
        total = total + (full_pose * ugP).sum()
    return total


def _grad(x):
    return np.zeros(tuple(x.shape)) if x.grad is None else x.grad.numpy()


def run_lbs(name, loss, dtype):
    _, fm = S.case_model(name)
    inp = S.case_inputs(name)
    gJ, gP = GR.case_upstream(name)
    c = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32)).to(dtype)         # the f32 model and inputs, cast
    theta, transl, coef = (c(inp[k]).requires_grad_(True) for k in ("theta", "transl", "coefficients"))
    J, hd, k = fm["J"], fm["hd"], fm["n_pca"]
    if k:
        nb = 3 * J - 2 * hd
        comps = c(fm["comps"])
        pose = torch.cat([theta[:nb], theta[nb:nb + k] @ comps[0], theta[nb + k:] @ comps[1]])
    else:
        pose = theta
    pose = (pose + c(fm["mean"]))[None]
    verts, joints = package_lbs.lbs(coef[None], pose, c(fm["v_template"]), c(fm["shapedirs"]), c(fm["posedirs"]), c(fm["J_regressor"]),
                                    torch.as_tensor(fm["parents"]), c(fm["weights"]))
    verts, joints = verts + transl, joints + transl
    _loss(loss, verts[0], joints[0], pose[0], c(inp["g"]), c(gJ), c(gP)).backward()
    return dict(grad_pose=_grad(theta), grad_transl=_grad(transl), grad_coef=_grad(coef))


def run_class(directory, loss, dtype):
    model, kw, g = S.class_case()
    gJ, gP = GR.class_upstream()
    body = smplx.create(model_path=directory, model_type="smplx", num_pca_comps=45, dtype=dtype)
    args = {k: torch.as_tensor(v).to(dtype).requires_grad_(True) for k, v in kw.items()}
    out = body(**args, return_verts=True, return_full_pose=True)
    assert out.joints.shape == (1, 127, 3)
    c = lambda a: torch.as_tensor(a).to(dtype)
    _loss(loss, out.vertices[0], out.joints[0], out.full_pose[0], c(g), c(gJ), c(gP)).backward()
    return dict(grad_pose=np.concatenate([_grad(args[k]).reshape(-1) for k in POSE_ORDER]), grad_transl=_grad(args["transl"]).reshape(-1),
                grad_coef=np.concatenate([_grad(args["betas"]).reshape(-1), _grad(args["expression"]).reshape(-1)]))


def main():
    store, errs = {}, {}

    def keep(name, loss, r32, r64):
        for q in GR.QUANTITIES:
            assert np.all(np.isfinite(r64[q])) and np.all(np.isfinite(r32[q])), (name, loss, q)
            store[f"{name}__r64_{loss}_{q}"] = r64[q].astype(np.float64)
        errs[(name, loss)] = {q: S.rel_dev(r32[q], r64[q]) for q in GR.QUANTITIES}

    for name in S.CASE_NAMES:
        for loss in GR.LOSSES:
            keep(name, loss, run_lbs(name, loss, torch.float32), run_lbs(name, loss, torch.float64))
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "smplx"))
        model, _, _ = S.class_case()
        np.savez(os.path.join(tmp, "smplx", "SMPLX_NEUTRAL.npz"), **model)
        for loss in GR.LOSSES:
            keep("class", loss, run_class(tmp, loss, torch.float32), run_class(tmp, loss, torch.float64))
    for (name, loss), e in errs.items():
        print(f"{name:12s} {loss:10s} " + "  ".join(f"{q} {v:.3e}" for q, v in e.items()))
    for q in GR.QUANTITIES:
        per_case = {name: max(e[q] for (n, _), e in errs.items() if n == name) for name in S.CASE_NAMES + ("class",)}
        pool = max(per_case.values())
        regular = sorted(v for name, v in per_case.items() if name not in S.ILL_CONDITIONED)
        assert regular[-1] <= 10 * regular[-2], f"one more case inflates e_reg_{q}: {regular[-1]:.3e} against {regular[-2]:.3e}"
        store[f"e_ref_{q}"], store[f"e_reg_{q}"] = np.float64(pool), np.float64(regular[-1])
        print(f"e_ref_{q} = {pool:.3e}   e_reg_{q} = {regular[-1]:.3e}")
    np.savez_compressed(OUT, **store)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
