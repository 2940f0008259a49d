#!/usr/bin/env python
"""Generate tests/golden/smplx_batch_golden.npz: the SMPL-X body model at batch_size = 3, from the third-party package the reference
vendors, on the CPU.

Run where a checkout of the reference is available (COMA_REFERENCE, default: a directory `reference` beside this repository):
    python tests/golden/make_golden_smplx_batch.py

As tests/golden/make_golden_smplx.py: the package's directory is put on sys.path and its OWN code is executed; nothing of it is
copied, the fixture holds arrays only.  The cases are those of tests/smplx_batch_ref.py, every one with three bodies of distinct pose
(one at zero pose, one with a joint near |r| = pi), once with one set of coefficients for all bodies and once with one per body:
  * lbs_*: the package's `lbs.lbs` on the seeded V = 300 model with a leading dimension of 3, under CPU autograd against the seeded
    upstream gradient (loss = sum(vertices * g)), every tensor in f32 (R32) and in f64 (R64); the pose is assembled from the packed
    parameters in torch as make_golden_smplx.py does.
  * class_*: the package's SMPLX class constructed with batch_size=3 from a synthetic SMPLX_NEUTRAL.npz (V = 10 475), every call
    argument [3, n] and a leaf (the package does not broadcast betas: the shared coefficients are repeated).  Stored: a fixed
    256-vertex subset of the vertices, all joints, full_pose and the gradients to the pose arguments and transl.
e_ref_{vertices,joints,grad_pose,grad_transl} = max|R32 - R64| / max|R64| over a case's whole batch, the largest over the cases.
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

from tests import smplx_batch_ref as B  # noqa: E402
from tests import smplx_ref as S  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "smplx_batch_golden.npz")


def run_lbs(case, dtype):
    _, fm = B.model_of("lbs")
    inp = B.case_inputs(case)
    c = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32)).to(dtype)
    theta = c(inp["theta"]).requires_grad_(True)
    transl = c(inp["transl"]).requires_grad_(True)
    J, hd, k = fm["J"], fm["hd"], fm["n_pca"]
    nb = 3 * J - 2 * hd
    comps = c(fm["comps"])
    pose = torch.cat([theta[:, :nb], theta[:, nb:nb + k] @ comps[0], theta[:, nb + k:] @ comps[1]], 1) + c(fm["mean"])
    verts, joints = package_lbs.lbs(c(inp["coefficients"]).expand(B.N, -1), pose, c(fm["v_template"]), c(fm["shapedirs"]), c(fm["posedirs"]),
                                    c(fm["J_regressor"]), torch.as_tensor(fm["parents"]), c(fm["weights"]))
    verts, joints = verts + transl[:, None], joints + transl[:, None]
    (verts * c(inp["g"])).sum().backward()
    return dict(vertices=verts.detach().numpy(), joints=joints.detach().numpy(), full_pose=pose.detach().numpy(), grad_pose=theta.grad.numpy(),
                grad_transl=transl.grad.numpy())


def run_class(case, directory, dtype):
    _, fm = B.model_of("class")
    inp = B.case_inputs(case)
    body = smplx.create(model_path=directory, model_type="smplx", num_pca_comps=45, batch_size=B.N, dtype=dtype)
    leaf = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dtype).requires_grad_(True)
    args = {k: leaf(v) for k, v in B.split_theta(fm, inp["theta"]).items()}
    args["transl"] = leaf(inp["transl"])
    coef = torch.as_tensor(inp["coefficients"]).to(dtype).expand(B.N, -1)
    out = body(betas=coef[:, :10], expression=coef[:, 10:], **args, return_verts=True, return_full_pose=True)
    subset = B.class_subset()
    (out.vertices * torch.as_tensor(inp["g"]).to(dtype)).sum().backward()
    return dict(vertices=out.vertices[:, subset].detach().numpy(), joints=out.joints.detach().numpy(), full_pose=out.full_pose.detach().numpy(),
                grad_pose=np.concatenate([args[k].grad.numpy() for k in B.POSE_KEYS], 1), grad_transl=args["transl"].grad.numpy())


def main():
    store, errs = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "smplx"))
        np.savez(os.path.join(tmp, "smplx", "SMPLX_NEUTRAL.npz"), **B.model_of("class")[0])
        for case in B.CASES:
            run = (lambda dt: run_lbs(case, dt)) if case.startswith("lbs") else (lambda dt: run_class(case, tmp, dt))
            r32, r64 = run(torch.float32), run(torch.float64)
            inp = B.case_inputs(case)
            for key in ("coefficients", "theta", "transl"):         # g is large and seeded: the tests regenerate it
                store[f"{case}__{key}"] = inp[key]
            for q in B.QUANTITIES + ("full_pose",):
                store[f"{case}__r64_{q}"], store[f"{case}__r32_{q}"] = r64[q].astype(np.float64), r32[q].astype(np.float32)
                assert np.all(np.isfinite(r64[q])) and np.all(np.isfinite(r32[q])), (case, q)
            errs[case] = {q: S.rel_dev(r32[q], r64[q]) for q in B.QUANTITIES}
            print(f"{case:16s} " + "  ".join(f"{q} {v:.3e}" for q, v in errs[case].items()))
    for q in B.QUANTITIES:
        store[f"e_ref_{q}"] = np.float64(max(e[q] for e in errs.values()))
        print(f"e_ref_{q} = {store[f'e_ref_{q}']:.3e}")
    np.savez_compressed(OUT, **store)
    size, limit = os.path.getsize(OUT), os.path.getsize(os.path.join(ROOT, "tests", "golden", "smplx_golden.npz"))
    print(OUT, size, "bytes; smplx_golden.npz has", limit)
    assert size <= limit


if __name__ == "__main__":
    main()
