#!/usr/bin/env python
"""Generate tests/golden/vposer_golden.npz: VPoser's decoder and encoder and the SMPLify angle prior, from the code the reference
vendors, on the CPU.

Run where a checkout of the reference is available (COMA_REFERENCE, default: a directory `reference` beside this repository):
    python tests/golden/make_golden_vposer.py

The reference's OWN code is executed; nothing of it is copied, the fixture holds results only (weights and inputs are regenerated
from the seeds of tests/vposer_ref.py).  imports/vposer/vposer_smpl.py, imports/vposer/prior.py and utils/transformations.py are loaded
by file path; the last is registered as `utils.transformations` (the name vposer_smpl.py imports it by; this repository has a `utils`
package of its own), and an empty module stands in for `torchgeometry`, which only aa2matrot uses and nothing here calls.
  * Every case of tests/vposer_ref.CASES: the VPoser class with the seeded state dict loaded, in eval mode: decode(z, "aa") under
    CPU autograd against the seeded upstream gradient g (loss = sum(aa * g)) for dL/dz, decode(z, "matrot"), encode(pose).mean /
    .scale; SMPLifyAnglePrior on the seeded [N,63] pose and autograd against its seeded upstream gradient.  Once with every tensor in
    f32 (R32), once in f64 (R64).
  * The branch id of every joint is read off the class's own matrices by the selection rule (the reference keeps its masks to
    itself); its rotation_matrix_to_quaternion gives the sign of cos.
Conditions (a case that misses one is refused, not recorded): R32 and R64 select the same branch for every joint; no joint at the
exact identity (the reference's own gradient is NaN there); every output finite; `branches` and `odd` reach all four branches;
`cos_negative` has a joint with cos < 0.
e_ref_{aa,grad_z,mean,scale,prior,grad_prior} = max|R32 - R64| / max|R64|, the largest over all cases: the reference's own f32 error;
e_reg_* the same without tests/vposer_ref.ILL_CONDITIONED -- which is empty: `small_angle` (every joint at about 1e-3 rad) was expected
to lose digits in the reference's f32 and does not (2.2e-7 for aa against 4.5e-7 for `random_init`).  The generator prints every case's
figures and checks that no case inflates a pool by more than 10x."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.environ.get("COMA_REFERENCE") or os.path.join(os.path.dirname(ROOT), "reference")
sys.path.insert(0, ROOT)

from tests import vposer_ref as V  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "vposer_golden.npz")


def _load(name, *parts):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, *parts))
    module = importlib.util.module_from_spec(spec)
    sys.modules[name] = module
    spec.loader.exec_module(module)
    return module


import utils  # noqa: E402,F401  (this repository's package: the parent of the name registered next)

transformations = _load("utils.transformations", "utils", "transformations.py")
sys.modules.setdefault("torchgeometry", types.ModuleType("torchgeometry"))
vposer_smpl = _load("reference_vposer_smpl", "imports", "vposer", "vposer_smpl.py")
prior_module = _load("reference_vposer_prior", "imports", "vposer", "prior.py")


def run(name, dtype):
    c, inp = V.case_shape(name), V.case_inputs(name)
    model = vposer_smpl.VPoser(num_neurons=c["H"], latentD=c["D"], data_shape=[1, c["NJ"], 3])
    state = {k: torch.as_tensor(v) for k, v in V.case_weights(name).items()}
    for bn in V.NORMS:
        state[bn + ".num_batches_tracked"] = torch.tensor(0)
    model.load_state_dict(state)
    model = model.to(dtype).eval()
    t = lambda a: torch.as_tensor(a).to(dtype)
    z = t(inp["z"]).requires_grad_(True)
    aa = model.decode(z, output_type="aa")
    (aa.reshape(c["N"], -1) * t(inp["g"])).sum().backward()
    with torch.no_grad():
        matrot = model.decode(z.detach(), output_type="matrot").reshape(-1, 3, 3)
        quat = transformations.rotation_matrix_to_quaternion(torch.nn.functional.pad(matrot, [0, 1]))
        q_z = model.encode(t(inp["pose"]))
    prior = prior_module.SMPLifyAnglePrior(dtype=dtype)
    pose = t(inp["prior_pose"]).requires_grad_(True)
    out = prior(pose)
    (out * t(inp["prior_g"])).sum().backward()
    R = matrot.numpy().astype(np.float64)
    return dict(aa=aa.detach().reshape(c["N"], -1).numpy(), grad_z=z.grad.numpy(), mean=q_z.mean.numpy(), scale=q_z.scale.numpy(),
                prior=out.detach().numpy(), grad_prior=pose.grad.numpy(), matrot=matrot.numpy().reshape(c["N"], c["NJ"], 9),
                branch=V.select_branch(np.swapaxes(R, 1, 2)).reshape(c["N"], c["NJ"]), cos=quat[:, 0].numpy().reshape(c["N"], c["NJ"]))


def main():
    store, errs = {}, {}
    for name in V.CASE_NAMES:
        r32, r64 = run(name, torch.float32), run(name, torch.float64)
        assert np.array_equal(r32["branch"], r64["branch"]), f"{name}: R32 and R64 select different branches"
        assert np.all(np.abs(r64["aa"].reshape(-1, 3)).max(1) > 0), f"{name}: a joint at the exact identity"
        if name in ("branches", "odd"):
            assert sorted(set(r64["branch"].reshape(-1).tolist())) == [0, 1, 2, 3], (name, r64["branch"])
        if name == "cos_negative":
            assert (r64["cos"] < 0).any() and (r32["cos"] < 0).any(), name
        for q in V.QUANTITIES:
            assert np.all(np.isfinite(r64[q])) and np.all(np.isfinite(r32[q])), (name, q)
            store[f"{name}__r64_{q}"], store[f"{name}__r32_{q}"] = r64[q].astype(np.float64), r32[q].astype(np.float32)
        store[f"{name}__r64_branch"], store[f"{name}__r64_matrot"] = r64["branch"].astype(np.int8), r64["matrot"].astype(np.float64)
        errs[name] = {q: V.rel_dev(r32[q], r64[q]) for q in V.QUANTITIES}
        angle = np.linalg.norm(r64["aa"].reshape(-1, 3), axis=1)
        print(f"{name:12s} " + "  ".join(f"{q} {v:.3e}" for q, v in errs[name].items()) + f"  angles {angle.min():.3g}..{angle.max():.3g}"
              f"  branches {np.bincount(r64['branch'].reshape(-1), minlength=4).tolist()}  cos<0 {int((r64['cos'] < 0).sum())}")
    for q in V.QUANTITIES:
        pool = max(e[q] for e in errs.values())
        regular = sorted(e[q] for name, e in errs.items() if name not in V.ILL_CONDITIONED)
        assert regular[-1] <= 10 * regular[-2], f"one case inflates e_reg_{q}: {regular[-1]:.3e} against {regular[-2]:.3e}"
        store[f"e_ref_{q}"], store[f"e_reg_{q}"] = np.float64(pool), np.float64(regular[-1])
        print(f"e_ref_{q} = {pool:.3e}   e_reg_{q} = {regular[-1]:.3e}")
    np.savez_compressed(OUT, **store)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
