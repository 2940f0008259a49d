#!/usr/bin/env python3
"""Timing aid for the fitting app's loop at the app's sizes: V = 10 475, F = 20 908, J = 55, 45 hand components (a seeded synthetic
model), VPoser with 512 neurons and a latent of 32 (seeded weights), k selected vertices in {500, 5000}.

A  src/application/optimize.py::fit with the three device hooks (DeviceSMPLX, DeviceVPoser, DeviceAnglePrior) around
   ComaObjective.loss: the Python loop -- four autograd Functions, torch.optim.Adam, about 25 library calls per iteration.
B  coma_amd.app.DeviceFit.run: the same iterations enqueued by coma_app_fit_f32.
Both run --iters iterations per round after --warmup untimed ones, alternating A B A B over --rounds rounds.  The clock is the host's,
around work that ends in a device synchronise (both paths end by copying their results to the host): A is bound by the host, so wall
time is the honest figure for both.  For B also: the device's span by HIP events around run(), and the host time of the C calls alone
(taken before anything waits), which shows whether the C loop stays ahead of the device.  Before any timing the warm-up runs of A and
B are compared: global_orient and transl after every warm-up step, within 4 e_ref of the golden `app` case.  Names the device.

    python scripts/time_fit.py [--rounds 5] [--iters 200] [--warmup 20] [--out file.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    import torch
    from coma_amd.app import ComaObjective, DeviceFit
    from coma_amd.body_model import DeviceSMPLX
    from coma_amd.pose_prior import DeviceAnglePrior, DeviceVPoser
    from src.application import optimize as app
    from tests import fit_ref as R
    from tests import smplx_ref as S
    from tests import vposer_ref as V
    assert torch.cuda.is_available(), "a timing needs the MI355X"
    dev = "cuda:0"
    Vn, F, J, n_pca, H, D, NJ = 10475, 20908, 55, 45, 512, 32, 21
    model = S.synthetic_model(Vn, J, 20, n_pca, "random", seed=31, n_faces=F)
    weights = V.synthetic_weights(H, D, NJ, seed=21, kind="near_rest")
    bound = 4 * float(R.load_golden()[0]["app__e_ref"])
    w = R.WEIGHTS
    print(f"device: {torch.cuda.get_device_name(0)}; V {Vn}, F {F}, J {J}, n_pca {n_pca}, neurons {H}, latent {D}; {a.rounds} rounds of {a.iters} iterations, "
          f"A B A B, {a.warmup} warm-up iterations each")
    report = dict(device=torch.cuda.get_device_name(0), V=Vn, F=F, J=J, n_pca=n_pca, H=H, D=D, rounds=a.rounds, iters=a.iters, warmup=a.warmup, cases={})
    for k in (500, 5000):
        rng = np.random.default_rng(k)
        unit = lambda n: (lambda x: (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32))(rng.normal(size=(n, 3)))
        body = DeviceSMPLX(model, n_pca=n_pca, device=dev, extra_joint_vertex_ids=[])
        decoder, prior = DeviceVPoser(weights, H, D, [1, NJ, 3], device=dev), DeviceAnglePrior(dev)
        objective = ComaObjective(model["f"], unit(Vn), unit(1)[0], np.sort(rng.permutation(Vn)[:k]),
                                  (rng.uniform(-1, 1, size=(k, 3)) * [0.3, 0.9, 0.2] + [3, 1, 0]).astype(np.float32), device=dev)
        fit = DeviceFit(body, decoder, prior, objective)

        def python_loop(n):
            return app.fit(lambda v: objective.loss(v, w["orientation_weight"], w["contact_weight"]), body, decoder, prior, lr=w["lr"],
                           body_pose_weight=w["body_pose_weight"], bending_prior_weight=w["bending_prior_weight"], pprior_weight=w["pprior_weight"],
                           scale_factor=w["scale_factor"], num_iters=n, device=dev, record=True)

        def device_loop(n):
            return fit.run(num_iters=n, betas=[R.DEFAULT_BETAS], record=True, **w)

        def wall(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(a.iters)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / a.iters

        warm_a, warm_b = python_loop(a.warmup), device_loop(a.warmup)
        agree = float(np.max(np.abs(np.asarray(warm_a["trajectory"]) - warm_b["trajectory"])))
        agree_v = float(np.max(np.abs(warm_a["vertices"] - warm_b["vertices"])) / np.max(np.abs(warm_a["vertices"])))
        print(f"k {k}: A against B over the {a.warmup} warm-up iterations: global_orient / transl {agree:.3e} (bound {bound:.3e}), last vertices {agree_v:.3e}")
        if not agree <= bound:
            raise SystemExit(f"k {k}: the two loops disagree ({agree:.3e} > {bound:.3e}); faster and different is not faster")
        times = dict(A=[], B=[], B_device=[], B_enqueue=[])
        for _ in range(a.rounds):
            times["A"].append(wall(python_loop))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            device_loop(a.iters)
            e1.record()
            torch.cuda.synchronize()
            times["B"].append((time.perf_counter() - t0) / a.iters)
            times["B_device"].append(1e-3 * e0.elapsed_time(e1) / a.iters)
            times["B_enqueue"].append(fit.enqueue_seconds / a.iters)
        med = {n: float(np.median(x)) for n, x in times.items()}
        line = "   ".join(f"{n} {1e6 * med[n]:8.1f} us (min {1e6 * min(x):.1f}, max {1e6 * max(x):.1f})" for n, x in times.items())
        print(f"k {k}: per iteration, median of {a.rounds} rounds: {line}   A / B {med['A'] / med['B']:.2f}")
        report["cases"][str(k)] = dict(seconds_per_iteration=times, median=med, agreement=agree, agreement_vertices=agree_v, bound=bound)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(report, fh, indent=1)


if __name__ == "__main__":
    main()
