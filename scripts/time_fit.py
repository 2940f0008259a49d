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

--starts N (N >= 2) times the multi-start fit instead, at k = 500, same protocol (warm-up, rounds of --iters iterations, host clock to
a device synchronise, alternating):
M  fit(starts=default_starts(N)): ONE Python loop over N starts -- DeviceSMPLX(batch_size=N), DeviceVPoser and DeviceAnglePrior on N
   rows, ComaObjective.loss on [N,V,3];
S  N Python loops of one start each, one after the other, on batch_size=1 models (what a caller had to do before).
Neither records (a recorded N-start iteration reads N losses back, which is not what is compared), and both figures are per
iteration of the WHOLE N-start fit, so M / S = 1 / N would be perfect batching.  Before any timing the warm-up runs are compared: every
start's last vertices, bit for bit.  Also: one batched ComaObjective.evaluate on [N,V,3] against N single ones, --iters calls per round.

    python scripts/time_fit.py --starts 8
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
    ap.add_argument("--starts", type=int, default=1, help="N >= 2: time the N-start Python loop against N single-start loops (k = 500)")
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
    if a.starts > 1:
        report["starts"] = multi_start(a, model, weights, dev)
        return write(a, report)
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
    write(a, report)


def write(a, report):
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(report, fh, indent=1)


def multi_start(a, model, weights, dev, k=500):
    import torch
    from coma_amd.app import ComaObjective
    from coma_amd.body_model import DeviceSMPLX
    from coma_amd.pose_prior import DeviceAnglePrior, DeviceVPoser
    from src.application import optimize as app
    from tests import fit_ref as R
    N, w, Vn = a.starts, R.WEIGHTS, len(model["v_template"])
    rng = np.random.default_rng(k)
    unit = lambda n: (lambda x: (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32))(rng.normal(size=(n, 3)))
    bodies = {n: DeviceSMPLX(model, n_pca=45, device=dev, extra_joint_vertex_ids=[], batch_size=n) for n in (1, N)}
    decoder, prior = DeviceVPoser(weights, 512, 32, [1, 21, 3], device=dev), DeviceAnglePrior(dev)
    objective = ComaObjective(model["f"], unit(Vn), unit(1)[0], np.sort(rng.permutation(Vn)[:k]),
                              (rng.uniform(-1, 1, size=(k, 3)) * [0.3, 0.9, 0.2] + [3, 1, 0]).astype(np.float32), device=dev)
    starts = app.default_starts(N)

    def loop(rows, n):
        return app.fit(lambda v: objective.loss(v, w["orientation_weight"], w["contact_weight"]), bodies[len(rows)], decoder, prior, lr=w["lr"],
                       body_pose_weight=w["body_pose_weight"], bending_prior_weight=w["bending_prior_weight"], pprior_weight=w["pprior_weight"],
                       scale_factor=w["scale_factor"], num_iters=n, device=dev, starts=rows)

    many = lambda n: loop(starts, n)
    sequential = lambda n: [loop(starts[i:i + 1], n) for i in range(N)]

    def wall(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(n)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    warm_m, warm_s = many(a.warmup), sequential(a.warmup)
    same = all(np.array_equal(warm_m["vertices_all"][i].view(np.int32), warm_s[i]["vertices_all"][0].view(np.int32)) for i in range(N))
    print(f"{N} starts, k {k}: every start's vertices after {a.warmup} warm-up iterations equal its single-start run's bit for bit: {same}")
    if not same:
        raise SystemExit("the N-start loop and the single-start loops disagree; faster and different is not faster")
    verts = torch.as_tensor(np.stack([r["vertices_all"][0] for r in warm_s])).to(dev)
    batched_eval = lambda n: [objective.evaluate(verts) for _ in range(n)]
    single_evals = lambda n: [objective.evaluate(verts[i]) for _ in range(n) for i in range(N)]
    times = dict(M=[], S=[], evaluate_batched=[], evaluate_singles=[])
    for _ in range(a.rounds):
        for name, fn in (("M", many), ("S", sequential), ("evaluate_batched", batched_eval), ("evaluate_singles", single_evals)):
            times[name].append(wall(fn, a.iters))
    med = {n: float(np.median(x)) for n, x in times.items()}
    line = "   ".join(f"{n} {1e6 * med[n]:9.1f} us (min {1e6 * min(x):.1f}, max {1e6 * max(x):.1f})" for n, x in times.items())
    print(f"{N} starts, k {k}: per iteration of the whole {N}-start fit / per evaluation of {N} bodies, median of {a.rounds} rounds: {line}   "
          f"S / M {med['S'] / med['M']:.2f}   singles / batched {med['evaluate_singles'] / med['evaluate_batched']:.2f}")
    return dict(N=N, k=k, seconds=times, median=med, bit_identical=same)


if __name__ == "__main__":
    main()
