#!/usr/bin/env python3
"""Timing aid for the device SMPL-X body model: device time of ONE forward + backward (vertices, then dL/dtheta and dL/dtransl from a
given dL/dvertices; and the full backward through joints and full_pose, to the coefficients as well) at the app's sizes, V = 10 475, J = 55, NB = 20, n_pca = 45, on a seeded synthetic model.

A  coma_amd.body_model.DeviceSMPLX through its autograd function (coma_smplx_forward_f32 + coma_smplx_extra_joints_f32, then
   coma_smplx_backward_f32; the shape stage is cached: the app never changes betas);
B  the same arithmetic in eager torch f32 on the same GPU in the same process (tests/smplx_ref.torch_forward, backward by autograd):
   what the `body_model` hook costs with the third-party package.  The parent commit has no path of its own to compare with.
C  DeviceSMPLX(differentiable=("joints", "full_pose", "shape")): forward, then coma_smplx_backward_full_f32 from dL/dvertices,
   dL/djoints (55 posed joints, 21 vertex picks, 51 landmarks) and dL/dfull_pose to dL/dtheta, dL/dtransl and dL/dcoefficients; the
   coefficients are fixed leaves, so the shape stage is cached as in A;
D  eager torch as B with the coefficients a leaf too: dL/dvertices to dL/dtheta, dL/dtransl and dL/dcoefficients (torch_forward has
   no joints output, so D does less than C: its shape stage is re-evaluated and differentiated every time, the joints are not).
They alternate A B C D A B C D ... in rounds of --iters evaluations, each round timed by HIP events after --warmup untimed
evaluations; the median, fastest and slowest rounds are printed.  Names the device.

--batch N times the batched path instead: A is ONE forward + backward of DeviceSMPLX(batch_size=N) over N bodies of distinct pose
(coma_smplx_forward_batch_f32 + coma_smplx_extra_joints_batch_f32, then coma_smplx_backward_batch_f32), B is the only way to do the
same work without it, a loop of N single-body forward + backward calls on the same build; A B A B in the same rounds, with the
largest difference between their results (they must be bit-identical).

    python scripts/time_body_model.py [--rounds 7] [--iters 50] [--batch N] [--out file.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=0, help="time one batched call of N bodies against N single-body calls")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    import torch
    from coma_amd.body_model import DeviceSMPLX
    from tests import smplx_ref as S
    assert torch.cuda.is_available(), "a timing needs the MI355X"
    dev = "cuda:0"
    V, J, NB, n_pca = 10475, 55, 20, 45
    model = S.synthetic_model(V, J, NB, n_pca, "random", seed=11, n_faces=20908, n_landmarks=51)
    fm = S.flat_model(model, n_pca=n_pca)
    body = DeviceSMPLX(model, n_pca=n_pca, device=dev, extra_joint_vertex_ids=list(range(21)))
    tm = S.torch_model(fm, dev, torch.float32)
    rng = np.random.RandomState(12)
    t = lambda x: torch.as_tensor(np.asarray(x, dtype=np.float32)).to(dev)
    theta, transl, coef, g = t(rng.normal(size=S.n_theta(fm)) * 0.3), t(rng.uniform(-1, 1, 3)), t(rng.normal(size=NB)), t(rng.normal(size=(V, 3)))
    sizes = (3, body.num_body, 3, 3, 3, body.hand_size, body.hand_size)
    keys = ("global_orient", "body_pose", "jaw_pose", "leye_pose", "reye_pose", "left_hand_pose", "right_hand_pose")
    print(f"device: {torch.cuda.get_device_name(0)}; V {V}, J {J}, NB {NB}, n_pca {n_pca}; {a.rounds} rounds of {a.iters} forward + backward, "
          f"A B A B, {a.warmup} warm-up evaluations each")

    betas, expression = coef[None, :10], coef[None, 10:]

    def round_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters

    if a.batch:
        N = a.batch
        batched = DeviceSMPLX(model, n_pca=n_pca, device=dev, extra_joint_vertex_ids=list(range(21)), batch_size=N)
        thetas, transls, gs = t(rng.normal(size=(N, S.n_theta(fm))) * 0.3), t(rng.uniform(-1, 1, (N, 3))), t(rng.normal(size=(N, V, 3)))

        def batched_path():
            th = thetas.clone().requires_grad_(True)
            tr = transls.clone().requires_grad_(True)
            out = batched(betas=betas, expression=expression, transl=tr, **dict(zip(keys, torch.split(th, sizes, 1))))
            g_th, g_tr = torch.autograd.grad(out.vertices, (th, tr), gs)
            return out.vertices.detach(), g_th, g_tr

        def looped_path():
            res = []
            for n in range(N):
                th = thetas[n].clone().requires_grad_(True)
                tr = transls[n].clone().requires_grad_(True)
                out = body(betas=betas, expression=expression, transl=tr[None], **dict(zip(keys, (x[None] for x in torch.split(th, sizes)))))
                g_th, g_tr = torch.autograd.grad(out.vertices[0], (th, tr), gs[n])
                res.append((out.vertices[0].detach(), g_th, g_tr))
            return tuple(torch.stack(x) for x in zip(*res))

        for fn in (batched_path, looped_path):
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        differ = [float((x - y).abs().max()) for x, y in zip(batched_path(), looped_path())]
        times = dict(A=[], B=[])
        for _ in range(a.rounds):
            times["A"].append(round_ms(batched_path))
            times["B"].append(round_ms(looped_path))
        med = {n: float(np.median(x)) for n, x in times.items()}
        print(f"batch {N}: A one batched call {1e3 * med['A']:9.1f} us (min {1e3 * min(times['A']):.1f}, max {1e3 * max(times['A']):.1f})   "
              f"B {N} single-body calls {1e3 * med['B']:9.1f} us (min {1e3 * min(times['B']):.1f}, max {1e3 * max(times['B']):.1f})   B / A {med['B'] / med['A']:.2f}   "
              f"max abs difference A vs B: vertices {differ[0]:.1e}, grad theta {differ[1]:.1e}, grad transl {differ[2]:.1e}")
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                json.dump(dict(device=torch.cuda.get_device_name(0), V=V, J=J, NB=NB, n_pca=n_pca, batch=N, rounds=a.rounds, iters=a.iters, ms=times,
                               median_ms=med, difference=differ), fh, indent=1)
        return

    def device_path():
        th = theta.clone().requires_grad_(True)
        tr = transl.clone().requires_grad_(True)
        kw = dict(zip(keys, (x[None] for x in torch.split(th, sizes))))
        out = body(betas=betas, expression=expression, transl=tr[None], **kw)
        g_th, g_tr = torch.autograd.grad(out.vertices[0], (th, tr), g)
        return out.vertices[0].detach(), g_th, g_tr

    def eager_path():
        th = theta.clone().requires_grad_(True)
        tr = transl.clone().requires_grad_(True)
        verts = S.torch_forward(tm, coef, th, tr)
        g_th, g_tr = torch.autograd.grad(verts, (th, tr), g)
        return verts.detach(), g_th, g_tr

    full = DeviceSMPLX(model, n_pca=n_pca, device=dev, extra_joint_vertex_ids=list(range(21)), differentiable=("joints", "full_pose", "shape"))
    b_leaf, e_leaf = betas.clone().requires_grad_(True), expression.clone().requires_grad_(True)
    gJ, gP = t(rng.normal(size=(J + full.num_extra, 3))), t(rng.normal(size=3 * J))

    def device_full_path(upstream=None):
        th = theta.clone().requires_grad_(True)
        tr = transl.clone().requires_grad_(True)
        kw = dict(zip(keys, (x[None] for x in torch.split(th, sizes))))
        out = full(betas=b_leaf, expression=e_leaf, transl=tr[None], return_full_pose=True, **kw)
        outs, ups = (out.vertices[0], out.joints[0], out.full_pose[0]), (g, gJ, gP)
        if upstream == "vertices":
            outs, ups = outs[:1], ups[:1]
        g_th, g_tr, g_b, g_e = torch.autograd.grad(outs, (th, tr, b_leaf, e_leaf), ups)
        return out.vertices[0].detach(), g_th, g_tr, torch.cat([g_b.reshape(-1), g_e.reshape(-1)])

    def eager_full_path():
        th = theta.clone().requires_grad_(True)
        tr = transl.clone().requires_grad_(True)
        cf = coef.clone().requires_grad_(True)
        verts = S.torch_forward(tm, cf, th, tr)
        g_th, g_tr, g_cf = torch.autograd.grad(verts, (th, tr, cf), g)
        return verts.detach(), g_th, g_tr, g_cf

    for fn in (device_path, eager_path, device_full_path, eager_full_path):
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    agree = [float((x - y).abs().max() / y.abs().max()) for x, y in zip(device_path(), eager_path())]      # faster and different is not faster
    agree_full = [float((x - y).abs().max() / y.abs().max()) for x, y in zip(device_full_path("vertices"), eager_full_path())]
    times = dict(A=[], B=[], C=[], D=[])
    for _ in range(a.rounds):
        times["A"].append(round_ms(device_path))
        times["B"].append(round_ms(eager_path))
        times["C"].append(round_ms(device_full_path))
        times["D"].append(round_ms(eager_full_path))
    med = {n: float(np.median(x)) for n, x in times.items()}
    print(f"A device {1e3 * med['A']:9.1f} us (min {1e3 * min(times['A']):.1f}, max {1e3 * max(times['A']):.1f})   "
          f"B eager torch {1e3 * med['B']:9.1f} us (min {1e3 * min(times['B']):.1f}, max {1e3 * max(times['B']):.1f})   B / A {med['B'] / med['A']:.1f}   "
          f"max rel difference A vs B: vertices {agree[0]:.1e}, grad theta {agree[1]:.1e}, grad transl {agree[2]:.1e}")
    print(f"C device, full backward {1e3 * med['C']:9.1f} us (min {1e3 * min(times['C']):.1f}, max {1e3 * max(times['C']):.1f})   "
          f"D eager torch, coefficients a leaf {1e3 * med['D']:9.1f} us (min {1e3 * min(times['D']):.1f}, max {1e3 * max(times['D']):.1f})   D / C {med['D'] / med['C']:.1f}   "
          f"max rel difference C (from dL/dvertices alone) vs D: vertices {agree_full[0]:.1e}, grad theta {agree_full[1]:.1e}, grad transl {agree_full[2]:.1e}, "
          f"grad coefficients {agree_full[3]:.1e}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(0), V=V, J=J, NB=NB, n_pca=n_pca, rounds=a.rounds, iters=a.iters, ms=times,
                           median_ms=med, agreement=agree, agreement_full=agree_full), fh, indent=1)


if __name__ == "__main__":
    main()
