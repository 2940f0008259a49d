#!/usr/bin/env python3
"""Timing aid for the device SMPL-X body model: device time of ONE forward + backward (vertices, then dL/dtheta and dL/dtransl from a
given dL/dvertices) at the app's sizes, V = 10 475, J = 55, NB = 20, n_pca = 45, on a seeded synthetic model.

A  coma_amd.body_model.DeviceSMPLX through its autograd function (coma_smplx_forward_f32 + coma_smplx_extra_joints_f32, then
   coma_smplx_backward_f32; the shape stage is cached: the app never changes betas);
B  the same arithmetic in eager torch f32 on the same GPU in the same process (tests/smplx_ref.torch_forward, backward by autograd):
   what the `body_model` hook costs with the third-party package.  The parent commit has no path of its own to compare with.
The two alternate A B A B ... in rounds of --iters evaluations, each round timed by HIP events after --warmup untimed evaluations;
the median, fastest and slowest rounds are printed.  Names the device.

    python scripts/time_body_model.py [--rounds 7] [--iters 50] [--out file.json]
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

    def round_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters

    for fn in (device_path, eager_path):
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    agree = [float((x - y).abs().max() / y.abs().max()) for x, y in zip(device_path(), eager_path())]      # faster and different is not faster
    times = dict(A=[], B=[])
    for _ in range(a.rounds):
        times["A"].append(round_ms(device_path))
        times["B"].append(round_ms(eager_path))
    med = {n: float(np.median(x)) for n, x in times.items()}
    print(f"A device {1e3 * med['A']:9.1f} us (min {1e3 * min(times['A']):.1f}, max {1e3 * max(times['A']):.1f})   "
          f"B eager torch {1e3 * med['B']:9.1f} us (min {1e3 * min(times['B']):.1f}, max {1e3 * max(times['B']):.1f})   B / A {med['B'] / med['A']:.1f}   "
          f"max rel difference A vs B: vertices {agree[0]:.1e}, grad theta {agree[1]:.1e}, grad transl {agree[2]:.1e}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(0), V=V, J=J, NB=NB, n_pca=n_pca, rounds=a.rounds, iters=a.iters, ms=times,
                           median_ms=med, agreement=agree), fh, indent=1)


if __name__ == "__main__":
    main()
