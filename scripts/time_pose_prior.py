#!/usr/bin/env python3
"""Timing aid for the device VPoser decoder: device time of ONE decode + backward (axis-angle pose from the embedding, then dL/dz from
a given dL/daa) at the app's sizes, N = 1, latent 32, 512 neurons, 21 joints, on seeded synthetic weights.

A  coma_amd.pose_prior.DeviceVPoser through its autograd function (coma_vposer_decode_f32, then coma_vposer_decode_backward_f32);
B  the same network in eager torch f32 on the same GPU in the same process, written here (three Linear + leaky ReLU, Gram-Schmidt,
   the four quaternion candidates blended through float masks, 2 atan2, backward by autograd): what the `pose_decoder` hook costs
   with the third-party module.  The parent commit has no path of its own to compare with.
The two alternate A B A B ... in rounds of --iters evaluations, each round timed by HIP events after --warmup untimed evaluations;
the median, fastest and slowest rounds are printed.  Launch counts: A's are the library's (4 forward + 4 backward, stated in
include/coma_hip.h); B's kernel launches are counted with torch.profiler over one evaluation, outside the timed rounds.  Names the device.

    python scripts/time_pose_prior.py [--rounds 7] [--iters 200] [--out file.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def eager_decoder(w, dev):
    """The decoder as a chain of torch operations, one per step of the rule set, every candidate evaluated and blended by masks."""
    import torch
    import torch.nn.functional as F
    p = {k: torch.as_tensor(v).to(dev) for k, v in w.items()}

    def decode(z):
        h = F.leaky_relu(F.linear(z, p["bodyprior_dec_fc1.weight"], p["bodyprior_dec_fc1.bias"]), 0.2)
        h = F.leaky_relu(F.linear(h, p["bodyprior_dec_fc2.weight"], p["bodyprior_dec_fc2.bias"]), 0.2)
        o = F.linear(h, p["bodyprior_dec_out.weight"], p["bodyprior_dec_out.bias"]).view(-1, 3, 2)
        b1 = F.normalize(o[:, :, 0], dim=1)
        b2 = F.normalize(o[:, :, 1] - (b1 * o[:, :, 1]).sum(1, keepdim=True) * b1, dim=1)
        T = torch.stack([b1, b2, torch.cross(b1, b2, dim=1)], 1)                    # rows b1, b2, b3: the transposed rotation
        d0, d1, d2 = T[:, 0, 0], T[:, 1, 1], T[:, 2, 2]
        low, m01, m0n1 = (d2 < 1e-6).float(), (d0 > d1).float(), (d0 < -d1).float()
        t = [1 + d0 - d1 - d2, 1 - d0 + d1 - d2, 1 - d0 - d1 + d2, 1 + d0 + d1 + d2]
        a, b, c = T[:, 1, 2], T[:, 2, 0], T[:, 0, 1]
        at, bt, ct = T[:, 2, 1], T[:, 0, 2], T[:, 1, 0]
        cand = [torch.stack([a - at, t[0], c + ct, b + bt], -1), torch.stack([b - bt, c + ct, t[1], a + at], -1),
                torch.stack([c - ct, b + bt, a + at, t[2]], -1), torch.stack([t[3], a - at, b - bt, c - ct], -1)]
        masks = [low * m01, low * (1 - m01), (1 - low) * m0n1, (1 - low) * (1 - m0n1)]
        q = sum(x * m[:, None] for x, m in zip(cand, masks)) / torch.sqrt(sum(x * m for x, m in zip(t, masks)))[:, None] * 0.5
        s2 = (q[:, 1:] * q[:, 1:]).sum(1)
        s = torch.sqrt(s2)
        two_theta = 2.0 * torch.where(q[:, 0] < 0, torch.atan2(-s, -q[:, 0]), torch.atan2(s, q[:, 0]))
        k = torch.where(s2 > 0, two_theta / s, torch.full_like(s, 2.0))
        return (q[:, 1:] * k[:, None]).reshape(z.shape[0], -1)
    return decode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    import torch
    from coma_amd.pose_prior import DeviceVPoser
    from tests import vposer_ref as V
    assert torch.cuda.is_available(), "a timing needs the MI355X"
    dev = "cuda:0"
    N, D, H, NJ = 1, 32, 512, 21
    w = V.synthetic_weights(H, D, NJ, seed=21, kind="near_rest")
    vp = DeviceVPoser(w, H, D, [1, NJ, 3], device=dev)
    eager = eager_decoder(w, dev)
    rng = np.random.RandomState(22)
    t = lambda x: torch.as_tensor(np.asarray(x, dtype=np.float32)).to(dev)
    z, g = t(rng.normal(size=(N, D))), t(rng.normal(size=(N, 3 * NJ)))
    print(f"device: {torch.cuda.get_device_name(0)}; N {N}, latent {D}, neurons {H}, joints {NJ}; {a.rounds} rounds of {a.iters} decode + backward, "
          f"A B A B, {a.warmup} warm-up evaluations each")

    def device_path():
        zz = z.clone().requires_grad_(True)
        aa = vp.decode(zz, output_type="aa").reshape(N, -1)
        return aa.detach(), torch.autograd.grad(aa, zz, g)[0]

    def eager_path():
        zz = z.clone().requires_grad_(True)
        aa = eager(zz)
        return aa.detach(), torch.autograd.grad(aa, zz, g)[0]

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
          f"max rel difference A vs B: aa {agree[0]:.1e}, grad z {agree[1]:.1e}")
    launches = {}
    for name, fn in (("A", device_path), ("B", eager_path)):      # after the timed rounds: tracing slows the host
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        launches[name] = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
    print(f"device activities of one evaluation (kernels and copies, torch's clone and reshape included): A {launches['A']} "
          f"(the library's own: 4 forward + 4 backward), B {launches['B']}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(0), N=N, D=D, H=H, NJ=NJ, rounds=a.rounds, iters=a.iters, ms=times, median_ms=med,
                           agreement=agree, device_activities=launches), fh, indent=1)


if __name__ == "__main__":
    main()
