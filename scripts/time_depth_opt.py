#!/usr/bin/env python3
"""Timing aid for the depth optimisation: device milliseconds (HIP events, after warm-up) of coma_shift_columns_prepare, of one
coma_shift_profile call (K = 1 and K = 64) and of the whole coma_depth_optimize_f64 loop (200 epochs, both terms), at a 512 x 512 grid
for a 20 480-face human against a 102 400-face asset with 32 inlier views of 25 joints.  Names the device.

Meshes as in scripts/time_intersection.py: an icosphere at subdivision 5 as the human; an icosphere at subdivision 6 plus its
subdivision-5 shell as the asset.

    python scripts/time_depth_opt.py [--iters 20] [--epochs 200]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import raster_ref as RR  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--views", type=int, default=32)
    a = ap.parse_args()
    import torch
    from coma_amd import depth_opt as D, metrics as M
    from coma_amd.triangulate import view_record
    dev = "cuda:0"
    human = RR.icosphere(5, 0.8, (0.0, 0.0, 0.1))
    big_a, big_b = RR.icosphere(6, 0.9, (0.3, 0.3, 0.0)), RR.icosphere(5, 0.5, (0.3, 0.3, 0.0))
    asset = (np.concatenate([big_a[0], big_b[0]]), np.concatenate([big_a[1], big_b[1] + len(big_a[0])]).astype(np.int32))
    grid = M.overlap_grid_xy(human[0], asset[0], a.size)
    print(f"device: {torch.cuda.get_device_name(0)}; grid {grid[3]} x {grid[4]}, {len(human[1])} + {len(asset[1])} faces, "
          f"{a.iters} iterations after {a.warmup} warm-up calls")

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters

    # the wrappers copy their arguments and read the results back, so these are upper bounds on the device time of one call
    cols = D.prepare_columns(human[0], human[1], asset[0], asset[1], *grid, device=dev)
    print(f"coma_shift_columns_prepare  {cols.crossings} crossings, L_A {cols.L_A}  {timed(lambda: D.prepare_columns(human[0], human[1], asset[0], asset[1], *grid, device=dev)):8.3f} ms (with copies)")
    for K in (1, 64):
        d = np.linspace(-0.5, 0.5, K)
        print(f"coma_shift_profile  K = {K:2d}  {timed(lambda: D.shift_profile(cols, d)):8.3f} ms (with copies)")
    rng = np.random.default_rng(0)
    joints0 = rng.normal(scale=0.4, size=(25, 3))
    cams = [dict(R=RR.look_at(e, (0.0, 0.0, 0.0)), t=e, scale=2.4, resolution=(512, 512)) for e in rng.normal(size=(a.views, 3)) * 0.3 + np.array([0.0, -3.0, 0.5])]
    views = np.stack([view_record(c) for c in cams])
    cand_xy = rng.normal(scale=40.0, size=(a.views, 25, 2)) + 256.0
    run = lambda: D.optimize_displacement(cols, views, joints0, (0.0, 0.0, 1.0), np.arange(a.views), cand_xy, 0.0, 0.01, 1e-3, 0.4, a.epochs, device=dev)  # noqa: E731
    ms = timed(run)
    print(f"coma_depth_optimize_f64  {a.epochs} epochs, {a.views} views  {ms:8.3f} ms = {1e3 * ms / a.epochs:7.2f} us per epoch (with copies)   d = {run()['d']!r}")


if __name__ == "__main__":
    main()
