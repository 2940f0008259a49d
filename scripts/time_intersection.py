#!/usr/bin/env python3
"""Timing aid for the intersection-volume metric: device milliseconds per call (HIP events, after warm-up) of
coma_intersection_columns at 512 x 512 for a 20 480-face human against a 102 400-face asset, and of coma_mesh_volume_f64 on the
human, next to the NumPy restatement's time.  Names the device.

Meshes: an icosphere at subdivision 5 (20 480 faces, the size of SMPL-X) as the human; an icosphere at subdivision 6 plus its
subdivision-5 shell (102 400 faces) as the asset.

    python scripts/time_intersection.py [--iters 100] [--skip-numpy]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import raster_ref as RR  # noqa: E402
from tests import volume_ref as VR  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--skip-numpy", action="store_true")
    a = ap.parse_args()
    import torch
    from coma_amd import _lib, metrics as M
    L = _lib.lib()
    dev = "cuda:0"
    human = RR.icosphere(5, 0.8, (0.0, 0.0, 0.1))
    big_a, big_b = RR.icosphere(6, 0.9, (0.3, 0.3, 0.0)), RR.icosphere(5, 0.5, (0.3, 0.3, 0.0))
    asset = (np.concatenate([big_a[0], big_b[0]]), np.concatenate([big_a[1], big_b[1] + len(big_a[0])]).astype(np.int32))
    x0, y0, s, W, H = M.overlap_grid(human[0], asset[0], a.size)
    print(f"device: {torch.cuda.get_device_name(0)}; grid {W} x {H}, {len(human[1])} + {len(asset[1])} faces, {a.iters} iterations after {a.warmup} warm-up calls")

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

    t = [torch.tensor(np.ascontiguousarray(m[0], dtype=np.float64), device=dev) for m in (human, asset)]
    f = [torch.tensor(np.ascontiguousarray(m[1], dtype=np.int32), device=dev) for m in (human, asset)]
    capacity = 8 * W * H
    ws = torch.empty([L.coma_column_crossings_workspace_bytes(len(human[0]), len(human[1]), len(asset[0]), len(asset[1]), W, H, capacity) // 16 + 1, 2],
                     dtype=torch.int64, device=dev)
    sums = torch.zeros([3], dtype=torch.int64, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def columns():
        rc = L.coma_intersection_columns(_lib.ptr(t[0]), len(human[0]), _lib.ptr(f[0]), len(human[1]), _lib.ptr(t[1]), len(asset[0]), _lib.ptr(f[1]),
                                         len(asset[1]), x0, y0, s, W, H, capacity, _lib.ptr(ws), _lib.ptr(sums), None, st)
        assert rc == 0, L.coma_last_error()
    ms = timed(columns)
    needed = C.c_int64(0)
    assert L.coma_intersection_status(_lib.ptr(ws), st, C.byref(needed)) == 0, L.coma_last_error()
    got = sums.cpu().numpy()
    line = f"coma_intersection_columns  {needed.value} crossings  V_AB {VR.volumes(got, s)[0]:.6f}  device {ms:8.4f} ms"
    if not a.skip_numpy:
        t0 = time.perf_counter()
        ref = VR.intersection_columns(human[0], human[1], asset[0], asset[1], x0, y0, s, W, H)[0]
        line += f"   NumPy restatement {1e3 * (time.perf_counter() - t0):9.1f} ms   sums equal: {np.array_equal(ref, got)}"
    print(line)

    out = torch.zeros([1], dtype=torch.float64, device=dev)
    vws = torch.empty([L.coma_mesh_volume_workspace_bytes(len(human[1])) // 8 + 1], dtype=torch.int64, device=dev)

    def volume():
        rc = L.coma_mesh_volume_f64(_lib.ptr(t[0]), len(human[0]), _lib.ptr(f[0]), len(human[1]), _lib.ptr(out), _lib.ptr(vws), st)
        assert rc == 0, L.coma_last_error()
    ms = timed(volume)
    print(f"coma_mesh_volume_f64       {len(human[1])} faces  volume {out.item():.6f} (NumPy {VR.mesh_volume(*human)[0]:.6f})  device {ms:8.4f} ms")


if __name__ == "__main__":
    main()
