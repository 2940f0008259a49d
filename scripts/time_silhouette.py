#!/usr/bin/env python3
"""Timing aid for depth initialisation's silhouette test: device milliseconds per call (HIP events, after warm-up) of the two draws
(coma_raster_depth_f64) and the count pass (coma_silhouette_iou) at 512 x 512, K = 7, next to the NumPy restatement's time.

Meshes: an icosphere at subdivision 5 (20 480 faces, the size of SMPL-X) as the human; as assets an icosphere at subdivision 6
plus its subdivision-5 shell (102 400 faces) and a 12-face box whose triangles each cover much of the image.

    python scripts/time_silhouette.py [--iters 200] [--skip-numpy]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--skip-numpy", action="store_true")
    a = ap.parse_args()
    import torch
    from coma_amd import _lib
    L = _lib.lib()
    dev = "cuda:0"
    W = H = a.size
    K = 7
    eye = np.array([2.0, -2.0, 1.5])
    R, t = RR.look_at(eye), eye
    human = RR.icosphere(5, 0.8, (0.0, 0.0, 0.1))
    big_a, big_b = RR.icosphere(6, 0.9, (0.3, 0.3, 0.0)), RR.icosphere(5, 0.5, (0.3, 0.3, 0.0))
    dense = (np.concatenate([big_a[0], big_b[0]]), np.concatenate([big_a[1], big_b[1] + len(big_a[0])]).astype(np.int32))
    meshes = {"human (icosphere 5)": human, "dense asset": dense, "12-face box": RR.box((-0.9, -0.9, -0.8), (1.0, 0.9, 0.7))}
    dp = C.POINTER(C.c_double)
    Rh, th = np.ascontiguousarray(R.reshape(9)), np.ascontiguousarray(t)
    print(f"device: {torch.cuda.get_device_name(0)}; {W} x {H}, K = {K}, {a.iters} iterations after {a.warmup} warm-up calls")

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

    keys = {}
    for name, (v, f) in meshes.items():
        vd = torch.tensor(np.ascontiguousarray(v, dtype=np.float64), device=dev)
        fd = torch.tensor(np.ascontiguousarray(f, dtype=np.int32), device=dev)
        ws = torch.empty([L.coma_raster_workspace_bytes(len(v), len(f)) // 8 + 2], dtype=torch.int64, device=dev)
        key = torch.empty([H, W], dtype=torch.int64, device=dev)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def draw():
            rc = L.coma_raster_depth_f64(_lib.ptr(vd), len(v), _lib.ptr(fd), len(f), Rh.ctypes.data_as(dp), th.ctypes.data_as(dp), 2.5, W, H,
                                         _lib.ptr(ws), _lib.ptr(key), st)
            assert rc == 0, L.coma_last_error()
        ms = timed(draw)
        assert L.coma_raster_status(_lib.ptr(ws), st) == 0, L.coma_last_error()
        keys[name] = key
        line = f"draw  {name:22s} {len(f):7d} faces  {int((key != -1).sum()):7d} covered pixels  device {ms:8.4f} ms"
        if not a.skip_numpy:
            t0 = time.perf_counter()
            ref = RR.raster_depth(v, f, R, t, 2.5, W, H)
            line += f"   NumPy restatement {1e3 * (time.perf_counter() - t0):9.1f} ms   keys equal: {np.array_equal(ref, key.cpu().numpy().view(np.uint64))}"
        print(line)

    off = torch.tensor(np.linspace(-1.5, 1.5, K), device=dev)
    yy, xx = np.mgrid[0:H, 0:W]
    gt_h = (((xx - W / 2) ** 2 + (yy - H / 2) ** 2) < (0.3 * W) ** 2).astype(np.uint8)
    gt = torch.tensor(gt_h, device=dev)
    counts = torch.empty([3, K], dtype=torch.int64, device=dev)
    masks = torch.empty([K, H, W], dtype=torch.uint8, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    hk = keys["human (icosphere 5)"]
    for name in ("dense asset", "12-face box"):
        for with_masks in (False, True):
            def count():
                rc = L.coma_silhouette_iou(_lib.ptr(hk), _lib.ptr(keys[name]), _lib.ptr(off), K, _lib.ptr(gt), W, H, _lib.ptr(counts[0]), _lib.ptr(counts[1]),
                                           _lib.ptr(counts[2]), _lib.ptr(masks) if with_masks else None, st)
                assert rc == 0, L.coma_last_error()
            ms = timed(count)
            line = f"count vs {name:19s} masks {'yes' if with_masks else 'no ':3s} visible {counts[0].tolist()}  device {ms:8.4f} ms"
            if not a.skip_numpy and with_masks:
                t0 = time.perf_counter()
                RR.silhouette_iou(hk.cpu().numpy().view(np.uint64), keys[name].cpu().numpy().view(np.uint64), off.cpu().numpy(), gt_h)
                line += f"   NumPy restatement {1e3 * (time.perf_counter() - t0):9.1f} ms"
            print(line)


if __name__ == "__main__":
    main()
