#!/usr/bin/env python3
"""Time coma_sample_eliminate_f64 (HIP events, after warm-up) and its NumPy restatement on the host for the same input:
python scripts/time_sample_elim.py [--n 1500 2048] [--reps 5] [--no-host]

Candidates are 5 N uniform samples of the unit-box test mesh (tests/sample_elim_ref.py).  Prints one JSON line per N: the whole
call, the initial-weight kernel alone (a call with n_keep = M - 1 runs it and a single loop step), and time per elimination step."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from coma_amd import _lib
from tests import sample_elim_ref as R


def device_ms(L, pts, n_keep, r_max, r_min, reps):
    M = pts.shape[0]
    ws = torch.empty([L.coma_sample_eliminate_workspace_bytes(M) // 8], dtype=torch.float64, device=pts.device)
    keep = torch.empty([n_keep], dtype=torch.int64, device=pts.device)
    def run():
        rc = L.coma_sample_eliminate_f64(_lib.ptr(pts), M, n_keep, r_max, r_min, 8.0, _lib.ptr(ws), _lib.ptr(keep), _lib.stream_ptr(pts.device))
        _lib.check(rc, "coma_sample_eliminate_f64")
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), keep.cpu().numpy()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1500, 2048])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    L = _lib.lib()
    for n in args.n:
        cand, r_max, r_min = R.case("grid_box", n, 0)
        pts = torch.tensor(cand, device="cuda:0")
        M = len(cand)
        full, keep = device_ms(L, pts, n, r_max, r_min, args.reps)
        init, _ = device_ms(L, pts, M - 1, r_max, r_min, args.reps)
        out = {"N": n, "M": M, "device_ms": round(full, 3), "init_plus_one_step_ms": round(init, 3),
               "us_per_step": round(1e3 * (full - init) / max(1, M - n - 1), 3), "device": torch.cuda.get_device_name(0)}
        if not args.no_host:
            t = time.perf_counter()
            ref = R.sample_eliminate(cand, n, r_max, r_min)
            out["host_numpy_ms"] = round(1e3 * (time.perf_counter() - t), 1)
            out["equal"] = bool(np.array_equal(ref, keep))
        print(json.dumps(out), flush=True)
