#!/usr/bin/env python3
"""Timing aid for COAP on the device: device time of encode_body (n_samples = 1000), of ONE query at T = 2 000 and T = 20 000 points
(values only, and values with the derivative along the front vector), and of one epoch's collision term, on the seeded model and
weights of tests/coap_ref.py (K = 15 parts, 330 vertices).

A  coma_amd.coap.DeviceCOAP (coma_coap_encode_f32, coma_coap_query_f32, coma_coap_collision_f32);
B  the restatement's arithmetic in eager torch f32 on the same GPU in the same process, written here as the reference computes it:
   every (part, point) pair through both networks (K T rows), inside or not; the epoch's term with its derivative by autograd with
   respect to d.  The parent commit has no path of its own to compare with.
A and B alternate in rounds of --iters evaluations timed by HIP events after --warmup untimed ones; the median round is printed, with
the list length (the rows A evaluates), the matrix-unit time those rows need at the fp32 MFMA peak, and A against B.  Names the device.

    python scripts/time_coap.py [--rounds 5] [--iters 20] [--out file.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FLOP_PER_ROW = 2 * (8 * 256 + 256 * 109 + 112 * 256 + 256 * 128 + 136 * 256 + 256 * 256 + 256 * 125 + 3 * 256 * 256 + 256)      # K = 15
PEAK = 157.3e12


def eager(w, code, dev):
    """query(points, d, f) -> occupancy [T] in torch f32: the dense evaluation of tests/coap_ref.query."""
    import torch
    import torch.nn.functional as F
    p = {k: torch.as_tensor(v).to(dev) for k, v in w.items()}
    B = torch.as_tensor(code["bone_trans"], dtype=torch.float32, device=dev)
    centre, half = (torch.as_tensor(code[k], dtype=torch.float32, device=dev) for k in ("centre", "size"))
    latent = torch.as_tensor(code["latent"], dtype=torch.float32, device=dev)
    K = B.shape[0]
    hot = torch.eye(K, device=dev)
    act = torch.nn.Softplus(beta=100)

    def net(prefix, n, skip, x):
        inp = x
        for i in range(n):
            if i == skip:
                x = torch.cat([x, inp], -1) / np.sqrt(2)
            x = F.linear(x, p[f"{prefix}lin{i}.weight"], p[f"{prefix}lin{i}.bias"])
            if i < n - 1:
                x = act(x)
        return x

    def query(points, d, f):
        T = points.shape[0]
        x = points - d * f
        q = torch.einsum("krc,tc->ktr", B[:, :, :3], x) + B[:, None, :, 3]
        inside = ((q - centre[:, None]).abs() < half[:, None] * 0.5).all(-1)
        z = torch.cat([q, inside[..., None].float(), hot[:, None].expand(K, T, K), latent[:, None].expand(K, T, -1)], -1)
        out = net("decoder.", 7, 3, torch.cat([q, net("query_encoder.", 4, 2, z)], -1))[..., 0]
        return (torch.sigmoid(-out) * inside).max(0).values
    return query


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    import torch
    from coma_amd.coap import DeviceCOAP, draw_samples
    from tests import coap_ref as R
    assert torch.cuda.is_available(), "a timing needs the MI355X"
    dev = "cuda:0"
    M, c = R.model_arrays(), R.case_inputs("ragged")
    body = dict(v_template=M["v_template"], faces=M["faces"], lbs_weights=M["lbs_weights"], parents=M["parents"])
    m = DeviceCOAP(body, M["weights"], n_samples=1000, seed=0, device=dev)
    so = dict(full_pose=c["full_pose"], joints=c["joints"], vertices=c["vertices"])
    table = draw_samples(np.random.RandomState(1), c["vertices"], m.part, 1000)
    m.encode_body(so, samples=table)
    code = R.encode(M["weights"], M["part"], M["parents"], c["full_pose"], c["joints"], c["vertices"], *table)
    ref = eager(M["weights"], code, dev)
    front = c["front"]
    f_t = torch.as_tensor(front, device=dev)
    rng = np.random.RandomState(2)
    print(f"device: {torch.cuda.get_device_name(0)}; K {m.K}, n_samples 1000; {a.rounds} rounds of {a.iters}, A B A B, {a.warmup} warm-up evaluations")

    def round_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters

    def measure(name, fa, fb, rows=None):
        for fn in (fa, fb):
            if fn is not None:
                for _ in range(a.warmup):
                    fn()
        torch.cuda.synchronize()
        ta, tb = [], []
        for _ in range(a.rounds):
            ta.append(round_ms(fa))
            if fb is not None:
                tb.append(round_ms(fb))
        ma, mb = float(np.median(ta)), float(np.median(tb)) if tb else None
        line = f"{name:34s} A device {1e3 * ma:9.1f} us (min {1e3 * min(ta):.1f}, max {1e3 * max(ta):.1f})"
        if mb is not None:
            line += f"   B eager torch {1e3 * mb:9.1f} us   B / A {mb / ma:.1f}"
        if rows is not None:
            line += f"   rows {rows}, at the fp32 MFMA peak {1e6 * rows * FLOP_PER_ROW / PEAK:.1f} us"
        print(line, flush=True)
        return dict(A_ms=ta, B_ms=tb, rows=rows)

    out = {"encode": measure("encode_body (15 x 1000 samples)", lambda: m.encode_body(so, samples=table), None)}
    m.encode_body(so, samples=table)
    for T in (2000, 20000):
        pts = torch.as_tensor((c["vertices"][rng.randint(0, len(c["vertices"]), T)] + rng.normal(size=(T, 3)) * 0.05).astype(np.float32), device=dev)
        d = torch.tensor([0.02], dtype=torch.float64, device=dev)
        d32 = d.float()
        occ = m.query(pts, d=d, front=front)
        want = ref(pts, d32, f_t)
        torch.cuda.synchronize()
        ws = m._ws["query"]
        rows = int(ws[:4].cpu().numpy().view(np.int32)[0])
        print(f"T = {T}: max |A - B| of the occupancy {float((occ - want).abs().max()):.2e}; {rows} of {m.K * T} (part, point) pairs lie in a box")
        out[f"query_{T}"] = measure(f"query T = {T}", lambda: m.query(pts, d=d, front=front), lambda: ref(pts, d32, f_t), rows)
        out[f"query_derivative_{T}"] = measure(f"query + derivative T = {T}", lambda: m.query(pts, d=d, front=front, derivative=True), None, 2 * rows)

        def eager_epoch():
            dd = d32.clone().requires_grad_(True)
            o = ref(pts, dd, f_t)
            torch.relu(o - 0.5).sum().backward()
            return dd.grad
        out[f"epoch_{T}"] = measure(f"epoch's term T = {T}", lambda: m.collision_term(pts, d=d, front=front), eager_epoch, 2 * rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(0), rounds=a.rounds, iters=a.iters, results=out), fh, indent=1)


if __name__ == "__main__":
    main()
