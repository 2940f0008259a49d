#!/usr/bin/env python3
"""Timing aid for the optimisation app's ComA objective: device time of ONE evaluation (both terms and both gradients) at the app's
sizes, V = 10 475 vertices, F = 20 908 faces, k in {500, 5000} selected vertices, O = 2048 object points.

A  coma_amd.app.ComaObjective.evaluate (coma_app_objective_f32: seven kernels and one memset);
B  the same lines of the reference (src/application/optimize.py:274-289, :295-296) restated in eager torch on the same GPU in the same
   process, forward and backward by autograd: three index_add calls, three normalisations, the canonicalisation over ALL O object
   normals of which one column is used, two k x k cdist matrices.  The parent commit has no path of its own to compare with.
The two alternate A B A B ... in rounds of --iters evaluations, each round timed by HIP events after --warmup untimed evaluations;
the median, fastest and slowest rounds are printed, then the number of device kernels one evaluation of each launches (torch.profiler,
in a pass of its own after the timing).  Names the device.

    python scripts/time_app_objective.py [--rounds 7] [--iters 50] [--out file.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V_APP, F_APP, O_APP = 10475, 20908, 2048


def app_sized_mesh(seed=0):
    """A 25 x 419 bumpy grid (10 475 vertices, 20 064 faces) plus 844 more faces between neighbouring rows: the app's sizes, and
    5 to 8 faces around most vertices as on a body mesh."""
    rng = np.random.default_rng(seed)
    n, m = 25, 419
    i, j = np.meshgrid(np.arange(n), np.arange(m), indexing="ij")
    verts = np.stack([i * 0.02 + rng.uniform(-0.004, 0.004, i.shape), j * 0.004 + rng.uniform(-0.001, 0.001, i.shape),
                      0.1 * np.sin(0.3 * i) * np.cos(0.05 * j)], -1).reshape(-1, 3).astype(np.float32)
    idx = np.arange(n * m).reshape(n, m)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    faces = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)])
    more = rng.choice(len(a), size=F_APP - len(faces), replace=False)
    faces = np.concatenate([faces, np.stack([b[more], c[more], d[more]], 1)]).astype(np.int64)
    assert verts.shape == (V_APP, 3) and faces.shape == (F_APP, 3)
    return verts, faces


def eager_objective(torch, vertices, faces, gt, obj_normals, ref_index, p, sub_p, eps, sel, targets):
    """The reference's lines in eager torch, f32, shapes as there ([V,O,3] canonicalisation, cdist); returns the two unweighted terms."""
    F = torch.nn.functional
    unit = lambda v: v / (torch.sqrt(torch.sum(torch.square(v), dim=-1, keepdim=True)) + eps)
    vf = vertices[faces]
    normals = torch.zeros_like(vertices)
    normals = normals.index_add(0, faces[:, 1], torch.cross(vf[:, 2] - vf[:, 1], vf[:, 0] - vf[:, 1], dim=1))
    normals = normals.index_add(0, faces[:, 2], torch.cross(vf[:, 0] - vf[:, 2], vf[:, 1] - vf[:, 2], dim=1))
    normals = normals.index_add(0, faces[:, 0], torch.cross(vf[:, 1] - vf[:, 0], vf[:, 2] - vf[:, 0], dim=1))
    a = unit(unit(F.normalize(normals, eps=1e-6, dim=1)))
    b, p, s = unit(obj_normals), unit(p[None])[0], unit(sub_p[None])[0]
    b_dot_p = torch.sum(b * p[None], dim=-1)[None]
    a_dot_b = torch.sum(a[:, None] * b[None], dim=-1)
    a_dot_p = torch.sum(a * p[None], dim=-1)[:, None]
    a_dot_s = torch.sum(a * s[None], dim=-1)[:, None]
    replace = ((1 + b_dot_p) < eps)[:, :, None]
    replacer = 2 * a_dot_s[:, :, None] * s[None, None] - a[:, None]
    bx = torch.zeros([b.shape[0], 3, 3], dtype=b.dtype, device=b.device)
    bx[:, 0, 1], bx[:, 0, 2], bx[:, 1, 0], bx[:, 1, 2], bx[:, 2, 0], bx[:, 0, 0] = -b[:, 2], b[:, 1], b[:, 2], -b[:, 0], -b[:, 1], b[:, 0]
    c = torch.einsum("bij,j->bi", bx, p)
    a_dot_c = torch.sum(a[:, None] * c[None], dim=-1)
    f = c[None] * a_dot_c[:, :, None]
    f = torch.where(replace, 0, f / (1 + b_dot_p[:, :, None]))
    f = f + b_dot_p[:, :, None] * a[:, None] + a_dot_b[:, :, None] * p[None, None] - a_dot_p[:, :, None] * b[None]
    f = torch.where(replace, replacer, f)
    f = f / torch.sqrt(torch.sum(torch.square(f), dim=-1, keepdim=True))
    rel = f[:, ref_index]
    orientation = torch.mean(torch.nan_to_num(1 - (torch.bmm(gt.view(-1, 1, 3), rel.reshape(-1, 3, 1)).squeeze() + 1) / 2))
    A = vertices[sel]
    contact = torch.mean(torch.min(torch.cdist(A, targets), dim=1)[0]) + torch.mean(torch.min(torch.cdist(targets, A), dim=1)[0])
    return orientation, contact


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    import torch
    from coma_amd.app import ComaObjective
    assert torch.cuda.is_available(), "a timing needs the MI355X"
    dev = "cuda:0"
    verts, faces = app_sized_mesh()
    rng = np.random.default_rng(1)
    unit_rows = lambda n: (lambda x: (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32))(rng.normal(size=(n, 3)))
    gt, obj_normals = unit_rows(V_APP), unit_rows(O_APP)
    obj_verts = (rng.uniform(0, 1, size=(O_APP, 3)) * [0.5, 1.7, 0.2] + [0.0, 0.0, 0.15]).astype(np.float32)
    print(f"device: {torch.cuda.get_device_name(0)}; V {V_APP}, F {F_APP}, O {O_APP}; {a.rounds} rounds of {a.iters} evaluations, A B A B, "
          f"{a.warmup} warm-up evaluations each")
    result = dict(device=torch.cuda.get_device_name(0), V=V_APP, F=F_APP, O=O_APP, rounds=a.rounds, iters=a.iters, cases=[])
    for k in (500, 5000):
        sel = np.sort(rng.choice(V_APP, size=k, replace=False))
        objects = rng.integers(0, O_APP, size=k)
        objective = ComaObjective(faces, gt, obj_normals[0], sel, obj_verts[objects], device=dev)
        t = lambda x, dt=torch.float32: torch.as_tensor(np.ascontiguousarray(x)).to(device=dev, dtype=dt)
        v = t(verts)
        const = dict(faces=t(faces, torch.int64), gt=t(gt), obj_normals=t(obj_normals), ref_index=0, p=t([0.0, 0.0, 1.0]), sub_p=t([0.0, 1.0, 0.0]),
                     eps=1e-6, sel=t(sel, torch.int64), targets=t(obj_verts[objects]))

        def device_path():
            return objective.evaluate(v)

        def eager_path():
            x = v.clone().requires_grad_(True)
            t_o, t_c = eager_objective(torch, x, **const)
            g_o, = torch.autograd.grad(t_o, x, retain_graph=True)
            g_c, = torch.autograd.grad(t_c, x)
            return torch.stack([t_o.detach(), t_c.detach()]), g_o, g_c

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
        # faster and different is not faster: the two paths agree at the size that is timed (argmin flips between the reference's
        # matrix-product cdist and coordinate differences move single rows, hence the loose figure on the contact gradient)
        d, e = device_path(), eager_path()
        agree = [float((x - y).abs().max() / y.abs().max()) for x, y in zip(d, e)]
        times = dict(A=[], B=[])
        for _ in range(a.rounds):
            times["A"].append(round_ms(device_path))
            times["B"].append(round_ms(eager_path))
        launches = {}
        try:
            from torch.profiler import ProfilerActivity, profile
            for name, fn in (("A", device_path), ("B", eager_path)):
                with profile(activities=[ProfilerActivity.CUDA]) as prof:
                    fn()
                    torch.cuda.synchronize()
                launches[name] = sum(1 for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA)
        except Exception as exc:            # the count is a by-product; the timing stands without it
            launches = dict(error=repr(exc))
        med = {n: float(np.median(x)) for n, x in times.items()}
        print(f"k = {k:5d}  A device {1e3 * med['A']:9.1f} us (min {1e3 * min(times['A']):.1f}, max {1e3 * max(times['A']):.1f})   "
              f"B eager torch {1e3 * med['B']:9.1f} us (min {1e3 * min(times['B']):.1f}, max {1e3 * max(times['B']):.1f})   B / A {med['B'] / med['A']:.1f}   "
              f"device launches per evaluation {launches}   max rel difference A vs B: terms {agree[0]:.1e}, orientation gradient {agree[1]:.1e}, "
              f"contact gradient {agree[2]:.1e}")
        result["cases"].append(dict(k=k, ms=times, median_ms=med, launches=launches, agreement=agree))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
