#!/usr/bin/env python3
"""Golden vectors for the multiview term and the Adam loop of the depth optimisation, produced by the REAL reference function
`multiview_joint_loss` (/root/reference/src/generation/optimize_depth.py:371-400) under `torch.optim.Adam([displacement])`, the
optimiser of :690-695, with w_collision = 0.

The function is imported from /root/reference with its third-party imports stubbed and every `torch.tensor(.., device="cuda")` inside
that module redirected to the CPU (as make_golden_triangulation.py does for `to_tensor`).  It runs, in f32 as the reference does, on
seeded synthetic joints and cameras for 200 epochs with joints = J0 + displacement * front (:732-736), and the trajectory of the
displacement and the loss of every epoch are stored in tests/golden/depth_opt_golden.npz together with the inputs and the reference's
own joint table (use_hands=False).  Two cases:
  far       the optimum lies farther than lr * E from the start: the gradient never changes sign
  converge  the optimum is reached well inside the 200 epochs
The restatement (tests/shift_ref.py, f64) is run on the same inputs and max |d_ref - d_restated| is printed: tests/test_depth_opt_host.py
allows 4x that.   Run: python tests/golden/make_golden_depth_opt.py
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
E = 200


def import_reference():
    class _Any(types.ModuleType):
        def __getattr__(self, k):
            if k.startswith("__"):
                raise AttributeError(k)
            return lambda *a, **kw: None
    for name in ["pytorch3d", "pytorch3d.io", "trimesh", "trimesh.boolean", "smplx", "smplx.utils", "imports", "imports.coap",
                 "open3d", "cv2", "easydict"]:
        sys.modules.setdefault(name, _Any(name))
    sys.modules["smplx.utils"].SMPLXOutput = object
    assert ROOT not in sys.path          # the reference's src / utils / constants must be the ones imported
    sys.path.insert(0, REF)
    m = importlib.import_module("src.generation.optimize_depth")
    assert m.__file__.startswith(REF), m.__file__
    from utils.smpl import smpl_to_openpose
    idx = smpl_to_openpose(model_type="smplx", use_hands=False, use_face=False, use_face_contour=False)
    sys.path.remove(REF)
    for name in [k for k in sys.modules if k.split(".")[0] in ("src", "utils", "constants")]:
        del sys.modules[name]            # so that the repository's own packages can be imported afterwards
    sys.path.insert(0, ROOT)
    return m, np.asarray(idx)


class TorchOnCpu:
    """torch, with the device argument of `tensor` dropped."""
    def __getattr__(self, k):
        return getattr(torch, k)

    def tensor(self, *a, device=None, **kw):
        return torch.tensor(*a, **kw)


def look_at(eye, target):
    f = target - eye
    f /= np.linalg.norm(f)
    r = np.cross(f, [0.0, 0.0, 1.0])
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    return np.stack([r, u, -f], axis=1)


def make_case(seed, n_views, d_true, noise):
    rng = np.random.default_rng(seed)
    J = 137
    joints0 = (rng.normal(scale=[0.25, 0.15, 0.45], size=(J, 3)) + np.array([0.0, 0.0, 0.9])).astype(np.float32)
    centre = np.array([0.0, 0.0, 0.9])
    ref_eye = np.array([0.3, -2.6, 1.3])
    front = look_at(ref_eye, centre)[:, 2].astype(np.float32)
    target = joints0.astype(np.float64) + d_true * front.astype(np.float64)
    C = np.diag([1.0, -1.0, -1.0])
    cams, xy = [], []
    for v in range(n_views):
        ang = 2 * np.pi * (v + 1) / (n_views + 2) + rng.normal(scale=0.05)
        eye = np.array([2.6 * np.cos(ang), 2.6 * np.sin(ang), 1.2 + rng.normal(scale=0.2)])
        R, t, scale, res = look_at(eye, centre).astype(np.float32), eye.astype(np.float32), float(2.4 + 0.1 * v), (512, 512)
        q = target @ (R.astype(np.float64) @ C) - t.astype(np.float64).reshape((1, 3)) @ (R.astype(np.float64) @ C)
        px = q[:, :2] / scale * max(res) + np.array(res) / 2 + rng.normal(scale=noise, size=(J, 2))
        cams.append(dict(R=R, t=t, scale=scale, resolution=res))
        xy.append(px.astype(np.float32))
    return joints0, front, cams, np.stack(xy)


def run_reference(m, joints0, front, cams, xy, lr, w_multiview):
    inliers = [dict(camera_config=dict(R=torch.from_numpy(c["R"]), t=torch.from_numpy(c["t"]), scale=c["scale"], resolution=c["resolution"]),
                    joints_proj=torch.from_numpy(p).unsqueeze(0)) for c, p in zip(cams, xy)]
    J0, f = torch.from_numpy(joints0).unsqueeze(0), torch.from_numpy(front)
    displacement = torch.nn.Parameter(torch.tensor([0.0]), requires_grad=True)
    optimizer = torch.optim.Adam([displacement], lr=lr)
    traj, losses = [float(displacement.item())], []
    for _ in range(E):
        optimizer.zero_grad()
        loss = w_multiview * m.multiview_joint_loss(J0 + displacement * f, inliers)
        loss.backward()
        optimizer.step()
        losses.append(float(loss.item()) / w_multiview)
        traj.append(float(displacement.item()))
    return np.array(traj), np.array(losses)


def main():
    m, idx = import_reference()
    m.torch = TorchOnCpu()
    from coma_amd.triangulate import view_record
    from tests import shift_ref as SR
    out = {"body_indices": idx.astype(np.int64)}
    for tag, scene, lr, w in (("far", dict(seed=11, n_views=5, d_true=5.0, noise=1.5), 0.01, 1e-3),
                              ("converge", dict(seed=12, n_views=4, d_true=0.3, noise=1.0), 0.01, 1e-3)):
        joints0, front, cams, xy = make_case(**scene)
        traj, losses = run_reference(m, joints0, front, cams, xy, lr, w)
        views = np.stack([view_record(dict(R=c["R"].astype(np.float64), t=c["t"].astype(np.float64), scale=c["scale"], resolution=c["resolution"]))
                          for c in cams])
        mine = SR.optimize(None, views, joints0.astype(np.float64)[idx], front.astype(np.float64), np.arange(len(cams)),
                           xy.astype(np.float64)[:, idx], 0.0, lr, w, 0.0, E)
        steps = np.diff(traj)
        print(f"  {tag}: d goes 0 -> {traj[-1]:.6f} (lr * E = {lr * E}), sign changes of the step {int((np.sign(steps[1:]) != np.sign(steps[:-1])).sum())}, "
              f"max |d_ref - d_restated| = {np.abs(traj - mine['traj']).max():.3e}, "
              f"max relative loss difference = {np.abs(losses / mine['losses'][:, 0] - 1).max():.3e}")
        out[f"{tag}_joints0"], out[f"{tag}_front"], out[f"{tag}_xy"] = joints0, front, xy
        out[f"{tag}_cam_R"], out[f"{tag}_cam_t"] = np.stack([c["R"] for c in cams]), np.stack([c["t"] for c in cams])
        out[f"{tag}_cam_scale"] = np.array([c["scale"] for c in cams])
        out[f"{tag}_cam_res"] = np.array([c["resolution"] for c in cams], dtype=np.int64)
        out[f"{tag}_params"] = np.array([lr, w], dtype=np.float64)
        out[f"{tag}_traj"], out[f"{tag}_losses"] = traj, losses
    pth = os.path.join(HERE, "depth_opt_golden.npz")
    np.savez_compressed(pth, **out)
    print(f"wrote depth_opt_golden.npz ({os.path.getsize(pth) / 1e3:.0f} kB)")


if __name__ == "__main__":
    main()
