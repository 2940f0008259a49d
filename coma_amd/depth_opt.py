"""Depth optimisation on MI355X: the stage of the reference's src/generation/optimize_depth.py between the depth initialisation and
the sample metrics, without a body model in the loop; COAP's collision loss is opt-in (optimize_displacement_coap).

The reference's optimiser holds one parameter, the displacement d along the camera's front vector f (optimize_depth.py:690-695): the
pose, shape and orientation residuals it creates never reach the optimiser, so the SMPL-X forward gives the same vertices V0 and
joints J0 in every epoch and the human of epoch t is V0 + d f, J0 + d f.  Its loss is w_multiview * multiview_joint_loss +
w_collision * collision (:757).

COAP's collision loss (a learned occupancy network) runs through coma_amd.coap and optimize_displacement_coap; its architecture is
pinned against the code the reference vendors with seeded weights, its downloaded checkpoint has never been executed here.  The
default collision term (optimize_displacement) is geometric: with both meshes rotated into the camera-aligned frame (front vector =
+z) the human's column crossings only shift by a constant, so the intersection length L_AB is an exact integer, piecewise-linear
function of the shift, and the term is the intersection ratio L_AB / L_A in [0, 1] -- the quantity compute_metrics.py reports and
filter.py thresholds.  `w_collision` there weights a ratio, not COAP's loss.  Rule set: include/coma_hip.h; restated in
tests/shift_ref.py.

Everything per epoch runs on the device (coma_amd/csrc/depth_opt.hip); no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .metrics import _mesh, _scratch, overlap_grid_xy
from .triangulate import COMPATIBILITY_MATRIX_OPENGL_TO_BLENDER, view_record

# Rows of the 137-joint SMPL-X skeleton in the multiview term: utils.smpl.smpl_to_openpose("smplx", use_hands=False, use_face=False,
# use_face_contour=False), the body rows only (tests/golden/depth_opt_golden.npz holds the reference's own copy).
BODY_INDICES = np.array([55, 12, 17, 19, 21, 16, 18, 20, 0, 2, 5, 8, 1, 4, 7, 56, 57, 58, 59, 60, 61, 62, 63, 64, 65], dtype=np.int64)
MAX_SHIFTS = 64


# ---- host mirrors ----
def convert_cam2real(verts, transl, cam_resolution, camera_data, convert_data):
    """Body-model output [.., 3] (camera space of the pose estimator) -> world space: translate, weak-perspective scaling to
    pixels around the principal point with the mean depth put at 500, pixels -> the orthographic camera's world scale, camera axes
    -> world (optimize_depth.py:79-101; the same pixel-to-world chain as initialize_depth.human_world).  Works in the dtype of
    `verts`; the input is not modified."""
    v = np.array(verts, copy=True)
    v = v + np.asarray(transl, dtype=v.dtype).reshape((1, 3))
    focals, princpt, z_mean = convert_data["focals"], convert_data["princpt"], convert_data["z_mean"]
    per_axis = (focals[0], focals[1], (focals[0] + focals[1]) / 2.0)
    for k in range(3):
        v[..., k] *= per_axis[k] / z_mean
    depth_shift = 500.0 - v[..., 2].mean()
    side, scale = max(cam_resolution), camera_data["scale"]
    offsets = (princpt[0], princpt[1], depth_shift)
    centre = (cam_resolution[0] / 2, cam_resolution[1] / 2, 0)
    for k in range(3):
        v[..., k] += offsets[k]
        v[..., k] = (v[..., k] - centre[k]) / side * scale
    to_world = (COMPATIBILITY_MATRIX_OPENGL_TO_BLENDER @ np.asarray(camera_data["R"], dtype=np.float64).T).astype(v.dtype)
    return v @ to_world + np.asarray(camera_data["t"], dtype=v.dtype).reshape((1, 3))


def camera_frame(verts, R):
    """p' = p R in f64: the camera-aligned frame, where the front vector R[:, 2] is +z."""
    return np.asarray(verts, dtype=np.float64) @ np.asarray(R, dtype=np.float64)


def inlier_views(inliers, indices=BODY_INDICES):
    """(views f64 [N,28], cand_view i32 [N], cand_xy f64 [N,J,2]) from the list compute_ransac_inclusives_with_triangulation returns:
    one view record per inlier, from the camera configuration the inlier carries."""
    def host(x):
        return x.detach().cpu().numpy() if torch.is_tensor(x) else x
    views, xy = [], []
    for item in inliers:
        cfg = item["camera_config"]
        views.append(view_record(dict(R=np.asarray(host(cfg["R"]), dtype=np.float64), t=np.asarray(host(cfg["t"]), dtype=np.float64),
                                      scale=float(host(cfg["scale"])), resolution=[float(r) for r in cfg["resolution"]])))
        xy.append(np.asarray(host(item["joints_proj"]), dtype=np.float64).reshape((-1, 2))[indices])
    J = len(indices)
    return (np.stack(views) if views else np.zeros((0, 28)), np.arange(len(views), dtype=np.int32),
            np.stack(xy) if xy else np.zeros((0, J, 2)))


# ---- device ----
class ShiftColumns:
    """A prepared shift workspace: the sorted column crossings of the human (A) and the asset (B) on one grid."""

    def __init__(self, ws, s, W, H, L_A, L_B, crossings):
        self.ws, self.s, self.W, self.H, self.L_A, self.L_B, self.crossings = ws, s, W, H, L_A, L_B, crossings

    @property
    def device(self):
        return self.ws.device


def prepare_columns(vertsA, facesA, vertsB, facesB, x0, y0, s, W, H, capacity=None, device="cuda"):
    """coma_shift_columns_prepare + coma_shift_columns_status: the meshes (already in the camera-aligned frame) -> ShiftColumns.
    capacity defaults to 8 crossings per column; when the device reports that more are needed the call is repeated ONCE with the
    reported count.  Raises ComaHipError on every other refusal."""
    L = _lib.lib()
    va, fa = _mesh(vertsA, facesA, device)
    vb, fb = _mesh(vertsB, facesB, device)
    dev = va.device
    lengths = torch.zeros([2], dtype=torch.int64, device=dev)
    capacity = int(capacity) if capacity is not None else max(1 << 16, 8 * W * H)
    for attempt in range(2):
        nbytes = L.coma_shift_columns_workspace_bytes(va.shape[0], fa.shape[0], vb.shape[0], fb.shape[0], W, H, capacity)
        ws = _scratch(nbytes, dev)
        needed = C.c_int64(0)
        with _lib.on_device(dev) as stream:
            rc = L.coma_shift_columns_prepare(_lib.ptr(va, torch.float64, "vertsA"), va.shape[0], _lib.ptr(fa, torch.int32, "facesA"), fa.shape[0],
                                              _lib.ptr(vb, torch.float64, "vertsB"), vb.shape[0], _lib.ptr(fb, torch.int32, "facesB"), fb.shape[0],
                                              float(x0), float(y0), float(s), W, H, capacity, _lib.ptr(ws), _lib.ptr(lengths), stream)
            if rc == 0:
                rc = L.coma_shift_columns_status(_lib.ptr(ws), stream, C.byref(needed))
        if rc != 0 and attempt == 0 and needed.value > capacity:
            capacity = needed.value
            continue
        _lib.check(rc, "coma_shift_columns_prepare")
        break
    la, lb = (int(x) for x in lengths.cpu().numpy())
    return ShiftColumns(ws, float(s), W, H, la, lb, int(needed.value))


def shift_profile(columns, d):
    """coma_shift_profile: displacements d [K] (world units, K <= 64) -> i64 [K,3] as NumPy, L_AB at Delta - 1, Delta, Delta + 1."""
    dev = columns.device
    dd = torch.as_tensor(np.ascontiguousarray(np.asarray(d, dtype=np.float64).reshape(-1)), device=dev)
    K = int(dd.numel())
    out = torch.zeros([K, 3], dtype=torch.int64, device=dev)
    with _lib.on_device(dev) as stream:
        rc = _lib.lib().coma_shift_profile(_lib.ptr(columns.ws), _lib.ptr(dd, torch.float64, "d"), K, _lib.ptr(out), stream)
    _lib.check(rc, "coma_shift_profile")
    return out.cpu().numpy()


def optimize_displacement(columns, views, joints0, front, cand_view, cand_xy, d0=0.0, lr=0.01, w_multiview=1e-3, w_collision=0.4,
                          num_epoch=200, device="cuda"):
    """coma_depth_optimize_f64: Adam on d for num_epoch epochs -> dict(d, traj f64 [E+1], Ltraj i64 [E,3], losses f64 [E,2]) as NumPy.
    columns: a ShiftColumns, or None for no collision term.  views [n_views,28] (triangulate.view_record), joints0 [J,3] the joints
    at d = 0, front [3], cand_view [N] the view of each inlier, cand_xy [N,J,2] its pixel joints.  Raises ComaHipError when d stops
    being finite."""
    L = _lib.lib()
    dev = columns.device if columns is not None else torch.device(device)
    f64 = torch.float64

    def dev_f64(x):
        return torch.as_tensor(np.ascontiguousarray(np.asarray(x, dtype=np.float64)), device=dev)
    v, j0, cxy = dev_f64(views).reshape(-1, 28), dev_f64(joints0).reshape(-1, 3), dev_f64(cand_xy)
    cv = torch.as_tensor(np.ascontiguousarray(np.asarray(cand_view, dtype=np.int32)), device=dev)
    N, J, E = int(cv.numel()), int(j0.shape[0]), int(num_epoch)
    assert cxy.numel() == N * J * 2 and (N == 0 or (int(cv.min()) >= 0 and int(cv.max()) < v.shape[0]))
    traj = torch.full([max(E, 0) + 1], float("nan"), dtype=f64, device=dev)
    Ltraj = torch.zeros([max(E, 1), 3], dtype=torch.int64, device=dev)
    losses = torch.zeros([max(E, 1), 2], dtype=f64, device=dev)
    state = torch.zeros([max(1, int(L.coma_depth_optimize_state_bytes()) // 8)], dtype=torch.int64, device=dev)
    fr = (C.c_double * 3)(*(float(x) for x in np.asarray(front, dtype=np.float64).reshape(3)))
    epoch = C.c_int(0)
    with _lib.on_device(dev) as stream:
        rc = L.coma_depth_optimize_f64(_lib.ptr(columns.ws) if columns is not None else None, _lib.ptr(v, f64, "views") if N else None,
                                       int(v.shape[0]), _lib.ptr(j0, f64, "joints0") if N else None, fr, _lib.ptr(cv, torch.int32) if N else None,
                                       _lib.ptr(cxy, f64, "cand_xy") if N else None, N, J, float(d0), float(lr), float(w_multiview),
                                       float(w_collision), E, _lib.ptr(traj), _lib.ptr(Ltraj), _lib.ptr(losses), _lib.ptr(state), stream)
        if rc == 0:
            rc = L.coma_depth_optimize_status(_lib.ptr(state), stream, C.byref(epoch))
    _lib.check(rc, "coma_depth_optimize_f64")
    traj_h = traj.cpu().numpy()
    return dict(d=float(traj_h[-1]), traj=traj_h, Ltraj=Ltraj.cpu().numpy(), losses=losses.cpu().numpy())


def optimize_displacement_coap(coap, points, views, joints0, front, cand_view, cand_xy, d0=0.0, lr=0.01, w_multiview=1e-3, w_collision=0.4,
                               num_epoch=200, filter_threshold=0.01):
    """coma_depth_optimize_coap_f64: optimize_displacement with COAP's collision term (coma_amd.coap.DeviceCOAP, a body already
    encoded at d = 0) over the scene points [T,3] in place of the column profile -> dict(d, traj f64 [E+1], Ctraj f64 [E,2] = {COAP
    loss, d loss / d d} at traj[e], losses f64 [E,2] = {multiview loss, COAP loss}) as NumPy.  points None or empty: no collision
    term.  Every epoch filters the points as the reference's sample_scene_points does (the posed vertices' box, occupancy above
    filter_threshold); where it keeps a random 10 000 of more survivors, here all count."""
    L = _lib.lib()
    f64 = torch.float64
    if coap is not None and coap.code is None:
        raise _lib.ComaHipError("optimize_displacement_coap: the DeviceCOAP holds no encoded body")
    dev = coap.code.device if coap is not None else torch.device("cuda", torch.cuda.current_device())

    def dev_f64(x):
        return torch.as_tensor(np.ascontiguousarray(np.asarray(x, dtype=np.float64)), device=dev)
    v, j0, cxy = dev_f64(views).reshape(-1, 28), dev_f64(joints0).reshape(-1, 3), dev_f64(cand_xy)
    cv = torch.as_tensor(np.ascontiguousarray(np.asarray(cand_view, dtype=np.int32)), device=dev)
    N, J, E = int(cv.numel()), int(j0.shape[0]), int(num_epoch)
    assert cxy.numel() == N * J * 2 and (N == 0 or (int(cv.min()) >= 0 and int(cv.max()) < v.shape[0]))
    p = None if points is None or coap is None else coap._f32(points, [-1, 3])
    T = 0 if p is None else int(p.shape[0])
    w_collision = float(w_collision) if T else 0.0
    traj = torch.full([max(E, 0) + 1], float("nan"), dtype=f64, device=dev)
    Ctraj = torch.zeros([max(E, 1), 2], dtype=f64, device=dev)
    losses = torch.zeros([max(E, 1), 2], dtype=f64, device=dev)
    state = torch.zeros([max(1, int(L.coma_depth_optimize_state_bytes()) // 8)], dtype=torch.int64, device=dev)
    fr = (C.c_double * 3)(*(float(x) for x in np.asarray(front, dtype=np.float64).reshape(3)))
    ws = coap._scratch("query", L.coma_coap_query_workspace_bytes(coap.K, T)) if T else None
    epoch = C.c_int(0)
    with _lib.on_device(dev) as stream:
        rc = L.coma_depth_optimize_coap_f64(_lib.ptr(coap.weights) if T else None, coap.weights.numel() if T else 0, _lib.ptr(coap.code) if T else None,
                                            coap.K if T else 0, _lib.ptr(p) if T else None, T, float(filter_threshold), _lib.ptr(ws) if T else None,
                                            ws.numel() if T else 0, _lib.ptr(v, f64, "views") if N else None, int(v.shape[0]),
                                            _lib.ptr(j0, f64, "joints0") if N else None, fr, _lib.ptr(cv, torch.int32) if N else None,
                                            _lib.ptr(cxy, f64, "cand_xy") if N else None, N, J, float(d0), float(lr), float(w_multiview), w_collision, E,
                                            _lib.ptr(traj), _lib.ptr(Ctraj), _lib.ptr(losses), _lib.ptr(state), stream)
        if rc == 0:
            rc = L.coma_depth_optimize_status(_lib.ptr(state), stream, C.byref(epoch))
    _lib.check(rc, "coma_depth_optimize_coap_f64")
    traj_h = traj.cpu().numpy()
    return dict(d=float(traj_h[-1]), traj=traj_h, Ctraj=Ctraj.cpu().numpy(), losses=losses.cpu().numpy())


def collision_columns(human_verts, human_faces, asset_verts, asset_faces, R, resolution=512, device="cuda"):
    """The collision term's columns for world-space meshes and the camera rotation R: both meshes into the camera-aligned frame, the
    grid over the xy overlap of their bounding boxes, the sorted crossings.  None (the term is 0, nothing is launched) when the boxes
    are disjoint in x or y."""
    a, b = camera_frame(human_verts, R), camera_frame(asset_verts, R)
    grid = overlap_grid_xy(a, b, resolution)
    if grid is None:
        return None
    return prepare_columns(a, human_faces, b, asset_faces, *grid, device=device)
