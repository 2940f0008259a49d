"""Depth initialisation (the reference's src/generation/initialize_depth.py) without Blender: the host arithmetic in f64 NumPy
and the silhouette test on the device.

The reference pushes 2 * retrieval_range + 1 copies of the fitted human along the viewing axis of an ORTHOGRAPHIC camera, renders
an instance-segmentation map of {asset, copy} with Blender for each, and keeps the copy whose visible pixels have the best IoU
with the person mask of the inpainted picture (:134-201).  All copies share one screen footprint -- only their occlusion by the
asset changes -- so here the human and the asset are drawn ONCE each (coma_raster_depth_f64: orthographic nearest-depth maps)
and one compare-and-count pass (coma_silhouette_iou) answers every copy from its depth offset.

Blender's own render is UNPINNED (bpy is not available to this project): its coverage rule at a pixel centre, its behaviour for
coincident surfaces and its clip planes are third party.  What is pinned is the rule set stated in include/coma_hip.h, restated
in tests/raster_ref.py; the reference's own Python around the render is pinned by tests/golden/depth_init_golden.npz.

Deviation from the reference's signatures: the asset arrives as world-space arrays (asset_verts, asset_faces) -- the reference
reads it from the live Blender scene.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib

EMPTY_KEY = -1          # the all-ones u64 key, seen through the int64 tensors the keys are stored in


# ---- host mirrors (f64 NumPy, the reference's expressions) ----
def compute_directional_size(mesh_verts, direction):
    """Extent of the mesh along `direction` (initialize_depth.py:31-38)."""
    direction = direction / np.linalg.norm(direction)
    proj = np.dot(mesh_verts, direction)
    return np.max(proj) - np.min(proj)


def compute_nearest_point(asset_verts, point, direction):
    """The asset vertex closest to the line through `point` along `direction`, as (foot of `point` on that vertex's plane [3,1],
    signed distance from `point` to it along `direction`) (initialize_depth.py:41-62)."""
    direction = (direction / np.linalg.norm(direction)).reshape((1, 3))
    point = point.copy().reshape((1, 3))
    column = direction.reshape((3, 1))
    disp = point - asset_verts
    perpendicular = disp - (disp @ column) * direction
    nearest = asset_verts[np.argmin(np.linalg.norm(perpendicular, axis=1))]
    disp = point - nearest
    along = disp @ column
    return (point - along * direction).reshape((3, 1)), -float(along[0, 0])


def candidate_displacements(distance_from_point, retrieval_interval, retrieval_range):
    """2 * retrieval_range + 1 displacements centred on the asset's depth (initialize_depth.py:355)."""
    return [distance_from_point + (index - retrieval_range) * retrieval_interval for index in range(retrieval_range * 2 + 1)]


def extract_candidates(human_verts, human_faces, asset_verts, asset_faces, displacements, direction, kernel_size=9, max_collisions=1000,
                       filter_out=False):
    """One shifted copy of the human per displacement (initialize_depth.py:92-131, filter_out=False).  The collision-filtered branch
    is dead code in the reference (nothing passes filter_out=True and its BVH import is missing)."""
    if filter_out:
        raise NotImplementedError("extract_candidates(filter_out=True): the reference never takes this branch (its BVH is not imported)")
    direction = direction.reshape((1, 3))
    return [dict(verts=human_verts + d * direction, faces=human_faces, displacement=d * direction) for d in displacements]


def person_mask(segmentation_human_gt):
    """The reference's `(np.array(Image.fromarray(m).convert("L")) / 255).astype(np.uint8)`: a boolean mask as it is, an 8-bit one
    only where it is 255."""
    m = np.asarray(segmentation_human_gt)
    if m.dtype == np.bool_:
        return m.astype(np.uint8)
    return (m.astype(np.float64) / 255).astype(np.uint8)


# ---- device ----
def _camera(camera_data, resolution=None):
    R = np.ascontiguousarray(np.asarray(camera_data["R"], dtype=np.float64).reshape(3, 3))
    t = np.ascontiguousarray(np.asarray(camera_data["t"], dtype=np.float64).reshape(3))
    W, H = (int(x) for x in (resolution if resolution is not None else camera_data["resolution"]))
    return R, t, float(camera_data["scale"]), W, H


def raster_depth(verts, faces, camera_data, device="cuda", resolution=None):
    """coma_raster_depth_f64: the orthographic nearest-depth key map of one world-space mesh, an int64 tensor [H,W] on the device
    holding the u64 keys (empty = -1).  Raises ComaHipError when the call is refused (non-finite vertex, coordinate beyond 2^25
    sub-pixel units, face index out of range): this wrapper is where the status word is read, so it waits for the stream."""
    L = _lib.lib()
    R, t, scale, W, H = _camera(camera_data, resolution)
    v = torch.as_tensor(np.ascontiguousarray(np.asarray(verts, dtype=np.float64)), device=device) if not torch.is_tensor(verts) else verts
    f = torch.as_tensor(np.ascontiguousarray(np.asarray(faces).astype(np.int32)), device=device) if not torch.is_tensor(faces) else faces
    assert v.dim() == 2 and v.shape[1] == 3 and f.dim() == 2 and f.shape[1] == 3
    ws = torch.empty([max(1, (int(L.coma_raster_workspace_bytes(v.shape[0], f.shape[0])) + 15) // 16), 2], dtype=torch.int64, device=v.device)
    key = torch.empty([H, W], dtype=torch.int64, device=v.device)
    dp = C.POINTER(C.c_double)
    with _lib.on_device(v.device) as stream:
        rc = L.coma_raster_depth_f64(_lib.ptr(v, torch.float64, "verts"), v.shape[0], _lib.ptr(f, torch.int32, "faces"), f.shape[0],
                                     R.ctypes.data_as(dp), t.ctypes.data_as(dp), scale, W, H, _lib.ptr(ws), _lib.ptr(key), stream)
        if rc == 0:
            rc = L.coma_raster_status(_lib.ptr(ws), stream)
    _lib.check(rc, "coma_raster_depth_f64")
    return key


def silhouette_counts(human_key, asset_key, offsets, gt, want_masks=True):
    """coma_silhouette_iou: (visible, inter, uni) as NumPy i64 [K] and masks u8 [K,H,W] (NumPy, or None)."""
    L = _lib.lib()
    dev = human_key.device
    H, W = human_key.shape
    off = torch.as_tensor(np.ascontiguousarray(np.asarray(offsets, dtype=np.float64).reshape(-1)), device=dev)
    K = off.shape[0]
    g = torch.as_tensor(np.ascontiguousarray(np.asarray(gt, dtype=np.uint8)), device=dev)
    assert g.shape == (H, W) and (asset_key is None or asset_key.shape == (H, W))
    counts = torch.empty([3, max(1, K)], dtype=torch.int64, device=dev)
    masks = torch.empty([K, H, W], dtype=torch.uint8, device=dev) if want_masks else None
    with _lib.on_device(dev) as stream:
        rc = L.coma_silhouette_iou(_lib.ptr(human_key, torch.int64), _lib.ptr(asset_key, torch.int64), _lib.ptr(off), K, _lib.ptr(g), W, H,
                                   _lib.ptr(counts[0]), _lib.ptr(counts[1]), _lib.ptr(counts[2]), _lib.ptr(masks), stream)
    _lib.check(rc, "coma_silhouette_iou")
    c = counts.cpu().numpy()
    return c[0], c[1], c[2], (masks.cpu().numpy() if want_masks else None)


def _asset_key(asset_verts, asset_faces, camera_data, device):
    if asset_verts is None or asset_faces is None or len(asset_faces) == 0:
        return None
    return raster_depth(asset_verts, asset_faces, camera_data, device)


def render_human_segmap(human_verts, human_faces, asset_verts, asset_faces, camera_data, device="cuda"):
    """The human's visible pixels in front of the asset, u8 [H,W] 0 / 255, or None when there is none
    (compute_metrics.py:39-82 up to the 255 -> 1 conversion, initialize_depth.py:159-170)."""
    hk = raster_depth(human_verts, human_faces, camera_data, device)
    vis, _, _, masks = silhouette_counts(hk, _asset_key(asset_verts, asset_faces, camera_data, device), [0.0],
                                         np.zeros(tuple(hk.shape), dtype=np.uint8))
    return masks[0] if int(vis[0]) > 0 else None


def compute_IoU(segmentation_human_gt, human_verts, human_faces, asset_verts, asset_faces, camera_data, device="cuda"):
    """IoU of the rendered human with the person mask; 0.0 when the human is invisible (compute_metrics.py:101-112)."""
    hk = raster_depth(human_verts, human_faces, camera_data, device)
    vis, inter, uni, _ = silhouette_counts(hk, _asset_key(asset_verts, asset_faces, camera_data, device), [0.0],
                                           person_mask(segmentation_human_gt), want_masks=False)
    return int(inter[0]) / int(uni[0]) if int(vis[0]) > 0 else 0.0


def depth_offsets(candidate_lists, camera_data):
    """Depth of candidate k minus depth of candidate 0: the projection of the difference of their displacements onto the camera's
    depth axis, c.z = -(R[:,2] . (p - t))."""
    R = np.asarray(camera_data["R"], dtype=np.float64).reshape(3, 3)
    d0 = np.asarray(candidate_lists[0]["displacement"], dtype=np.float64).reshape(3)
    out = []
    for c in candidate_lists:
        d = np.asarray(c["displacement"], dtype=np.float64).reshape(3) - d0
        out.append(-((R[0, 2] * d[0] + R[1, 2] * d[1]) + R[2, 2] * d[2]))
    return np.array(out, dtype=np.float64)


def choose(candidates):
    """The reference's selection (initialize_depth.py:197-201): best IoU, then the smallest interval_from_center; `max` keeps the
    first maximal element.  None for an empty list."""
    if len(candidates) == 0:
        return None
    return max(candidates, key=lambda c: (c["IoU"], -c["interval_from_center"]))


def select_human(candidate_lists, camera_data, segmentation_human_gt, asset_verts, asset_faces, device="cuda"):
    """initialize_depth.py:134-201.  The first candidate and the asset are drawn once; every candidate is that footprint at its own
    depth offset.  Candidates without a visible pixel are skipped; None when none is visible."""
    if len(candidate_lists) == 0:
        return None
    hk = raster_depth(candidate_lists[0]["verts"], candidate_lists[0]["faces"], camera_data, device)
    ak = _asset_key(asset_verts, asset_faces, camera_data, device)
    vis, inter, uni, masks = silhouette_counts(hk, ak, depth_offsets(candidate_lists, camera_data), person_mask(segmentation_human_gt))
    candidates = []
    for idx, candidate in enumerate(candidate_lists):
        if int(vis[idx]) == 0:
            continue
        candidates.append(dict(idx=idx, verts=candidate["verts"], faces=candidate["faces"], IoU=int(inter[idx]) / int(uni[idx]),
                               human_segmentation=masks[idx],
                               # len, not len // 2: every interval is counted from PAST the last candidate (the reference's quirk)
                               interval_from_center=np.abs(idx - len(candidate_lists)), displacement=candidate["displacement"]))
    return choose(candidates)
