"""The two metrics of the reference's src/generation/compute_metrics.py without Blender or trimesh: the intersection-volume ratio
on the device, next to the IoU that coma_amd.depth_init already has, and the host arithmetic around them in f64 NumPy.

The reference forms `interscetion_ratio = |volume(human ∩ asset) / volume(human)|` with a Blender boolean through trimesh
(:86-99).  Here the intersection volume is counted by columns (coma_intersection_columns: every crossing of a grid cell's column
with either surface, one sweep per column; rule set in include/coma_hip.h, restated in tests/volume_ref.py) and the denominator is
the signed volume of the human mesh (coma_mesh_volume_f64, the sum trimesh's `volume` forms).

Blender's boolean is UNPINNED (neither bpy nor trimesh is available to this project).  The column rule set measures a volume for
closed, consistently oriented meshes; for an open mesh the number is deterministic but it is not a volume -- trimesh's boolean
does not define one for such a mesh either.

Deviation from the reference's signatures: `compute_metrics` takes the person mask and the world-space asset arrays (the reference
reads the mask from a pickle path and the asset from the live Blender scene); `get_asset_info` takes the directory the dataset
folders live in.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib

TRIMESH_P3D_TO_BLENDER = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, -1.0, 0.0]])     # constants/generation/visualizers.py
FLOOR_SHIFTED = ("SHAPENET", "SKETCHFAB", "INTERCAP", "BEHAVE")                                # compute_metrics.py:164
ASSET_INFO = dict()


# ---- host mirrors (f64 NumPy, the reference's expressions) ----
def asset_transform(obj_verts, camera_data, dataset_type):
    """(world-space asset vertices, z_min) from the OBJ file's vertices: PyTorch3D axes -> Blender axes, the object's pose of this view,
    and for the floor-shifted datasets the lowest point (taken BEFORE the pose) put back on z = 0.  Same operations in the same
    order as compute_metrics.py:154-165, so the result is bit-identical."""
    upright = np.array(obj_verts) @ TRIMESH_P3D_TO_BLENDER
    z_min = upright[:, 2].min()
    world = upright @ camera_data["obj_R"].T + camera_data["obj_t"].reshape((1, 3))
    if dataset_type in FLOOR_SHIFTED:
        world -= [0.0, 0.0, z_min]
    return world, z_min


def get_asset_info(supercategory, category, asset_id, view_id, camera_data, disable_lowres_switch_for_behave, asset_obj_root="data"):
    """dict(verts, faces, z_min) of one (asset, view), cached like the reference's ASSET_INFO (compute_metrics.py:122-169).  The mesh
    is read by the project's OBJ reader where the reference calls trimesh.load(process=False) [3rd-party, unpinned: trimesh may
    split a vertex that carries several texture coordinates; the surface, and with it both metrics, is the same]."""
    key = (supercategory, category, asset_id, view_id)
    if key not in ASSET_INFO:
        from constants.generation.assets import CATEGORY2DATASET_TYPE
        from src.generation.initialize_depth import asset_obj_path
        from .downsample import load_obj
        dataset_type = CATEGORY2DATASET_TYPE[key[:2]]
        if dataset_type not in ("3D-FUTURE", "SHAPENET", "SKETCHFAB", "BEHAVE", "INTERCAP"):
            raise NotImplementedError(dataset_type)                 # the reference's metrics stage knows these five (:125-150)
        obj_verts, obj_faces = load_obj(asset_obj_path(asset_obj_root, supercategory, category, asset_id, disable_lowres_switch_for_behave))
        world, z_min = asset_transform(obj_verts, camera_data, dataset_type)
        ASSET_INFO[key] = dict(verts=world, faces=np.array(obj_faces), z_min=z_min)
    return ASSET_INFO[key]


def to_object_frame(human_verts, z_min, camera_data):
    """World-space human vertices -> the object-canonical (trimesh / PyTorch3D) frame the sample pickles store: undo the floor shift
    and the object's pose, then go back from Blender axes to PyTorch3D axes.  The floor offset is subtracted in Blender axes and added
    again in PyTorch3D axes, as compute_metrics.py:240-241 does; operations in that order, so the result is bit-identical."""
    lift = np.array([0.0, 0.0, z_min])
    back_to_p3d = TRIMESH_P3D_TO_BLENDER.T
    posed = human_verts + lift - camera_data["obj_t"].reshape((1, 3))
    canonical = posed @ camera_data["obj_R"] - lift
    return canonical @ back_to_p3d + lift @ back_to_p3d


def parallel_slice(n_items, parallel_num, parallel_idx):
    """(start, end) of one process's share of the sorted work list: shares of n // parallel_num + 1 items, the last ones possibly
    empty (compute_metrics.py:200-202)."""
    share = n_items // parallel_num + 1
    return share * parallel_idx, share * (parallel_idx + 1)


MAX_REACH_CELLS = 65536.0        # half of the 2^25 / 256 = 131 072 cells the device lets a vertex lie from the grid origin


def _overlap_grid(vertsA, vertsB, resolution, axes):
    """The grid over the xy overlap of the two bounding boxes; None when the boxes are disjoint (or only touch) on one of `axes`."""
    a, b = np.asarray(vertsA, dtype=np.float64), np.asarray(vertsB, dtype=np.float64)
    lo, hi = np.maximum(a.min(axis=0), b.min(axis=0)), np.minimum(a.max(axis=0), b.max(axis=0))
    if not (hi[:axes] > lo[:axes]).all():
        return None
    ex, ey = float(hi[0] - lo[0]), float(hi[1] - lo[1])
    reach = max(float(np.abs(m[:, :2] - lo[:2]).max()) for m in (a, b))
    s = min(resolution / max(ex, ey), MAX_REACH_CELLS / reach)
    W, H = max(1, math.ceil(ex * s)), max(1, math.ceil(ey * s))
    return float(lo[0]), float(lo[1]), float(s), int(min(W, resolution)), int(min(H, resolution))


def overlap_grid(vertsA, vertsB, resolution):
    """The grid laid over the xy overlap of the two bounding boxes: (x0, y0, s, W, H) with `resolution` square cells along the
    longer side and ceil(shorter side in those cells) along the other, or None when the boxes are disjoint (or only touch) on any
    axis, z included.
    Every vertex of BOTH meshes is snapped relative to (x0, y0), and the device refuses a coordinate beyond 2^25 sub-cell units, so
    the cells may not be arbitrarily small against the meshes: s is capped at MAX_REACH_CELLS / (largest |x - x0|, |y - y0| of any
    vertex).  The cap binds only when the overlap is thinner than resolution / 65536 of the meshes' extent (two boxes that graze);
    the grid then has fewer than `resolution` cells, each still under 1 / 65536 of that extent."""
    return _overlap_grid(vertsA, vertsB, resolution, 3)


def overlap_grid_xy(vertsA, vertsB, resolution):
    """overlap_grid() for a mesh A that slides along z (the depth optimisation, coma_amd/depth_opt.py): the same grid and the same cap
    on the scale, but only x and y decide whether the boxes meet; the z extent does not enter, because the footprint of A never
    changes while its depth does.  None when the boxes are disjoint (or only touch) in x or y."""
    return _overlap_grid(vertsA, vertsB, resolution, 2)


# ---- device ----
def _mesh(verts, faces, device):
    v = torch.as_tensor(np.ascontiguousarray(np.asarray(verts, dtype=np.float64)), device=device) if not torch.is_tensor(verts) else verts
    f = torch.as_tensor(np.ascontiguousarray(np.asarray(faces).astype(np.int32)), device=device) if not torch.is_tensor(faces) else faces
    assert v.dim() == 2 and v.shape[1] == 3 and f.dim() == 2 and f.shape[1] == 3
    return v, f


def _scratch(nbytes, device):
    return torch.empty([max(1, (int(nbytes) + 15) // 16), 2], dtype=torch.int64, device=device)


def mesh_volume(verts, faces, device="cuda"):
    """coma_mesh_volume_f64: the signed volume, sum of det[a b c] / 6 (positive for outward-facing triangles)."""
    L = _lib.lib()
    v, f = _mesh(verts, faces, device)
    out = torch.empty([1], dtype=torch.float64, device=v.device)
    ws = _scratch(L.coma_mesh_volume_workspace_bytes(f.shape[0]), v.device)
    with _lib.on_device(v.device) as stream:
        rc = L.coma_mesh_volume_f64(_lib.ptr(v, torch.float64, "verts"), v.shape[0], _lib.ptr(f, torch.int32, "faces"), f.shape[0], _lib.ptr(out),
                                    _lib.ptr(ws), stream)
    _lib.check(rc, "coma_mesh_volume_f64")
    return float(out.item())


def intersection_columns(vertsA, facesA, vertsB, facesB, x0, y0, s, W, H, capacity=None, want_columns=False, device="cuda"):
    """coma_intersection_columns + coma_intersection_status on one grid: (sums i64 [3] = L_AB, L_A, L_B as NumPy, col_ab i64 [H,W] as
    NumPy or None).  capacity (crossings of A plus B the workspace holds) defaults to 8 per column; when the device reports that more
    are needed the call is repeated ONCE with the reported count.  Raises ComaHipError on every other refusal."""
    L = _lib.lib()
    va, fa = _mesh(vertsA, facesA, device)
    vb, fb = _mesh(vertsB, facesB, device)
    dev = va.device
    sums = torch.zeros([3], dtype=torch.int64, device=dev)
    col = torch.zeros([H, W], dtype=torch.int64, device=dev) if want_columns else None
    capacity = int(capacity) if capacity is not None else max(1 << 16, 8 * W * H)
    for attempt in range(2):
        nbytes = L.coma_column_crossings_workspace_bytes(va.shape[0], fa.shape[0], vb.shape[0], fb.shape[0], W, H, capacity)
        ws = _scratch(nbytes, dev)
        needed = C.c_int64(0)
        with _lib.on_device(dev) as stream:
            rc = L.coma_intersection_columns(_lib.ptr(va, torch.float64, "vertsA"), va.shape[0], _lib.ptr(fa, torch.int32, "facesA"), fa.shape[0],
                                             _lib.ptr(vb, torch.float64, "vertsB"), vb.shape[0], _lib.ptr(fb, torch.int32, "facesB"), fb.shape[0],
                                             float(x0), float(y0), float(s), W, H, capacity, _lib.ptr(ws), _lib.ptr(sums), _lib.ptr(col), stream)
            if rc == 0:
                rc = L.coma_intersection_status(_lib.ptr(ws), stream, C.byref(needed))
        if rc != 0 and attempt == 0 and needed.value > capacity:
            capacity = needed.value
            continue
        _lib.check(rc, "coma_intersection_columns")
        break
    return sums.cpu().numpy(), (col.cpu().numpy() if want_columns else None)


def intersection_volume(vertsA, facesA, vertsB, facesB, resolution=512, device="cuda"):
    """Volume of A ∩ B in world units: L_AB / (256 s^3) on the grid of overlap_grid(); 0.0 without a launch when the bounding boxes
    are disjoint on any axis."""
    grid = overlap_grid(vertsA, vertsB, resolution)
    if grid is None:
        return 0.0
    x0, y0, s, W, H = grid
    sums, _ = intersection_columns(vertsA, facesA, vertsB, facesB, x0, y0, s, W, H, device=device)
    return float(int(sums[0])) / (256.0 * s * s * s)


def compute_instersection_ratio(vertsA, facesA, vertsB, facesB, resolution=512, device="cuda"):
    """|volume(A ∩ B) / volume(A)| (compute_metrics.py:86-99; the name is the reference's)."""
    return np.abs(intersection_volume(vertsA, facesA, vertsB, facesB, resolution, device) / mesh_volume(vertsA, facesA, device))


def compute_metrics(camera_data, segmentation_human_gt, human_verts, human_faces, asset_verts, asset_faces, volume_resolution=512, device="cuda"):
    """dict(interscetion_ratio, IoU) of one sample (compute_metrics.py:85-119; the key is the reference's spelling)."""
    from .depth_init import compute_IoU
    interscetion_ratio = compute_instersection_ratio(human_verts, human_faces, asset_verts, asset_faces, volume_resolution, device)
    IoU = compute_IoU(segmentation_human_gt, human_verts, human_faces, asset_verts, asset_faces, camera_data, device)
    return dict(interscetion_ratio=interscetion_ratio, IoU=IoU)
