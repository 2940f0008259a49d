"""The optimisation app's ComA objective on MI355X: the part of the reference's src/application/optimize.py that is ComA's own.

The app fits a posed body mesh to an object under two terms read off a learned ComA state (optimize.py:274-296): an orientation
term -- the vertex normals of the posed mesh, canonicalised against one object normal, compared with each vertex's most likely
orientation bin -- and a contact term, the chamfer distance between the selected human vertices and their most-contacted object
points.  `ComaObjective` evaluates both terms and their gradients with respect to the vertices in one device pass
(coma_amd/csrc/app_objective.hip; rule set in include/coma_hip.h, restated in tests/app_ref.py); `.loss` wraps that in a
torch.autograd.Function so that a caller's body model (SMPL-X, VPoser: third party, hooks of src/application/optimize.py) keeps
differentiating from the vertices on.  There is no CPU fallback.
"""
from __future__ import annotations

import pickle

import numpy as np
import torch

from . import _lib
from .ingest import vertex_face_csr


def _host_f32(x, shape, name):
    a = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    a = np.ascontiguousarray(a, dtype=np.float32)
    try:
        return a.reshape(shape)
    except ValueError:
        raise ValueError(f"{name}: expected shape {shape}, got {a.shape}") from None


def _host_index(x, name):
    if isinstance(x, tuple):                       # np.nonzero's return value, as optimize.py:195 keeps it
        if len(x) != 1:
            raise ValueError(f"{name}: expected one index array, got a tuple of {len(x)}")
        x = x[0]
    a = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise TypeError(f"{name}: expected integers, got {a.dtype}")
    return np.ascontiguousarray(a.reshape(-1), dtype=np.int64)


def state_targets(affordance_info, asset_downsample, reference_object_vertex_index, contact_threshold, device="cuda", select=None):
    """What the objective needs of a learned state and of the asset's down-sampling pickle (paths or the dicts they hold):
    (relative_orientation_GT [V,3], the reference object point's normal [3], selected_human_indices i64 [k], target points [k,3] =
    obj_verts[corresponding_object_indices], duplicates kept).  `select` is the target selection, by default the device's
    consumer.orientation_and_contact_targets."""
    if select is None:
        from .consumer import orientation_and_contact_targets
        select = lambda info, o_ref, thr: orientation_and_contact_targets(info, o_ref, thr, device)
    if isinstance(affordance_info, (str, bytes)):
        with open(affordance_info, "rb") as handle:
            affordance_info = pickle.load(handle)
    if isinstance(asset_downsample, (str, bytes)):
        with open(asset_downsample, "rb") as handle:
            asset_downsample = pickle.load(handle)
    obj_verts = np.asarray(asset_downsample["downsampled_pcd_points_raw"]).reshape(-1, 3)
    obj_normals = np.asarray(asset_downsample["downsampled_pcd_normal_raw"]).reshape(-1, 3)
    _, gt, selected, objects = select(affordance_info, reference_object_vertex_index, contact_threshold)
    return np.asarray(gt), obj_normals[reference_object_vertex_index], np.asarray(selected[0]), obj_verts[np.asarray(objects)]


class ComaObjective:
    """The constants of one fit, uploaded once: topology (faces + vertex->face CSR table), the per-vertex orientation targets, one
    object normal, the selected human vertices and their target points."""

    def __init__(self, faces, relative_orientation_GT, obj_normal, selected_human_indices, target_points, principle_vec=(0, 0, 1),
                 sub_principle_vec=(0, 1, 0), eps=1e-6, device="cuda"):
        gt = _host_f32(relative_orientation_GT, (-1, 3), "relative_orientation_GT")
        V = int(gt.shape[0])
        faces = _host_index(faces, "faces").reshape(-1, 3)
        F = int(faces.shape[0])
        if V <= 0 or F <= 0:
            raise ValueError(f"ComaObjective: V = {V}, F = {F}; both must be positive")
        if faces.min() < 0 or faces.max() >= V:
            raise IndexError(f"faces: indices must lie in [0, {V}), got [{faces.min()}, {faces.max()}]")
        sel = _host_index(selected_human_indices, "selected_human_indices")
        k = int(sel.size)
        if k and (sel.min() < 0 or sel.max() >= V):
            raise IndexError(f"selected_human_indices: indices must lie in [0, {V}), got [{sel.min()}, {sel.max()}]")
        if np.unique(sel).size != k:
            raise ValueError("selected_human_indices: entries must be distinct (np.nonzero gives them so)")
        tgt = _host_f32(target_points, (-1, 3), "target_points")
        if tgt.shape[0] != k:
            raise ValueError(f"target_points: {tgt.shape[0]} rows for {k} selected vertices")
        dev = _lib.need_device(device, "ComaObjective")
        off, vf = vertex_face_csr(faces, V)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.V, self.F, self.k, self.eps = V, F, k, float(eps)
        self.faces, self.vf_offsets, self.vf_faces = up(faces.astype(np.int32)), up(off), up(vf)
        self.orientation_gt = up(gt)
        self.selected = up(sel.astype(np.int32)) if k else None
        self.targets = up(tgt) if k else None
        self._b = _lib.vec3(_host_f32(obj_normal, (3,), "obj_normal"))
        self._p = _lib.vec3(_host_f32(principle_vec, (3,), "principle_vec"))
        self._s = _lib.vec3(_host_f32(sub_principle_vec, (3,), "sub_principle_vec"))
        nbytes = int(_lib.lib().coma_app_objective_workspace_bytes(V, F, k))
        self._ws = torch.empty([max(16, nbytes)], dtype=torch.uint8, device=dev)
        self._ws_bytes = nbytes
        self.device = dev

    @classmethod
    def from_state(cls, affordance_info, asset_downsample, faces, reference_object_vertex_index, contact_threshold,
                   principle_vec=(0, 0, 1), sub_principle_vec=(0, 1, 0), eps=1e-6, device="cuda"):
        """From a learned state (the dict ComA.export pickles, or its path) and the asset's down-sampling pickle (dict or path):
        target selection through consumer.orientation_and_contact_targets (optimize.py:190-196), the object's points and normals
        from `downsampled_pcd_points_raw` / `downsampled_pcd_normal_raw` (:215-216)."""
        gt, obj_normal, selected, target_points = state_targets(affordance_info, asset_downsample, reference_object_vertex_index,
                                                                contact_threshold, device)
        return cls(faces, gt, obj_normal, selected, target_points, principle_vec, sub_principle_vec, eps, device)

    def _vertices(self, vertices):
        v = vertices
        if v.dim() == 3 and v.shape[0] == 1:
            v = v[0]
        if v.dim() != 2 or tuple(v.shape) != (self.V, 3):
            raise ValueError(f"vertices: expected [{self.V},3] or [1,{self.V},3], got {tuple(vertices.shape)}")
        if not v.is_cuda or v.device != self.device:
            raise _lib.ComaHipError(f"vertices must live on {self.device} (got {v.device}); there is no CPU path")
        return v.detach().to(torch.float32).contiguous()

    def evaluate(self, vertices):
        """vertices [V,3] or [1,V,3] on the device -> (terms f32 [2] = {orientation, contact} unweighted, grad_orientation f32 [V,3],
        grad_contact f32 [V,3]), device tensors; nothing waits for the device."""
        v = self._vertices(vertices)
        terms = torch.empty([2], dtype=torch.float32, device=self.device)
        g_o = torch.empty([self.V, 3], dtype=torch.float32, device=self.device)
        g_c = torch.empty([self.V, 3], dtype=torch.float32, device=self.device)
        i32, f32 = torch.int32, torch.float32
        with _lib.on_device(self.device) as stream:
            rc = _lib.lib().coma_app_objective_f32(
                _lib.ptr(v, f32, "vertices"), _lib.ptr(self.faces, i32), _lib.ptr(self.vf_offsets, i32), _lib.ptr(self.vf_faces, i32),
                self.V, self.F, _lib.ptr(self.orientation_gt, f32), self._b, self._p, self._s, self.eps, _lib.ptr(self.selected, i32),
                _lib.ptr(self.targets, f32), self.k, _lib.ptr(terms), _lib.ptr(g_o), _lib.ptr(g_c), _lib.ptr(self._ws), self._ws_bytes,
                stream)
        _lib.check(rc, "coma_app_objective_f32")
        return terms, g_o, g_c

    def loss(self, vertices, orientation_weight, contact_weight):
        """orientation_weight * orientation term + contact_weight * contact term as a scalar of the caller's graph."""
        return _ObjectiveFunction.apply(vertices, self, float(orientation_weight), float(contact_weight))


class _ObjectiveFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vertices, objective, w_o, w_c):
        terms, g_o, g_c = objective.evaluate(vertices)
        ctx.save_for_backward(w_o * g_o + w_c * g_c)
        ctx.shape, ctx.dtype = vertices.shape, vertices.dtype
        return (w_o * terms[0] + w_c * terms[1]).to(vertices.dtype)

    @staticmethod
    def backward(ctx, grad_output):
        (g,) = ctx.saved_tensors
        return (grad_output * g).to(ctx.dtype).reshape(ctx.shape), None, None, None
