"""The optimisation app's ComA objective on MI355X: the part of the reference's src/application/optimize.py that is ComA's own.

The app fits a posed body mesh to an object under two terms read off a learned ComA state (optimize.py:274-296): an orientation
term -- the vertex normals of the posed mesh, canonicalised against one object normal, compared with each vertex's most likely
orientation bin -- and a contact term, the chamfer distance between the selected human vertices and their most-contacted object
points.  `ComaObjective` evaluates both terms and their gradients with respect to the vertices in one device pass
(coma_amd/csrc/app_objective.hip; rule set in include/coma_hip.h, restated in tests/app_ref.py); `.loss` wraps that in a
torch.autograd.Function so that a caller's body model (SMPL-X, VPoser: third party, hooks of src/application/optimize.py) keeps
differentiating from the vertices on.  Both take N bodies [N,V,3] against the one set of constants -- several starts of one fit -- in
the launches of one body (coma_app_objective_batch_f32; body n has the single call's bits); `DeviceFit` below is still one body.
`DeviceFit` goes one step further when the body model, the pose decoder and the angle prior are
the library's own too: the whole Adam loop of the app runs as one device call per 4096 iterations (coma_amd/csrc/app_fit.hip).  There
is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import pickle
import time

import numpy as np
import torch

from . import _abi, _lib
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
        self._batch_ws = {}                        # N -> (workspace, bytes) of coma_app_objective_batch_f32, made on first use and kept
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
        """-> (f32 contiguous [V,3] or, for N >= 2 bodies, [N,V,3]; N)."""
        v = vertices
        if v.dim() == 3 and v.shape[0] == 1:
            v = v[0]
        if v.dim() not in (2, 3) or tuple(v.shape[-2:]) != (self.V, 3) or (v.dim() == 3 and v.shape[0] < 2):
            raise ValueError(f"vertices: expected [{self.V},3], [1,{self.V},3] or [N,{self.V},3], got {tuple(vertices.shape)}")
        if not v.is_cuda or v.device != self.device:
            raise _lib.ComaHipError(f"vertices must live on {self.device} (got {v.device}); there is no CPU path")
        return v.detach().to(torch.float32).contiguous(), (int(v.shape[0]) if v.dim() == 3 else 1)

    def _batch_workspace(self, N):
        if N not in self._batch_ws:
            nbytes = int(_lib.lib().coma_app_objective_batch_workspace_bytes(self.V, self.F, self.k, N))
            if not nbytes:
                raise ValueError(f"vertices: {N} bodies are outside what coma_app_objective_batch_f32 accepts (at most 1024)")
            self._batch_ws[N] = (torch.empty([nbytes], dtype=torch.uint8, device=self.device), nbytes)
        return self._batch_ws[N]

    def evaluate(self, vertices):
        """vertices [V,3] or [1,V,3] on the device -> (terms f32 [2] = {orientation, contact} unweighted, grad_orientation f32 [V,3],
        grad_contact f32 [V,3]), device tensors; nothing waits for the device.  vertices [N,V,3], N >= 2 bodies against the same
        constants -> (terms [N,2], grad_orientation [N,V,3], grad_contact [N,V,3]) from one coma_app_objective_batch_f32 call: body n
        has the bits of evaluate(vertices[n])."""
        v, N = self._vertices(vertices)
        lead = [N] if v.dim() == 3 else []
        terms = torch.empty(lead + [2], dtype=torch.float32, device=self.device)
        g_o = torch.empty(lead + [self.V, 3], dtype=torch.float32, device=self.device)
        g_c = torch.empty(lead + [self.V, 3], dtype=torch.float32, device=self.device)
        i32, f32 = torch.int32, torch.float32
        batch = (N,) if lead else ()
        entry = "coma_app_objective_batch_f32" if lead else "coma_app_objective_f32"
        ws, ws_bytes = self._batch_workspace(N) if lead else (self._ws, self._ws_bytes)
        with _lib.on_device(self.device) as stream:
            rc = getattr(_lib.lib(), entry)(
                _lib.ptr(v, f32, "vertices"), _lib.ptr(self.faces, i32), _lib.ptr(self.vf_offsets, i32), _lib.ptr(self.vf_faces, i32),
                self.V, self.F, _lib.ptr(self.orientation_gt, f32), self._b, self._p, self._s, self.eps, _lib.ptr(self.selected, i32),
                _lib.ptr(self.targets, f32), self.k, *batch, _lib.ptr(terms), _lib.ptr(g_o), _lib.ptr(g_c), _lib.ptr(ws), ws_bytes, stream)
        _lib.check(rc, entry)
        return terms, g_o, g_c

    def loss(self, vertices, orientation_weight, contact_weight):
        """orientation_weight * orientation term + contact_weight * contact term as a scalar of the caller's graph; for N >= 2 bodies
        [N,V,3] a tensor [N], one weighted loss per body (its backward gives body n grad_output[n] times that body's gradient)."""
        return _ObjectiveFunction.apply(vertices, self, float(orientation_weight), float(contact_weight))


MAX_FIT_ITERATIONS = 4096                          # E of one coma_app_fit_f32 call


def fit_chunks(num_iters, limit=MAX_FIT_ITERATIONS):
    """num_iters split into calls of at most `limit` iterations, in order."""
    num_iters, limit = int(num_iters), int(limit)
    if num_iters < 0 or limit < 1:
        raise ValueError(f"fit_chunks: num_iters = {num_iters} must not be negative and limit = {limit} must be positive")
    return [min(limit, num_iters - start) for start in range(0, num_iters, limit)]


def fit_parameter_layout(hand_size, latent, num_body):
    """The index bookkeeping of coma_app_fit_f32, as slices.  `p`: where each group sits in the parameter vector p = [global_orient 3
    | transl 3 | left hand | right hand | embedding], `theta`: where it sits in the body model's packed pose [global_orient |
    body_pose | jaw | leye | reye | left hand | right hand] (DeviceSMPLX.__call__'s order; transl and the embedding have no place
    there), `P` and `n_theta` the two lengths."""
    hs, D, nb = int(hand_size), int(latent), int(num_body)
    if hs < 0 or D < 1 or nb < 1:
        raise ValueError(f"fit_parameter_layout: hand_size = {hs}, latent = {D}, num_body = {nb}")
    p = dict(global_orient=slice(0, 3), transl=slice(3, 6), left_hand_pose=slice(6, 6 + hs), right_hand_pose=slice(6 + hs, 6 + 2 * hs),
             embedding=slice(6 + 2 * hs, 6 + 2 * hs + D))
    lead = 3 + nb + 9
    theta = dict(global_orient=slice(0, 3), body_pose=slice(3, 3 + nb), jaw_pose=slice(3 + nb, 6 + nb), leye_pose=slice(6 + nb, 9 + nb),
                 reye_pose=slice(9 + nb, lead), left_hand_pose=slice(lead, lead + hs), right_hand_pose=slice(lead + hs, lead + 2 * hs))
    return dict(p=p, theta=theta, P=6 + 2 * hs + D, n_theta=lead + 2 * hs)


class FitDesc(C.Structure):
    _fields_ = _abi.STRUCTS["coma_app_fit_desc"]


def _host_address(array):
    return C.cast(array, C.c_void_p)


class DeviceFit:
    """The fitting app's Adam loop as one device call per (at most) 4096 iterations: coma_app_fit_f32 enqueues decode, skinning,
    objective, both backwards and the Adam step of every iteration on the current stream and keeps the parameters, Adam's moments and
    the records on the device (rule set: include/coma_hip.h, "The fitting app's whole Adam loop"; restated in tests/fit_ref.py).
    Parameters and initial values are fit()'s (src/application/optimize.py): global_orient 0, transl (3, 1, 0), both hands 0, the
    embedding the decoder's encoding of the T-pose; betas fixed, expression, jaw and eyes zero.  There is no CPU fallback."""

    def __init__(self, body, decoder, prior, objective):
        from .body_model import DeviceSMPLX
        from .pose_prior import DeviceAnglePrior, DeviceVPoser
        for obj, cls, name in ((body, DeviceSMPLX, "body"), (decoder, DeviceVPoser, "decoder"), (prior, DeviceAnglePrior, "prior"),
                               (objective, ComaObjective, "objective")):
            if not isinstance(obj, cls):
                raise TypeError(f"DeviceFit: {name} must be a {cls.__name__}, got {type(obj).__name__}")
        if 3 * decoder.num_joints != body.num_body:
            raise ValueError(f"DeviceFit: the decoder gives {3 * decoder.num_joints} body-pose entries, the body model takes {body.num_body}")
        if objective.V != body.V:
            raise ValueError(f"DeviceFit: the objective was built for {objective.V} vertices, the body model has {body.V}")
        devices = {name: _lib.need_device(obj.device, "DeviceFit") for name, obj in (("body", body), ("decoder", decoder), ("prior", prior),
                                                                                     ("objective", objective))}
        if len(set(devices.values())) != 1:
            raise _lib.ComaHipError("DeviceFit: its parts live on different devices: " + ", ".join(f"{k} on {v}" for k, v in devices.items()))
        self.body, self.decoder, self.prior, self.objective, self.device = body, decoder, prior, objective, devices["body"]
        self.layout = fit_parameter_layout(body.hand_size, decoder.latentD, body.num_body)
        self.P = self.layout["P"]
        self._state = None
        self._ws = None

    def _buffers(self):
        if self._ws is None:
            L, b, d, o = _lib.lib(), self.body, self.decoder, self.objective
            self._state_bytes = int(L.coma_app_fit_state_bytes(self.P))
            self._ws_bytes = int(L.coma_app_fit_workspace_bytes(b.V, o.F, b.J, o.k, d.num_neurons, d.num_joints, self.layout["n_theta"]))
            if not self._state_bytes or not self._ws_bytes:
                raise _lib.ComaHipError(f"DeviceFit: sizes V={b.V} F={o.F} J={b.J} k={o.k} H={d.num_neurons} NJ={d.num_joints} P={self.P} are "
                                        "outside what coma_app_fit_f32 accepts")
            self._ws = torch.empty([self._ws_bytes], dtype=torch.uint8, device=self.device)
            self._lead_fixed = torch.zeros([9], dtype=torch.float32, device=self.device)
        return self._ws

    def start(self):
        """fit()'s initial values as p f64 [P] on the device."""
        mean = self.decoder.encode(torch.zeros([1, 3 * self.decoder.num_joints], dtype=torch.float32, device=self.device)).mean
        p0 = torch.zeros([self.P], dtype=torch.float64, device=self.device)
        p0[self.layout["p"]["transl"]] = torch.tensor([3.0, 1.0, 0.0], dtype=torch.float64, device=self.device)
        p0[self.layout["p"]["embedding"]] = mean.reshape(-1).to(torch.float64)
        return p0

    def descriptor(self, E, weights, traj, losses, grad0, vertices):
        """The coma_app_fit_desc of one call and the host arrays it points into (to be kept until the call has returned)."""
        b, dec, o, w, f32, i32 = self.body, self.decoder, self.objective, self.decoder._w, torch.float32, torch.int32
        index, sign = self.prior.vectors(False)
        keep = (index, sign, b._parents, o._b, o._p, o._s)
        d = FitDesc()
        d.posedirs, d.weights, d.parents = _lib.ptr(b._posedirs, f32), _lib.ptr(b._weights, f32), _host_address(b._parents)
        d.hand_components, d.pose_mean, d.shape_state = _lib.ptr(b._comps, f32), _lib.ptr(b._mean, f32), _lib.ptr(b._shape_state)
        d.lead_fixed = _lib.ptr(self._lead_fixed, f32)
        d.V, d.J, d.hand_dim, d.n_pca = b.V, b.J, b.hand_dim, b.num_pca_comps
        for name, key in (("W1", "bodyprior_dec_fc1.weight"), ("b1", "bodyprior_dec_fc1.bias"), ("W2", "bodyprior_dec_fc2.weight"),
                          ("b2", "bodyprior_dec_fc2.bias"), ("W3", "bodyprior_dec_out.weight"), ("b3", "bodyprior_dec_out.bias")):
            setattr(d, name, _lib.ptr(w[key], f32))
        d.D, d.H, d.NJ = dec.latentD, dec.num_neurons, dec.num_joints
        d.prior_index, d.prior_sign, d.prior_K = _host_address(index), _host_address(sign), len(index)
        d.faces, d.vf_offsets, d.vf_faces = _lib.ptr(o.faces, i32), _lib.ptr(o.vf_offsets, i32), _lib.ptr(o.vf_faces, i32)
        d.orientation_gt = _lib.ptr(o.orientation_gt, f32)
        d.obj_normal, d.principle_vec, d.sub_principle_vec = _host_address(o._b), _host_address(o._p), _host_address(o._s)
        d.selected, d.targets = _lib.ptr(o.selected, i32), _lib.ptr(o.targets, f32)
        d.F, d.k, d.eps = o.F, o.k, o.eps
        d.P, d.E = self.P, int(E)
        for name, value in weights.items():
            setattr(d, name, float(value))
        d.traj, d.losses, d.grad0, d.vertices = traj, losses, grad0, _lib.ptr(vertices, f32)
        return d, keep

    def run(self, lr, body_pose_weight, bending_prior_weight, pprior_weight, orientation_weight, contact_weight, scale_factor, num_iters=2000,
            betas=None, record=False, resume=False):
        """num_iters Adam iterations -> fit()'s dict: vertices [V,3] of the last iteration's forward (None when num_iters == 0), losses
        (the totals, one per iteration), trajectory (global_orient and transl after every step, [num_iters + 1, 6], when record); with
        record also parameters f64 [num_iters + 1, P], loss_terms f64 [num_iters, 5] = {total, pose prior, weighted angle prior,
        orientation term, contact term (both unweighted)} and first_gradient f64 [P].  betas [1, num_betas]: the shape the fit runs
        on (None = zeros); the shape stage runs once.  resume: continue from where the previous run() of this object stopped (Adam's
        moments included) instead of from fit()'s initial values.  The device is waited for once, at the end; a gradient or parameter
        that stopped being finite raises ComaHipError naming the iteration (the parameters stay at their last finite values)."""
        chunks = fit_chunks(num_iters)
        if resume and self._state is None:
            raise _lib.ComaHipError("DeviceFit.run: resume=True, but this object has not run yet")
        b, L, dev, f64 = self.body, _lib.lib(), self.device, torch.float64
        b._shape_stage(None if betas is None else torch.as_tensor(np.asarray(betas, dtype=np.float32)), None)
        self.decoder._upload()
        self._buffers()
        E = int(num_iters)
        weights = dict(lr=lr, body_pose_weight=body_pose_weight, bending_prior_weight=bending_prior_weight, pprior_weight=pprior_weight,
                       orientation_weight=orientation_weight, contact_weight=contact_weight, scale_factor=scale_factor)
        traj = torch.empty([E + 1, self.P], dtype=f64, device=dev) if record else None
        losses = torch.empty([max(E, 1), 5], dtype=f64, device=dev)
        grad0 = torch.empty([self.P], dtype=f64, device=dev) if record else None
        vertices = torch.empty([b.V, 3], dtype=torch.float32, device=dev)
        p0 = None if resume else self.start()
        with _lib.on_device(dev) as stream:
            rc = 0
            if not resume:
                self._state = torch.empty([self._state_bytes], dtype=torch.uint8, device=dev)
                rc = L.coma_app_fit_init_f64(_lib.ptr(p0, f64), self.P, _lib.ptr(self._state), self._state_bytes, stream)
            done, began = 0, time.perf_counter()
            for n in chunks:
                if rc:
                    break
                at = lambda t, row: None if t is None else C.c_void_p(t.data_ptr() + 8 * row * t.shape[1])
                d, keep = self.descriptor(n, weights, at(traj, done), at(losses, done), _lib.ptr(grad0, f64) if done == 0 else None, vertices)
                rc = L.coma_app_fit_f32(C.byref(d), _lib.ptr(self._state), self._state_bytes, _lib.ptr(self._ws), self._ws_bytes, stream)
                del keep
                done += n
            self.enqueue_seconds = time.perf_counter() - began        # host time of the C calls alone: nothing has waited yet
            iteration = C.c_int(0)
            status = L.coma_app_fit_status(_lib.ptr(self._state), stream, C.byref(iteration)) if rc == 0 else 0
        _lib.check(rc, "coma_app_fit_f32")
        host = lambda t: t.cpu().numpy()
        out = dict(vertices=host(vertices) if E else None, losses=[float(x) for x in host(losses[:E, 0])], trajectory=[])
        if record:
            if E == 0:
                traj.copy_(self.parameters()[None])
            out.update(parameters=host(traj), loss_terms=host(losses[:E]), first_gradient=host(grad0) if E else None, trajectory=host(traj[:, :6]))
        self.last = out
        if status != 0:
            raise _lib.ComaHipError(f"DeviceFit.run: stopped stepping in iteration {iteration.value}: {L.coma_last_error().decode()}")
        return out

    def parameters(self):
        """The current parameter vector f64 [P] (device), as the state block holds it."""
        if self._state is None:
            raise _lib.ComaHipError("DeviceFit.parameters: this object has not run yet")
        return self._state[64:64 + 8 * self.P].view(torch.float64)


class _ObjectiveFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vertices, objective, w_o, w_c):
        terms, g_o, g_c = objective.evaluate(vertices)
        ctx.save_for_backward(w_o * g_o + w_c * g_c)
        ctx.shape, ctx.dtype = vertices.shape, vertices.dtype
        return (w_o * terms[..., 0] + w_c * terms[..., 1]).to(vertices.dtype)

    @staticmethod
    def backward(ctx, grad_output):
        (g,) = ctx.saved_tensors
        if g.dim() == 3:
            grad_output = grad_output.reshape(-1, 1, 1)                # [N]: body n's gradient times its own factor
        return (grad_output * g).to(ctx.dtype).reshape(ctx.shape), None, None, None
