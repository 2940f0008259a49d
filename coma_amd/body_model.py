"""The SMPL-X body model on MI355X: linear blend skinning forward and backward by the library's own kernels
(coma_amd/csrc/smplx.hip; rule set in include/coma_hip.h, restated in tests/smplx_ref.py).

`DeviceSMPLX` has the call shape of the third-party `smplx` package's model object, which is what the `body_model` hooks of
src/application/optimize.py and src/generation/optimize_depth.py call: keyword tensors in, an object with .vertices [1,V,3],
.joints, .full_pose and .faces out.  `batch_size=N` (the package's own constructor argument) poses N bodies per call through the
batched entry points (coma_smplx_*_batch_f32): every output gains the leading dimension N, and body n has the bits of a single-body
call on the same inputs.  `.vertices` is the output of a torch.autograd.Function whose backward is the device backward, so
a pose decoder or a prior on the other side of the hook keeps differentiating through torch.

By default `.joints` and `.full_pose` carry no gradient and betas / expression must not require grad.  `differentiable=` opts in, any
subset of {"joints", "full_pose", "shape"}: with "joints" / "full_pose" those outputs take part in autograd too, with "shape" betas
and expression may require grad and receive gradients from whichever outputs are differentiable (coma_smplx_backward_full_f32; the
backward is once_differentiable at every setting of `differentiable=`, the empty one included: a double backward raises).  With any
of them, every forward keeps the shape state it ran on, so a backward after the coefficients have changed still differentiates ITS
forward; with "shape" the shape stage reads the coefficients
from the device tensors (nothing is copied to the host) and re-runs whenever a tensor or its version counter differs.

Deviations from the package, all refused or stated rather than silently different:
  * by default NO gradient with respect to betas or expression (the call raises if either requires grad) and none through `.joints`
    or `.full_pose`; each needs its entry in `differentiable=`;
  * no gradient with respect to the model's own tensors (shapedirs, posedirs, weights), no double backward;
  * at batch_size > 1 no gradient to betas or expression ("shape" is refused in the constructor), and betas / expression are one row
    for all bodies or one row per body; DeviceFit is not batched (ComaObjective takes N bodies, DeviceVPoser and DeviceAnglePrior up
    to 64 rows, and src/application/optimize.py --num_starts N, a policy of this project, runs N starts of one fit through them);
  * the package's table of vertex ids for the extra joints (nose, eyes, ears, toes, heels, finger tips) is not shipped: it is taken
    from `smplx.vertex_ids` when that package imports, may be passed in, and otherwise `.joints` is [J posed joints | landmarks] and
    `extra_joint_source` says "landmarks only";
  * no dynamic face contour, no joint mapper.
There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib

SHAPE_SPACE_DIM, EXPRESSION_SPACE_DIM = 300, 100
MAX_JOINTS = 64
MAX_BATCH = 1024                                                         # the batched entry points' bound on N
MAX_GRAD_EXTRA_JOINTS = 4096                                             # the full backward's bound on E
DIFFERENTIABLE = ("joints", "full_pose", "shape")
# the package's order of the extra joints (vertex_joint_selector.py): face and feet, then the finger tips of both hands
_FACE_FEET = ("nose", "reye", "leye", "rear", "lear", "LBigToe", "LSmallToe", "LHeel", "RBigToe", "RSmallToe", "RHeel")
_TIPS = ("thumb", "index", "middle", "ring", "pinky")


def _package_vertex_ids():
    try:
        from smplx.vertex_ids import vertex_ids
    except ImportError:
        return None
    table = vertex_ids["smplx"]
    return [table[n] for n in _FACE_FEET] + [table[side + n] for side in ("l", "r") for n in _TIPS]


class DeviceSMPLX:
    def __init__(self, model, n_pca=45, flat_hand_mean=False, use_pca=True, device="cuda", num_betas=10, num_expression_coeffs=10,
                 extra_joint_vertex_ids=None, differentiable=(), batch_size=1):
        """model: a dict of arrays with the keys of an SMPL-X model file (v_template, shapedirs, posedirs, J_regressor, kintree_table,
        weights, f, hands_components{l,r}, hands_mean{l,r}, lmk_faces_idx, lmk_bary_coords).  differentiable: a subset of
        DIFFERENTIABLE, what besides .vertices -> pose / transl takes part in autograd (module docstring); empty = none.  batch_size: the
        bodies posed per call; every pose argument and transl is then [batch_size, n] or [1, n], betas and expression likewise."""
        dev = _lib.need_device(device, "DeviceSMPLX", resolve=False)
        if isinstance(batch_size, bool) or not isinstance(batch_size, (int, np.integer)) or not 1 <= batch_size <= MAX_BATCH:
            raise ValueError(f"DeviceSMPLX: batch_size={batch_size!r} must be an integer in [1, {MAX_BATCH}]")
        self.batch_size = int(batch_size)
        if isinstance(differentiable, str) or not set(differentiable) <= set(DIFFERENTIABLE):
            raise ValueError(f"DeviceSMPLX: differentiable={differentiable!r} must be a collection of names out of {DIFFERENTIABLE}")
        self.differentiable = frozenset(differentiable)
        if "shape" in self.differentiable and self.batch_size > 1:
            raise ValueError(f"DeviceSMPLX: differentiable \"shape\" with batch_size={self.batch_size}: the batched backward has no gradient to "
                             f"betas or expression; use batch_size=1 for it")
        need = ("v_template", "shapedirs", "posedirs", "J_regressor", "kintree_table", "weights", "f", "hands_componentsl", "hands_componentsr",
                "hands_meanl", "hands_meanr", "lmk_faces_idx", "lmk_bary_coords")
        missing = [k for k in need if k not in model]
        if missing:
            raise KeyError(f"DeviceSMPLX: the model lacks {missing}")
        f32 = lambda a: np.ascontiguousarray(np.asarray(a), dtype=np.float32)
        v_template = f32(model["v_template"]).reshape(-1, 3)
        V = int(v_template.shape[0])
        J_regressor = f32(model["J_regressor"])
        J = int(J_regressor.shape[0])
        if J_regressor.shape != (J, V):
            raise ValueError(f"J_regressor: expected [J,{V}], got {J_regressor.shape}")
        if not 5 <= J <= MAX_JOINTS:
            raise ValueError(f"DeviceSMPLX: {J} joints; between 5 and {MAX_JOINTS} are supported")
        # shape directions [:, :, :num_betas]; expression directions from 300 on, or 10:20 in a file with fewer than 400 directions
        sd = np.asarray(model["shapedirs"])
        if sd.ndim < 3:
            sd = sd[:, :, None]
        num_betas = min(num_betas, 10) if sd.shape[-1] < SHAPE_SPACE_DIM else min(num_betas, SHAPE_SPACE_DIM)
        if sd.shape[-1] < SHAPE_SPACE_DIM + EXPRESSION_SPACE_DIM:
            start, end = 10, 20
        else:
            start, end = SHAPE_SPACE_DIM, SHAPE_SPACE_DIM + num_expression_coeffs
        shape_dirs, expr_dirs = sd[:, :, :num_betas], sd[:, :, start:end]
        self.num_betas, self.num_expression_coeffs = int(shape_dirs.shape[-1]), int(expr_dirs.shape[-1])
        shapedirs = f32(np.concatenate([shape_dirs, expr_dirs], -1))
        if shapedirs.shape[:2] != (V, 3) or shapedirs.shape[-1] < 1:
            raise ValueError(f"shapedirs: expected [{V},3,NB >= 1], got {shapedirs.shape}")
        pd = np.asarray(model["posedirs"])
        P = 9 * (J - 1)
        if pd.shape != (V, 3, P):
            raise ValueError(f"posedirs: expected [{V},3,{P}], got {pd.shape}")
        posedirs = f32(pd.reshape(-1, P).T)                         # [P, 3V], the layout the package keeps too
        weights = f32(model["weights"])
        if weights.shape != (V, J):
            raise ValueError(f"weights: expected [{V},{J}], got {weights.shape}")
        parents = np.asarray(model["kintree_table"])[0].astype(np.int64).copy()
        parents[0] = -1
        if parents.shape != (J,) or any(not 0 <= parents[i] < i for i in range(1, J)):
            raise ValueError("kintree_table: every joint after the root needs a parent with a smaller index")
        hd = int(np.asarray(model["hands_meanl"]).size)
        if hd % 3 or 2 * hd > 3 * (J - 5) or np.asarray(model["hands_meanr"]).size != hd:
            raise ValueError(f"hands_mean: {hd} entries per hand do not fit {J} joints")
        self.use_pca, self.flat_hand_mean = bool(use_pca), bool(flat_hand_mean)
        self.num_pca_comps = int(n_pca) if use_pca else 0
        comps = None
        if use_pca:
            cl, cr = f32(model["hands_componentsl"])[:n_pca], f32(model["hands_componentsr"])[:n_pca]
            if cl.shape != (n_pca, hd) or cr.shape != (n_pca, hd):
                raise ValueError(f"hands_components: expected at least [{n_pca},{hd}], got {cl.shape} and {cr.shape}")
            comps = np.stack([cl, cr])
        mean = np.zeros(3 * J, np.float32)
        if not flat_hand_mean and hd:
            mean[3 * J - 2 * hd:3 * J - hd], mean[3 * J - hd:] = f32(model["hands_meanl"]).reshape(-1), f32(model["hands_meanr"]).reshape(-1)
        self.faces = np.asarray(model["f"]).astype(np.int64).reshape(-1, 3)
        lmk_faces = np.asarray(model["lmk_faces_idx"]).astype(np.int64).reshape(-1)
        lmk_bary = f32(model["lmk_bary_coords"]).reshape(-1, 3)
        if extra_joint_vertex_ids is None:
            extra_joint_vertex_ids = _package_vertex_ids()
            self.extra_joint_source = "landmarks only" if extra_joint_vertex_ids is None else "smplx.vertex_ids"
        else:
            self.extra_joint_source = "caller"
        ids = np.asarray([] if extra_joint_vertex_ids is None else list(extra_joint_vertex_ids), dtype=np.int64).reshape(-1)
        idx = np.concatenate([np.repeat(ids[:, None], 3, 1), self.faces[lmk_faces]])
        if idx.size and (idx.min() < 0 or idx.max() >= V):
            raise IndexError(f"extra joints: vertex indices must lie in [0, {V}), got [{idx.min()}, {idx.max()}]")
        w = np.concatenate([np.tile(np.float32([1, 0, 0]), (len(ids), 1)), lmk_bary]).astype(np.float32)

        self.V, self.J, self.P, self.hand_dim, self.device = V, J, P, hd, dev
        self.num_lead = 3 * J - 2 * hd                                  # axis-angle entries before the hands
        self.num_body = self.num_lead - 12                               # body_pose entries
        self.hand_size = self.num_pca_comps if use_pca else hd          # entries of one hand's argument
        self.num_theta = self.num_lead + 2 * self.hand_size
        self.num_extra = int(idx.shape[0])
        if "joints" in self.differentiable and self.num_extra > MAX_GRAD_EXTRA_JOINTS:
            raise ValueError(f"DeviceSMPLX: {self.num_extra} extra joints; the gradient through .joints handles at most {MAX_GRAD_EXTRA_JOINTS}")
        # host copies (read by the tests) and their device uploads
        self.host = dict(v_template=v_template, shapedirs=shapedirs, posedirs=posedirs, J_regressor=J_regressor, weights=weights,
                         parents=parents, hand_components=comps, pose_mean=mean, extra_index=idx, extra_weight=w)
        self._parents = (C.c_int32 * J)(*[int(p) for p in parents])
        self._uploaded = False                                           # the device is first touched by the first call
        self._shape_keys, self._shape_source, self._shape_version = None, None, None    # the last shape stage: its rows of coefficients, its tensors
        self.shape_stage_runs = 0                                        # how often the shape stage ran (tests count it)

    @classmethod
    def from_file(cls, model_path, gender="neutral", num_pca_comps=45, flat_hand_mean=False, use_pca=True, device="cuda", num_betas=10,
                  num_expression_coeffs=10, extra_joint_vertex_ids=None, differentiable=(), batch_size=1):
        """model_path: the model file itself, or -- the path rule of the package's `create(model_path, model_type="smplx")` -- a
        directory whose `smplx/` sub-directory holds SMPLX_{GENDER}.npz; read with NumPy alone."""
        pth = model_path
        if os.path.isdir(pth):
            pth = os.path.join(pth, "smplx")
            if os.path.isdir(pth):
                pth = os.path.join(pth, f"SMPLX_{gender.upper()}.npz")
        if not os.path.exists(pth):
            raise FileNotFoundError(f"DeviceSMPLX: {pth} does not exist")
        with np.load(pth, allow_pickle=True) as data:
            model = {k: data[k] for k in data.files}
        return cls(model, n_pca=num_pca_comps, flat_hand_mean=flat_hand_mean, use_pca=use_pca, device=device, num_betas=num_betas,
                   num_expression_coeffs=num_expression_coeffs, extra_joint_vertex_ids=extra_joint_vertex_ids, differentiable=differentiable,
                   batch_size=batch_size)

    def _upload(self):
        if self._uploaded:
            return
        self.device = _lib.need_device(self.device, "DeviceSMPLX")      # "cuda" means the current device; tensors report cuda:N
        h, dev, N = self.host, self.device, self.batch_size
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self._v_template, self._shapedirs, self._posedirs = up(h["v_template"]), up(h["shapedirs"]), up(h["posedirs"])
        self._J_regressor, self._weights, self._mean = up(h["J_regressor"]), up(h["weights"]), up(h["pose_mean"])
        self._comps = up(h["hand_components"]) if h["hand_components"] is not None and self.hand_dim else None
        self._extra_index, self._extra_weight = (up(h["extra_index"].astype(np.int32)), up(h["extra_weight"])) if self.num_extra else (None, None)
        L = _lib.lib()
        self._shape_bytes, self._saved_bytes = int(L.coma_smplx_shape_state_bytes(self.V, self.J)), int(L.coma_smplx_saved_bytes(self.V, self.J))
        self._shape_stride = (self._shape_bytes + 15) // 16 * 16           # between the states of a batch with a row of coefficients per body
        self._shape_state = torch.empty([self._shape_bytes], dtype=torch.uint8, device=dev)
        # scratch of the calls (`saved` is per forward): one body has the single-body entry points' sizes, and a backward workspace of
        # its own only for the full backward
        self._grad_ws_bytes = 0
        if N > 1:
            self._ws_bytes, self._grad_ws_bytes = (int(f(self.V, self.J, N)) for f in (
                L.coma_smplx_batch_workspace_bytes, L.coma_smplx_batch_grad_workspace_bytes))
        else:
            self._ws_bytes = int(L.coma_smplx_workspace_bytes(self.V, self.J))
            if self.differentiable:
                self._grad_ws_bytes = int(L.coma_smplx_grad_workspace_bytes(self.V, self.J, self.num_betas + self.num_expression_coeffs))
        self._ws = torch.empty([self._ws_bytes], dtype=torch.uint8, device=dev)
        self._grad_ws = torch.empty([self._grad_ws_bytes], dtype=torch.uint8, device=dev) if self._grad_ws_bytes else None
        self._uploaded = True

    def _rows(self, x, n, name):
        """A call argument as a 2-D tensor [1 or batch_size, n] (None stays None); nothing here touches the device."""
        if x is None:
            return None
        if not torch.is_tensor(x):
            x = torch.as_tensor(np.asarray(x, dtype=np.float32))
        if self.batch_size == 1:
            if x.dim() == 2 and x.shape[0] != 1:
                raise ValueError(f"{name}: batch size {x.shape[0]}; DeviceSMPLX handles batch size 1 only")
            if x.numel() != n:
                raise ValueError(f"{name}: expected {n} numbers ([1,{n}]), got shape {tuple(x.shape)}")
            return x.reshape(1, n)
        if x.dim() == 1:
            x = x[None]
        if x.dim() != 2 or x.shape[1] != n:
            raise ValueError(f"{name}: expected [{self.batch_size},{n}] or [1,{n}], got shape {tuple(x.shape)}")
        if x.shape[0] not in (1, self.batch_size):
            raise ValueError(f"{name}: leading dimension {x.shape[0]} is neither 1 nor batch_size={self.batch_size}")
        return x

    # ---- the device calls ----
    def _same_source(self, source):
        """Whether `source` = (betas, expression) are the tensor objects of the last shape stage at the same version counters, and
        those counters.  LIMITATION: a write that does not move the version counter -- through `.data`, or from outside torch -- is
        not seen; pass a new tensor, or write in place through torch."""
        version = tuple(x._version if torch.is_tensor(x) else None for x in source)
        same = self._shape_source is not None and version == self._shape_version and all(
            (x is None and y is None) or (torch.is_tensor(x) and x is y) for x, y in zip(source, self._shape_source))
        return same, version

    def _shape_stage(self, betas, expression):
        """Leaves `_shape_state` ready for the call: ONE state when betas and expression are both [1, n] (or absent), else batch_size
        states `_shape_stride` apart (`_stride()` says which).  A state is re-run only when ITS row of coefficients differs from the
        last call's.  The same tensor objects at the same version counter (the app passes its fixed betas every iteration) are not
        looked at again, so nothing is read back from the device for them; anything else is compared on the host copy made here (one
        device-to-host copy when the coefficients live on the device).  -> the coefficients as a device tensor with differentiable
        "shape", else None."""
        if "shape" in self.differentiable:
            return self._shape_stage_on_device(betas, expression)
        for x, name in ((betas, "betas"), (expression, "expression")):     # looked at on every call, whichever path follows
            if torch.is_tensor(x) and x.requires_grad:
                raise _lib.ComaHipError(
                    f"DeviceSMPLX: {name} requires grad, and the batched device body model has no gradient with respect to {name}" if self.batch_size > 1
                    else f"DeviceSMPLX: {name} requires grad, and the device body model has no gradient with respect to {name} unless it is built "
                         f"with \"shape\" in differentiable=")
        source = (betas, expression)
        same, version = self._same_source(source)
        if same:
            return None
        parts = []
        for x, n, name in ((betas, self.num_betas, "betas"), (expression, self.num_expression_coeffs, "expression")):
            x = self._rows(x, n, name)
            parts.append(np.zeros([1, n], np.float32) if x is None else x.detach().to(torch.float32).cpu().numpy())
        B = max(p.shape[0] for p in parts)
        coef = np.ascontiguousarray(np.concatenate([np.broadcast_to(p, (B, p.shape[1])) for p in parts], 1), dtype=np.float32)
        self._upload()
        keys = [row.tobytes() for row in coef]
        old = self._shape_keys if self._shape_keys is not None and len(self._shape_keys) == B else [None] * B
        stale = [n for n in range(B) if keys[n] != old[n]]
        if stale:
            if self.differentiable or self._shape_state.numel() != B * self._shape_stride:
                stale = list(range(B))          # all of them into a NEW buffer: with `differentiable`, forwards in flight keep the states they ran on
                self._shape_state = torch.empty([B * self._shape_stride], dtype=torch.uint8, device=self.device)
            d_coef = torch.from_numpy(coef).to(self.device)
            with _lib.on_device(self.device) as stream:
                for n in stale:
                    self._run_shape(d_coef[n], n, stream)
        self._shape_keys, self._shape_source, self._shape_version = keys, source, version
        return None

    def _stride(self):
        """The shape_stride of a call on the current shape states: 0 = one state for all bodies."""
        return self._shape_stride if self._shape_keys is not None and len(self._shape_keys) > 1 else 0

    def _run_shape(self, d_coef, n, stream):
        """The shape stage from device coefficients f32 [NB] into state n of `_shape_state`, on the caller's `on_device` stream."""
        f32 = torch.float32
        rc = _lib.lib().coma_smplx_shape_f32(_lib.ptr(self._v_template, f32), _lib.ptr(self._shapedirs, f32), _lib.ptr(d_coef, f32),
                                             _lib.ptr(self._J_regressor, f32), self.V, self.J, int(d_coef.numel()),
                                             C.c_void_p(self._shape_state.data_ptr() + n * self._shape_stride), self._shape_bytes, stream)
        _lib.check(rc, "coma_smplx_shape_f32")
        self.shape_stage_runs += 1

    def _shape_stage_on_device(self, betas, expression):
        """differentiable "shape" (batch size 1): the coefficients as ONE device tensor f32 [NB] that is part of the autograd graph (its
        gradient splits back into betas and expression through torch), built without copying anything to the host.  The shape stage
        is skipped for the same tensor objects at the same version counters and re-run otherwise, into a NEW state (forwards that ran
        on the previous one hold on to it for their backward): values are never compared, that would take a read-back."""
        self._upload()
        parts = []
        for x, n, name in ((betas, self.num_betas, "betas"), (expression, self.num_expression_coeffs, "expression")):
            x = self._rows(x, n, name)
            parts.append(torch.zeros([n], dtype=torch.float32, device=self.device) if x is None
                         else x.reshape(-1).to(device=self.device, dtype=torch.float32))
        coef = torch.cat(parts)
        source = (betas, expression)
        same, version = self._same_source(source)
        if not same:
            self._shape_state = torch.empty([self._shape_bytes], dtype=torch.uint8, device=self.device)
            with _lib.on_device(self.device) as stream:
                self._run_shape(coef.detach().contiguous(), 0, stream)
            self._shape_source, self._shape_version, self._shape_keys = source, version, None
        return coef

    def _forward(self, theta, transl):
        """theta f32 [N, num_theta], transl f32 [N, 3] or None (device, contiguous), on the current shape states -> vertices [N,V,3],
        joints [N, J + extra, 3], full_pose [N, 3J], saved: all new tensors."""
        f32, dev, N, E = torch.float32, self.device, self.batch_size, self.num_extra
        vertices = torch.empty([N, self.V, 3], dtype=f32, device=dev)
        joints = torch.empty([N, self.J + (E if N == 1 else 0), 3], dtype=f32, device=dev)   # one body: the extra joints go in place behind the posed
        full_pose = torch.empty([N, 3 * self.J], dtype=f32, device=dev)
        saved = torch.empty([N * self._saved_bytes], dtype=torch.uint8, device=dev)
        extra = torch.empty([N, E, 3], dtype=f32, device=dev) if N > 1 and E else None
        L = _lib.lib()
        ins = (_lib.ptr(theta, f32, "theta"), _lib.ptr(transl, f32, "transl"), _lib.ptr(self._posedirs, f32), _lib.ptr(self._weights, f32),
               self._parents, _lib.ptr(self._comps, f32), _lib.ptr(self._mean, f32), self.V, self.J, self.hand_dim, self.num_pca_comps)
        table = (_lib.ptr(vertices), _lib.ptr(transl, f32), _lib.ptr(self._extra_index, torch.int32), _lib.ptr(self._extra_weight, f32), self.V, E)
        with _lib.on_device(dev) as stream:
            outs = (_lib.ptr(vertices), _lib.ptr(joints), _lib.ptr(full_pose), _lib.ptr(saved), saved.numel(), _lib.ptr(self._ws), self._ws_bytes, stream)
            if N == 1:
                rc = L.coma_smplx_forward_f32(*ins, _lib.ptr(self._shape_state), *outs)
                if rc == 0 and E:
                    rc = L.coma_smplx_extra_joints_f32(*table, C.c_void_p(joints.data_ptr() + 12 * self.J), stream)
                _lib.check(rc, "coma_smplx_forward_f32")
            else:
                _lib.check(L.coma_smplx_forward_batch_f32(*ins, N, _lib.ptr(self._shape_state), self._stride(), *outs), "coma_smplx_forward_batch_f32")
                if E:
                    _lib.check(L.coma_smplx_extra_joints_batch_f32(*table, N, _lib.ptr(extra), stream), "coma_smplx_extra_joints_batch_f32")
                    joints = torch.cat([joints, extra], 1)
        return vertices, joints, full_pose, saved

    def _backward(self, grad_vertices, saved):
        """The vertices-only backward of one body (coma_smplx_backward_f32, on the forward's workspace) -> (g_theta [1, NT], g_transl [1, 3])."""
        f32, dev = torch.float32, self.device
        g_theta = torch.empty([1, self.num_theta], dtype=f32, device=dev)
        g_transl = torch.empty([1, 3], dtype=f32, device=dev)
        with _lib.on_device(dev) as stream:
            rc = _lib.lib().coma_smplx_backward_f32(_lib.ptr(grad_vertices, f32, "grad_vertices"), _lib.ptr(self._posedirs, f32),
                                                    _lib.ptr(self._weights, f32), self._parents, _lib.ptr(self._comps, f32), self.V, self.J,
                                                    self.hand_dim, self.num_pca_comps, _lib.ptr(self._shape_state), _lib.ptr(saved),
                                                    self._saved_bytes, _lib.ptr(g_theta), _lib.ptr(g_transl), _lib.ptr(self._ws), self._ws_bytes,
                                                    stream)
        _lib.check(rc, "coma_smplx_backward_f32")
        return g_theta, g_transl

    def _backward_full(self, grad_vertices, grad_joints, grad_full_pose, saved, shape_state, want_coefficients, shape_stride=0):
        """The backward of ONE forward (its saved state and the shape states it ran on) from every output: each gradient f32 on the
        device or None = absent -> (g_theta [N, NT], g_transl [N, 3], g_coefficients [NB] or None).  One body: the full backward; a batch:
        the batched one, which has no gradient to the coefficients."""
        f32, dev, N = torch.float32, self.device, self.batch_size
        NB = self.num_betas + self.num_expression_coeffs
        g_theta = torch.empty([N, self.num_theta], dtype=f32, device=dev)
        g_transl = torch.empty([N, 3], dtype=f32, device=dev)
        g_coef = torch.empty([NB], dtype=f32, device=dev) if want_coefficients else None
        L = _lib.lib()
        ins = (_lib.ptr(grad_vertices, f32, "grad_vertices"), _lib.ptr(grad_joints, f32, "grad_joints"), _lib.ptr(grad_full_pose, f32, "grad_full_pose"),
               _lib.ptr(self._posedirs, f32), _lib.ptr(self._weights, f32), self._parents, _lib.ptr(self._comps, f32),
               _lib.ptr(self._extra_index, torch.int32), _lib.ptr(self._extra_weight, f32), self.num_extra)
        sizes = (self.V, self.J, self.hand_dim, self.num_pca_comps)
        with _lib.on_device(dev) as stream:
            ws = (_lib.ptr(self._grad_ws), self._grad_ws_bytes, stream)
            if N == 1:
                name = "coma_smplx_backward_full_f32"
                rc = L.coma_smplx_backward_full_f32(*ins, _lib.ptr(self._shapedirs, f32), _lib.ptr(self._J_regressor, f32), NB, *sizes,
                                                    _lib.ptr(shape_state), _lib.ptr(saved), saved.numel(), _lib.ptr(g_theta), _lib.ptr(g_transl),
                                                    _lib.ptr(g_coef, f32), *ws)
            else:
                name = "coma_smplx_backward_batch_f32"
                rc = L.coma_smplx_backward_batch_f32(*ins, *sizes, N, _lib.ptr(shape_state), shape_stride, _lib.ptr(saved), saved.numel(),
                                                     _lib.ptr(g_theta), _lib.ptr(g_transl), *ws)
        _lib.check(rc, name)
        return g_theta, g_transl, g_coef

    def __call__(self, betas=None, global_orient=None, body_pose=None, left_hand_pose=None, right_hand_pose=None, transl=None, expression=None,
                 jaw_pose=None, leye_pose=None, reye_pose=None, return_verts=True, return_full_pose=False, **unused):
        """The package's call: every argument [batch_size, n] or [1, n] (None = zeros).  Gradients flow from .vertices to the seven pose
        arguments and transl; betas and expression must not require grad.  `differentiable=` (constructor) adds .joints, .full_pose (ask
        for it with return_full_pose=True) and, at batch size 1, the gradient to betas / expression.  A [1, n] argument is expanded to
        [batch_size, n] BEFORE the autograd function, so autograd sums its gradient over the bodies."""
        N = self.batch_size
        sizes = (("global_orient", global_orient, 3), ("body_pose", body_pose, self.num_body), ("jaw_pose", jaw_pose, 3),
                 ("leye_pose", leye_pose, 3), ("reye_pose", reye_pose, 3), ("left_hand_pose", left_hand_pose, self.hand_size),
                 ("right_hand_pose", right_hand_pose, self.hand_size), ("transl", transl, 3))
        rows = [(name, self._rows(x, n, name), n) for name, x, n in sizes]     # shapes first: nothing has touched the device yet
        coefficients = self._shape_stage(betas, expression)                 # a device tensor with differentiable "shape", else None
        parts = []
        for name, x, n in rows:
            if x is None:
                x = None if name == "transl" else torch.zeros([N, n], dtype=torch.float32, device=self.device)
            elif not x.is_cuda or x.device != self.device:
                raise _lib.ComaHipError(f"{name} must live on {self.device} (got {x.device}); there is no CPU path")
            elif x.shape[0] != N:
                x = x.expand(N, n)
            parts.append(x if x is None else x.to(torch.float32))
        transl = parts.pop()
        theta = torch.cat(parts, 1)
        vertices, joints, full_pose = _Function.apply(self, theta, transl, coefficients)
        return SimpleNamespace(vertices=vertices if return_verts else None, joints=joints, full_pose=full_pose if return_full_pose else None,
                               faces=self.faces, betas=betas, expression=expression, global_orient=global_orient, body_pose=body_pose,
                               jaw_pose=jaw_pose, transl=transl)


class _Function(torch.autograd.Function):
    """The forward, with the outputs named in `differentiable` left differentiable, and the device backward from them.  The forward's
    saved block and the shape states it ran on belong to this node: a second forward before the backward disturbs nothing, and a
    later call with other coefficients writes new states."""

    @staticmethod
    def forward(ctx, model, theta, transl, coefficients):
        vertices, joints, full_pose, saved = model._forward(theta.detach().contiguous(), None if transl is None else transl.detach().contiguous())
        ctx.model, ctx.saved, ctx.has_transl = model, saved, transl is not None
        ctx.shape_state, ctx.shape_stride = model._shape_state, model._stride()
        dead = [t for name, t in (("joints", joints), ("full_pose", full_pose)) if name not in model.differentiable]
        if dead:
            ctx.mark_non_differentiable(*dead)
        ctx.set_materialize_grads(False)                      # an output the loss does not read arrives as None and is passed as absent
        return vertices, joints, full_pose

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_vertices, grad_joints, grad_full_pose):
        model = ctx.model
        f32 = lambda g: None if g is None else g.to(torch.float32).contiguous()
        if model.batch_size == 1 and not model.differentiable:          # the fit loop's path: the backward on the forward's workspace
            g_theta, g_transl = model._backward(f32(grad_vertices), ctx.saved)
            return None, g_theta, (g_transl if ctx.has_transl else None), None
        grad_joints = f32(grad_joints) if "joints" in model.differentiable else None
        grad_full_pose = f32(grad_full_pose) if "full_pose" in model.differentiable else None
        g_theta, g_transl, g_coef = model._backward_full(f32(grad_vertices), grad_joints, grad_full_pose, ctx.saved, ctx.shape_state,
                                                         ctx.needs_input_grad[3], ctx.shape_stride)
        return None, g_theta, (g_transl if ctx.has_transl else None), g_coef

