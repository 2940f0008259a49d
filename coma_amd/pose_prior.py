"""VPoser's pose decoder and encoder and the SMPLify angle prior on MI355X, by the library's own kernels (coma_amd/csrc/vposer.hip;
rule set in include/coma_hip.h, restated in tests/vposer_ref.py).

`DeviceVPoser` has the call shape of the `pose_decoder` hook of src/application/optimize.py (the reference's VPoser object):
.encode(pose).mean / .scale and .decode(embedding, output_type="aa") -> [N,1,NJ,3], the latter the output of a
torch.autograd.Function whose backward is the device backward, so the optimiser on the other side of the hook keeps differentiating
through torch.  `DeviceAnglePrior` has the call shape of the `angle_prior` hook (the reference's SMPLifyAnglePrior).

Deviations from the reference, all refused or stated rather than silently different:
  * eval mode only: no dropout, no training, NO gradient with respect to the weights, none through encode (it raises if its input
    requires grad) and none through output_type="matrot" (likewise);
  * the continuous rotation representation only (`use_cont_repr`; the tanh decoder is refused by from_dir); no aa2matrot;
  * at the exact identity rotation the reference's gradient is NaN; the device returns the finite gradient of its k = 2 branch;
  * the angle prior only: the GMM and L2 priors are not reproduced.
There is no CPU path.
"""
from __future__ import annotations

import ast
import configparser
import ctypes as C
import glob
import os
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib

MAX_BATCH, MAX_LATENT, MAX_NEURONS, MAX_JOINTS = 64, 256, 2048, 64
_LAYERS = {"bodyprior_enc_fc1": ("H", "F"), "bodyprior_enc_fc2": ("H", "H"), "bodyprior_enc_mu": ("D", "H"), "bodyprior_enc_logvar": ("D", "H"),
           "bodyprior_dec_fc1": ("H", "D"), "bodyprior_dec_fc2": ("H", "H"), "bodyprior_dec_out": ("O", "H")}
_NORMS = {"bodyprior_enc_bn1": "F", "bodyprior_enc_bn2": "H"}


class DeviceVPoser:
    def __init__(self, state_dict, num_neurons, latentD, data_shape, device="cuda"):
        """state_dict: a VPoser snapshot (tensors or arrays under the names of its layers); data_shape: [1, NJ, 3]."""
        dev = _lib.need_device(device, "DeviceVPoser", resolve=False)
        shape = [int(x) for x in data_shape]
        if len(shape) != 3 or shape[0] != 1 or shape[2] != 3:
            raise ValueError(f"DeviceVPoser: data_shape must be [1, NJ, 3], got {list(data_shape)}")
        H, D, NJ = int(num_neurons), int(latentD), shape[1]
        for name, v, top in (("num_neurons", H, MAX_NEURONS), ("latentD", D, MAX_LATENT), ("joints", NJ, MAX_JOINTS)):
            if not 1 <= v <= top:
                raise ValueError(f"DeviceVPoser: {name} = {v}; between 1 and {top} are supported")
        size = dict(H=H, D=D, F=3 * NJ, O=6 * NJ)
        f32 = lambda a: np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a), dtype=np.float32)
        host = {}
        for layer, (out, inn) in _LAYERS.items():
            for part, want in ((".weight", (size[out], size[inn])), (".bias", (size[out],))):
                if layer + part not in state_dict:
                    raise KeyError(f"DeviceVPoser: the snapshot lacks {layer + part}")
                host[layer + part] = f32(state_dict[layer + part])
                if host[layer + part].shape != want:
                    raise ValueError(f"{layer + part}: expected {list(want)}, got {list(host[layer + part].shape)}")
        for norm, c in _NORMS.items():
            rows = []
            for part in (".weight", ".bias", ".running_mean", ".running_var"):
                if norm + part not in state_dict:
                    raise KeyError(f"DeviceVPoser: the snapshot lacks {norm + part}")
                rows.append(f32(state_dict[norm + part]))
                if rows[-1].shape != (size[c],):
                    raise ValueError(f"{norm + part}: expected [{size[c]}], got {list(rows[-1].shape)}")
            host[norm] = np.stack(rows)
        # the mu layer's rows, then the logvar layer's: one launch gives mean and scale
        host["enc_ml.weight"] = np.concatenate([host.pop("bodyprior_enc_mu.weight"), host.pop("bodyprior_enc_logvar.weight")])
        host["enc_ml.bias"] = np.concatenate([host.pop("bodyprior_enc_mu.bias"), host.pop("bodyprior_enc_logvar.bias")])
        self.host, self.device = host, dev
        self.num_neurons, self.latentD, self.num_joints = H, D, NJ
        self._uploaded = False                                           # the device is first touched by the first call

    @classmethod
    def from_dir(cls, expr_dir, device="cuda"):
        """An experiment directory as the reference's loader reads it: the settings from its *.ini (num_neurons, latentD, data_shape,
        use_cont_repr), the weights from the newest snapshots/*.pt by modification time."""
        if not os.path.isdir(expr_dir):
            raise FileNotFoundError(f"DeviceVPoser: the experiment directory {expr_dir} does not exist")
        inis = sorted(glob.glob(os.path.join(expr_dir, "*.ini")))
        if not inis:
            raise FileNotFoundError(f"DeviceVPoser: no *.ini settings file in {expr_dir}")
        parser = configparser.ConfigParser()
        parser.optionxform = str                                         # keys keep their case (latentD)
        parser.read(inis[0])
        settings = {k: v for section in parser.sections() for k, v in parser[section].items()}
        missing = [k for k in ("num_neurons", "latentD", "data_shape") if k not in settings]
        if missing:
            raise KeyError(f"DeviceVPoser: {inis[0]} lacks {missing}")
        if settings.get("use_cont_repr", "True").strip().lower() not in ("true", "1", "yes"):
            raise NotImplementedError(f"DeviceVPoser: {inis[0]} sets use_cont_repr = {settings['use_cont_repr']}; only the continuous "
                                      "rotation representation is supported (the tanh decoder is not)")
        snapshots = sorted(glob.glob(os.path.join(expr_dir, "snapshots", "*.pt")), key=os.path.getmtime)
        if not snapshots:
            raise FileNotFoundError(f"DeviceVPoser: no snapshot (snapshots/*.pt) in {expr_dir}")
        state = torch.load(snapshots[-1], map_location="cpu", weights_only=True)
        return cls(state, int(settings["num_neurons"]), int(settings["latentD"]), ast.literal_eval(settings["data_shape"]), device=device)

    def _upload(self):
        if self._uploaded:
            return
        self.device = _lib.need_device(self.device, "DeviceVPoser")      # "cuda" means the current device; tensors report cuda:N
        self._w = {k: torch.from_numpy(v).to(self.device) for k, v in self.host.items()}
        self._uploaded = True

    def _sizes(self, N):
        L = _lib.lib()
        return (int(L.coma_vposer_saved_bytes(N, self.num_neurons, self.num_joints)),
                int(L.coma_vposer_workspace_bytes(N, self.num_neurons, self.num_joints)))

    def _rows(self, x, width, name):
        """[N, width] f32 on this object's device, from any shape with N leading rows."""
        if not torch.is_tensor(x):
            raise TypeError(f"{name} must be a tensor")
        if not x.is_cuda:
            raise _lib.ComaHipError(f"{name} must live on a HIP device (got {x.device}); there is no CPU path")
        if x.dim() < 2 or x.numel() != x.shape[0] * width:
            raise ValueError(f"{name}: expected [N, {width}], got {list(x.shape)}")
        if not 1 <= x.shape[0] <= MAX_BATCH:
            raise ValueError(f"{name}: batch size {x.shape[0]}; between 1 and {MAX_BATCH} are supported")
        self._upload()
        if x.device != self.device:
            raise _lib.ComaHipError(f"{name} must live on {self.device} (got {x.device})")
        return x.detach().reshape(x.shape[0], width).to(torch.float32).contiguous()

    # ---- the three device calls; every output is a new tensor, `saved` belongs to its forward ----
    def _decode(self, z, want_matrices=False, want_branch=False):
        N, dev, w, f32 = z.shape[0], self.device, self._w, torch.float32
        saved_bytes, _ = self._sizes(N)
        aa = torch.empty([N, 3 * self.num_joints], dtype=f32, device=dev)
        matrices = torch.empty([N, self.num_joints, 9], dtype=f32, device=dev) if want_matrices else None
        branch = torch.empty([N, self.num_joints], dtype=torch.int8, device=dev) if want_branch else None
        saved = torch.empty([saved_bytes], dtype=torch.uint8, device=dev)
        with _lib.on_device(dev) as stream:
            rc = _lib.lib().coma_vposer_decode_f32(
                _lib.ptr(z, f32, "embedding"), _lib.ptr(w["bodyprior_dec_fc1.weight"]), _lib.ptr(w["bodyprior_dec_fc1.bias"]),
                _lib.ptr(w["bodyprior_dec_fc2.weight"]), _lib.ptr(w["bodyprior_dec_fc2.bias"]), _lib.ptr(w["bodyprior_dec_out.weight"]),
                _lib.ptr(w["bodyprior_dec_out.bias"]), N, self.latentD, self.num_neurons, self.num_joints, _lib.ptr(aa), _lib.ptr(matrices),
                _lib.ptr(branch), _lib.ptr(saved), saved_bytes, stream)
        _lib.check(rc, "coma_vposer_decode_f32")
        return aa, matrices, branch, saved

    def _decode_backward(self, grad_aa, saved):
        N, dev, w, f32 = grad_aa.shape[0], self.device, self._w, torch.float32
        saved_bytes, ws_bytes = self._sizes(N)
        grad_z = torch.empty([N, self.latentD], dtype=f32, device=dev)
        ws = torch.empty([ws_bytes], dtype=torch.uint8, device=dev)
        with _lib.on_device(dev) as stream:
            rc = _lib.lib().coma_vposer_decode_backward_f32(
                _lib.ptr(grad_aa, f32, "grad_aa"), _lib.ptr(w["bodyprior_dec_fc1.weight"]), _lib.ptr(w["bodyprior_dec_fc2.weight"]),
                _lib.ptr(w["bodyprior_dec_out.weight"]), N, self.latentD, self.num_neurons, self.num_joints, _lib.ptr(saved), saved_bytes,
                _lib.ptr(grad_z), _lib.ptr(ws), ws_bytes, stream)
        _lib.check(rc, "coma_vposer_decode_backward_f32")
        return grad_z

    def encode(self, pose):
        """pose [N, 3 NJ] (any shape with N leading rows) -> object with .mean and .scale, [N, latentD]; forward only."""
        if torch.is_tensor(pose) and pose.requires_grad:
            raise _lib.ComaHipError("DeviceVPoser.encode: pose requires grad, and the device encoder has no backward")
        x = self._rows(pose, 3 * self.num_joints, "pose")
        N, dev, w, f32 = x.shape[0], self.device, self._w, torch.float32
        _, ws_bytes = self._sizes(N)
        mean = torch.empty([N, self.latentD], dtype=f32, device=dev)
        scale = torch.empty([N, self.latentD], dtype=f32, device=dev)
        ws = torch.empty([ws_bytes], dtype=torch.uint8, device=dev)
        with _lib.on_device(dev) as stream:
            rc = _lib.lib().coma_vposer_encode_f32(
                _lib.ptr(x, f32, "pose"), _lib.ptr(w["bodyprior_enc_bn1"]), _lib.ptr(w["bodyprior_enc_fc1.weight"]),
                _lib.ptr(w["bodyprior_enc_fc1.bias"]), _lib.ptr(w["bodyprior_enc_bn2"]), _lib.ptr(w["bodyprior_enc_fc2.weight"]),
                _lib.ptr(w["bodyprior_enc_fc2.bias"]), _lib.ptr(w["enc_ml.weight"]), _lib.ptr(w["enc_ml.bias"]), N, self.latentD,
                self.num_neurons, self.num_joints, _lib.ptr(mean), _lib.ptr(scale), _lib.ptr(ws), ws_bytes, stream)
        _lib.check(rc, "coma_vposer_encode_f32")
        return SimpleNamespace(mean=mean, scale=scale)

    def decode(self, embedding, output_type="aa"):
        """embedding [N, latentD] -> "aa": [N,1,NJ,3], differentiable with respect to the embedding; "matrot": [N,1,NJ,9], forward only."""
        if output_type not in ("aa", "matrot"):
            raise ValueError(f"DeviceVPoser.decode: output_type must be 'aa' or 'matrot', got {output_type!r}")
        z = self._rows(embedding, self.latentD, "embedding")
        if output_type == "matrot":
            if embedding.requires_grad:
                raise _lib.ComaHipError("DeviceVPoser.decode: output_type='matrot' has no backward and the embedding requires grad")
            return self._decode(z, want_matrices=True)[1].view(-1, 1, self.num_joints, 9)
        return _DecodeFunction.apply(self, embedding).view(-1, 1, self.num_joints, 3)

    def branches(self, embedding):
        """The quaternion branch id (0 .. 3) of every joint, i8 [N, NJ]: what the tests compare with the reference's selection."""
        return self._decode(self._rows(embedding, self.latentD, "embedding"), want_branch=True)[2]


class _DecodeFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, embedding):
        aa, _, _, saved = model._decode(model._rows(embedding, model.latentD, "embedding"))
        ctx.model, ctx.saved, ctx.shape, ctx.dtype = model, saved, embedding.shape, embedding.dtype
        return aa

    @staticmethod
    def backward(ctx, grad_aa):
        grad_z = ctx.model._decode_backward(grad_aa.to(torch.float32).contiguous(), ctx.saved)
        return None, grad_z.reshape(ctx.shape).to(ctx.dtype)


class DeviceAnglePrior:
    """out[n, i] = exp(sign_i pose[n, index_i])^2 over the elbow and knee bending angles: entries 55, 58, 12, 15 of the pose with the
    global orientation, 3 less without (with_global_pose=False, the app's call), signs 1, -1, -1, -1."""
    INDEX, SIGN = (55, 58, 12, 15), (1.0, -1.0, -1.0, -1.0)

    def __init__(self, device="cuda"):
        self.device = _lib.need_device(device, "DeviceAnglePrior", resolve=False)

    def vectors(self, with_global_pose=False):
        index = [i - (0 if with_global_pose else 3) for i in self.INDEX]
        return (C.c_int32 * len(index))(*index), (C.c_float * len(index))(*self.SIGN)

    def __call__(self, pose, with_global_pose=False):
        """pose [N, P] (P = 63 in the app) -> [N, 4], differentiable with respect to pose."""
        if not torch.is_tensor(pose) or pose.dim() != 2:
            raise ValueError(f"DeviceAnglePrior: pose must be a tensor [N, P], got {list(getattr(pose, 'shape', []))}")
        if not pose.is_cuda:
            raise _lib.ComaHipError(f"pose must live on a HIP device (got {pose.device}); there is no CPU path")
        need = max(self.INDEX) - (0 if with_global_pose else 3) + 1
        if pose.shape[1] < need or not 1 <= pose.shape[0] <= MAX_BATCH:
            raise ValueError(f"DeviceAnglePrior: pose must be [N <= {MAX_BATCH}, P >= {need}], got {list(pose.shape)}")
        return _PriorFunction.apply(self, pose, bool(with_global_pose))


class _PriorFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, prior, pose, with_global_pose):
        x = pose.detach().to(torch.float32).contiguous()
        index, sign = prior.vectors(with_global_pose)
        out = torch.empty([x.shape[0], len(index)], dtype=torch.float32, device=x.device)
        rc = _lib.lib().coma_angle_prior_f32(_lib.ptr(x, torch.float32, "pose"), x.shape[0], x.shape[1], index, sign, len(index), _lib.ptr(out),
                                             _lib.stream_ptr(x.device))
        _lib.check(rc, "coma_angle_prior_f32")
        ctx.x, ctx.vectors, ctx.dtype = x, (index, sign), pose.dtype
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, (index, sign) = ctx.x, ctx.vectors
        grad_pose = torch.empty_like(x)
        rc = _lib.lib().coma_angle_prior_backward_f32(_lib.ptr(x), _lib.ptr(grad_out.to(torch.float32).contiguous(), torch.float32, "grad_out"),
                                                      x.shape[0], x.shape[1], index, sign, len(index), _lib.ptr(grad_pose),
                                                      _lib.stream_ptr(x.device))
        _lib.check(rc, "coma_angle_prior_backward_f32")
        return None, grad_pose.to(ctx.dtype), None
