"""ctypes binding of libcoma_hip.so (the C ABI declared in include/*.h, read by _abi.py).

There is deliberately NO fallback: if the shared library is missing or a call is made with tensors
that are not on a HIP device, this module raises.  The CPU oracle under oracle/ is test
infrastructure and is never imported from here.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

import torch

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# COMA_HIP_LIB=<path>: tuning aid -- load another BUILD of the library (A/B of two builds inside one GPU call: box-to-box spread is larger
# than most of the effects being measured); the product and the tests use the in-tree library
LIB_PATH = os.environ.get("COMA_HIP_LIB") or os.path.join(_HERE, "libcoma_hip.so")
# COMA_ABI_VERSION of include/coma_hip.h.  Bumped only when an EXISTING signature changes: a library that merely lacks an added
# function is refused by lib() anyway, through the getattr of the missing symbol.
ABI_VERSION = _abi.DEFINES["COMA_ABI_VERSION"]

_lib = None

# name -> (restype, argtypes) and name -> parameter names of every function the headers declare (see _abi.py: there is no table to extend)
SIGNATURES = {name: (res, [t for _, t in params]) for name, (res, params) in _abi.FUNCTIONS.items()}
PARAMS = {name: tuple(n for n, _ in params) for name, (_, params) in _abi.FUNCTIONS.items()}


class ComaHipError(RuntimeError):
    pass


def lib():
    """Load (once) and return the ctypes handle; raises if the library has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ComaHipError(
                f"{LIB_PATH} is missing: build it with `python -m coma_amd.build` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        if os.environ.get("COMA_HIP_LIB"):
            import sys
            print(f"coma_amd: COMA_HIP_LIB override active -- loading {LIB_PATH} instead of the in-tree library (tuning aid)", file=sys.stderr, flush=True)
        h = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(h, name)      # AttributeError here = header/library mismatch
            fn.restype, fn.argtypes = res, args
        if h.coma_abi_version() != ABI_VERSION:
            raise ComaHipError(f"ABI version mismatch: {LIB_PATH} reports {h.coma_abi_version()}, this package binds version {ABI_VERSION} "
                               "(rebuild with `python -m coma_amd.build`)")
        _lib = h
    return _lib


_switched = threading.local()       # device that was current before stream_ptr() switched it for one launch


def check(rc: int, what: str):
    """Raise on a non-zero return code.  Every wrapper calls this right after its launch, so it is also where the device that
    stream_ptr() made current for that launch is handed back to the caller (the process-wide current device is not ours to change)."""
    _restore()
    if rc != 0:
        raise ComaHipError(f"{what} failed ({rc}): {lib().coma_last_error().decode()}")


def ptr(t: torch.Tensor | None, dtype=None, name="tensor"):
    """Device pointer of a contiguous HIP tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise ComaHipError(f"{name} must live on a HIP device (got {t.device}); there is no CPU path")
    if dtype is not None and t.dtype != dtype:
        raise ComaHipError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ComaHipError(f"{name} must be contiguous")
    return C.c_void_p(t.data_ptr())


def stream_ptr(device=None):
    """Current stream of `device`, and that device made current for the ONE launch that follows (the C ABI launches under HIP's
    current device, so a tensor on cuda:1 with cuda:0 current would otherwise meet a stream of another device); check() puts
    the caller's device back."""
    _restore()              # a launch that raised between its stream_ptr() and its check() left the switch behind: undo it first
    if device is not None:
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is not None and dev.index != torch.cuda.current_device():
            _switched.dev = torch.cuda.current_device()          # restored by check() after the launch
            torch.cuda.set_device(dev)
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _restore():
    prev = getattr(_switched, "dev", None)
    if prev is not None:
        _switched.dev = None
        torch.cuda.set_device(prev)


import contextlib  # noqa: E402


@contextlib.contextmanager
def on_device(device):
    """`with _lib.on_device(t.device) as stream:` -- the stream pointer for ANY NUMBER of launches on `device`, that device current
    inside the block and the caller's device back afterwards whatever happens (exceptions included).  The one-shot stream_ptr() /
    check() pair is for wrappers with exactly one launch; a wrapper that launches twice uses this."""
    _restore()
    dev = torch.device(device) if device is not None else None
    prev = None
    if dev is not None and dev.type == "cuda" and dev.index is not None and dev.index != torch.cuda.current_device():
        prev = torch.cuda.current_device()
        torch.cuda.set_device(dev)
    try:
        yield C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    finally:
        if prev is not None:
            torch.cuda.set_device(prev)


def need_device(device, who, resolve=True):
    """`device` as a torch.device of a HIP device, or ComaHipError: there is no CPU path.  With resolve (the default) a bare "cuda"
    becomes cuda:N of the current device, as tensors report it -- that asks the runtime, so an object that must not touch the device
    before its first call checks with resolve=False when it is built and resolves from its first upload."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ComaHipError(f"{who} needs a HIP device (got {dev}); there is no CPU path")
    if resolve and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def vec3(v):
    return (C.c_float * 3)(float(v[0]), float(v[1]), float(v[2]))
