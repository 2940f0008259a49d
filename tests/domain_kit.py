"""What the "whole accepted domain" suites (attention_ref, gemm_ref, norm_ref, dconv_ref, elementwise_ref, reduce_ref, seg_ref and their tests)
share, each thing once.  Not product code; CPU-importable: pytest and torch.cuda are touched inside functions only.  The CASES / REFUSALS /
REACHABLE tables, references, emulations, a-priori bounds and each suite's own row error stay with the suite.

* constants, buffers   GUARD, FLOOR, U32, COMA_E_INVALID (from the parsed headers), SENTINELS; ``bits``, ``sentinel``, ``sentinel_bits``,
                       ``guarded`` / ``guards_intact``; the torch flavour ``Operand`` / ``Out`` / ``pack`` / ``new_out`` / ``masks`` / ``body``; the
                       numpy ``pack_rows`` (elementwise_ref and reduce_ref keep their In / Out records, which hold different things, on it).
* seeds, arithmetic    ``seed`` / ``gen`` / ``rng`` (crc32 of the case name), ``exp32``, ``silu``, ``sum32``, ``randn16``; ``device_bound``, ``row_error``.
* refusals             ``PTR``, ``Off``, ``call``, ``host_resolver``, ``device_resolver``, ``check_refusals``, ``refusal_outputs_untouched``.
* fault policy         ``device_guard``, ``launch_twice``: a refusal by the argument checks fails its own case, any other error ends the
                       session, so that nothing more is started on a device that has just reported a fault.
* (b) / (c) / (d)      ``check_written``.

tests/test_domain_kit_host.py checks on the CPU that these assertions fire.  DESIGN.md section 3i has the file map and the numbers."""
from __future__ import annotations

import contextlib
import ctypes
import re
import zlib
from typing import NamedTuple, Optional

import numpy as np
import torch

from coma_amd import _abi, _lib
from coma_amd._lib import ComaHipError

F16, F32, F64 = torch.float16, torch.float32, torch.float64
GUARD = 256                      # NaN (operands) / sentinel (outputs) elements in front of and behind every buffer
FLOOR = 2.0 ** -10               # one fp16 ulp of a row's largest value
U32 = 2.0 ** -24                 # unit roundoff of fp32
COMA_E_INVALID = _abi.DEFINES["COMA_E_INVALID"]
# what outputs are prefilled with: quiet NaNs with a payload no kernel produces for the floats, 0xA5 bytes for the integers
SENTINELS = {"f2": 0x7E5A, "f4": 0x7FC5A5A5, "f8": 0x7FF8A5A5A5A5A5A5, "i1": 0xA5, "i4": 0xA5A5A5A5, "i8": 0xA5A5A5A5A5A5A5A5}


# ------------------------------------------------------------------------------------------------------------------ buffers
def bits(t):
    """The bit patterns of a float tensor / array as integers of its width (torch: signed, numpy: unsigned); integers pass through."""
    if isinstance(t, torch.Tensor):
        return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]) if t.dtype.is_floating_point else t
    a = np.ascontiguousarray(t)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def sentinel_bits(dtype):
    """The sentinel of a torch or numpy dtype as the integer bits() shows."""
    return int(bits(sentinel(1, dtype))[0])


def sentinel(n, dtype):
    """n elements of the sentinel: a torch tensor for a torch dtype, a numpy array for a numpy one"""
    dt = torch.empty(0, dtype=dtype).numpy().dtype if isinstance(dtype, torch.dtype) else np.dtype(dtype)
    a = np.full(n, SENTINELS[("f" if dt.kind == "f" else "i") + str(dt.itemsize)], dtype=f"u{dt.itemsize}").view(dt)
    return torch.from_numpy(a) if isinstance(dtype, torch.dtype) else a


def guarded(body, fill=None, guard=GUARD):
    """body flattened between two guards: NaN for floats, `fill` (default -1, 0xA5 for bytes) for integers."""
    body = body.contiguous().reshape(-1)
    if fill is None:
        fill = float("nan") if body.dtype.is_floating_point else (0xA5 if body.dtype == torch.uint8 else -1)
    g = torch.full((guard,), fill, dtype=body.dtype)
    return torch.cat([g, body, g])


def guards_intact(flat, fill=None, guard=GUARD):
    """Both guards of a buffer built by guarded() still hold their fill, bit for bit."""
    g = guarded(flat.new_zeros(0), fill, guard)
    return torch.equal(bits(flat[:guard]), bits(g[:guard])) and torch.equal(bits(flat[-guard:]), bits(g[guard:]))


class Operand(NamedTuple):
    t: torch.Tensor             # [rows, width], fp16 or fp32
    ld: int
    off: int = 0                # extra NaN elements between the front guard and the data (a pointer moved off its alignment)


class Out(NamedTuple):
    rows: int
    width: int
    ld: int
    dtype: torch.dtype
    must: Optional[int] = None  # flat outputs (rows == 1): the first `must` elements have to be written, the others up to `width` may be


def pack(op: Operand):
    """guard | off | rows x ld with NaN gap columns | guard, everything outside the data NaN"""
    r, wd = op.t.shape
    buf = torch.full((GUARD + op.off + r * op.ld + GUARD,), float("nan"), dtype=op.t.dtype)
    buf[GUARD + op.off:GUARD + op.off + r * op.ld].view(r, op.ld)[:, :wd] = op.t
    return buf


def pack_rows(body, poison, ld=None, off=0):
    """The numpy flavour of pack: body [rows, width] (or flat) -> guard | off | rows x ld | guard, everything outside the data `poison`"""
    body = np.atleast_2d(np.ascontiguousarray(body))
    r, w = body.shape
    ld = w if ld is None else ld
    buf = np.full(GUARD + off + r * ld + GUARD, poison, dtype=body.dtype)
    buf[GUARD + off:GUARD + off + r * ld].reshape(r, ld)[:, :w] = body
    return buf


def new_out(o: Out):
    return sentinel(GUARD + o.rows * o.ld + GUARD, o.dtype)


def masks(o: Out):
    """(must, may): elements of new_out(o) the launch has to write / is allowed to write"""
    may = torch.zeros(GUARD + o.rows * o.ld + GUARD, dtype=torch.bool)
    may[GUARD:GUARD + o.rows * o.ld].view(o.rows, o.ld)[:, :o.width] = True
    if o.must is None:
        return may, may
    must = torch.zeros_like(may)
    must[GUARD:GUARD + o.must] = True
    return must, may


def body(o: Out, buf):
    return buf[GUARD:GUARD + o.rows * o.ld].view(o.rows, o.ld)[:, :o.width]


# ------------------------------------------------------------------------------------------------------------------ seeds, exact arithmetic
def seed(name, salt=0):
    return zlib.crc32(name.encode()) + salt


def gen(name, salt=0):
    return torch.Generator().manual_seed(seed(name, salt))


def rng(name, salt=0):
    return np.random.default_rng(seed(name, salt))


def randn16(g, *shape, scale=1.0, shift=0.0):
    return (torch.randn(*shape, generator=g) * scale + shift).to(F16)


def exp32(v):
    """a correctly rounded fp32 exp of a torch tensor or numpy array, whatever the host's vector library does"""
    return torch.exp(v.to(F64)).to(F32) if isinstance(v, torch.Tensor) else np.exp(v.astype(np.float64)).astype(np.float32)


def silu(v):
    """SiLU of fp32 or float64 `v` in its own precision, the exponential exact."""
    return v / (1 + (torch.exp(-v) if v.dtype == F64 else exp32(-v)))


def sum32(t, dim=-1):
    """fp32 sum along `dim`, one addition after the other in index order (numpy's accumulate is a sequential fp32 loop;
    tests/test_norm_ref_host.py checks that against a Python loop)."""
    a = np.ascontiguousarray(t.to(F32).movedim(dim, -1).numpy())
    return torch.from_numpy(np.add.accumulate(a, axis=-1, dtype=np.float32)[..., -1].copy())


# ------------------------------------------------------------------------------------------------------------------ the bound
def row_error(got, ref):
    """max over an output row of |got - ref| / max |ref| of that row -> [R].  A row whose reference is zero throughout (planes of an
    upsampled image, where B^T d B subtracts a pixel from its own copy) has to be reproduced exactly: 0 if it is, inf if not."""
    num, den = (got.to(F64) - ref).abs().amax(-1), ref.abs().amax(-1)
    exact = torch.where(num > 0, torch.full_like(num, float("inf")), torch.zeros_like(num))
    return torch.where(den > 0, num / den.clamp(min=1e-300), torch.where(num.isnan(), num, exact))


def device_bound(e_emu, floor=FLOOR):
    """Four times the emulation's own error, never below the floor: one fp16 ulp of the row's largest value."""
    return max(4.0 * e_emu, floor)


# ------------------------------------------------------------------------------------------------------------------ refusals
class _Ptr:
    def __repr__(self):
        return "PTR"


PTR = _Ptr()        # "a valid non-null pointer": the tests put a dummy address (CPU) or a small device buffer (GPU) here


class Off(NamedTuple):
    """a valid pointer moved by `bytes`"""
    bytes: int


def call(lib, entry, kw, resolve):
    """entry(**kw, stream = NULL) through the ctypes library, the keywords in the order of the header's own parameter names
    (_lib.PARAMS); resolve(name) -> the address to put where kw says PTR; Off(b) is that address + b"""
    *names, last = _lib.PARAMS[entry]
    assert last == "stream", entry
    args = []
    for name in names:
        v = kw[name]
        args.append(resolve(name) if v is PTR else resolve(name) + v.bytes if isinstance(v, Off) else v)
    return getattr(lib, entry)(*args, None)


def _with_host_args(resolve, host_args):
    """Arguments an entry point reads on the host (principle_vec) get real host memory: the unit vector (0, 0, 1)."""
    vec = (ctypes.c_float * 3)(0.0, 0.0, 1.0)
    out = lambda name: ctypes.addressof(vec) if name in host_args else resolve(name)
    out.keep = vec
    return out


def host_resolver(host_args=()):
    """PTR -> a dummy address that is never dereferenced; on a machine with a device, small real buffers instead"""
    if not torch.cuda.is_available():
        return _with_host_args(lambda name: 0x7000000000 + 0x1000 * (sum(name.encode()) % 251), host_args)
    keep = {}
    return _with_host_args(lambda name: keep.setdefault(name, torch.zeros(1 << 16, dtype=F32, device="cuda")).data_ptr(), host_args)


def device_resolver(output_args, host_args=(), device="cuda:0"):
    """-> (resolve, outs, small): PTR -> a sentinel-filled device buffer of its own for every output argument, one zero buffer for all
    operands; refusal_outputs_untouched(outs, small) is the check after the rows"""
    small = torch.zeros(1 << 16, dtype=F32, device=device)
    outs = {name: sentinel(1 << 16, F32).to(device) for name in output_args}
    return _with_host_args(lambda name: (outs[name] if name in outs else small).data_ptr(), host_args), outs, small


def check_refusals(lib, refusals, resolve, *, expect_control):
    """Every row of `refusals` (entry point -> (accepted base, [(text, change), ...])) through the real entry point: the code and the text.
    expect_control (a machine without a device): the base row passes every argument check and only fails where the launch needs a
    device.  -> the number of rows"""
    n = 0
    for entry, (base, rows) in sorted(refusals.items()):
        for text, change in rows:
            rc = call(lib, entry, {**base, **change}, resolve)
            msg = lib.coma_last_error().decode()
            if rc == 0 and torch.cuda.is_available():           # wrongly accepted and launched: let it finish before the case fails
                torch.cuda.synchronize()
            assert rc == COMA_E_INVALID and re.search(re.escape(entry) + ": .*" + re.escape(text), msg), (entry, change, rc, msg)
            n += 1
        if expect_control:
            rc = call(lib, entry, dict(base), resolve)
            assert rc not in (0, COMA_E_INVALID), (entry, rc, lib.coma_last_error().decode())
    assert n == sum(len(rows) for _, rows in refusals.values())
    return n


def refusal_outputs_untouched(outs, small):
    """After the refused rows: every output buffer of device_resolver still holds its sentinel, the operand buffer is still zero."""
    torch.cuda.synchronize()
    for name, buf in outs.items():
        assert bool((bits(buf.cpu()) == sentinel_bits(buf.dtype)).all()), name
    assert not bool(small.cpu().any())


# ------------------------------------------------------------------------------------------------------------------ fault policy
@contextlib.contextmanager
def device_guard(what):
    """The launches of one case, and the synchronize behind them.  A refusal by the argument checks fails its own case; any other error
    ends the session: nothing more is started on the device."""
    import pytest
    try:
        yield
        torch.cuda.synchronize()
    except Exception as e:
        if isinstance(e, ComaHipError) and f"failed ({COMA_E_INVALID})" in str(e):
            raise
        pytest.exit(f"{what}: {type(e).__name__}: {e}", returncode=3)


def launch_twice(make_outputs, launch, what):
    """Two launches of a case, each into the fresh outputs make_outputs() gives, then ONE synchronize -> the two sets of outputs."""
    both = []
    with device_guard(what):
        for _ in range(2):
            bufs = make_outputs()
            launch(bufs)
            both.append(bufs)
    return both


# ------------------------------------------------------------------------------------------------------------------ (b), (c), (d)
def check_written(name, first, second, start, must, may, finite=True):
    """One output after two launches, as host tensors with their guards: `first` and `second` what the launches left, `start` what both
    began as (the sentinel; for an operand written in place, its data between sentinel guards), `must` / `may` the elements the launch
    has to write / is allowed to write.  (b) nothing in `must` is still the sentinel or, with `finite`, NaN / Inf; (c) everything outside
    `may` keeps its first bits; (d) the second launch gives the same bits."""
    b, b0 = bits(first), bits(start)
    if first.dtype != torch.uint8:                              # (every u8 value is a legitimate result: the exact comparison speaks for those)
        assert not bool((b[must] == b0[0]).any()), f"(b) an element the launch owns of `{name}` still holds the sentinel"
    if finite and first.dtype.is_floating_point:
        assert bool(torch.isfinite(first[must]).all()), f"(b) NaN / Inf in what the launch owns of `{name}`"
    assert torch.equal(b[~may], b0[~may]), f"(c) `{name}` was written outside what the contract allows: a guard, a gap column, a foreign slot"
    assert torch.equal(b, bits(second)), f"(d) the second launch differs in `{name}`"
