"""The ten entry points of coma_amd/csrc/reduce.hip, nearest.hip, normals.hip and triangulate.hip (coma_contact_map_f32, coma_entropy_f32,
coma_significant_pairs_u8, coma_masked_max_f32, coma_row_argmax_i64, coma_contact_select_u8, coma_nearest_vertex_i64,
coma_vertex_normals_f64, coma_dlt_score_f64, coma_ransac_mse_f64) through the C ABI over the domain their argument checks accept.  The
table is tests/reduce_ref.CASES; tests/test_reduce_ref_host.py checks on the CPU that it reaches every regime and that a broken kernel
fails it.

Per case: (a) reduce_ref.check -- the exact contracts (the masks, the masked maximum, argmax index and value, contact_select, the nearest
vertex, the vertex normals, ransac's counts against the device's own mse) bit for bit, NaN-ness compared for NaNs, and the arithmetic
results (normalised prob, contact, score, tri, the mses) within max(4 * e_emu, floor) of the float64 / longdouble reference, e_emu being
what the kernel's own formula and summation shape, emulated on the CPU, loses on the same case (DESIGN.md section 3h lists it beside the
measured device error); (b) everything the contract says is written is free of the sentinel and, where the case is finite, of NaN / Inf;
(c) guards, rows past M and outputs the call was told not to write (contact = NULL, idx / val = NULL, P = 0, C = 0) keep their first
bits; (d) a second launch into fresh buffers gives the same bits.  Float operands sit between NaN guards and everything the contract
says is not read is NaN (contact outside the mask, a row outside [col_offset, col_offset + n)), so a read outside the contract fails (a)
or (b).  Every case is inside the accepted domain; two launches and one synchronize per case."""
import ctypes
import re

import numpy as np
import pytest
import torch

from tests import reduce_ref as rr

COMA_E_INVALID = -1
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = rr.GUARD


def _upload(buf):
    return torch.from_numpy(np.ascontiguousarray(buf)).to(DEV)


def _body_ptr(t):
    return t.data_ptr() + G * t.element_size()


def launch_twice(lib, c, ins, outs):
    """Two launches of the case, each into fresh outputs, then ONE synchronize -> two dicts name -> device buffer (guards included).
    A refusal by the argument checks fails its own case; any other error ends the session: nothing more is started on the device."""
    both = []
    try:
        for _ in range(2):
            bufs = {name: _upload(rr.pack(o.init, rr.SENTINEL[o.init.dtype])) for name, o in outs.items()}
            rc = rr.launch(lib, c, {**{k: _body_ptr(t) for k, t in ins.items()}, **{k: _body_ptr(t) for k, t in bufs.items()}})
            if rc != 0:
                msg = lib.coma_last_error().decode()
                if rc == COMA_E_INVALID:
                    pytest.fail(f"{c.id}: refused inside the accepted domain: {msg}")
                raise RuntimeError(f"{c.entry} returned {rc}: {msg}")
            both.append(bufs)
        torch.cuda.synchronize()
    except Exception as e:
        pytest.exit(f"{c.id}: {type(e).__name__}: {e}", returncode=3)
    return both


@pytest.mark.parametrize("case", rr.CASES, ids=lambda c: c.id)
def test_small_domain(hip_lib, case):
    c = case
    assert torch.cuda.is_available()
    pins, outs = rr.plan(c)
    ins = {k: _upload(rr.pack(i.body, i.poison)) for k, i in pins.items()}
    first, second = launch_twice(hip_lib, c, ins, outs)

    got = {}
    for name, o in outs.items():
        buf, again = first[name].cpu().numpy(), second[name].cpu().numpy()
        start = rr.pack(o.init, rr.SENTINEL[o.init.dtype])
        assert np.array_equal(rr.bits(buf[:G]), rr.bits(start[:G])) and np.array_equal(rr.bits(buf[-G:]), rr.bits(start[-G:])), f"(c) a guard of `{name}` was written"
        assert np.array_equal(rr.bits(buf), rr.bits(again)), f"(d) the second launch differs in `{name}`"
        got[name] = buf[G:-G]
    for k, i in pins.items():                                   # operands come back as they went in
        assert np.array_equal(rr.bits(ins[k].cpu().numpy()), rr.bits(rr.pack(i.body, i.poison))), f"operand `{k}` was written"
    fig = rr.check(c, got)                                      # (a), (b), and (c) inside the bodies
    for name, f in fig.items():
        print(f"SMALL_DOMAIN {c.id} entry={c.entry} out={name} e_emu={f.e_emu:.3e} bound={f.bound:.3e} device={f.err:.3e}")
    exact = sorted(set(outs) - set(fig))
    if exact:
        print(f"SMALL_DOMAIN {c.id} entry={c.entry} out={','.join(exact)} exact")


def test_refusals_are_reported_not_launched(hip_lib):
    """Every row of reduce_ref.REFUSALS through the real entry points, with small device buffers where the row wants a pointer: the code
    and the text, and every output buffer keeps its sentinel.  tests/test_reduce_ref_host.py has put the same rows to the same entry points
    on the CPU, where a wrongly accepted row cannot launch."""
    assert torch.cuda.is_available()
    small = torch.zeros(1 << 16, dtype=torch.float32, device=DEV)
    start = rr.sentinel(1 << 16, np.float32)
    outs = {name: _upload(start) for name in rr.OUTPUT_ARGS}
    vec = (ctypes.c_float * 3)(0.0, 0.0, 1.0)                   # principle_vec is read on the host
    resolve = lambda name: ctypes.addressof(vec) if name in rr.HOST_ARGS else (outs[name] if name in outs else small).data_ptr()
    n = 0
    for entry, (base, rows) in sorted(rr.REFUSALS.items()):
        for text, change in rows:
            rc = rr.call(hip_lib, entry, {**base, **change}, resolve)
            msg = hip_lib.coma_last_error().decode()
            assert rc == COMA_E_INVALID and re.search(re.escape(entry) + ": .*" + re.escape(text), msg), (entry, change, rc, msg)
            n += 1
    assert n == sum(len(rows) for _, rows in rr.REFUSALS.values()) and n >= 80
    torch.cuda.synchronize()
    for name, buf in outs.items():
        assert np.array_equal(rr.bits(buf.cpu().numpy()), rr.bits(start)), name
    assert not bool(small.cpu().any())
