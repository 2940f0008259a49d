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
import numpy as np
import pytest
import torch

from tests import domain_kit as kit
from tests import reduce_ref as rr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = kit.GUARD


def _upload(buf):
    return torch.from_numpy(np.ascontiguousarray(buf)).to(DEV)


def _body_ptr(t):
    return t.data_ptr() + G * t.element_size()


def launch_twice(lib, c, ins, outs):
    """Two launches of the case through the C ABI, each into fresh outputs -> two dicts name -> device buffer (guards included).  The fault
    policy is the kit's: here a refusal is a return code, which fails the case; any other code ends the session."""
    def launch(bufs):
        rc = rr.launch(lib, c, {**{k: _body_ptr(t) for k, t in ins.items()}, **{k: _body_ptr(t) for k, t in bufs.items()}})
        if rc == kit.COMA_E_INVALID:
            pytest.fail(f"{c.id}: refused inside the accepted domain: {lib.coma_last_error().decode()}")
        if rc != 0:
            raise RuntimeError(f"{c.entry} returned {rc}: {lib.coma_last_error().decode()}")

    return kit.launch_twice(lambda: {name: _upload(rr.pack(o.init, rr.SENTINEL[o.init.dtype])) for name, o in outs.items()}, launch, c.id)


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
        assert np.array_equal(kit.bits(buf[:G]), kit.bits(start[:G])) and np.array_equal(kit.bits(buf[-G:]), kit.bits(start[-G:])), f"(c) a guard of `{name}` was written"
        assert np.array_equal(kit.bits(buf), kit.bits(again)), f"(d) the second launch differs in `{name}`"
        got[name] = buf[G:-G]
    for k, i in pins.items():                                   # operands come back as they went in
        assert np.array_equal(kit.bits(ins[k].cpu().numpy()), kit.bits(rr.pack(i.body, i.poison))), f"operand `{k}` was written"
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
    resolve, outs, small = kit.device_resolver(rr.OUTPUT_ARGS, rr.HOST_ARGS)
    assert kit.check_refusals(hip_lib, rr.REFUSALS, resolve, expect_control=False) >= 80
    kit.refusal_outputs_untouched(outs, small)
