"""The four direct 3x3 convolution entry points of coma_amd/csrc/sd_haloconv.hip and sd_smallconv.hip (sd_conv3x3_halo_f16,
sd_conv3x3_small_n_f16, sd_conv3x3_c3_f16, sd_im2col3x3_c3_f16) over the domain their argument checks accept.  The table is
tests/dconv_ref.CASES; tests/test_dconv_ref_host.py checks on the CPU that it reaches every branch of the kernels.

Per case: (a) every element of the fp16 output is within the case's bound of the float64 reference, the error normalised by the largest
|ref| of the element's output row (a pixel's n channels; for small_n, whose pixels hold at most four values, the sample); the bound is
max(4 * e_emu, 2^-10), e_emu being what the kernel's formula in fp32 with fp16 storage, emulated on the CPU, loses on the same case
(DESIGN.md section 3f lists it beside the measured device error).  Channels n .. 7 of a small_n pixel are +0 and im2col equals the gather
bit for bit, columns 27 .. 31 +0.  The column sums have a counted bound: a slot is 256 stored values added in some fixed order, so each
entry lies within 1.001 * 2^-16 of the sum of magnitudes (squares) of the float64 sums of the device's own stored output for that tile,
slot index (sample, tile row, tile column), global column index.  (b) nothing the launch owns is NaN / Inf or still the sentinel;
(c) every guard, every gap column n .. ldo - 1, channels >= 8 of a small_n pixel and the slots behind the last tile keep the sentinel bit
for bit; (d) a second launch into fresh buffers gives the same bits, colstats included.  Every operand element the contract says is not
read is NaN (guards, res's gap columns, channels 3 .. ldx - 1 of the 3-channel image, rows of w and entries of bias at and beyond n for
small_n), so a read outside the contract poisons (a) or (b).  Every case is inside the accepted domain; one synchronize per case."""
import re

import pytest
import torch

from coma_amd._lib import ComaHipError
from tests import dconv_ref as dr
from tests import norm_ref as nr

COMA_E_INVALID = -1
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16, F32, F64 = torch.float16, torch.float32, torch.float64
G = nr.GUARD


@pytest.fixture(scope="module")
def ops(hip_lib):
    assert torch.cuda.is_available()
    from coma_amd.sd import ops
    return ops


def launch_twice(ops, c, dev, outs):
    """Two launches of the case, each into fresh sentinel-filled outputs, then ONE synchronize -> two dicts name -> flat device buffer
    (guards included).  A refusal by the argument checks fails its own case; any other error ends the session: nothing more is started
    on the device."""
    both = []
    try:
        for _ in range(2):
            bufs = {name: nr.new_out(o).to(DEV) for name, o in outs.items()}
            dr.launch(ops, c, {**dev, **{name: buf[G:] for name, buf in bufs.items()}})
            both.append(bufs)
        torch.cuda.synchronize()
    except Exception as e:
        if isinstance(e, ComaHipError) and f"failed ({COMA_E_INVALID})" in str(e):
            raise
        pytest.exit(f"{c.id}: {type(e).__name__}: {e}", returncode=3)
    return both


@pytest.mark.parametrize("case", dr.CASES, ids=lambda c: c.id)
def test_dconv_domain(ops, case):
    c = case
    y = dr.yardstick(c)
    r = dr.results(c)["out"]
    inp, outs = dr.inputs(c), dr.outputs(c)
    dev = {k: nr.pack(op).to(DEV)[G:] for k, op in inp.items()}
    first, second = launch_twice(ops, c, dev, outs)

    host = {}
    for name, o in outs.items():
        buf, sent = first[name].cpu(), nr.sentinel_bits(o.dtype)
        must, may = nr.masks(o)
        assert bool(torch.isfinite(buf[must].float()).all()), f"(b) NaN / Inf (or an unwritten element) in what the launch owns of `{name}`"
        assert bool((nr.bits(buf)[~may] == sent).all()), f"(c) a guard or gap column of `{name}` was written"
        assert torch.equal(nr.bits(buf), nr.bits(second[name].cpu())), f"(d) the second launch differs in `{name}`"
        host[name] = buf
    got = nr.body(outs["out"], host["out"])
    if isinstance(c, dr.IC):
        assert torch.equal(nr.bits(got.contiguous()), nr.bits(r.emu)), "im2col differs from the gather (columns 27 .. 31: +0)"
    if isinstance(c, dr.SN):
        assert not bool(nr.bits(got[:, c.n:].contiguous()).any()), "channels n .. 7 of a small_n pixel must be +0"
    err = dr.row_error(c, got, r.ref).nan_to_num(nan=float("inf"))
    device, worst = float(err.max()), int(err.argmax())
    print(f"DCONV_DOMAIN {c.id} family={c.family} e_emu={y.e_emu:.3e} bound={y.bound:.3e} device={device:.3e}")
    assert device <= y.bound, f"(a) row error {device:.3e} > {y.bound:.3e} (e_emu {y.e_emu:.3e}) at row {worst} of `out`"
    if "colstats" in outs:
        sums, squares, mags = dr.colstats_expected(c, host["out"])
        cs = nr.body(outs["colstats"], host["colstats"]).view(-1, 2, c.n).to(F64)
        ds, dq = (cs[:, 0] - sums).abs() / mags.clamp(min=1e-300), (cs[:, 1] - squares).abs() / squares.clamp(min=1e-300)
        print(f"DCONV_COLSTATS {c.id} sums={float(ds.max()) / dr.COLSTATS_REL:.3f} squares={float(dq.max()) / dr.COLSTATS_REL:.3f} of the counted bound")
        assert bool((ds <= dr.COLSTATS_REL).all()), f"colstats: column sums, slot {int(ds.amax(1).argmax())}"
        assert bool((dq <= dr.COLSTATS_REL).all()), f"colstats: sums of squares, slot {int(dq.amax(1).argmax())}"


def test_refusals_are_reported_not_launched(ops, hip_lib):
    """Every row of dconv_ref.REFUSALS through the real entry points, with small device buffers where the row wants a pointer: the code
    and the text, and every output buffer keeps its sentinel.  tests/test_dconv_ref_host.py has put the same rows to the same entry points
    on the CPU, where a wrongly accepted row cannot launch."""
    small = torch.zeros(1 << 16, dtype=F32, device=DEV)
    outs = {name: nr.sentinel(1 << 16, F32).to(DEV) for name in dr.OUTPUT_ARGS}
    resolve = lambda name: (outs[name] if name in outs else small).data_ptr()
    n = 0
    for entry, (base, rows) in sorted(dr.REFUSALS.items()):
        for text, change in rows:
            rc = dr.call(hip_lib, entry, {**base, **change}, resolve)
            msg = hip_lib.coma_last_error().decode()
            assert rc == COMA_E_INVALID and re.search(re.escape(entry) + ": .*" + re.escape(text), msg), (entry, change, rc, msg)
            n += 1
    assert n == sum(len(rows) for _, rows in dr.REFUSALS.values()) and n > 60
    torch.cuda.synchronize()
    for name, buf in outs.items():
        assert bool((nr.bits(buf.cpu()) == nr.SENTINEL_BITS32).all()), name
    assert not bool(small.cpu().any())
