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
import pytest
import torch

from tests import dconv_ref as dr
from tests import domain_kit as kit

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16, F32, F64 = torch.float16, torch.float32, torch.float64
G = kit.GUARD


@pytest.fixture(scope="module")
def ops(hip_lib):
    assert torch.cuda.is_available()
    from coma_amd.sd import ops
    return ops


@pytest.mark.parametrize("case", dr.CASES, ids=lambda c: c.id)
def test_dconv_domain(ops, case):
    c = case
    y = dr.yardstick(c)
    r = dr.results(c)["out"]
    inp, outs = dr.inputs(c), dr.outputs(c)
    dev = {k: kit.pack(op).to(DEV)[G:] for k, op in inp.items()}
    first, second = kit.launch_twice(lambda: {name: kit.new_out(o).to(DEV) for name, o in outs.items()},        # flat, guards included
                                     lambda bufs: dr.launch(ops, c, {**dev, **{name: buf[G:] for name, buf in bufs.items()}}), c.id)

    host = {}
    for name, o in outs.items():
        host[name] = first[name].cpu()
        kit.check_written(name, host[name], second[name].cpu(), kit.new_out(o), *kit.masks(o))
    got = kit.body(outs["out"], host["out"])
    if isinstance(c, dr.IC):
        assert torch.equal(kit.bits(got.contiguous()), kit.bits(r.emu)), "im2col differs from the gather (columns 27 .. 31: +0)"
    if isinstance(c, dr.SN):
        assert not bool(kit.bits(got[:, c.n:].contiguous()).any()), "channels n .. 7 of a small_n pixel must be +0"
    err = dr.row_error(c, got, r.ref).nan_to_num(nan=float("inf"))
    device, worst = float(err.max()), int(err.argmax())
    print(f"DCONV_DOMAIN {c.id} family={c.family} e_emu={y.e_emu:.3e} bound={y.bound:.3e} device={device:.3e}")
    assert device <= y.bound, f"(a) row error {device:.3e} > {y.bound:.3e} (e_emu {y.e_emu:.3e}) at row {worst} of `out`"
    if "colstats" in outs:
        sums, squares, mags = dr.colstats_expected(c, host["out"])
        cs = kit.body(outs["colstats"], host["colstats"]).view(-1, 2, c.n).to(F64)
        ds, dq = (cs[:, 0] - sums).abs() / mags.clamp(min=1e-300), (cs[:, 1] - squares).abs() / squares.clamp(min=1e-300)
        print(f"DCONV_COLSTATS {c.id} sums={float(ds.max()) / dr.COLSTATS_REL:.3f} squares={float(dq.max()) / dr.COLSTATS_REL:.3f} of the counted bound")
        assert bool((ds <= dr.COLSTATS_REL).all()), f"colstats: column sums, slot {int(ds.amax(1).argmax())}"
        assert bool((dq <= dr.COLSTATS_REL).all()), f"colstats: sums of squares, slot {int(dq.amax(1).argmax())}"


def test_refusals_are_reported_not_launched(ops, hip_lib):
    """Every row of dconv_ref.REFUSALS through the real entry points, with small device buffers where the row wants a pointer: the code
    and the text, and every output buffer keeps its sentinel.  tests/test_dconv_ref_host.py has put the same rows to the same entry points
    on the CPU, where a wrongly accepted row cannot launch."""
    resolve, outs, small = kit.device_resolver(dr.OUTPUT_ARGS)
    assert kit.check_refusals(hip_lib, dr.REFUSALS, resolve, expect_control=False) > 60
    kit.refusal_outputs_untouched(outs, small)
