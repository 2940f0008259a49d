"""The ten entry points of coma_amd/csrc/sd_norm.hip and sd_winograd.hip over the whole domain their argument checks accept: both GroupNorm
routes, the column-sum finalize behind its three entry points and slot layouts, the nine LayerNorm instantiations on both sides of their
row thresholds, softmax, the Winograd transforms and both vector widths of the fused GroupNorm + Winograd input kernel.  The table is
tests/norm_ref.CASES; tests/test_norm_ref_host.py checks on the CPU that it reaches every branch.

Per case: (a) every compared element of an fp16 output is within the case's bound of the float64 reference, the error normalised by the
largest |ref| of the element's output row (one pixel's channels, one LayerNorm / softmax row, one tile's row of v); the bound is
max(4 * e_emu, 2^-10), e_emu being what a careful fp32 kernel with fp16 storage, emulated on the CPU, loses on the same case (DESIGN.md
section 3e lists it beside the measured device error).  The fp32 outputs have bounds derived by counting fp32 roundings: an affine table
(scale, shift) element by element within norm_ref.gn_affine's bound, which holds for every summation order (an n-term sum: n - 1 roundings
of 2^-24 of a partial sum, then the formula's own operations); the colstats of winograd_output_cs_kernel against float64 sums of the
device's own stored output, 32 stored values per slot and column in any order: 31 roundings <= 2^-19 of the sum of magnitudes / squares.
(b) nothing the launch owns is NaN / Inf or still the sentinel; (c) every guard and gap column of every output (`stats` is guarded where
batch * C * 2 + batch * ceil(hw / 64) * groups * 2 floats end) keeps the sentinel bit for bit; (d) a second launch into fresh buffers
gives the same bits.  Every operand element the contract says is not read is NaN, so a read outside the contract poisons (a) or (b).
Where include/sd_hip.h promises bit equality it is asserted: mode 0 of sd_gn_winograd_input_f16 against sd_groupnorm_f16 (one-launch route)
-> sd_winograd_input_f16."""
import pytest
import torch

from tests import domain_kit as kit
from tests import norm_ref as nr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16, F32, F64 = torch.float16, torch.float32, torch.float64
G = kit.GUARD


@pytest.fixture(scope="module")
def ops(hip_lib):
    assert torch.cuda.is_available()
    from coma_amd.sd import ops
    return ops


def run(ops, c, dev, outs):
    """The launch of the case into fresh sentinel-filled outputs -> name -> flat device buffer (guards included)."""
    bufs = {}
    for name, o in outs.items():
        buf = kit.new_out(o).to(DEV)
        if isinstance(c, nr.SM):                                 # in place: the data between sentinel gap columns and guards
            buf[G:-G].view(o.rows, o.ld)[:, :o.width] = dev["x_data"]
        bufs[name] = buf
    p = {k: v for k, v in dev.items() if k != "x_data"}
    p.update({name: buf[G:] for name, buf in bufs.items()})
    with kit.device_guard(c.id):
        nr.launch(ops, c, p)
    return bufs


@pytest.mark.parametrize("case", nr.CASES, ids=lambda c: c.id)
def test_norm_domain(ops, case):
    c = case
    y = nr.yardstick(c)
    rows, res = nr.reference_rows(c)
    inp, outs = nr.inputs(c), nr.outputs(c)
    if isinstance(c, nr.SM):
        dev = dict(x_data=inp["x"].t.to(DEV))
    else:
        dev = {k: kit.pack(op).to(DEV)[G + op.off:] for k, op in inp.items()}
    first = run(ops, c, dev, outs)
    second = run(ops, c, dev, outs)

    device = 0.0
    for name, o in outs.items():
        buf = first[name].cpu()
        kit.check_written(name, buf, second[name].cpu(), kit.new_out(o), *kit.masks(o))
        if name not in res:
            continue
        r = res[name]
        got = buf[G:G + o.must].view(-1, 2) if o.must else kit.body(o, buf)        # the table at the start of `stats`, or the whole output
        got = got if rows is None else got[rows]
        if o.dtype == F16:
            err = kit.row_error(got, r.ref).nan_to_num(nan=float("inf"))
            device = float(err.max())
            worst = int(err.argmax())
            print(f"NORM_DOMAIN {c.id} family={c.family} e_emu={y.e_emu:.3e} bound={y.bound:.3e} device={device:.3e}")
            assert device <= y.bound, f"(a) row error {device:.3e} > {y.bound:.3e} (e_emu {y.e_emu:.3e}) at compared row {worst} of `{name}`"
        else:                                                   # the affine table: (scale, shift) per (sample, channel)
            over = ((got.to(F64) - r.ref).abs() / r.stated).nan_to_num(nan=float("inf"))
            rel = float(((got.to(F64) - r.ref).abs() / r.ref.abs().amax()).max())
            print(f"NORM_DOMAIN {c.id} family={c.family}-table device/stated={float(over.max()):.3e} device={rel:.3e} (of the largest entry)")
            assert float(over.max()) <= 1.0, f"(a) table entry {divmod(int(over.argmax()), 2)} is {float(over.max()):.3e} of its fp32 bound"
    if isinstance(c, nr.WO) and c.cs:
        sums, squares, mags = nr.colstats_expected(c, first["out"].cpu())
        body = kit.body(outs["colstats"], first["colstats"]).cpu().view(-1, 2, c.n).to(F64)
        # 32 fp32 additions in any order: 31 roundings of at most 2^-24 of a partial sum <= 2^-19 of the sum of magnitudes
        assert bool(((body[:, 0] - sums).abs() <= 2.0 ** -19 * mags).all()), "colstats: column sums"
        assert bool(((body[:, 1] - squares).abs() <= 2.0 ** -19 * squares).all()), "colstats: sums of squares"
    if isinstance(c, nr.GW) and c.mode == 0:
        # sd_hip.h: every output bit equals sd_groupnorm_f16 (one launch, same statistics order) -> sd_winograd_input_f16
        assert nr.groupnorm_route(c.c0, c.c1, c.h * c.w, c.G) == "gn_small_kernel"
        n1 = torch.empty(c.B * c.h * c.w, c.C, dtype=F16, device=DEV)
        stats = torch.empty(ops.gn_scratch_floats(c.B, c.h * c.w, c.G, c.C), dtype=F32, device=DEV)
        v2 = torch.empty(16 * c.B * c.h * c.w // 4, c.C, dtype=F16, device=DEV)
        with kit.device_guard(c.id + " (unfused GroupNorm)"):
            ops.groupnorm(dev["x0"], dev["gamma"], dev["beta"], n1, stats, batch=c.B, hw=c.h * c.w, c0=c.c0, x1=dev.get("x1"), c1=c.c1, groups=c.G,
                          eps=c.eps, silu=bool(c.silu))
        with kit.device_guard(c.id + " (unfused input transform)"):
            ops.winograd_input(n1, v2, batch=c.B, h=c.h, w=c.w, c0=c.C)
        assert torch.equal(kit.bits(kit.body(outs["v"], first["v"])), kit.bits(v2)), "mode 0 differs from sd_groupnorm_f16 -> sd_winograd_input_f16"


def test_refusals_are_reported_not_launched(ops, hip_lib):
    """Every row of norm_ref.REFUSALS through the real entry points, with small device buffers where the row wants a pointer: the code and
    the text, and every output buffer keeps its sentinel.  tests/test_norm_ref_host.py has put the same rows to the same entry points on
    the CPU, where a wrongly accepted row cannot launch."""
    resolve, outs, small = kit.device_resolver(nr.OUTPUT_ARGS)
    assert kit.check_refusals(hip_lib, nr.REFUSALS, resolve, expect_control=False) > 120
    kit.refusal_outputs_untouched(outs, small)
