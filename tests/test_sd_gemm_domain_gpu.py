"""sd_conv_gemm_f16 (coma_amd/csrc/sd_gemm.hip) over the whole domain its entry point accepts: every instantiation the dispatch can produce,
ragged rows and columns, leading dimensions with gaps, every gather form, every epilogue, z-batching, split-K, colstats, the sub-pixel
phases and out_t.  The table is tests/gemm_ref.CASES; tests/test_gemm_ref_host.py checks on the CPU that each row reaches the kernel it
names.

Per case: (a) every compared element is within the case's bound of the float64 reference, the error normalised by the largest |ref| of the
element's output row; the bound is max(4 * e_emu, 2^-10), e_emu being what a careful fp16 kernel emulated on the CPU loses on the same case
(DESIGN.md section 3c lists it beside the measured device error); (b) nothing the kernel had to write is NaN / Inf or still the sentinel;
(c) every gap column, guard, foreign parity and inter-problem gap of `out` / `out_t` / `colstats` keeps the sentinel bit for bit, and
colstats holds the column sums of the device's own stored output; (d) a second launch into fresh buffers gives the same bits.  Every operand
element the contract says is not read is NaN (guards in front of and behind each operand, gap columns, gaps between z-batched problems, the
whole workspace), so a read outside the contract poisons (a) or (b)."""
import pytest
import torch

from coma_amd._lib import ComaHipError
from tests import domain_kit as kit
from tests import gemm_ref as gr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16, F64 = torch.float16, torch.float64
G = kit.GUARD


@pytest.fixture(scope="module")
def ops(hip_lib):
    assert torch.cuda.is_available()
    from coma_amd.sd import ops
    return ops


def run(ops, c, dev):
    """All launches of the case into fresh sentinel-filled outputs and a fresh NaN workspace -> (out, out_t, colstats, workspace) on the CPU."""
    out = gr.new_out(c).to(DEV)
    out_t = gr.new_out_t(c).to(DEV) if c.out_t else None
    cs = gr.new_colstats(c).to(DEV) if c.colstats else None
    ws = gr.new_workspace(c).to(DEV) if c.ws_slabs else None
    ptr = dict(dev, out=out[G:], out_t=None if out_t is None else out_t[G:], colstats=None if cs is None else cs[G:],
               workspace=None if ws is None else ws[G:])
    with kit.device_guard(c.id):
        for launch in range(max(1, len(c.phases))):
            ops.conv_gemm(ptr["a0"], dev["w"][launch], ptr["out"], **gr.launch_kwargs(c, ptr, launch))
    return tuple(None if t is None else t.cpu() for t in (out, out_t, cs, ws))


@pytest.mark.parametrize("case", gr.CASES, ids=lambda c: c.id)
def test_conv_gemm_domain(ops, case):
    c = case
    y = gr.yardstick(c)
    pk = gr.pack(c, gr.make_inputs(c))
    dev = {k: (None if v is None else v.to(DEV)[G:]) for k, v in pk._asdict().items() if k != "w"}
    dev["w"] = tuple(w.to(DEV)[G:] for w in pk.w)
    out, out_t, cs, ws = run(ops, c, dev)
    out2, out_t2, cs2, _ = run(ops, c, dev)

    prow = y.rows                                               # rows of `out` compared (a phase case: pixels of the upsampled image)
    got = gr.out_values(c, out, prow)
    if c.out_t:
        got = torch.cat([got, gr.out_t_values(c, out_t, prow)[None]], -1)
    err = gr.row_error(got, y.ref, y.cols, c.out_t[0] if c.out_t else None)
    device = float(err.nan_to_num(nan=float("inf")).max())
    print(f"GEMM_DOMAIN {c.id} family={c.pool} e_emu={y.e_emu:.3e} bound={y.bound:.3e} device={device:.3e}")

    mask = gr.written_mask(c)                                   # (outside it: gap columns, guards, foreign parity, inter-problem gaps)
    kit.check_written("out", out, out2, gr.new_out(c), mask, mask)
    if c.out_t:
        mt = gr.out_t_written_mask(c)
        kit.check_written("out_t", out_t, out_t2, gr.new_out_t(c), mt, mt)
    if c.ws_slabs:
        assert bool(ws[:G].isnan().all()) and bool(ws[-G:].isnan().all()), "(c) the workspace was written outside its workspace_bytes"
    if c.colstats:
        slots, sums, squares, mags = gr.colstats_expected(c, out)
        body = cs[G:-G].view(gr.colstats_slots(c), 2, c.n)
        mine = torch.zeros(cs.numel(), dtype=torch.bool)        # (outside it: the slots of another phase and the guards)
        mine[G:-G].view(gr.colstats_slots(c), 2 * c.n)[slots] = True
        kit.check_written("colstats", cs, cs2, gr.new_colstats(c), mine, mine)
        gs, gq = body[slots, 0].to(F64), body[slots, 1].to(F64)
        # 32 fp32 additions in any order: 31 roundings of at most 2^-24 of a partial sum <= 2^-19 of the sum of magnitudes
        assert bool(((gs - sums).abs() <= 2.0 ** -19 * mags).all()), "colstats: column sums"
        assert bool(((gq - squares).abs() <= 2.0 ** -19 * squares).all()), "colstats: sums of squares"
    worst = int(err.nan_to_num(nan=float("inf")).flatten().argmax())
    assert device <= y.bound, (f"(a) row error {device:.3e} > {y.bound:.3e} (e_emu {y.e_emu:.3e}) at problem / compared row "
                               f"{divmod(worst, prow.numel())} = out row {int(prow[worst % prow.numel()])}")


def test_conv_gemm_refusals_are_reported_not_launched(ops):
    """Every refusal of tests/gemm_ref.REFUSALS through the real entry point: the error text, and `out` keeps its sentinel.  Each row is
    first put to sd_conv_gemm_describe, which launches nothing: a row the library accepted would otherwise launch over these small buffers."""
    small = torch.zeros(4096, dtype=F16, device=DEV)
    small32 = torch.zeros(4096, dtype=torch.float32, device=DEV)
    out = kit.sentinel(4096, F16).to(DEV)
    base = dict(gr.REFUSAL_BASE, a0=small, w=small, out=out)
    n = 0
    for text, change in gr.REFUSALS:
        kw = {k: ((small32 if k == "colstats" else small) if v is kit.PTR else v) for k, v in {**base, **change}.items()}
        if kw["out"] is None:
            continue                                             # the wrapper takes its stream from `out`; the host test covers this row
        with pytest.raises(ComaHipError, match=text):
            ops.conv_gemm_describe(**kw)
        with pytest.raises(ComaHipError, match=r"sd_conv_gemm_f16 failed \(-1\): sd_conv_gemm_f16: .*" + text):
            ops.conv_gemm(**kw)
        n += 1
    assert n == len(gr.REFUSALS) - 1
    torch.cuda.synchronize()
    assert bool((kit.bits(out.cpu()) == kit.sentinel_bits(F16)).all())
