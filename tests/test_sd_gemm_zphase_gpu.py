"""GPU: the four sub-pixel phase products of an Upsample2D convolution as ONE launch of sd_conv_gemm_f16 (phase = 5, nbatch_z = 4, the
weights of phase p at w + (p - 1) * stride_w) against the four single-phase launches of the same descriptor and against float64.

Inputs, packing (NaN guards around every operand, sentinel-filled outputs), the float64 reference and the bound are those of
tests/gemm_ref.py, as tests/test_sd_gemm_domain_gpu.py applies them to a phase case: the row error, normalised by
the largest |ref| of the row, stays within max(4 * e_emu, 2^-10), e_emu being what a careful fp16 kernel emulated on the CPU loses on the
four launches of the case.  The unsummed weights lie on a grid on which the summed taps are exact, so the float64 phase products ARE
conv3x3(nearest_up(x)); the small cases are also compared with that convolution computed the long way.
  * both forms: outputs within the bound, nothing outside the written region touched, colstats = the column sums of the stored output
    (to 2^-19 of the sum of magnitudes: 32 fp32 additions in any order), each phase in its own slots;
  * where sd_conv_gemm_describe reports the same tile, MFMA shape and K order for both forms: outputs and statistics equal bit for bit;
  * every descriptor a single phase launch refuses is refused in the one-launch form too -- a residual among them: a phase launch takes
    a plain epilogue (bias, optional colstats) only, in either form.
Shapes: the smallest that reach a 320-column product (three 128-column tiles, the last one ragged), a 64-column tile, a ragged last row
tile (M = 96), bias + colstats, and the 256 x 320 tile the one-launch form exists for (48 x 1 tiles x 4 phases = 192: the threshold)."""
import pytest
import torch

from coma_amd._lib import ComaHipError
from tests import domain_kit as kit
from tests import gemm_ref as gr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16, F64 = torch.float16, torch.float64
G = kit.GUARD
SAME = ("bm", "bn", "bk", "stages", "waves", "tm", "spread", "m16", "ksplit", "tap_minor")     # what decides the bits of a launch


@pytest.fixture(scope="module")
def ops(hip_lib):
    assert torch.cuda.is_available()
    from coma_amd.sd import ops
    return ops


def tile_name(ch):
    key = (ch.bm, ch.bn, ch.bk, ch.stages, ch.waves, ch.tm, ch.spread)
    return next(k for k, v in gr.TILES.items() if v == key)


def make_case(ops, name, B, H, W, c0, n, **kw):
    """The gemm_ref case of the four single-phase launches, its tile as the library reports it (the emulation walks K in its bk steps)."""
    probe = gr.Case(name, "128x128k32", 0, B, H, W, c0, n, taps=4, phase=5, **kw)
    ch = gr.describe(ops, probe, 0)
    return gr.Case(name, tile_name(ch), ch.m16, B, H, W, c0, n, taps=4, phase=5, **kw)


def z_kwargs(c, ptr):
    kw = gr.launch_kwargs(c, ptr, 0)
    kw.update(phase=5, nbatch_z=4, stride_w=c.n * c.K)
    return kw


def run(ops, c, dev, w_all, one_launch):
    out = gr.new_out(c).to(DEV)
    cs = gr.new_colstats(c).to(DEV) if c.colstats else None
    ptr = dict(dev, out=out[G:], colstats=None if cs is None else cs[G:])
    with kit.device_guard(f"{c.id} ({'one launch' if one_launch else 'four launches'})"):
        if one_launch:
            ops.conv_gemm(ptr["a0"], w_all[G:], ptr["out"], **z_kwargs(c, ptr))
        else:
            for launch in range(4):
                ops.conv_gemm(ptr["a0"], dev["w"][launch], ptr["out"], **gr.launch_kwargs(c, ptr, launch))
    return out.cpu(), None if cs is None else cs.cpu()


def check_form(c, y, out, cs, what):
    err = gr.row_error(gr.out_values(c, out, y.rows), y.ref, y.cols, None)
    device = float(err.nan_to_num(nan=float("inf")).max())
    print(f"ZPHASE {c.id} {what}: tile={c.tile} e_emu={y.e_emu:.3e} bound={y.bound:.3e} device={device:.3e}")
    mask = gr.written_mask(c)
    assert bool(torch.isfinite(out[mask].float()).all()), f"{what}: NaN / Inf (or an unwritten element) in the written region of `out`"
    assert bool((kit.bits(out)[~mask] == kit.sentinel_bits(F16)).all()), f"{what}: a gap column or guard of `out` was written"
    if c.colstats:
        slots, sums, squares, mags = gr.colstats_expected(c, out)
        assert slots.numel() == gr.colstats_slots(c) and bool((kit.bits(cs)[:G] == kit.sentinel_bits(torch.float32)).all()) and bool((kit.bits(cs)[-G:] == kit.sentinel_bits(torch.float32)).all())
        body = cs[G:-G].view(gr.colstats_slots(c), 2, c.n)
        gs, gq = body[slots, 0].to(F64), body[slots, 1].to(F64)
        assert bool(torch.isfinite(gs).all()) and bool(torch.isfinite(gq).all()), f"{what}: NaN / Inf (or an unwritten slot) in colstats"
        assert bool(((gs - sums).abs() <= 2.0 ** -19 * mags).all()), f"{what}: colstats column sums"
        assert bool(((gq - squares).abs() <= 2.0 ** -19 * squares).all()), f"{what}: colstats sums of squares"
    assert device <= y.bound, f"{what}: row error {device:.3e} > {y.bound:.3e} (e_emu {y.e_emu:.3e})"


CASES = [
    # name, B, H, W, c0, n, flags
    ("z-n320", 2, 8, 8, 64, 320, dict(bias=True)),                               # 320 columns: three 128-column tiles, the last ragged
    ("z-n64", 2, 8, 8, 64, 64, dict()),                                           # the 64-column tile
    ("z-ragged-m96", 3, 8, 4, 64, 64, dict(bias=True, dldo=8)),                   # M = 96: a ragged last row tile; a gap column in `out`
    ("z-bias-colstats", 2, 8, 8, 64, 64, dict(bias=True, colstats=True)),         # per = 2 slots per (sample, phase)
    ("z-big-colstats", 3, 64, 64, 64, 320, dict(bias=True, colstats=True)),       # M = 12288: 48 x 1 x 4 = 192 tiles of 256 x 320 in one launch
]


@pytest.mark.parametrize("name, B, H, W, c0, n, flags", CASES, ids=[c[0] for c in CASES])
def test_one_launch_of_four_phases(ops, name, B, H, W, c0, n, flags):
    c = make_case(ops, name, B, H, W, c0, n, **flags)
    inp = gr.make_inputs(c)
    y = gr.yardstick(c)
    pk = gr.pack(c, inp)
    dev = {k: (None if v is None else v.to(DEV)[G:]) for k, v in pk._asdict().items() if k != "w"}
    dev["w"] = tuple(w.to(DEV)[G:] for w in pk.w)
    # the four phase matrices stride_w = n * K apart, NaN guards around them
    w_all = gr.pack_blocks(torch.stack([gr.phase_weights(inp.w[0], ph) for ph in (1, 2, 3, 4)]).reshape(1, 4 * c.n, c.K), c.K, c.K, 0).to(DEV)

    four, four_cs = run(ops, c, dev, w_all, one_launch=False)
    one, one_cs = run(ops, c, dev, w_all, one_launch=True)
    check_form(c, y, four, four_cs, "four launches")
    check_form(c, y, one, one_cs, "one launch")

    ch4 = [gr.describe(ops, c, launch) for launch in range(4)]
    ch1 = ops.conv_gemm_describe(gr.FAKE["a0"], gr.FAKE["w"], gr.FAKE["out"], **z_kwargs(c, gr.FAKE))
    assert ch1.grid_y == 4 and ch1.ksplit == 1
    same = all(getattr(ch1, k) == getattr(ch, k) for ch in ch4 for k in SAME)
    print(f"ZPHASE {c.id}: one launch {tile_name(ch1)} m16={ch1.m16} grid {ch1.grid_x} x {ch1.grid_y}; single phase {c.tile}; same kernel: {same}")
    if name == "z-big-colstats":
        assert tile_name(ch1) == "256x320" and not same          # what the form is for: the single phase takes the 128 x 320 tile
    else:
        assert same
    if same:
        assert torch.equal(kit.bits(one), kit.bits(four)), "one launch and four launches of the same kernel differ in `out`"
        if c.colstats:
            assert torch.equal(kit.bits(one_cs), kit.bits(four_cs)), "one launch and four launches of the same kernel differ in colstats"
    if c.M <= 512:
        # ... and the convolution the long way: 3x3 over the nearest-x2 image with the unsummed weights
        ref = gr.reference_3x3_upsampled(c, inp)
        got = one[G:G + c.Mo * c.ldo].view(c.Mo, c.ldo)[:, :c.n].to(F64)
        e = float(((got - ref).abs().amax(-1) / ref.abs().amax(-1)).max())
        print(f"ZPHASE {c.id}: against conv3x3(nearest_up(x)) in float64: {e:.3e} (bound {y.bound:.3e})")
        assert e <= y.bound


def test_what_a_single_phase_refuses_the_one_launch_form_refuses(ops):
    """Every row of gemm_ref.REFUSALS that a phase = 1 descriptor reaches, put to the one-launch form (phase = 5, nbatch_z = 4, stride_w
    given): refused with COMA_E_INVALID, nothing launched (`out` keeps its sentinel).  A residual is one of the rows."""
    small = torch.zeros(4096, dtype=F16, device=DEV)
    small32 = torch.zeros(4096, dtype=torch.float32, device=DEV)
    out = kit.sentinel(4096, F16).to(DEV)
    base = dict(gr.REFUSAL_BASE, a0=small, w=small, out=out)
    rows = [(text, change) for text, change in gr.REFUSALS if change.get("phase") == 1]
    assert len(rows) >= 12 and any("res" in ch for _, ch in rows) and any("colstats" in ch for _, ch in rows)
    ok = dict(base, **gr.PHASE_BASE)
    ok.update(phase=5, nbatch_z=4, stride_w=ok["n"] * 4 * ok["c0"])
    assert ops.conv_gemm_describe(**ok).grid_y == 4                              # the control: the rows are refused for their change alone
    for text, change in rows:
        kw = {k: ((small32 if k == "colstats" else small) if v is kit.PTR else v) for k, v in {**base, **change}.items()}
        with pytest.raises(ComaHipError, match=r"failed \(-1\)"):                # the single phase, as the table says
            ops.conv_gemm_describe(**kw)
        kw.update(phase=5, nbatch_z=change.get("nbatch_z", 4), stride_w=kw["n"] * 4 * kw["c0"])
        with pytest.raises(ComaHipError, match=r"sd_conv_gemm_describe failed \(-1\): sd_conv_gemm_f16: "):
            ops.conv_gemm_describe(**kw)
        with pytest.raises(ComaHipError, match=r"sd_conv_gemm_f16 failed \(-1\): sd_conv_gemm_f16: "):
            ops.conv_gemm(**kw)
    # the form's own preconditions: four phases, one source and one `out`, weights that do not overlap
    for change in (dict(nbatch_z=1), dict(nbatch_z=3), dict(nbatch_z=16), dict(stride_a=64), dict(stride_out=64), dict(stride_w=0)):
        with pytest.raises(ComaHipError, match=r"failed \(-1\)"):
            ops.conv_gemm_describe(**dict(ok, **change))
    torch.cuda.synchronize()
    assert bool((kit.bits(out.cpu()) == kit.sentinel_bits(F16)).all())
