"""CPU checks of tests/gemm_ref.py and of sd_conv_gemm_describe: the float64 reference against a direct seven-loop convolution, the
summed-tap phase products against the 3x3 convolution of the upsampled image, the permutation helpers against the product's own, the poison
pattern of the packed buffers; for every row of the table the choice record the library gives against the declared one, and the fp16
emulation against its own a-priori bound; that the table reaches every instantiation the dispatch can produce; and every refusal of
sd_conv_gemm_f16 through sd_conv_gemm_describe, with pointers that are never dereferenced.  The per-case yardstick e_emu (and with it the
bound tests/test_sd_gemm_domain_gpu.py holds the device to) is printed here, without a GPU: `pytest -s tests/test_gemm_ref_host.py`."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import domain_kit as kit
from tests import gemm_ref as gr

F16, F64 = torch.float16, torch.float64


@pytest.fixture(scope="module")
def ops(hip_lib):
    from coma_amd.sd import ops
    return ops


def _seven_loops(c, inp):
    """out[b, oy, ox, n] = sum over dy, dx, ci of x[b, oy s - p + dy, ox s - p + dx, ci] w[n, (3 dy + dx) C + ci], the image upsampled first
    when the case says so: numpy scalars, one loop per index."""
    x = inp.x[0].double().numpy()
    if c.up:
        x = x.repeat(2, axis=1).repeat(2, axis=2)
    w = inp.w[0].double().numpy()
    Cc, k = x.shape[-1], 3 if c.taps == 9 else 1
    p = c.pad if c.taps == 9 else 0
    out = np.zeros((c.B, c.out_h, c.out_w, c.n))
    for b in range(c.B):
        for oy in range(c.out_h):
            for ox in range(c.out_w):
                for n in range(c.n):
                    acc = 0.0
                    for dy in range(k):
                        for dx in range(k):
                            iy, ix = oy * c.stride - p + dy, ox * c.stride - p + dx
                            if 0 <= iy < x.shape[1] and 0 <= ix < x.shape[2]:
                                for ci in range(Cc):
                                    acc += x[b, iy, ix, ci] * w[n, (k * dy + dx) * Cc + ci]
                    out[b, oy, ox, n] = acc
    return torch.from_numpy(out.reshape(c.M, c.n))


@pytest.mark.parametrize("kw", [dict(taps=9, stride=2, pad=1), dict(taps=9, stride=2, pad=0), dict(taps=9, up=1), dict(stride=2)],
                         ids=["stride2-pad1", "stride2-pad0", "upsample", "1x1-stride2"])
def test_reference_agrees_with_a_seven_loop_convolution(kw):
    c = gr.Case("loops-" + "-".join(f"{k}{v}" for k, v in kw.items()), "128x64k32", 1, 2, 5, 4, 32, 3, **kw)
    inp = gr.make_inputs(c)
    ref, direct = gr.reference(c, inp), _seven_loops(c, inp)
    assert ref.dtype == F64 and ref.shape == direct.shape == (c.M, c.n) and float(direct.abs().max()) > 0.5
    assert float((ref - direct).abs().max()) <= 1e-12


def test_two_sources_are_their_concatenation():
    c = gr.Case("loops-2src", "128x64k32", 1, 1, 3, 4, 32, 3, c1=64, taps=9)
    inp = gr.make_inputs(c)
    assert float((gr.reference(c, inp) - _seven_loops(c, inp)).abs().max()) <= 1e-12
    pk = gr.pack(c, inp)
    G = kit.GUARD
    assert torch.equal(pk.a0[G:-G].view(12, 32), inp.x[0].reshape(12, 96)[:, :32]) and torch.equal(pk.a1[G:-G].view(12, 64), inp.x[0].reshape(12, 96)[:, 32:])


@pytest.mark.parametrize("case", [c for c in gr.CASES if c.phase and c.M <= 512], ids=lambda c: c.id)
def test_phase_products_are_the_3x3_convolution_of_the_upsampled_image(case):
    """The four summed-tap 2 x 2 products, scattered to their parities, against conv3x3(upsample(x)) with the unsummed weights; and the
    summed weights against the product's own weight preparation."""
    from coma_amd.sd.weights import upsample_phase_weights
    c, inp = case, gr.make_inputs(case)
    long_way = gr.reference_3x3_upsampled(c, inp)
    theirs = upsample_phase_weights(inp.w[0].reshape(c.n, 3, 3, -1).permute(0, 3, 1, 2))
    rows = torch.arange(c.M)
    for ph in c.phases:
        mine = gr.reference(c, inp, phase=ph)
        assert float((mine - long_way[gr.out_row(c, rows, ph)]).abs().max()) <= 1e-12
        assert torch.equal(gr.phase_weights(inp.w[0], ph), theirs[ph - 1])
    o = torch.cat([gr.out_row(c, rows, ph) for ph in (1, 2, 3, 4)])
    assert torch.equal(o.sort().values, torch.arange(4 * c.M))          # the four parities tile the output


def test_perm_and_geglu_helpers_agree_with_the_products():
    from coma_amd.sd import ops, weights
    x = torch.arange(2 * 96, dtype=torch.float32).reshape(2, 96).to(F16)
    assert torch.equal(ops.perm16_columns(x), x[:, gr.kappa16(torch.arange(96))])
    assert torch.equal(ops.perm32_columns(x), x[:, gr.kappa32(torch.arange(96))])
    assert torch.equal(gr.kappa16(gr.kappa16(torch.arange(64))), torch.arange(64))
    w, b = torch.arange(256.0)[:, None].repeat(1, 2), torch.arange(256.0)
    wi, bi = weights.geglu_interleave(w, b)
    iv, ig = gr.geglu_rows(256)
    assert torch.equal(bi[iv], torch.arange(128.0)) and torch.equal(bi[ig], torch.arange(128.0) + 128) and torch.equal(wi[:, 0], bi)


def test_packed_buffers_poison_everything_the_contract_leaves_unread():
    c = next(x for x in gr.CASES if x.name == "z-gap-both")
    inp, G = gr.make_inputs(c), kit.GUARD
    pk = gr.pack(c, inp)
    sa, sw, so, _ = c.strides()
    npix = c.B * c.H * c.W
    assert pk.a0.numel() == 2 * G + 2 * sa + npix * c.c0 and int(pk.a0.isnan().sum()) == 2 * G + 2 * 8
    assert torch.equal(pk.a0[G + sa:G + sa + npix * c.c0], inp.x[1].reshape(-1))
    assert int(pk.w[0].isnan().sum()) == 2 * G + 2 * 16 and torch.equal(pk.w[0][G + 2 * sw:G + 2 * sw + c.n * c.K], inp.w[2].reshape(-1))
    c2 = next(x for x in gr.CASES if x.name == "cols-ldr+5")
    pk2 = gr.pack(c2, gr.make_inputs(c2))
    body = pk2.res[G:-G].view(c2.M, c2.ldr)
    assert bool(body[:, c2.n:].isnan().all()) and not bool(body[:, :c2.n].isnan().any()) and bool(pk2.res[:G].isnan().all())
    out = gr.new_out(c)
    m = gr.written_mask(c)
    assert m.numel() == out.numel() and int(m.sum()) == c.nz * c.M * c.n and not bool(m[:G].any()) and not bool(m[-G:].any())
    assert bool((kit.bits(out) == kit.sentinel_bits(out.dtype)).all()) and bool(gr.new_workspace(c2).isnan().all())
    assert bool((kit.bits(gr.new_colstats(c2)) == kit.sentinel_bits(torch.float32)).all())


def test_sampled_rows_hold_what_they_must():
    for c in gr.CASES:
        rows = gr.sampled_rows(c)
        if c.macs <= gr.SAMPLE_ABOVE:
            assert rows.numel() == c.M
            continue
        bm, have = gr.TILES[c.tile][0], set(rows.tolist())
        assert set(range(min(bm, c.M))) <= have and set(range((c.M - 1) // bm * bm, c.M)) <= have
        if c.B > 1:
            assert set(range(c.rpb // bm * bm, min(c.rpb // bm * bm + bm, c.M))) <= have and (c.rpb - 1) in have
        for m in (0, c.out_w - 1, c.rpb - 1, c.rpb - c.out_w, c.M - 1, c.M - c.rpb, (c.out_h // 2) * c.out_w, (c.out_h // 2 + 1) * c.out_w - 1):
            assert m in have
        assert c.M > rows.numel() >= 256


def test_describe_gives_every_case_its_declared_choice(ops):
    for c in gr.CASES:
        for launch in range(max(1, len(c.phases))):
            ch = gr.describe(ops, c, launch)
            got = (ch.bm, ch.bn, ch.bk, ch.stages, ch.waves, ch.tm, ch.spread)
            assert got == gr.TILES[c.tile] and ch.m16 == c.m16 and ch.ksplit == c.ksplit, (c.name, ch.asdict())
            bm, bn = got[:2]
            gx, gy = -(-c.M // bm), -(-c.N // bn)
            assert ch.grid_x == (8 * -(-gx // 8) * gy if gx >= 16 else gx * gy) and ch.grid_y == (c.ksplit if c.ksplit > 1 else c.nz), c.name
            assert ch.tap_minor == (1 if c.taps == 9 and not c.up and c.tile in ("256x320s", "128x320w8") and gy == 1 else 0), c.name


def test_the_table_reaches_every_instantiation_the_dispatch_can_produce(ops):
    seen = set()
    for c in gr.CASES:
        ch = gr.describe(ops, c)
        tile = next(k for k, v in gr.TILES.items() if v == (ch.bm, ch.bn, ch.bk, ch.stages, ch.waves, ch.tm, ch.spread))
        seen.add((tile, ch.m16))
    assert seen == gr.REACHABLE and len(gr.REACHABLE) == 19
    assert len({c.name for c in gr.CASES}) == len(gr.CASES) and 100 <= len(gr.CASES) <= 200
    # both K orders of a 3x3, split-K on both BK, and every edge list of the table
    assert {c.ksplit for c in gr.CASES} >= {1, 2, 3, 4, 16}
    assert {c.n for c in gr.CASES} >= {4, 12, 100, 328, 77, 80, 8, 64, 96, 192, 1280, 1920}
    assert {c.M for c in gr.CASES} >= {1, 31, 127, 129}


def test_reachable_is_what_a_sweep_of_describe_produces(ops):
    """gemm_ref.REACHABLE against the library itself: sd_conv_gemm_describe over a grid of (M, N, channels, taps, GEGLU, z-batching,
    workspace, colstats) that straddles every threshold of the dispatch.  A threshold change that makes another (tile, m16) pair
    reachable, or one of these unreachable, shows here before the table's coverage means anything."""
    from coma_amd._lib import ComaHipError
    by_choice = {v: k for k, v in gr.TILES.items()}
    seen, accepted = set(), 0
    for M in (64, 4096, 8192, 12288, 32768, 49152, 65536):
        for n in (8, 64, 96, 128, 192, 256, 320, 328, 384, 512, 640, 1280):
            for c0 in (32, 64, 96, 128, 192, 256, 352, 1024, 1056, 1280, 8192):
                for taps in (1, 9):
                    for epi in (0, gr.EPI_GEGLU):
                        for nz in (1, 16):
                            for extra in (dict(), dict(workspace=gr.FAKE["workspace"], workspace_bytes=64 << 20), dict(colstats=gr.FAKE["colstats"])):
                                try:
                                    ch = ops.conv_gemm_describe(gr.FAKE["a0"], gr.FAKE["w"], gr.FAKE["out"], batch=M // 64, in_h=8, in_w=8,
                                                                c0=c0, n=n, taps=taps, epi=epi, nbatch_z=nz, **extra)
                                except ComaHipError:
                                    continue
                                accepted += 1
                                seen.add((by_choice[(ch.bm, ch.bn, ch.bk, ch.stages, ch.waves, ch.tm, ch.spread)], ch.m16))
    assert accepted > 10000 and seen == gr.REACHABLE


def _resolve(kw, ptr):
    return {k: (ptr(k) if v is kit.PTR else v) for k, v in kw.items()}


def test_every_refusal_gives_its_code_and_text_through_describe(ops, hip_lib):
    from coma_amd._lib import ComaHipError
    fake = lambda name: gr.FAKE.get(name, 0x7000000000)
    base = dict(gr.REFUSAL_BASE, a0=gr.FAKE["a0"], w=gr.FAKE["w"], out=gr.FAKE["out"])
    assert ops.conv_gemm_describe(**base).bn == 64
    for text, change in gr.REFUSALS:
        kw = _resolve({**base, **change}, fake)
        with pytest.raises(ComaHipError, match=r"sd_conv_gemm_describe failed \(-1\): sd_conv_gemm_f16: .*" + text):
            ops.conv_gemm_describe(**kw)
    # ... and the controls next to them, accepted: a power of two of a large row count folds into the image, PERM with a row bias
    big_m = dict(base, taps=1, batch=131072, in_h=1, in_w=1)
    assert ops.conv_gemm_describe(**big_m).grid_x == 131072 // 128
    assert ops.conv_gemm_describe(**dict(base, taps=1, n=77, ldo=80, epi=gr.EPI_PERM16 | gr.EPI_BIAS_ROWS, bias=fake("bias"))).bn == 64
    assert ops.conv_gemm_describe(**dict(base, taps=1, epi=gr.EPI_PERM32 | gr.EPI_BIAS_ROWS, bias=fake("bias"))).bn == 64
    # the entry points themselves
    ch = ops.ConvGemmChoice()
    assert hip_lib.sd_conv_gemm_describe(None, C.byref(ch)) == -1 and b"sd_conv_gemm_f16: null descriptor" in hip_lib.coma_last_error()
    d = ops._conv_gemm_desc(lambda t, *a: t, **{k: v for k, v in base.items()})
    assert hip_lib.sd_conv_gemm_describe(C.byref(d), None) == -1 and b"null choice" in hip_lib.coma_last_error()


def test_describe_is_not_recorded_into_a_plan(ops, hip_lib):
    from tests.golden import make_plan_records as gen
    m = C.c_void_p()
    assert hip_lib.sd_model_create(C.byref(m)) == 0
    try:
        assert hip_lib.sd_model_register_buffer(m, C.c_void_p(gen.BASE), gen.SPAN, 0) == 0
        assert hip_lib.sd_model_record_begin(m, b"p") == 0
        try:
            assert ops.conv_gemm_describe(gen.BASE, gen.BASE + 64, gen.BASE + 128, **gr.REFUSAL_BASE).bn == 64
        finally:
            hip_lib.sd_model_record_end(m)
        assert hip_lib.sd_model_num_launches(m, b"p") == 0
    finally:
        hip_lib.sd_model_destroy(m)


@pytest.mark.parametrize("case", gr.CASES, ids=lambda c: c.id)
def test_emulation_is_within_its_stated_bound(case):
    """|emulation - float64| <= (K + 4) 2^-24 sum |a w| + the epilogue's terms (gemm_ref.epilogue) + 2^-11 |ref|, element by element, and
    the case's yardstick: e_emu and the device bound."""
    y = gr.yardstick(case)
    print(f"GEMM_YARD {case.id} family={case.pool} rows={y.rows.numel()}/{case.Mo} e_emu={y.e_emu:.3e} bound={y.bound:.3e} "
          f"emu/stated={y.emu_over_stated:.2f}")
    assert y.emu_over_stated <= 1.0
    assert y.bound == max(4 * y.e_emu, 2.0 ** -10) and 0 < y.e_emu < 2.0 ** -6            # a yardstick this loose would measure nothing
    assert y.ref.shape[:2] == (case.nz, y.rows.numel()) and bool(y.cols.any())
