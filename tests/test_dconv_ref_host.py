"""CPU checks of tests/dconv_ref.py and of the argument checks of coma_amd/csrc/sd_haloconv.hip / sd_smallconv.hip: the float64 reference
(a loop over the nine taps) against torch.nn.functional.conv2d in float64 and against oracle/sd_oracle.py, every emulation against its own
a-priori bound, the poison pattern of the packed buffers, that the table reaches every branch of the four kernels, and every refusal row
through the REAL entry points with dummy non-null pointers: the argument checks run before any HIP call, so without a device a refused row
returns COMA_E_INVALID with its text and a wrongly accepted one fails at launch with another code.  The per-case yardstick e_emu (and
with it the bound tests/test_sd_dconv_domain_gpu.py holds the device to) is printed here, without a GPU:
`pytest -s tests/test_dconv_ref_host.py`."""
import pytest
import torch
import torch.nn.functional as F

from coma_amd import _lib
from oracle import sd_oracle as so
from tests import dconv_ref as dr
from tests import domain_kit as kit
from tests import norm_ref as nr

F16, F32, F64 = torch.float16, torch.float32, torch.float64
_close = nr.close_to_oracle


def _conv2d64(a, w, B, h, wd):
    """a fp16 [B h w, C], w fp16 [n, 9, C] -> torch's own float64 convolution as [B h w, n]"""
    C, n = a.shape[-1], w.shape[0]
    img = a.to(F64).view(B, h, wd, C).permute(0, 3, 1, 2)
    return F.conv2d(img, w.to(F64).view(n, 3, 3, C).permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1).reshape(B * h * wd, n)


@pytest.mark.parametrize("case", dr.CASES, ids=lambda c: c.id)
def test_reference_is_conv2d_and_the_emulation_is_within_its_stated_bound(case):
    """The float64 reference equals float64 conv2d of the same stored fp16 tensor (+ bias + res) to 1e-12 of the largest value;
    |emulation - float64| <= the a-priori bound dconv_ref.convolve / activate derive, element by element; and the case's yardstick."""
    c, d = case, dr.inputs(case)
    y = dr.yardstick(c)
    r = dr.results(c)["out"]
    if isinstance(c, dr.IC):
        x = d["x"].t.view(c.B, c.h, c.w, 3)
        for m in range(0, c.B * c.h * c.w, 7):                  # the gather by scalar index arithmetic
            b, py, px = m // (c.h * c.w), m // c.w % c.h, m % c.w
            for tap in range(9):
                yy, xx = py + tap // 3 - 1, px + tap % 3 - 1
                want = x[b, yy, xx] if 0 <= yy < c.h and 0 <= xx < c.w else torch.zeros(3, dtype=F16)
                assert torch.equal(kit.bits(r.emu[m, 3 * tap:3 * tap + 3]), kit.bits(want.contiguous())), (m, tap)
        assert not bool(kit.bits(r.emu[:, 27:]).any())
    else:
        if isinstance(c, dr.C3):
            theirs = _conv2d64(d["x"].t, d["w32"].t[:, :27].reshape(c.n, 9, 3), c.B, c.h, c.w)
        else:
            theirs = _conv2d64(dr.activated(c)[0], d["w"].t[:c.n].reshape(c.n, 9, c.c), c.B, c.h, c.w)
        if c.bias:
            theirs = theirs + d["bias"].t[:, :c.n].to(F64)
        if isinstance(c, dr.HC) and c.res:
            theirs = theirs + d["res"].t.to(F64)
        assert float((r.ref[:, :c.n] - theirs).abs().max()) <= 1e-12 * float(theirs.abs().max())
        assert not isinstance(c, dr.SN) or not bool(r.ref[:, c.n:].any())
    print(f"DCONV_YARD {c.id} family={c.family} e_emu={y.e_emu:.3e} bound={y.bound:.3e} emu/stated={y.emu_over_stated:.2f}")
    assert y.emu_over_stated <= 1.0
    assert y.bound == max(4 * y.e_emu, 2.0 ** -10) and 0 <= y.e_emu < 2.0 ** -6            # a yardstick this loose would measure nothing


@pytest.mark.parametrize("silu", [False, True], ids=["affine", "affine+silu"])
def test_reference_agrees_with_the_oracle(silu):
    """GroupNorm (+ SiLU) -> conv3x3 + bias + res: the affine table of a real GroupNorm (float64 statistics) through dconv_ref.activate
    against the oracle's groupnorm_ref, and the convolution of the stored tensor against the oracle's conv_ref."""
    g = torch.Generator().manual_seed(11 + silu)
    B, h, wd, C, n, G = 2, 16, 32, 64, 128, 32
    x = kit.randn16(g, B * h * wd, C, scale=1.5, shift=0.3)
    gamma, beta = kit.randn16(g, C, shift=1.0, scale=0.5), kit.randn16(g, C)
    xg = x.to(F64).view(B, h * wd, G, C // G)
    mean, var = xg.mean((1, 3), keepdim=True), xg.var((1, 3), unbiased=False, keepdim=True)
    sc = ((var + 1e-6) ** -0.5).expand(B, 1, G, C // G).reshape(B, C) * gamma.to(F64)
    sh = beta.to(F64) - mean.expand(B, 1, G, C // G).reshape(B, C) * sc
    tab = torch.stack([sc, sh], -1).reshape(B * C, 2)
    y, _, _ = dr.activate(x, tab, B, 2 if silu else 1)
    assert nr.ORACLE_LIMIT == 2.0 ** -17 and _close(y, so.groupnorm_ref(x, gamma, beta, batch=B, hw=h * wd, groups=G, eps=1e-6, silu=silu))
    a = y.to(F16)
    w, bias, res = kit.randn16(g, n, 9, C, scale=(9 * C) ** -0.5), kit.randn16(g, n), kit.randn16(g, B * h * wd, n)
    ref, _, _ = dr.convolve(a, a, torch.zeros(a.shape, dtype=F64), w, B, h, wd, dr.CHUNK, bias[None], res)
    assert _close(ref, so.conv_ref(a.float(), w, batch=B, h=h, w_=wd, taps=9, bias=bias, res=res))


def test_packed_buffers_poison_everything_the_contract_leaves_unread():
    G = kit.GUARD
    by_id = {c.id: c for c in dr.CASES}
    c = by_id["halo-n256-ldo+8-ldr+24"]
    d, o = dr.inputs(c), dr.outputs(c)
    M = c.B * c.h * c.w
    res = kit.pack(d["res"])
    assert d["res"].ld == 280 and res.numel() == 2 * G + M * 280 and int(res.isnan().sum()) == 2 * G + M * 24
    for name in ("x", "w", "bias", "gn_affine"):
        buf = kit.pack(d[name])
        assert int(buf.isnan().sum()) == 2 * G and bool(buf[:G].isnan().all()) and bool(buf[-G:].isnan().all()), name
    must, may = kit.masks(o["out"])
    assert o["out"].ld == 264 and int(must.sum()) == M * 256 and not bool(must[G:-G].view(M, 264)[:, 256:].any())
    assert o["colstats"].rows == c.B * 2 * 2 and o["colstats"].dtype == F32 and bool(kit.new_out(o["colstats"]).isnan().all())
    # small_n: rows of w and entries of bias at and beyond n; 8 channels of a pixel owned, the others of ldo = 72 not
    s = by_id["small_n-ldo72-c320-n4"]
    d, o = dr.inputs(s), dr.outputs(s)
    assert d["w"].t.shape == (16, 9 * 320) and bool(d["w"].t[4:].isnan().all()) and not bool(d["w"].t[:4].isnan().any())
    assert d["bias"].t.shape == (1, 8) and bool(d["bias"].t[0, 4:].isnan().all())
    assert int(kit.masks(o["out"])[0].sum()) == s.h * s.w * 8 and o["out"].ld == 72
    # the 3-channel image: channels 3 .. ldx - 1 NaN; w32 keeps its five zero columns
    t = next(x for x in dr.CASES if isinstance(x, dr.C3) and x.ldx == 64)
    d = dr.inputs(t)
    xb = kit.pack(d["x"])[G:-G].view(-1, 64)
    assert bool(xb[:, 3:].isnan().all()) and not bool(xb[:, :3].isnan().any()) and not bool(d["w32"].t[:, 27:].any()) and bool(d["w32"].t[:, :27].any())
    # im2col: signed zeros in the data
    i = dr.inputs(by_id["im2col-11x13-b2-block-crossings"])["x"].t
    assert int((kit.bits(i) == -0x8000).sum()) > 10 and int((kit.bits(i) == 0).sum()) > 10


def test_stress_tables_hold_what_they_name_and_stay_finite():
    for c in (x for x in dr.CASES if not isinstance(x, (dr.C3, dr.IC)) and x.stress):
        d = dr.inputs(c)
        y, y32, _ = dr.activate(d["x"].t, d["gn_affine"].t, c.B, c.act)
        y, y32 = y.view(c.B, -1, c.c), y32.view(c.B, -1, c.c)
        tab = d["gn_affine"].t.view(c.B, c.c, 2)
        assert bool((tab[:, 2, 0] == 0).all()) and bool((tab[:, 3, 0] < 0).all())
        if c.act == 2:
            assert float(y[:, :, 0].abs().max()) < 1e-38 and bool((kit.bits(y32[:, :, 0].to(F16)) == -0x8000).all())       # exp overflows: -0
            assert bool((y[:, :, 2] == kit.silu(tab[:, None, 2, 1].to(F64))).all())
        else:
            assert float(y[:, :, 0].max()) < -95
        assert float(y[:, :, 1].min()) > 195 and float(y[:, :, c.c - 1].mean()) > 2 and float(y[:, :, 2].min()) > 1.5
        a, a_emu, _ = dr.activated(c)
        assert bool(torch.isfinite(a.float()).all()) and bool(torch.isfinite(a_emu.float()).all())
        # per-sample tables: the samples' stress rows differ
        assert c.B > 1 and not torch.equal(tab[0], tab[1])


def test_the_table_reaches_every_branch_of_the_four_kernels():
    seen = set()
    for c in dr.CASES:
        seen |= dr.branches(c)
    assert seen == dr.REACHABLE and len(dr.REACHABLE) == 40
    assert len({c.id for c in dr.CASES}) == len(dr.CASES)
    hc = [c for c in dr.CASES if isinstance(c, dr.HC)]
    sn = [c for c in dr.CASES if isinstance(c, dr.SN)]
    c3 = [c for c in dr.CASES if isinstance(c, dr.C3)]
    ic = [c for c in dr.CASES if isinstance(c, dr.IC)]
    print(f"DCONV_TABLE halo={len(hc)} small_n={len(sn)} c3={len(c3)} im2col={len(ic)}")
    # the transcript at c = 64: tap 1 takes one branch only
    assert dr.halo_tap1_waits(64, 1) == {"vmcnt<8>"} and dr.halo_tap1_waits(64, 0) == {"vmcnt<0>"} and dr.halo_tap1_waits(128, 1) == {"vmcnt<11>", "vmcnt<8>"}
    # the edges the table must hold
    every = {(a, b, r, s) for a in (0, 1, 2) for b in (0, 1) for r in (0, 1) for s in (0, 1)}
    for ch in (64, 128):
        assert {(c.act, c.bias, c.res, c.cs) for c in hc if c.c == ch and (c.h, c.w) == (16, 32) and c.n == 128} == every
    assert {(c.c, c.n) for c in hc if c.act == 2 and c.bias and c.res and c.cs and c.B == 2} >= {(ci, n) for ci in range(64, 513, 64) for n in (128, 256, 384, 512)}
    assert {(c.h, c.w) for c in hc} == {(16, 16), (16, 32), (32, 16), (48, 48)} == {(c.h, c.w) for c in c3}
    assert {c.B for c in hc} == {1, 2, 3} == {c.B for c in c3} == {c.B for c in ic} and {c.B for c in sn} == {1, 2, 3}
    assert any(c.ldo == 0 and c.ldr == 0 for c in hc) and any(c.ldo == c.n + 8 and c.ldr == c.n + 24 for c in hc)
    assert {c.n for c in hc if c.ldo > c.n and c.ldr > c.n} >= {128, 256, 384}
    assert {(c.c, c.n, c.act, c.bias) for c in sn if (c.h, c.w) == (17, 18)} >= {(ci, n, a, b) for ci in (128, 320) for n in (1, 2, 3, 4) for a in (0, 1, 2) for b in (0, 1)}
    assert {(c.h, c.w) for c in sn} >= {(1, 1), (1, 17), (17, 1), (16, 16), (15, 33), (33, 18)} and {c.ldo for c in sn} == {8, 16, 72}
    assert {c.ldx for c in c3} == {4, 8, 64} == {c.ldx for c in ic} and {c.ldo for c in c3} == {128, 136, 256}
    assert {(c.bias, c.cs) for c in c3} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {(c.h, c.w) for c in ic} >= {(1, 1), (1, 5), (5, 1), (7, 9), (16, 16), (11, 13)}
    assert {c.stress for c in hc} == {0, 1} == {c.stress for c in sn}


@pytest.mark.parametrize("entry", sorted(dr.REFUSALS), ids=str)
def test_every_refusal_gives_its_code_and_text_through_the_entry_point(entry, hip_lib):
    base, rows = dr.REFUSALS[entry]
    assert len(rows) >= 10 and set(base) == set(_lib.PARAMS[entry][:-1])      # the header's own parameter names
    # the control: the base row passes every argument check and only fails where the launch needs a device
    kit.check_refusals(hip_lib, {entry: dr.REFUSALS[entry]}, kit.host_resolver(), expect_control=not torch.cuda.is_available())
