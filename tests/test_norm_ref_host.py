"""CPU checks of tests/norm_ref.py and of the argument checks of coma_amd/csrc/sd_norm.hip / sd_winograd.hip: the float64 references against
oracle/sd_oracle.py (and the torch operators it calls), the Winograd reference chain against a direct float64 3x3 convolution, the poison
pattern of the packed buffers, that the table reaches every branch of the ten entry points, every emulation against its own a-priori bound,
and every refusal row through the REAL entry points with dummy non-null pointers: the argument checks run before any HIP call, so without a
device a refused row returns COMA_E_INVALID with its text and a wrongly accepted one fails at launch with another code.  The per-case
yardstick e_emu (and with it the bound tests/test_sd_norm_domain_gpu.py holds the device to) is printed here, without a GPU:
`pytest -s tests/test_norm_ref_host.py`."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from coma_amd import _lib
from oracle import sd_oracle as so
from tests import domain_kit as kit
from tests import norm_ref as nr

F16, F32, F64 = torch.float16, torch.float32, torch.float64
_close = nr.close_to_oracle


def test_sum32_adds_in_index_order():
    x = (torch.randn(3, 5000, generator=torch.Generator().manual_seed(1)) * 3 + 1).to(F32)
    got = kit.sum32(x)
    for r in range(3):
        s = np.float32(0)
        for v in x[r].numpy():
            s = np.float32(s + v)
        assert float(got[r]) == float(s)
    assert not torch.equal(got, x.sum(-1))          # (torch's own sum is pairwise: another value, which is why the helper exists)


@pytest.mark.parametrize("case", [c for c in nr.CASES if isinstance(c, nr.GN) and c.entry == "gn" and c.dist == "n" and c.B * c.hw * c.C <= 1 << 18],
                         ids=lambda c: c.id)
def test_groupnorm_reference_agrees_with_the_oracle(case):
    c, d = case, nr.inputs(case)
    ref = nr.results(c)["out"].ref
    theirs = so.groupnorm_ref(nr.cat(d), d["gamma"].t[0], d["beta"].t[0], batch=c.B, hw=c.hw, groups=c.G, eps=c.eps, silu=bool(c.silu))
    assert ref.dtype == F64 and ref.shape == theirs.shape and _close(ref, theirs)


def test_column_sum_statistics_are_the_tensor_statistics():
    """a GroupNorm fed by column sums against the oracle on the tensor: the fp32 column sums carry 2^-24 of each slot's sum"""
    c = next(x for x in nr.CASES if x.id == "gn_cs-c8-c24-g2")
    d = nr.inputs(c)
    theirs = so.groupnorm_ref(nr.cat(d), d["gamma"].t[0], d["beta"].t[0], batch=c.B, hw=c.hw, groups=c.G, eps=c.eps, silu=True)
    assert _close(nr.results(c)["out"].ref, theirs)
    t = next(x for x in nr.CASES if x.id == "table_cs-cg16-rps256")
    d = nr.inputs(t)
    x = d["x0"].t.to(F64).view(t.B, t.hw, t.G, t.cg)
    mean, var = x.mean((1, 3)), x.var((1, 3), unbiased=False)
    sc = (var + t.eps) ** -0.5 * d["gamma"].t.to(F64).view(1, t.G, t.cg).permute(2, 0, 1)
    sh = d["beta"].t.to(F64).view(1, t.G, t.cg).permute(2, 0, 1) - mean * sc
    tab = torch.stack([sc.permute(1, 2, 0).reshape(t.B, -1), sh.permute(1, 2, 0).reshape(t.B, -1)], -1).reshape(-1, 2)
    assert d["colstats0"].t.shape == (t.B * t.hw // 256 * 2, t.c0) and _close(nr.results(t)["stats"].ref, tab)


def test_layernorm_and_softmax_references_agree_with_torch():
    for c in (x for x in nr.CASES if isinstance(x, nr.LN) and x.rows <= 64):
        d = nr.inputs(c)
        theirs = F.layer_norm(d["x"].t.float(), (c.c,), d["gamma"].t[0].float(), d["beta"].t[0].float(), c.eps)
        assert _close(nr.results(c)["out"].ref, theirs), c.id
    for c in (x for x in nr.CASES if isinstance(x, nr.SM)):
        theirs = torch.softmax(nr.inputs(c)["x"].t.float() * c.scale, -1)
        assert _close(nr.results(c)["x"].ref, theirs), c.id


def _direct_conv3x3(img, w):
    """out[b, y, x, n] = sum over ky, kx, ci of img[b, y - 1 + ky, x - 1 + kx, ci] w[n, 3 ky + kx, ci] in float64, zero padding"""
    B, h, wd, C = img.shape
    pad = torch.zeros(B, h + 2, wd + 2, C, dtype=F64)
    pad[:, 1:-1, 1:-1] = img.to(F64)
    out = torch.zeros(B, h, wd, w.shape[0], dtype=F64)
    for ky in range(3):
        for kx in range(3):
            out += pad[:, ky:ky + h, kx:kx + wd] @ w[:, 3 * ky + kx].to(F64).t()
    return out.reshape(B * h * wd, -1)


@pytest.mark.parametrize("up", [0, 1], ids=["same-size", "upsample"])
def test_winograd_chain_is_the_direct_convolution(up):
    """input transform -> 16 plane products -> output transform, all float64, against the direct convolution and against the oracle's"""
    g = torch.Generator().manual_seed(7 + up)
    B, h, wd, C, n = 2, 4 << up, 6 << up, 16, 8
    src = kit.randn16(g, B, h >> up, wd >> up, C)
    w = kit.randn16(g, n, 9, C, scale=0.2)
    img = src.repeat_interleave(2, 1).repeat_interleave(2, 2) if up else src
    T = B * (h // 2) * (wd // 2)
    V = nr.wino_input(img, 0.25)[0].view(16, T, C)
    U = 0.25 * torch.einsum("ak,nklc,bl->abnc", nr.GM, w.view(n, 3, 3, C).to(F64), nr.GM).reshape(16, n, C)
    m = torch.einsum("ptc,pnc->ptn", V, U)
    Y = 16.0 * torch.einsum("ai,ijbtxn,cj->btaxcn", nr.AT, m.view(4, 4, B, h // 2, wd // 2, n), nr.AT).reshape(B * h * wd, n)
    direct = _direct_conv3x3(img, w)
    assert float(direct.abs().max()) > 1 and float((Y - direct).abs().max()) <= 1e-12
    theirs = so.conv_ref(src.reshape(-1, C), w, batch=B, h=h >> up, w_=wd >> up, taps=9, upsample=bool(up))
    assert _close(direct, theirs)
    # the fp16 path of norm_ref (wino_output on rounded planes) differs from it by the rounding of the planes only
    y, y32, _ = nr.wino_output(m.to(F16).reshape(16 * T, n), B, h, wd, 16.0, None, None, None, 0)
    assert float((y - direct).abs().max()) <= 16 * 9 * 2.0 ** -11 * float(m.abs().max())


def test_packed_buffers_poison_everything_the_contract_leaves_unread():
    G = kit.GUARD
    c = next(x for x in nr.CASES if x.id == "wino_out-cs-h4-n256-all")
    d, o = nr.inputs(c), nr.outputs(c)
    for name, ld in (("m", c.n + 8), ("res", c.n + 16), ("bias_bn", c.n + 8), ("bias", c.n)):
        buf = kit.pack(d[name])
        r = d[name].t.shape[0]
        assert d[name].ld == ld and buf.numel() == 2 * G + r * ld and bool(buf[:G].isnan().all()) and bool(buf[-G:].isnan().all())
        b2 = buf[G:-G].view(r, ld)
        assert torch.equal(b2[:, :c.n], d[name].t) and bool(b2[:, c.n:].isnan().all()) and int(buf.isnan().sum()) == 2 * G + r * (ld - c.n)
    out = kit.new_out(o["out"])
    must, may = kit.masks(o["out"])
    assert bool((kit.bits(out) == kit.sentinel_bits(F16)).all()) and bool(out.isnan().all()) and int(must.sum()) == c.B * c.h * c.w * c.n
    assert not bool(must[:G].any()) and not bool(must[-G:].any()) and not bool(must[G:-G].view(-1, c.n + 8)[:, c.n:].any()) and must is may
    cs = kit.new_out(o["colstats"])
    assert cs.numel() == 2 * G + c.B * c.h * c.w // 32 * 2 * c.n and bool((kit.bits(cs) == kit.sentinel_bits(F32)).all()) and bool(cs.isnan().all())
    # stats: guarded exactly where batch * C * 2 + batch * ceil(hw / 64) * groups * 2 floats end; only the table has to be written
    t = next(x for x in nr.CASES if x.id == "table-hw65-c320")
    st = nr.outputs(t)["stats"]
    must, may = kit.masks(st)
    assert st.width == 2 * 320 * 2 + 2 * 2 * 32 * 2 and int(may.sum()) == st.width and int(must.sum()) == 2 * 320 * 2 and bool(must[G:G + 1280].all())
    assert nr.outputs(next(x for x in nr.CASES if x.id == "gn-hw65-c320"))["stats"].must == 0
    # a pointer moved off its alignment: the halves in front of it are NaN too; softmax's buffer carries its data between NaN gap columns
    gm = nr.inputs(next(x for x in nr.CASES if x.id == "gn_wino-m0-cg8-gamma+4"))["gamma"]
    assert gm.off == 4 and bool(kit.pack(gm)[:G + 4].isnan().all()) and torch.equal(kit.pack(gm)[G + 4:-G], gm.t[0])
    s = next(x for x in nr.CASES if x.id == "softmax-n7-ld+3")
    assert int(kit.pack(nr.inputs(s)["x"]).isnan().sum()) == 2 * G + s.rows * 3


def test_the_table_reaches_every_branch_of_the_ten_entry_points():
    seen = set()
    for c in nr.CASES:
        seen |= nr.branches(c)
    assert seen == nr.REACHABLE and len(nr.REACHABLE) == 35
    assert len({c.id for c in nr.CASES}) == len(nr.CASES)
    # the transcript itself at the thresholds the entry points state
    assert nr.groupnorm_route(1280, 1280, 256, 32) == "gn_small_kernel" and nr.groupnorm_route(1280, 1280, 257, 32) == "partial-finalize-apply"
    assert nr.groupnorm_route(24, 0, 1, 4) == "partial-finalize-apply"
    assert [nr.layernorm_instantiation(r, 1280) for r in (16383, 16384, 32767, 32768)] == ["row<1,4>", "group<32,1>", "group<32,1>", "group<32,2>"]
    assert nr.layernorm_instantiation(65535, 640) == "group<16,1>" and nr.layernorm_instantiation(65536, 640) == "group<16,2>"
    assert nr.gn_wino_vec(8, 1, 36, 32, True) == 4 and nr.gn_wino_vec(8, 0, 36, 32, True) == 8 and nr.gn_wino_vec(8, 0, 32, 32, False) == 4
    # the edges the table must hold
    gn = [c for c in nr.CASES if isinstance(c, nr.GN)]
    assert {c.cg for c in gn if c.entry in ("gn_cs", "table_cs", "table_cat")} >= {1, 10, 80, 136, 256}
    assert {c.rps for c in gn} == {32, 64, 256} and {c.eps for c in gn} == {1e-5, 1e-6} and {c.dist for c in gn} == {"n", "shift", "const"}
    assert {c.hw % 4 for c in gn if c.C == 2048} == {1, 2, 3}
    assert {c.n for c in nr.CASES if isinstance(c, nr.SM)} == {1, 7, 255, 256, 257, 1000, 300, 600}
    wo = [c for c in nr.CASES if isinstance(c, nr.WO) and not c.cs]
    assert {(c.bias, c.bias_bn, c.res, c.silu) for c in wo} == {(a, b, r, s) for a in (0, 1) for b in (0, 1) for r in (0, 1) for s in (0, 1)}
    assert {(c.h, c.w) for c in nr.CASES if isinstance(c, nr.WI)} >= {(2, 2), (2, 6), (4, 2)}


@pytest.mark.parametrize("case", nr.CASES, ids=lambda c: c.id)
def test_emulation_is_within_its_stated_bound(case):
    """|emulation - float64| <= the a-priori bound norm_ref derives for the family (gn_affine, gn_apply, layernorm, softmax, wino_input,
    wino_output, results), element by element; and the case's yardstick: e_emu and the device bound."""
    y = nr.yardstick(case)
    print(f"NORM_YARD {case.id} family={case.family} e_emu={y.e_emu:.3e} bound={y.bound:.3e} emu/stated={y.emu_over_stated:.2f}")
    assert y.emu_over_stated <= 1.0
    assert y.bound == max(4 * y.e_emu, 2.0 ** -10) and 0 <= y.e_emu < 2.0 ** -6            # a yardstick this loose would measure nothing


@pytest.mark.parametrize("entry", sorted(nr.REFUSALS), ids=str)
def test_every_refusal_gives_its_code_and_text_through_the_entry_point(entry, hip_lib):
    base, rows = nr.REFUSALS[entry]
    assert len(rows) >= 5 and set(base) == set(_lib.PARAMS[entry][:-1])       # the header's own parameter names
    # the control: the base row passes every argument check and only fails where the launch needs a device
    kit.check_refusals(hip_lib, {entry: nr.REFUSALS[entry]}, kit.host_resolver(), expect_control=not torch.cuda.is_available())
