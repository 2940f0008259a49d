"""CPU checks of tests/attention_ref.py: the float64 reference against the project's oracle, the V^T packing helpers against the
product's own layout helpers, the poison pattern of the packed buffers, and -- for every row of the GPU case table -- the fp16 emulation
against its own stated bound.  The per-case yardstick e_emu (and with it the bound tests/test_sd_attention_domain_gpu.py holds the device
to) is computed and printed here, without a GPU: `pytest -s tests/test_attention_ref_host.py`."""
import pytest
import torch

from oracle import sd_oracle as so
from tests import attention_ref as ar
from tests import domain_kit as kit

F16 = torch.float16


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(F16)


@pytest.mark.parametrize("heads,d,lq,lk", [(3, 8, 5, 1), (8, 40, 70, 77), (2, 64, 33, 130), (1, 512, 65, 128)])
def test_f64_reference_agrees_with_the_oracle(heads, d, lq, lk):
    q, k, v = rnd(2, lq, heads * d, seed=1), rnd(2, lk, heads * d, seed=2), rnd(2, lk, heads * d, seed=3)
    ref = ar.attention_f64(q, k, v, heads, d ** -0.5)
    orc = so.attention_ref(q, k, v, heads, d ** -0.5)
    assert ref.dtype == torch.float64 and ref.shape == orc.shape
    # the oracle works in fp32: d-term dot products, an lk-term softmax and an lk-term weighted mean
    lim = (d + 2 * lk + 16) * 2.0 ** -24 * float(v.float().abs().max())
    assert float((ref - orc.double()).abs().max()) <= lim


def test_perm_helpers_agree_with_the_products_layout_helpers():
    from coma_amd.sd import ops
    for lk in (1, 7, 16, 65, 77, 200):
        v = rnd(2, lk, 24, seed=lk)
        ldv = ar.roundup(lk, 16)
        mine = ar.pack_vt_perm16(v, ldv)[:2 * 24 * ldv].view(2, 24, ldv)
        theirs = ops.perm16_columns(v.transpose(1, 2).contiguous())
        assert theirs.shape == mine.shape
        real = ar.perm16_source(ldv) < lk
        assert int(real.sum()) == lk
        assert torch.equal(mine[:, :, real], theirs[:, :, real])
        assert bool((mine[:, :, ~real] == ar.PAD_VALUE).all()) and bool((theirs[:, :, ~real] == 0).all())
    for lk in (64, 128, 192):
        v = rnd(2, lk, 32, seed=lk)
        mine = ar.pack_vt_perm32(v, lk + 64)[:2 * 32 * (lk + 64)].view(2, 32, lk + 64)
        assert torch.equal(mine[:, :, :lk], ops.perm32_columns(v.transpose(1, 2).contiguous()))
        assert bool((mine[:, :, lk:] == ar.PAD_VALUE).all())
    # the plain layout: keys in order, pads finite, one group above the minimum accepted
    v = rnd(2, 7, 16, seed=5)
    p = ar.pack_vt_plain(v, 16)
    assert torch.equal(p[:2 * 16 * 16].view(2, 16, 16)[:, :, :7], v.transpose(1, 2))
    assert bool((p[:2 * 16 * 16].view(2, 16, 16)[:, :, 7:] == ar.PAD_VALUE).all()) and bool(p[2 * 16 * 16:].isnan().all())


def test_packed_buffers_poison_everything_the_contract_leaves_unread():
    B, L, C = 2, 5, 24
    q, k = rnd(B, L, C, seed=1), rnd(B, L, C, seed=2)
    buf = ar.pack_rows(q, C + 16, col0=8)
    body = buf[8:8 + B * L * (C + 16)].view(B, L, C + 16)
    assert torch.equal(body[:, :, :C], q) and bool(body[:, :, C:].isnan().all())
    assert bool(buf[:8].isnan().all()) and bool(buf[8 + B * L * (C + 16):].isnan().all()) and buf.numel() == 8 + B * L * (C + 16) + kit.GUARD
    qk = ar.pack_fused_qk(q, k)
    body = qk[:B * L * 2 * C].view(B, L, 2 * C)
    assert torch.equal(body[:, :, :C], q) and torch.equal(body[:, :, C:], k)
    assert bool(qk[B * L * 2 * C:].isnan().all())
    out = ar.new_out(B, L, C + 8)
    written, rest = ar.split_out(out, B, L, C, C + 8)
    assert bool(written.isnan().all()) and rest.numel() == B * L * 8 + kit.GUARD and bool((rest == kit.sentinel_bits(F16)).all())


def test_the_table_reaches_every_kernel_of_the_file():
    """All ten attention_kernel instantiations in both V^T forms, the pipelined kernel, and both wave counts of the three wide ones."""
    seen = {(ar.generic_instantiation(c.d, c.B, c.H, c.lq, c.lk), c.vt) for c in ar.CASES if c.kind == "generic"}
    assert seen == {(i, vt) for i in ar.ALL_INSTANTIATIONS for vt in ("plain", "perm16")}
    assert {c.d for c in ar.CASES if c.family == "generic"} == set(range(8, 161, 8))
    # the pipelined kernel is only legal (and here forced) at d = 40, whole key tiles, at least two, PERM16
    sp = [c for c in ar.CASES if c.kind == "sp"]
    assert sp and all(c.d == 40 and c.lk % 64 == 0 and c.lk >= 128 and c.vt == "perm16" for c in sp)
    assert {c.lk // 64 for c in sp} == {2, 3, 4} and {77, 256, 300} <= {c.lq for c in sp}
    # ... and the library never picks it on its own for a `generic` row (its choice needs whole key tiles and >= 256 blocks)
    assert not any(c.d == 40 and c.vt == "perm16" and c.lk % 64 == 0 and c.lk >= 128 and c.B * c.H * ((c.lq + 255) // 256) >= 256
                   for c in ar.CASES if c.kind == "generic")
    wide = {(c.d, c.B * c.H * ((c.lq + 127) // 128) >= 256) for c in ar.CASES if c.kind == "wide"}
    assert wide == {(d, e) for d in (128, 256, 512) for e in (False, True)}
    assert len({c.id for c in ar.CASES}) == len(ar.CASES)
    for c in ar.CASES:                                   # every row is a launch the entry points accept
        ld = c.leading_dims()
        assert ld["ldq"] % 8 == 0 and ld["ldk"] % 8 == 0 and ld["ldo"] % 4 == 0 and ld["ldv"] % (16 if c.vt == "perm16" else 8) == 0
        assert min(ld["ldq"], ld["ldk"], ld["ldo"]) >= c.C and ld["ldv"] >= c.lk and (c.ld not in ("fused", "fusedx") or c.lq == c.lk)


def _yard_key(c):
    return (c.d, c.B, c.H, c.lq, c.lk, c.data, c.compared(), c.kind == "sp")


_UNIQUE = list({_yard_key(c): c for c in ar.CASES}.values())      # layouts and strides do not change the arithmetic


@pytest.mark.parametrize("case", _UNIQUE, ids=lambda c: c.id)
def test_emulation_is_within_its_stated_bound(case):
    """|emulation - float64| <= emulation_bound element by element, and the case's yardstick: e_emu and the device bound."""
    q, k, v = (ar.select(t, case.compared(), case.d) for t in ar.make_inputs(case))
    round_q = case.kind == "sp"
    ref = ar.attention_f64(q, k, v, 1, case.d ** -0.5)
    emu = ar.attention_fp16_emulation(q, k, v, 1, case.d ** -0.5, round_q=round_q)
    bound = ar.emulation_bound(q, k, v, 1, case.d ** -0.5, round_q=round_q)
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(emu.float()).all())
    worst = float(((emu.double() - ref).abs() / bound).max())
    y = ar.yardstick(case)
    print(f"ATTN_YARD {case.id} family={case.family} e_emu={y.e_emu:.3e} bound={y.bound:.3e} emu/stated={worst:.2f}")
    assert worst <= 1.0
    assert torch.equal(y.ref, ref) and y.e_emu == float(ar.query_error(emu, ref, 1).max()) and y.bound == max(4 * y.e_emu, 2.0 ** -10)
    assert y.e_emu < 2.0 ** -6                                     # a yardstick this loose would measure nothing
