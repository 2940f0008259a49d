"""CPU checks of tests/elementwise_ref.py and of the argument checks of coma_amd/csrc/sd_elementwise.hip / sd_text.hip: every reference
against an independent formulation (oracle/sd_oracle.py, scipy, G20 of tests/golden/inpaint_golden.npz, torch's softmax and fp16
conversion), every emulation against its own a-priori bound and through the very assertions the device is held to, the poison of the
packed buffers, that the table reaches every branch, that each deliberately broken emulation fails a named case, and every refusal row
through the REAL entry points with dummy non-null pointers: the argument checks run before any HIP call, so without a device a refused
row returns COMA_E_INVALID with its text and a wrongly accepted one fails at launch with another code.  The per-case yardstick e_emu is
printed here, without a GPU: `pytest -s tests/test_elementwise_ref_host.py`."""
import os

import numpy as np
import pytest
import torch

from coma_amd import _lib
from oracle import sd_oracle as so
from tests import domain_kit as kit
from tests import elementwise_ref as er

f16, f32, f64 = np.float16, np.float32, np.float64
BY_ID = {c.id: c for c in er.CASES}
G = kit.GUARD


def _bodies(c, src):
    """the bodies emulate() returns, completed with the first contents of what the launch leaves alone"""
    out = dict(src)
    for name, o in er.plan(c)[1].items():
        if out.get(name) is None:
            n = o.buf.numel() - 2 * G - o.off
            out[name] = o.buf.numpy()[G + o.off:G + o.off + n].copy()
    return out


@pytest.mark.parametrize("case", er.CASES, ids=lambda c: c.id)
def test_the_emulation_passes_the_device_checks_within_its_stated_bound(case):
    """check() -- the assertions tests/test_sd_elementwise_domain_gpu.py applies to the device -- on the fp32 emulation of the same case:
    the exact contracts hold bit for bit, the arithmetic stays within its a-priori counted bound, and the bound the device gets is
    max(4 e_emu, floor) with a yardstick that measures something."""
    c = case
    fig = er.check(c, _bodies(c, er.emulate(c)))
    for name, (e_emu, bound, share) in er.yardstick(c).items():
        print(f"ELEMENTWISE_YARD {c.id} {name} e_emu={e_emu:.3e} bound={bound:.3e} emu/stated={share:.2f}")
        assert share <= 1.0 and 0 <= e_emu < 2.0 ** -8, (name, e_emu, share)
        floor = er.reference(c)["lat" if name == "lat" else name].floor
        assert bound == max(4 * e_emu, floor)
    assert all(f.err <= f.bound or np.isnan(f.bound) for f in fig.values())
    # no guard element is ever owned by the launch; every float operand sits between NaN guards
    ins, outs = er.plan(c)
    for name, o in outs.items():
        assert int(o.must[:G + o.off].sum()) == 0 and int(o.must[-G:].sum()) == 0, name
    for name, i in ins.items():
        if i.buf.is_floating_point():
            assert bool(i.buf[:G].isnan().all()) and bool(i.buf[-G:].isnan().all()), name


def test_conversions_by_bits_are_torchs_and_numpys():
    h = np.arange(1 << 16, dtype=np.uint16)
    h = h[(h & 0x7FFF) <= 0x7C00]
    mine = er.f16_bits_to_f32(h)
    assert np.array_equal(kit.bits(mine), kit.bits(h.view(f16).astype(f32)))
    assert torch.equal(torch.from_numpy(mine).view(torch.int32), torch.from_numpy(h.view(f16).copy()).float().view(torch.int32))
    g = np.random.default_rng(3)
    x = np.concatenate([er.SPECIAL32, er.interesting32(g, 200000), (mine.astype(f64) * (1 + 2.0 ** -11)).astype(f32), np.nextafter(mine, f32(np.inf)),
                        np.nextafter(mine, f32(-np.inf)), ((mine.astype(f64) + np.roll(mine, 1).astype(f64)) / 2).astype(f32)])
    x = x[~np.isnan(x)]
    got = er.f32_to_f16_bits(x)
    with np.errstate(over="ignore"):
        assert np.array_equal(got, kit.bits(x.astype(f16)))
    assert torch.equal(torch.from_numpy(got.view(np.int16)), torch.from_numpy(x).to(torch.float16).view(torch.int16))
    b = lambda v: int(er.f32_to_f16_bits(np.array([v], f32))[0])
    assert b(65520.0) == 0x7C00 and b(-65520.0) == 0xFC00 and b(65519.996) == 0x7BFF and b(2.0 ** -25) == 0 and b(1.5 * 2.0 ** -24) == 2
    assert b(1 + 2.0 ** -11) == 0x3C00 and b(1 + 3 * 2.0 ** -11) == 0x3C02 and b(-0.0) == 0x8000 and b(3e-8) == 1


def test_ddim_reference_is_the_oracles():
    alphas = so.ddim_alphas()
    for cid, t in (("ddim-n1-ld4-first", 981), ("ddim-n255-ld8-g0-mid", 501), ("ddim-n513-ld72-keep-latents", 501)):
        c = BY_ID[cid]
        d, r = er.data(c), er.reference(c)
        assert (d["alpha_t"], d["alpha_prev"]) == (float(alphas[t]), float(alphas[t - 20]))
        n = c.B * c.hw
        eu, ec = torch.from_numpy(d["eps"][:n].astype(f64)), torch.from_numpy(d["eps"][n:].astype(f64))
        eps = eu + c.guidance * (ec - eu)
        prev, x0 = so.ddim_step_ref(eps, t, torch.from_numpy(d["latents"]), alphas)
        # the oracle takes the float64 alphas, the entry point their fp32 roundings: 2^-24 relative in each coefficient
        for mine, theirs in ((r["latents"], prev), (r["x0"], x0)):
            assert float((np.abs(mine.ref - theirs.numpy()) / mine.norm).max()) < 4 * 2.0 ** -24
    last = er.data(BY_ID["ddim-n256-ld64-g1-last"])
    assert (last["alpha_t"], last["alpha_prev"]) == (float(alphas[1]), float(alphas[0]))
    for c in (x for x in er.CASES if isinstance(x, er.DD) and x.mode != "step"):
        d = er.data(c)
        both = np.concatenate([kit.bits(d["mask"]), kit.bits(d["masked"]).reshape(-1)])
        if c.B * c.hw > 100:
            assert (both == 0x8000).any() and (both == 0).any() and ((both & 0x7C00 == 0) & (both & 0x3FF != 0)).any(), c.id     # -0, +0, subnormals
    p1, p0, t1 = (er.data(BY_ID[i]) for i in ("ddim-n257-ld72-g11-prev1", "ddim-n513-ld64-prev0", "ddim-n256-ld8-t1"))
    assert p1["alpha_prev"] == 1.0 and p0["alpha_prev"] == 0.0 and t1["alpha_t"] == 1.0
    r = er.reference(BY_ID["ddim-n257-ld72-g11-prev1"])
    assert np.array_equal(r["latents"].ref, r["x0"].ref)                                        # the final step: x_prev = x0


def test_timestep_embedding_reference_is_the_oracles():
    for c in (x for x in er.CASES if isinstance(x, er.TE)):
        r = er.reference(c)["out"]
        theirs = so.timestep_embedding_ref(torch.tensor(c.t), c.dim).numpy()
        assert r.ref.shape == theirs.shape and float(np.abs(r.ref - theirs).max()) < 2e-4       # the oracle is an fp32 evaluation
        for b, t in enumerate(c.t):
            if t == 0.0:
                assert np.array_equal(r.ref[b], np.r_[np.ones(c.dim // 2), np.zeros(c.dim // 2)])
    assert {t for c in er.CASES if isinstance(c, er.TE) for t in c.t} == {0.0, 1.0, 500.5, 981.0, 999.0, 1000.0}


def test_layout_references_are_torchs_permute_and_conversion():
    for c in (x for x in er.CASES if isinstance(x, er.NC)):
        x = torch.from_numpy(er.data(c)["x"]).view(c.B, c.c, c.hw)
        theirs = torch.zeros(c.B, c.hw, c.cpad, dtype=torch.float16)
        theirs[:, :, :c.c] = x.permute(0, 2, 1).to(torch.float16)
        assert np.array_equal(er.reference(c)["out"].view(np.int16), theirs.view(torch.int16).numpy().reshape(-1, c.cpad)), c.id
    for c in (x for x in er.CASES if isinstance(x, er.NH)):
        x = torch.from_numpy(er.data(c)["x"].copy()).view(c.B, c.hw, c.c)
        theirs = x.permute(0, 2, 1).float().reshape(1, -1)
        assert np.array_equal(kit.bits(er.reference(c)["out"]), kit.bits(theirs.numpy())), c.id
        assert bool(er.plan(c)[0]["x"].buf[G:-G].view(-1, c.ld)[:, c.c:].isnan().all())
    every = np.concatenate([er.f32_to_f16_bits(er.data(c)["x"]) for c in er.CASES if isinstance(c, er.NC)])
    assert {0, 0x8000, 0x7C00, 0xFC00, 1, 2, 0x3C00, 0x3C02}.issubset(set(every.tolist()))


def test_image_table_is_exhaustive_and_lands_on_ties():
    c = BY_ID["u8-ld64-round"]
    x = er.data(c)["x"]
    assert x.shape == (er.N_F16, 3) and er.N_F16 == 63490
    for ch in range(3):
        assert np.unique(kit.bits(x[:, ch])).size == er.N_F16
    v = np.clip(x[:, 0].astype(f64) * 0.5 + 0.5, 0, 1) * 255                                   # float64: exact for the halved value, one rounding away for the product
    v32 = (np.clip(x[:, 0].astype(f32) * f32(0.5) + f32(0.5), 0, 1) * f32(255)).astype(f64)
    ties = v32[(v32 - np.floor(v32)) == 0.5]
    assert ties.size >= 2 and 127.5 in ties                                                    # x = +0 and -0 at the least: 127.5 -> 128 (even), truncated 127
    print(f"ELEMENTWISE_U8 values landing on k + 0.5: {sorted(set(ties.tolist()))}")
    r, t = er.emulate(c)["out"][:, 0], er.emulate(BY_ID["u8-ld64-trunc"])["out"][:, 0]
    assert np.array_equal(t, np.floor(v32).astype(np.uint8)) and np.array_equal(r, np.rint(v32).astype(np.uint8))
    assert int(r[kit.bits(x[:, 0]) == 0][0]) == 128 and int(t[kit.bits(x[:, 0]) == 0][0]) == 127
    assert int((r != t).sum()) > 10000 and int(np.abs(r.astype(int) - np.rint(v)).max()) <= 1
    assert bool(er.plan(c)[0]["x"].buf[G:-G].view(-1, 64)[:, 3:].isnan().all())


def test_vae_sample_reference_is_the_oracles_and_reaches_both_clamps():
    seen = set()
    for c in (x for x in er.CASES if isinstance(x, er.VS)):
        d, r = er.data(c), er.reference(c)["lat"]
        seen |= set(d["mom"][:, 4:].astype(f64).reshape(-1).tolist())
        mom = torch.from_numpy(d["mom"].astype(f32)).t().reshape(1, 8, c.npix, 1)               # NCHW, as the oracle chunks it
        nz = torch.from_numpy(d["noise"]).t().reshape(1, 4, c.npix, 1) * (1 if c.noise else 0)
        theirs = so.vae_sample_ref(mom, nz, d["scale"]).reshape(4, c.npix).t().numpy()
        assert float((np.abs(r.ref - theirs) / r.norm).max()) < 8 * 2.0 ** -24, c.id          # the oracle is an fp32 evaluation
        emu = er.emulate(c)
        assert all(bool(np.isfinite(v.astype(f64)).all()) for v in emu.values()) and float(np.abs(r.ref).max()) < 60000
    assert {-40.0, -30.5, -30.0, 0.0, 19.5, 20.0, 25.0, np.inf, -np.inf}.issubset(seen)


def test_mask_reference_is_the_oracles_and_scipys():
    from scipy.ndimage import binary_dilation
    for c in (x for x in er.CASES if isinstance(x, er.MA)):
        d, r = er.data(c), er.reference(c)
        full = r["mask_full"].reshape(c.B, c.H, c.W)
        for b in range(c.B):
            seg = d["seg"][b]
            if c.iters <= 8:
                theirs = so.adapt_mask_ref(seg, d["dflt"][b], c.iters, bool(c.force), d["thres"] / (512 * 512))
                assert np.array_equal(full[b], theirs.astype(np.uint8)), (c.id, b)
            if not d["use_default"][b]:
                dil = binary_dilation(seg != 0, structure=np.ones((3, 3), bool), iterations=c.iters) if c.iters else seg != 0
                assert np.array_equal(full[b] != 0, dil & (d["dflt"][b] != 0)), (c.id, b)
        assert np.array_equal(r["mask_lat"].view(f16).astype(int).reshape(c.B, c.H // 8, c.W // 8), full[:, ::8, ::8])
        assert int(r["area"].max()) <= 255 * c.H * c.W and (c.force or np.array_equal(r["area"][0], d["seg"].reshape(c.B, -1).sum(-1, dtype=np.int64)))
        assert np.array_equal(er.emulate(c)["mask_full"], r["mask_full"])                         # the separable emulation against the window loops


def test_mask_reference_is_g20():
    """G20 of tests/golden/inpaint_golden.npz (scipy's binary_dilation at 512 x 512, recorded independently of the oracle): the reference on
    all four segmentations x k in {0, 1, 5, 20}, the area decision included -- two of the images lie below the threshold and take the
    default mask, two are dilated."""
    gi = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inpaint_golden.npz"))
    unpack = lambda a: np.unpackbits(a, axis=-1)
    segs, default, ks, adapted = unpack(gi["g20_segs"]), unpack(gi["g20_default"]), [int(k) for k in gi["g20_ks"]], unpack(gi["g20_adapted"])
    thres = 512 * 512 * float(gi["g20_thres"])
    use_default = [bool(s.sum() < thres) for s in segs]
    assert segs.shape == (4, 512, 512) and adapted.shape == (4, 4, 512, 512) and ks == [0, 1, 5, 20] and use_default == [False, True, True, False]
    dflt = np.broadcast_to(default, segs.shape)
    for j, k in enumerate(ks):
        mine = er.mask_reference(segs, dflt, k, use_default)
        for b in range(4):
            assert np.array_equal(mine[b], adapted[b, j]), (b, k)


def test_the_poison_is_effective():
    # u8 masks: reading one guard byte in place of a pixel changes the reference's output
    c = BY_ID["maskB-8x8-k1-corners-255-eq-pad16w"]
    d, r = er.data(c), er.reference(c)
    seg = d["seg"][0].copy()
    assert seg[3, 3] == 0 and er.SEG_GUARD != 0
    seg[3, 3] = er.SEG_GUARD
    assert int(seg.astype(np.int64).sum()) != int(d["area"][0])
    assert not np.array_equal(er.dilate_loops(seg, c.iters) & (d["dflt"][0] != 0), r["mask_full"].reshape(8, 8) != 0)
    # the default mask: one of its zero pixels read from the guard sets a pixel of the adapted mask, and of the forced default mask
    full = r["mask_full"].reshape(1, 8, 8)
    zeros = [tuple(z) for z in np.argwhere(d["dflt"][0] == 0) if er.dilate_loops(d["seg"][0], c.iters)[tuple(z)]]
    assert zeros and not d["use_default"][0]
    dm = d["dflt"].copy()
    dm[0][zeros[0]] = er.DFLT_GUARD
    assert not np.array_equal(er.mask_reference(d["seg"], dm, c.iters, d["use_default"]), full)
    forced = BY_ID["maskB-64x96-b3-force-pad64"]
    fd = er.data(forced)
    z = tuple(np.argwhere(fd["dflt"] == 0)[0])
    dm = fd["dflt"].copy()
    dm[z] = er.DFLT_GUARD
    assert not np.array_equal(er.mask_reference(fd["seg"], dm, forced.iters, fd["use_default"]), er.reference(forced)["mask_full"].reshape(fd["seg"].shape))
    ins, outs = er.plan(c)
    assert bool((ins["seg"].buf[:G] == er.SEG_GUARD).all()) and bool((ins["seg"].buf[-G:] == er.SEG_GUARD).all()) and bool((ins["dflt"].buf[:G] == er.DFLT_GUARD).all())
    assert "seg" not in er.plan(forced)[0] and "scratch" not in er.plan(forced)[1]
    # floats: NaN guards and gap columns
    for cid, name, ld, w in (("ddim-n513-ld72-keep-latents", "eps", 72, 4), ("vae-n64-ld64-f16", "mom", 64, 8), ("causal-len5-h12", "k", 12 * 64 + 16, 12 * 64)):
        b = er.plan(BY_ID[cid])[0][name].buf
        assert bool(b[:G].isnan().all()) and bool(b[-G:].isnan().all())
        rows = b[G:-G].view(-1, ld)
        assert bool(rows[:, w:].isnan().all()) and not bool(rows[:, :w].isnan().any())
    tx = BY_ID["embed-w512-len77-pos80-s3"]
    assert bool(er.plan(tx)[0]["pos"].buf[G:-G].view(80, 512)[77:].isnan().all()) and bool((er.plan(tx)[0]["ids"].buf[:G] == er.ID_GUARD).all())
    ids = er.data(tx)["ids"]
    assert -5 in ids and tx.vocab + 7 in ids
    # an id read from the guard is clamped to the last row of the table: with more than one row that changes the output row (with
    # vocab = 1 every id gives row 0, no id value can show a stray read there; the NaN guards of the tables still do)
    td = er.data(tx)
    row = next(i for i in range(ids.size) if 0 <= ids[i] < tx.vocab - 1)
    stray = er.f32_to_f16_bits(td["tok"][min(er.ID_GUARD, tx.vocab - 1)].astype(f32) + td["pos"][row % tx.len].astype(f32))
    assert not np.array_equal(stray, er.reference(tx)["out"][row])
    # outputs: the sentinel everywhere, guards and gap columns outside `must`
    o = er.plan(BY_ID["causal-len65-h1"])[1]["out"]
    assert o.off == 1 and bool((kit.bits(o.buf) == kit.sentinel_bits(o.buf.dtype)).all()) and int(o.must.sum()) == 65 * 64 and not bool(o.must[:G + 1].any())
    assert not bool(o.must[G + 1:G + 1 + 65 * 67].view(65, 67)[:, 64:].any())
    m = er.plan(BY_ID["maskB-8x8-k8-one-pad64"])[1]["masked"]
    assert int(m.must.sum()) == 64 * 8 and int(er.plan(BY_ID["maskB-16x264-k264-one-pad64w"])[1]["masked"].must.sum()) == 16 * 264 * 64
    la = er.plan(BY_ID["ddim-n513-ld72-keep-latents"])[1]["latents"]
    assert not bool(la.must.any()) and not bool(la.buf[G:-G].isnan().any()) and bool(la.buf[:G].isnan().all())


def test_text_and_causal_references_are_torchs():
    for c in (x for x in er.CASES if isinstance(x, er.TX)):
        d = er.data(c)
        ids = torch.from_numpy(np.clip(d["ids"], 0, c.vocab - 1)).long()
        tok, pos = torch.from_numpy(d["tok"]), torch.from_numpy(d["pos"][:c.len])
        theirs = (tok[ids].float().view(c.seqs, c.len, c.width) + pos.float()[None]).to(torch.float16)
        assert np.array_equal(er.reference(c)["out"].view(np.int16), theirs.view(torch.int16).numpy().reshape(-1, c.width)), c.id
    for c in (x for x in er.CASES if isinstance(x, er.CA)):
        d, r = er.data(c), er.reference(c)["out"]
        q, k, v = (torch.from_numpy(d[n].astype(f64)).view(c.seqs, c.len, c.heads, 64).transpose(1, 2) for n in "qkv")
        s = q @ k.transpose(-1, -2) * 0.125
        s = s.masked_fill(torch.triu(torch.ones(c.len, c.len, dtype=torch.bool), 1), float("-inf"))
        theirs = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(c.seqs * c.len, c.heads * 64).numpy()
        assert float(np.abs(r.ref - theirs).max()) <= 1e-12 * float(np.abs(theirs).max()), c.id
        ldq, ldk, ldv = er.ca_lds(c)
        w = c.heads * 64
        assert all(ld >= w and ld % 8 == 0 for ld in (ldq, ldk, ldv)) and (c.layout == "packed" or len({ldq, ldk, ldv}) == 3)
    sharp = er.reference(BY_ID["causal-len128-h12-s2-sharp"])["out"]
    assert {c.len for c in er.CASES if isinstance(c, er.CA)} >= {1, 2, 3, 4, 5, 63, 64, 65, 127, 128}
    assert {c.heads for c in er.CASES if isinstance(c, er.CA)} == {1, 3, 12} and {c.seqs for c in er.CASES if isinstance(c, er.CA)} == {1, 2}
    assert float(np.abs(sharp.ref).max()) > 1.0


def test_the_table_reaches_every_branch():
    seen = set()
    for c in er.CASES:
        seen |= er.branches(c)
    assert seen == er.REACHABLE, (sorted(seen - er.REACHABLE), sorted(er.REACHABLE - seen))
    assert len({c.id for c in er.CASES}) == len(er.CASES)
    count = {}
    for c in er.CASES:
        count[c.entry] = count.get(c.entry, 0) + 1
    print("ELEMENTWISE_TABLE " + " ".join(f"{k}={v}" for k, v in sorted(count.items())) + f" total={len(er.CASES)} branches={len(er.REACHABLE)}")
    assert set(count) == set(er.REFUSALS) <= set(_lib.PARAMS) and len(count) == 11
    dd = [c for c in er.CASES if isinstance(c, er.DD)]
    assert {c.B * c.hw for c in dd} == {1, 255, 256, 257, 513} and {c.B for c in dd} == {1, 2, 3} and {c.eps_ld for c in dd} == {4, 8, 64, 72}
    assert {c.guidance for c in dd} == {0.0, 1.0, 7.5, 11.0}
    te = [c for c in er.CASES if isinstance(c, er.TE)]
    assert {c.dim for c in te} == {2, 4, 6, 320, 1280, 258} and {c.B for c in te} == {1, 3, 5}
    for kind, ld in ((er.NC, "cpad"), (er.NH, "ld")):
        ly = [c for c in er.CASES if isinstance(c, kind)]
        assert {c.c for c in ly} == {1, 3, 4, 9} and {getattr(c, ld) - c.c for c in ly} >= {0, 1} and {getattr(c, ld) for c in ly} >= {8, 64}
        assert any(c.B == 2 and c.hw == 1 for c in ly)
    assert {(c.ld, c.round_mode) for c in er.CASES if isinstance(c, er.U8)} == {(l, r) for l in (3, 4, 64) for r in (0, 1)}
    vs = [c for c in er.CASES if isinstance(c, er.VS)]
    assert {c.npix for c in vs} == {1, 63, 64, 65, 257} and {c.ld for c in vs} == {8, 16, 64} and {(c.noise, c.outs) for c in vs} == {(n, o) for n in (0, 1) for o in ("f32", "f16", "both")}
    an = [c for c in er.CASES if isinstance(c, er.AN)]
    assert {c.n for c in an} == {1, 255, 256, 257, 1025} and {c.alpha for c in an} == {1.0, 0.9991, 0.0047, 1e-6}
    mb = [c for c in er.CASES if isinstance(c, er.MA) and not c.single]
    m1 = [c for c in er.CASES if isinstance(c, er.MA) and c.single]
    assert {(c.B, c.H, c.W) for c in mb} == {(1, 8, 8), (1, 8, 136), (1, 16, 264), (1, 24, 8), (3, 64, 96)}
    assert {(c.cpad, c.write_pad) for c in mb} == {(p, w) for p in (8, 16, 64) for w in (0, 1)} and {c.dval for c in mb} == {0, 1, 255}
    assert {c.segval for c in mb} == {"1", "255", "mixed"} and {c.cpad for c in m1} == {3, 5, 8, 64}
    tx = [c for c in er.CASES if isinstance(c, er.TX)]
    assert {c.width for c in tx} == {8, 512, 520, 768, 1032} and {c.len for c in tx} == {1, 77} and {c.vocab for c in tx} == {1, 300} and {c.seqs for c in tx} == {1, 3}


# mutation -> the cases that have to notice it
MUTANTS = {
    "ignore-write-latents": ("ddim-n513-ld72-keep-latents", "ddim-n255-ld4-keep-latents-last"),
    "area-le": ("maskB-8x8-k1-corners-255-eq-pad16w", "maskB-16x264-k1-lastcol-255-eq", "mask1-64x96-k3-random-eq-pad3"),
    "area-count-nonzero": ("maskB-8x8-k1-corners-255-eq-pad16w", "maskB-64x96-b3-k3-per-image-split"),
    "row-dilation-wraps": ("maskB-8x136-k1-lastcol-neg", "maskB-16x264-k1-lastcol-255-eq", "mask1-8x136-k3-lastcol-pad5"),
    "round-mode-truncates": ("u8-ld3-round", "u8-ld4-round", "u8-ld64-round"),
    "logvar-clamp-20": ("vae-n63-ld16-f32", "vae-n257-ld16-both", "vae-n64-ld64-f16"),
    "causal-key-i+1": ("causal-len2-h3-s2-sharp", "causal-len65-h1", "causal-len128-h12-s2-sharp"),
    "pos-row-not-mod-len": ("embed-w512-len77-pos80-s3", "embed-w768-len1-pos4-s3", "embed-w768-len77-s3"),
}


@pytest.mark.parametrize("mut", er.MUTATIONS)
def test_a_broken_kernel_fails_a_named_case(mut):
    """The emulation with one deliberate defect, put through check(): every case named for the mutation fails."""
    assert set(MUTANTS) == set(er.MUTATIONS)
    for cid in MUTANTS[mut]:
        c = BY_ID[cid]
        with pytest.raises(AssertionError):
            er.check(c, _bodies(c, er.emulate(c, mut)))
        er.check(c, _bodies(c, er.emulate(c)))


@pytest.mark.parametrize("entry", sorted(er.REFUSALS), ids=str)
def test_every_refusal_gives_its_code_and_text_through_the_entry_point(entry, hip_lib):
    base, rows = er.REFUSALS[entry]
    assert len(rows) >= 7 and set(base) == set(_lib.PARAMS[entry][:-1])       # the header's own parameter names
    # the control: the base row passes every argument check and only fails where the launch needs a device
    kit.check_refusals(hip_lib, {entry: er.REFUSALS[entry]}, kit.host_resolver(), expect_control=not torch.cuda.is_available())


def test_the_area_limit_is_where_the_int32_sum_ends():
    """2064 x 4096 at value 255 is the first multiple-of-8 shape of that width whose value sum leaves int32; one row of tiles less fits."""
    assert 2064 * 4096 * 255 == 2155806720 > er.INT32_MAX >= 2056 * 4096 * 255
    assert np.int32(np.int64(2155806720).astype(np.int32)) < 0                                 # what the unchecked sum wrapped to
