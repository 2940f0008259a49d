"""CPU checks of tests/contact_ref.py and tests/occupancy_ref.py and of the argument checks of coma_contact_accumulate_f32,
coma_occupancy_splat, coma_occupancy_reduce and coma_occupancy_fused: that the two tables reach every regime (counted through the
emulations), the conditions on the near-threshold cases and on what a case leaves out of its comparison, the references against
oracle/coma_oracle.py, the emulations through the very assertions the device is held to, that each deliberately broken emulation fails
named cases, and every refusal row through the REAL entry points with dummy non-null pointers (the argument checks run before any HIP
call).  The per-case yardsticks are printed here, without a GPU: `pytest -s tests/test_coma_core_ref_host.py`."""
import numpy as np
import pytest
import torch

from coma_amd import _lib
from coma_amd import coma_occupancy as co
from oracle import coma_oracle as orc
from tests import contact_ref as cr
from tests import domain_kit as kit
from tests import occupancy_ref as orf

f32, f64 = np.float32, np.float64


def _occ_got(c, mut=None):
    """the three routes as check() wants them, from the emulation of the fused pass (the splat route's raw counts are the reference's)"""
    e0, e1 = orf.emulate(c.id, mut), orf.emulate(c.id, mut, write_raw=1)
    return {"fused": e0, "fused_raw": e1, "splat": dict(e0, raw=orf.reference(c.id)["counts"].astype(f32).reshape(-1))}


# ------------------------------------------------------------------------------------------------------------------ the tables
def test_the_contact_table_reaches_every_regime():
    seen = set().union(*(cr.branches(c.id) for c in cr.CASES))
    assert seen == cr.REACHABLE, dict(unreached=sorted(cr.REACHABLE - seen), unlisted=sorted(seen - cr.REACHABLE))
    print(f"CONTACT_TABLE cases={len(cr.CASES)} regimes={len(cr.REACHABLE)}")
    assert {c.H * c.O for c in cr.CASES} >= {1, 7, 8, 9, 31, 32, 33, 63} and {c.N for c in cr.CASES} >= {1, 63, 64, 65, 255, 256, 257, 513}
    assert {c.S for c in cr.CASES} >= {0, 1, 7, 8, 9, 17, 300} and {c.sigma for c in cr.CASES} == {0.05, 0.2, 0.25, 2.0}
    assert any(8 % c.O for c in cr.CASES) and {bool(c.stride) for c in cr.CASES} == {False, True}
    for c in cr.CASES:                                            # no case leaves more than 5 % of its elements out of the comparison
        if c.S:
            _, skipped, total = cr.yardstick(c.id)
            assert skipped <= 0.05 * total, (c.id, skipped, total)


def test_the_contact_data_holds_what_the_table_says():
    c = cr.BY_ID["contact-ho13-n8-s2-straddle"]
    dist = cr._pairs(c, cr.data(c.id))[0]
    t = f32(cr.THRES)
    assert sorted(set(dist[0].tolist())) == sorted(float(cr._ulps(t, k)) for k in range(-6, 7))          # sqrt(fl(x^2)) == x for every one of them
    ref = cr.reference(c.id)
    assert np.array_equal(ref["cnt"] - cr.data(c.id)["state"]["cnt"], 1.0 * (np.arange(13) != 6))        # below in one of the two samples; k = 0: equal is not below
    c = cr.BY_ID["contact-ho20-n64-s8-special-zero"]
    d, ref = cr.data(c.id), cr.reference(c.id)
    P1 = ref["P1"].reshape(c.H, c.O, c.N)
    assert np.isnan(P1[1]).all() and np.isfinite(P1[[0, 2, 3]]).all()                                    # the zero normal: its own rows, no other
    assert np.isnan(ref["nom"].reshape(c.H, c.O)[3]).all() and (ref["nom"].reshape(c.H, c.O)[2] >= 0).all()
    assert np.array_equal(ref["cnt"].reshape(c.H, c.O)[2], np.sum(cr._terms(cr._pairs(c, d)[0])[1][1:], 0).reshape(c.H, c.O)[2])   # inf: not below thres
    o1 = cr._pairs(c, d)[3]
    assert (o1[:, 0::c.O][:, :1] == 0).all() and ((o1[:, 1] > 0) & (o1[:, 1] < 1e-6)).all()              # exactly antiparallel / a few ulps off
    shared = cr.data("contact-ho33-n257-s9-special")
    assert shared["ov"].shape[0] == 1 and cr.BY_ID["contact-ho33-n257-s9-special"].stride == 0


def test_the_occupancy_table_reaches_every_regime():
    seen = set().union(*(orf.branches(c.id) for c in orf.CASES))
    assert seen == orf.REACHABLE, dict(unreached=sorted(orf.REACHABLE - seen), unlisted=sorted(seen - orf.REACHABLE))
    print(f"OCC_TABLE cases={len(orf.CASES)} regimes={len(orf.REACHABLE)}")
    assert {c.R for c in orf.CASES} >= {2, 6, 8, 30, 64, 100, 102, 142} and {orf.data(c.id)["window"] for c in orf.CASES} >= {3, 4, 5, 7, 8, 9, 16}
    assert len(orf.NEAR_CASES) >= 6
    for cid in orf.NEAR_CASES:                                    # at least 32 cells inside the band on each side of the cut
        st = orf.emulate(cid)["stats"]
        print(f"OCC_BAND {cid} prep_recount_planes={st['prep_recount']} amb_hit={st['amb_hit']} amb_miss={st['amb_miss']} f32_hit={st['fast_hit']} f32_miss={st['fast_miss']}")
        assert st["amb_hit"] >= 32 and st["amb_miss"] >= 32 and st["prep_recount"] >= 32, (cid, st)
    # the buckets the issue names: exactly 512, 513, above 1024, and the pairs of rows that share a group
    bk = orf.emulate("occ-crowd-rounds")["stats"]["buckets"]
    assert bk[:, 1].tolist() == [512, 513, 1040] and orf.layout(30, 3) == (22, 2, 3)
    bk = orf.emulate("occ-crowd-hand-over")["stats"]["buckets"][:, 1]
    assert orf.layout(30, 260)[2] == 256 and [(260 * g // 256, 260 * (g + 1) // 256) for g in (63, 127, 191, 255)] == [(63, 65), (128, 130), (193, 195), (258, 260)]
    assert bk[63] <= 24 and bk[64] == 1040 and bk[128] == 1048 and bk[129] <= 24 and bk[193] == 512 and bk[194] == 513
    assert orf.layout(64, 5) == (5, 13, 5) and orf.layout(100, 2)[:2] == (2, 50) and orf.layout(102, 7) == (1, 102, 6) and orf.layout(142, 4) == (1, 142, 4)
    ref = orf.reference("occ-cell-255-256-5000")["counts"]
    assert ref[0].max() in (255, 256) and (ref[0] == 255).any() and (ref[1] == 256).any() and ref[2].max() >= 5000
    big = orf.reference("occ-rowsum-above-2^24")
    assert big["rowsum_exact"][0] > 2 ** 24 and float(big["rowsum"][0]) != big["rowsum_exact"][0] or big["rowsum_exact"][0] % 2 == 0


def test_the_occupancy_data_holds_what_the_table_says():
    # the centres are load_voxelgrid's
    for R in (6, 30):
        g, _, meta = co.load_voxelgrid(gridsize=2.4, resolution=R, center=[0, 0, 0])
        ax, voxel = orf.axis_table(R)
        assert voxel == meta["voxel_size"] and all(np.array_equal(a, ax) for a in (g[0, :, 0, 0], g[1, 0, :, 0], g[2, 0, 0, :]))
    # the window rule is ComA_Occupancy._window's, an ulp either side of an integer included
    for tol in (0.5, 1.0, 1.5, 2.5, 3.0, float(np.nextafter(3.0, 0.0)), float(np.nextafter(3.0, 4.0)), 3.5, 7.0):
        o = co.ComA_Occupancy.__new__(co.ComA_Occupancy)
        o.spatial_grid_metadata, o.rel_dist_thres = dict(voxel_size=2.4 / 30), 2.4 / 30 * tol
        assert o._window() == orf.window_needed(2.4 / 30, 2.4 / 30 * tol)
        assert orf.sqrt_cut(o.rel_dist_thres) == co.ComA_Occupancy._sqrt_cut(o.rel_dist_thres)
    assert [orf.data(i)["window"] for i in ("occ-r30-w8-tol-below-3", "occ-r30-w8-near", "occ-r30-w8-tol-above-3")] == [8, 8, 8]
    # the hand-made tables: d == thres exactly, the cell is not a hit; in `hand-cut` fl(thres^2) lies above the cut, which is the squared distance
    for cid in ("occ-hand-equal", "occ-hand-cut"):
        d = orf.data(cid)
        q, cen = d["q"][0, 0].astype(f64), d["cen"]
        d2 = ((cen[0][:, None, None] - q[0]) ** 2 + (cen[1][None, :, None] - q[1]) ** 2) + (cen[2][None, None, :] - q[2]) ** 2
        assert (d2 == d["t2"]).any() and (np.sqrt(d2) == d["thres"]).any()
    d = orf.data("occ-hand-cut")
    assert f64(d["thres"]) * f64(d["thres"]) > d["t2"] == 0.3125
    # an empty row is NaN and poisons the unselected maximum; an empty selection gives -inf
    ref = orf.reference("occ-r8-w4")
    assert ref["rowsum_exact"][2] == 0 and np.isnan(ref["norm"][2]).all() and np.isnan(ref["field"]).all()
    assert np.isneginf(orf.reference("occ-r30-w5-none")["field"]).all()
    ref = orf.reference("occ-r64-13-slabs")
    assert ref["rowsum_exact"][3] == 0 and np.isfinite(ref["field"]).all() and not orf.data("occ-r64-13-slabs")["select"][3]
    q = orf.data("occ-r8-w4")["q"][:, 3]
    assert np.isnan(q).any() and np.isinf(q).any() and (np.signbit(q) & np.isnan(q)).any() and (~np.signbit(q) & np.isnan(q)).any()


# ------------------------------------------------------------------------------------------------------------------ references
def test_the_contact_reference_is_the_oracle():
    """oracle/coma_oracle.ComAOracle.aggregate_sample, sample by sample from the same state, against reference(): cnt and den in every bit,
    nom and the histograms to the f32 accuracy of the oracle's own f32 steps (np.exp in f32, the einsum of the skew product)"""
    for cid in ("contact-ho7-n63-s7", "contact-ho15-n100-s300", "contact-ho9-n65-s9-special"):
        c, d, ref = cr.BY_ID[cid], cr.data(cid), cr.reference(cid)
        o = orc.ComAOracle(c.H, c.O, c.N, cr.SIZE, cr.THRES, principle_vec=c.p, sub_principle_vec=c.sp, sigma=c.sigma, eps=cr.EPS)
        st = d["state"]
        o.P_h_wrt_o, o.P_o_wrt_h = st["P1"].reshape(c.H, c.O, c.N).copy(), st["P2"].reshape(c.H, c.O, c.N).copy()
        o.nom, o.den, o.cnt = (st[k].reshape(c.H, c.O).copy() for k in ("nom", "den", "cnt"))
        with np.errstate(all="ignore"):
            for s in range(c.S):
                o.aggregate_sample(d["hv"][s], d["hn"][s], d["ov"][s if c.stride else 0], d["on"][s if c.stride else 0])
        assert np.array_equal(o.cnt.reshape(-1), ref["cnt"]) and np.array_equal(o.den.reshape(-1), ref["den"])
        fin = np.isfinite(ref["nom"])
        assert np.array_equal(np.isnan(o.nom.reshape(-1)), np.isnan(ref["nom"]))
        assert float(np.abs(o.nom.reshape(-1)[fin] - ref["nom"][fin]).max()) <= (c.S + 4) * kit.U32 * float(ref["norm_nom"][fin].max())
        for mine, theirs in ((ref["P1"], o.P_h_wrt_o), (ref["P2"], o.P_o_wrt_h)):
            theirs = theirs.reshape(mine.shape)
            assert np.array_equal(np.isnan(mine), np.isnan(theirs))
            ok = ~np.isnan(mine).any(1)
            tiny = cr._pairs(c, d)[3:]                                            # pairs whose 1 + c is a few ulps: the last bit of the skew product decides
            calm = ok & ~np.any((tiny[0] < 1e-5) | (tiny[1] < 1e-5), axis=0)
            assert float((np.abs(mine[calm] - theirs[calm]).max(1) / np.abs(mine[calm]).max(1)).max()) < 64 * kit.U32, cid


def test_the_occupancy_reference_is_the_oracle():
    for cid in ("occ-r8-w4", "occ-r30-w7", "occ-r30-w8-near"):
        c, d, ref = orf.BY_ID[cid], orf.data(cid), orf.reference(cid)
        o = orc.OccupancyOracle(c.H, c.R, scale_tolerance=c.tol)
        assert o.thres == d["thres"] and o.voxel == d["voxel"] and np.array_equal(o.centers[0, :, 0, 0], d["cen"][0])
        q = np.where(np.isfinite(d["q"]).all(-1, keepdims=True), d["q"], f32(orf.FAR))    # (the oracle's window arithmetic takes finite positions)
        o.aggregate_windowed(q)
        assert np.array_equal(o.occ.reshape(c.H, -1), ref["counts"].astype(f32))
        with np.errstate(all="ignore"):
            field = o.aggregated_grid()
        if d["select"] is None:
            orf.same(field.reshape(-1), ref["field"], cid)
        orf.same(o.occ.reshape(c.H, -1), ref["norm"], cid)


# ------------------------------------------------------------------------------------------------------------------ the emulations
@pytest.mark.parametrize("case", cr.CASES, ids=lambda c: c.id)
def test_the_contact_emulation_passes_the_device_checks(case):
    c = case
    fig = cr.check(c, cr.emulate(c.id))
    for k, f in fig.items():
        print(f"CONTACT_YARD {c.id} out={k} e_emu={f.e_emu:.3e} floor={f.floor:.3e} bound={f.bound:.3e}")
        assert f.bound == max(4 * f.e_emu, f.floor) and f.err == f.e_emu and f.bound < 1e-3


@pytest.mark.parametrize("case", orf.CASES, ids=lambda c: c.id)
def test_the_occupancy_emulation_is_the_reference(case):
    """the fused pass's own decisions -- ranges, f32 decision, band, recount, first-W-cells, counters, table -- give the dense result"""
    n = orf.check(case, _occ_got(case))
    assert n >= (2 if case.big else 3) * (case.H * case.R ** 3)


# ------------------------------------------------------------------------------------------------------------------ planted defects
CONTACT_MUTANTS = {
    "bias-dropped": ("contact-ho8-n64-s8-zero", "contact-ho32-n256-s1-zero", "contact-ho20-n64-s8-special-zero"),
    "ragged-chunk-written-past-n": ("contact-ho1-n1-s1", "contact-ho9-n65-s9-special", "contact-ho33-n257-s9-special", "contact-ho63-n513-s8"),
    "tile-h-from-first-pair": ("contact-ho9-n65-s9-special", "contact-ho33-n257-s9-special", "contact-ho63-n513-s8", "contact-ho15-n100-s300"),
    "slot-past-s-counted": ("contact-ho1-n1-s1", "contact-ho7-n63-s7", "contact-ho9-n65-s9-special", "contact-ho31-n255-s17"),
    "nom-by-every-chunk": ("contact-ho33-n257-s9-special", "contact-ho63-n513-s8"),
}
OCC_MUTANTS = {
    "lt-to-le": ("occ-hand-equal", "occ-hand-cut"),
    "band-dropped": ("occ-r30-w8-near", "occ-r30-w8-tol-below-3", "occ-r30-w8-tol-above-3", "occ-r64-13-slabs", "occ-r142-p1-h4"),
    "t2-is-thres-squared": ("occ-hand-cut",),
    "window-short": ("occ-r8-w4", "occ-r30-w8-near", "occ-r16-w16-near", "occ-r100-p2"),
    "last-slab-planes": ("occ-r30-w8-near", "occ-r64-13-slabs", "occ-r6-w7-edges"),
    "edge-mask-off-by-one": ("occ-r6-w7-edges", "occ-r30-w7", "occ-r64-13-slabs"),
    "counter-carry": ("occ-cell-255-256-5000", "occ-rowsum-above-2^24"),
    "table-index-clamped": ("occ-cell-255-256-5000", "occ-rowsum-above-2^24"),
    "group-max-not-sticky": ("occ-r8-w4", "occ-r102-p1-h7"),
    "select-ignored": ("occ-r8-w3-some", "occ-r30-w5-none", "occ-r64-13-slabs"),
    "raw-normalises": ("occ-r6-w7-edges", "occ-r30-w8-near", "occ-r142-p1-h4"),
}


@pytest.mark.parametrize("mut", cr.MUTATIONS)
def test_a_broken_contact_kernel_fails_a_named_case(mut):
    assert set(CONTACT_MUTANTS) == set(cr.MUTATIONS)
    for cid in CONTACT_MUTANTS[mut]:
        with pytest.raises(AssertionError):
            cr.check(cr.BY_ID[cid], cr.emulate(cid, mut))
        cr.check(cr.BY_ID[cid], cr.emulate(cid))
    print(f"CONTACT_MUTANT {mut} caught by {' '.join(CONTACT_MUTANTS[mut])}")


@pytest.mark.parametrize("mut", orf.MUTATIONS)
def test_a_broken_occupancy_kernel_fails_a_named_case(mut):
    assert set(OCC_MUTANTS) == set(orf.MUTATIONS)
    for cid in OCC_MUTANTS[mut]:
        with pytest.raises(AssertionError):
            orf.check(orf.BY_ID[cid], _occ_got(orf.BY_ID[cid], mut))
        orf.check(orf.BY_ID[cid], _occ_got(orf.BY_ID[cid]))
    print(f"OCC_MUTANT {mut} caught by {' '.join(OCC_MUTANTS[mut])}")


# ------------------------------------------------------------------------------------------------------------------ refusals
ALL_REFUSALS = {**cr.REFUSALS, **orf.REFUSALS}


@pytest.mark.parametrize("entry", sorted(ALL_REFUSALS), ids=str)
def test_every_refusal_gives_its_code_and_text_through_the_entry_point(entry, hip_lib):
    base, rows = ALL_REFUSALS[entry]
    assert len(rows) >= 6 and set(base) == set(_lib.PARAMS[entry][:-1])       # the header's own parameter names
    n = kit.check_refusals(hip_lib, {entry: ALL_REFUSALS[entry]}, kit.host_resolver(cr.HOST_ARGS), expect_control=not torch.cuda.is_available())
    print(f"CORE_REFUSALS {entry} rows={n}")


def test_empty_launches_return_ok_without_a_device(hip_lib):
    """S = 0 returns COMA_OK before any HIP call and writes nothing"""
    resolve = kit.host_resolver(cr.HOST_ARGS)
    for entry, refusals in (("coma_contact_accumulate_f32", cr.REFUSALS), ("coma_occupancy_splat", orf.REFUSALS)):
        assert kit.call(hip_lib, entry, {**refusals[entry][0], "S": 0}, resolve) == 0, entry
    assert sum(len(rows) for _, rows in ALL_REFUSALS.values()) >= 80
    # the workspace the fused pass asks for is a multiple of 16 bytes and grows with the rounded window
    ws = hip_lib.coma_occupancy_fused_workspace_bytes
    assert ws(4, 2, 30, 8) % 16 == 0 and ws(4, 2, 30, 5) == ws(4, 2, 30, 8) < ws(4, 2, 30, 9) == ws(4, 2, 30, 16) and ws(4, 2, 30, 17) == 0
