"""CPU checks of tests/reduce_ref.py and of the argument checks of coma_amd/csrc/reduce.hip, nearest.hip, normals.hip and triangulate.hip:
that the table reaches every regime and every entry point in each of its output modes, every reference against an independent
formulation (oracle/coma_oracle.py, oracle/triangulation_oracle.py's np.linalg.pinv, NumPy's argmax / argmin), the emulation through the
very assertions the device is held to, the poison, that each deliberately broken emulation fails named cases, every refusal row through
the REAL entry points with dummy non-null pointers (the argument checks run before any HIP call, so without a device a refused row
returns COMA_E_INVALID with its text and a wrongly accepted one fails at launch with another code), and the host-side index checks of
coma_amd/triangulate.py.  The per-case yardstick e_emu is printed here, without a GPU: `pytest -s tests/test_reduce_ref_host.py`."""
import numpy as np
import pytest
import torch

from coma_amd import _lib
from oracle import coma_oracle as orc
from oracle import triangulation_oracle as T
from tests import domain_kit as kit
from tests import reduce_ref as rr

f32, f64 = np.float32, np.float64
BY_ID = rr.BY_ID


# ------------------------------------------------------------------------------------------------------------------ the table
def test_the_table_reaches_every_regime_and_every_output_mode():
    seen, count = set(), {}
    for c in rr.CASES:
        seen |= rr.branches(c)
        count[c.entry] = count.get(c.entry, 0) + 1
    assert seen == rr.REACHABLE, dict(unreached=sorted(rr.REACHABLE - seen), unlisted=sorted(seen - rr.REACHABLE))
    print("REDUCE_TABLE " + " ".join(f"{k[5:]}={v}" for k, v in sorted(count.items())) + f" total={len(rr.CASES)} regimes={len(rr.REACHABLE)}")
    assert len(count) == 10 and set(count) == set(rr.REFUSALS)
    # the regimes the issue names, under the names branches() gives them
    for name in ("masked_max_f32:which0:lane-stride-many", "significant_pairs_u8:lane-stride-many", "masked_max_f32:which1:second-workgroup",
                 "significant_pairs_u8:second-workgroup", "contact_map_f32:ragged-last-block", "contact_map_f32:ragged-last-wave", "row_argmax_i64:tie-across-lanes",
                 "row_argmax_i64:tie-across-strides", "nearest_vertex_i64:tie-across-lanes", "nearest_vertex_i64:tie-across-waves", "nearest_vertex_i64:tie-across-strides",
                 "nearest_vertex_i64:nan-path", "row_argmax_i64:nan-path", "masked_max_f32:which0:empty-mask", "masked_max_f32:which1:empty-mask",
                 "significant_pairs_u8:empty-mask", "vertex_normals_f64:eps>=0", "vertex_normals_f64:zero-normal", "nearest_vertex_i64:P==0", "dlt_score_f64:P==0",
                 "ransac_mse_f64:C==0", "nearest_vertex_i64:idle-threads"):
        assert name in seen, name
    # the shapes
    of = lambda e: [c for c in rr.CASES if c.entry == "coma_" + e]
    for e in ("contact_map_f32", "entropy_f32"):
        assert {(c.M, c.N) for c in of(e)} == set(rr.MN) | {(2, 8)}
    assert {(c.M, c.N, c.with_contact) for c in of("contact_map_f32")} == {(m, n, w) for m, n in rr.MN + ((2, 8),) for w in (0, 1)}
    assert {(c.M, c.N, c.n_bin) for c in of("entropy_f32")} == {(m, n, b) for m, n in rr.MN + ((2, 8),) for b in (20.0, 1e6)}
    for e in ("significant_pairs_u8", "contact_select_u8"):
        assert {(c.H, c.O) for c in of(e)} == set(rr.HO)
    assert {(c.H, c.O, c.which, c.mask) for c in of("masked_max_f32")} == {(h, o, w, m) for h, o in rr.HO for w in (0, 1) for m in ("random", "none", "one")}
    am = of("row_argmax_i64")
    assert {(c.rows, c.n) for c in am} == {(r, n) for r in (1, 5) for n in (1, 63, 64, 65, 250)} and {c.outs for c in am} == {"both", "idx", "val"}
    assert any(c.row_stride > c.n and c.col_offset > 0 for c in am) and any(c.row_stride == c.n and c.col_offset == 0 for c in am)
    for rows in (1, 5):                                         # every pattern with one row and with five, at a size that holds it
        assert {rr.ARGMAX_PATTERNS[(c.first_pattern + r) % 5] for c in am if c.rows == rows and c.n > 1 for r in range(rows)} == set(rr.ARGMAX_PATTERNS)
    assert {(c.P, c.V) for c in of("nearest_vertex_i64")} >= set(rr.PV) | {(0, 5)}
    vn = of("vertex_normals_f64")
    assert {(c.S, c.V) for c in vn} == {(s, v) for s in (1, 3) for v in (4, 127, 128, 129)} and {c.eps for c in vn} == {-1.0, 0.0, 1e-8}
    assert {c.P for c in of("dlt_score_f64")} == {0, 1, 3} and {c.J for c in of("dlt_score_f64")} == {1, 17, 127, 128, 129, 300}
    assert {c.C for c in of("ransac_mse_f64")} == {0, 1, 2, 127, 128, 129}


def test_the_data_holds_what_the_table_says():
    # contact_map / entropy: the zero row, the row that eps decides, den = 0 with nom = 0 and with nom > 0, the tie, the q == 0 branch
    d = rr.data(BY_ID["contact-map-5x65-contact"])
    assert not d["prob"][0].any() and 0 < float(d["prob"][4].sum()) < 1e-7 and (d["den"][1], d["nom"][1]) == (0.0, 0.0) and d["den"][2] == 0.0 < d["nom"][2]
    r = rr.reference(BY_ID["contact-map-5x65-contact"])["contact"].ref
    assert np.isnan(r[1]) and np.isposinf(r[2]) and np.isfinite(r[[0, 3, 4]]).all()
    tie = rr.data(BY_ID["entropy-2x8-nbin20"])["prob"]
    assert tie.shape == (2, 8) and bool((tie[1] == 1.0).all()) and f32(0.125) * f32(20.0) == f32(2.5)
    for c in (x for x in rr.CASES if x.entry == "coma_entropy_f32"):
        x = rr.data(c)["prob"].astype(f64)
        t = x / (x.sum(-1, keepdims=True) + f64(f32(1e-8))) * c.n_bin
        gap = np.abs(t - np.floor(t) - 0.5)
        if c.id != "entropy-2x8-nbin20":
            assert float(gap.min()) >= 0.14, (c.id, float(gap.min()))           # no element near a rounding boundary but the deliberate tie
        if c.n_bin == 20.0 and c.N >= 63:
            assert bool(((t < 0.5) & (t > 0)).any()), c.id                      # small entries that round to q = 0
    # the masks
    for c in (x for x in rr.CASES if x.entry == "coma_significant_pairs_u8"):
        d = rr.data(c)
        if c.mask == "none":
            assert not d["pairs"].any()
        elif c.mask == "one":
            assert int(d["pairs"].sum()) == 1 and d["pairs"][rr.one_cell(c.H, c.O)] == 1 and d["cnt"][rr.one_cell(c.H, c.O)] == d["thr"]
        elif c.H * c.O > 1:
            assert np.isnan(d["cnt"]).sum() == 1 and bool((d["cnt"] == d["thr"]).any()) and 0 < d["pairs"].sum() < d["pairs"].size
    assert rr.one_cell(4, 257) == (3, 256) and rr.one_cell(7, 300) == (6, 299) and rr.one_cell(5, 65)[1] == 64 and rr.one_cell(130, 3)[0] == 129
    for c in (x for x in rr.CASES if x.entry == "coma_masked_max_f32"):
        d, ref = rr.data(c), rr.reference(c)["out"]
        live = np.outer(np.ones(c.H, bool), d["col_any"] != 0) if c.which == 0 else np.outer(d["row_any"] != 0, np.ones(c.O, bool))
        assert bool(np.isnan(d["contact"][~live]).all())                        # everything outside the mask is poison
        if c.mask == "none":
            assert not ref.any() and not np.signbit(ref).any()
        if c.mask == "random" and min(c.H, c.O) > 1:
            assert np.isnan(ref).sum() == 1 and bool(np.isneginf(ref).any()) and bool(np.isneginf(d["contact"][live]).any())
    for c in (x for x in rr.CASES if x.entry == "coma_contact_select_u8" and x.H >= 4):
        d, ref = rr.data(c), rr.reference(c)["selected"]
        with np.errstate(all="ignore"):
            q = d["nom"] / d["den"]
        assert ref[0] == 1 and ref[1] == 0 and np.nanmax(q[1]) == d["thr"] and np.isnan(q[2]).any() and np.nanmax(q[2]) > d["thr"] and ref[2] == 0
        assert bool(np.isneginf(q[3]).all()) and ref[3] == 0 and int((q[0] > d["thr"]).sum()) == 1 and q[0, c.O - 1] > d["thr"]
    # row_argmax: everything outside the windows is NaN; the expected answers of the patterns
    for c in (x for x in rr.CASES if x.entry == "coma_row_argmax_i64"):
        d, ref = rr.data(c), rr.reference(c)
        inside = np.zeros(d["x"].size, bool)
        for r in range(c.rows):
            inside[r * c.row_stride + c.col_offset:r * c.row_stride + c.col_offset + c.n] = True
        assert bool(np.isnan(d["x"][~inside]).all())
        for r in range(c.rows):
            pat = rr.ARGMAX_PATTERNS[(c.first_pattern + r) % 5]
            row, k = d["body"][r], int(ref["idx"][r])
            if pat == "all-ninf":
                assert k == 0 and np.isneginf(ref["val"][r])
            elif c.n > 1 and pat in ("tie-next", "tie-64"):
                assert row[k] == 9.0 and int((row == 9.0).sum()) == 2 and k == int(np.nonzero(row == 9.0)[0][0])
            elif c.n > 1 and pat == "nan-first":
                assert k == 0 and np.isnan(row[[0, c.n - 1]]).all() and np.isnan(ref["val"][r])
            elif c.n > 1:
                assert k == c.n - 1 and row[0] == 9.0 and np.isnan(ref["val"][r])
    # nearest
    for c in (x for x in rr.CASES if x.entry == "coma_nearest_vertex_i64" and x.P):
        d, ref = rr.data(c), rr.reference(c)["idx"]
        with np.errstate(over="ignore", invalid="ignore"):
            assert np.array_equal(ref, orc.nearest_vertex(d["points"], d["verts"]))
        for p, q in enumerate(c.queries):
            want = min(c.nan_verts) if c.nan_verts and q[0] != "nan-point" else {"dup": q[-1 if q[0] == "at" else 1] if len(q) > 1 else None, "far": 0, "nan-point": 0}.get("dup" if q[0] == "at" else q[0])
            if want is not None:
                assert ref[p] == want, (c.id, p, q)
            if q[0] == "dup":
                assert np.array_equal(d["verts"][q[1]], d["verts"][q[2]]) and np.array_equal(d["points"][p], d["verts"][q[1]])
    # the normals: the zero normal, the isolated vertices, the poisoned twin
    for c in (x for x in rr.CASES if x.entry == "coma_vertex_normals_f64" and x.V > 4):
        d = rr.data(c)
        n = rr.reference(c)["normals"].reshape(c.S, c.V, 3)
        iso = [v for v in range(c.V) if d["off"][v] == d["off"][v + 1]]
        assert iso == [60, c.V - 3, c.V - 2, c.V - 1] and d["off"][51] < d["off"][52]
        up = np.array([0.0, 0.0, 1.0]) / (1.0 + max(c.eps, 0.0))
        for v in iso + [50, 51]:
            assert np.array_equal(n[:, v], np.broadcast_to(up, (c.S, 3))), (c.id, v)
        assert int(d["off"][-1]) == d["vf"].size == d["faces"].size and bool((np.diff(d["off"]) >= 0).all())
    a, b = (rr.reference(BY_ID[i])["normals"].reshape(3, 129, 3) for i in ("normals-s3-v129-eps0", "normals-s3-v129-eps0-others-poisoned"))
    assert np.array_equal(a[1], b[1]) and not np.array_equal(a[0], b[0]) and bool(np.isnan(rr.data(BY_ID["normals-s3-v129-eps0-others-poisoned"])["verts"][[0, 2]]).all())
    # ransac: duplicates, out of order, the threshold is one entry of the emulation's matrix and decides a count
    for c in (x for x in rr.CASES if x.entry == "coma_ransac_mse_f64" and x.C > 1):
        d, emu = rr.data(c), rr.emulate(c)
        assert (len(set(d["sel"].tolist())) < c.C or c.C == 2) and bool((np.diff(d["sel"]) < 0).any()) and int((emu["mse"] == d["thr"]).sum()) >= 1
        le = (emu["mse"].reshape(c.C, c.C) <= d["thr"]).sum(1)
        assert not np.array_equal(le, emu["counts"]) and 0 < int(emu["counts"].sum()) < c.C * c.C


# ------------------------------------------------------------------------------------------------------------------ references
def test_reducer_references_are_the_oracles():
    """oracle/coma_oracle.ComAOracle (the reference's formulas in f32 NumPy) on the same accumulator state: contact_map, aggregated_contact
    and nonphysical against reference() in float64, to the f32 accuracy of the oracle."""
    for M, N in ((5, 65), (9, 250)):
        c, ce = BY_ID[f"contact-map-{M}x{N}-contact"], BY_ID[f"entropy-{M}x{N}-nbin1000000"]
        for case, which in ((c, "contact"), (ce, "score")):
            d, ref = rr.data(case), rr.reference(case)
            o = orc.ComAOracle(M, 1, N, 1.0, 1.0, principle_vec=(0.0, 0.6, 0.8))
            o.grid = d["grid"].astype(f64) if which == "contact" else o.grid
            o.P_h_wrt_o, o.P_o_wrt_h = d["prob"].reshape(M, 1, N).copy(), d["prob"].reshape(M, 1, N).copy()
            with np.errstate(all="ignore"):
                if which == "contact":
                    o.nom, o.den = d["nom"].reshape(M, 1).copy(), d["den"].reshape(M, 1).copy()
                    theirs = o.contact_map(grid_f32=True)[0].reshape(M)
                else:
                    theirs = o.nonphysical(n_bin=1e6)[0].reshape(M)
            fin = np.isfinite(ref[which].ref)
            assert np.array_equal(np.isnan(theirs), np.isnan(ref[which].ref))
            assert float((np.abs(theirs[fin] - ref[which].ref[fin]) / ref[which].norm[fin]).max()) < 64 * rr.U32, case.id
            assert float(np.abs(o.P_h_wrt_o.reshape(M, N) - ref["prob"].ref).max()) < 16 * rr.U32
    for H, O in ((5, 65), (7, 300)):
        for which in (0, 1):
            c = BY_ID[f"masked-max-{H}x{O}-random-which{which}"]
            d = rr.data(c)
            col, row = d["col_any"].astype(bool), d["row_any"].astype(bool)
            theirs = d["contact"][:, col].max(-1) if which == 0 else d["contact"][row, :].max(0)       # aggregated_contact's own expression
            rr.same(rr.reference(c)["out"], theirs, c.id)
            assert np.array_equal(d["pairs"], (d["cnt"] >= d["thr"]).astype(np.uint8))                  # significant_pairs


def test_normals_reference_and_emulation_agree_bit_for_bit():
    for c in (x for x in rr.CASES if x.entry == "coma_vertex_normals_f64"):
        rr.same(rr.emulate(c)["normals"], rr.reference(c)["normals"], c.id)
        d = rr.data(c)
        if c.eps >= 0 and not c.poison_others:                               # the eps step is oracle.normalize_rows
            first = orc.vertex_normals(d["verts"][0], d["faces"])
            rr.same(rr.reference(c)["normals"].reshape(c.S, c.V, 3)[0], orc.normalize_rows(first, c.eps), c.id)


def test_triangulation_reference_is_the_oracles_pinv():
    """np.longdouble normal equations against oracle/triangulation_oracle (np.linalg.pinv per joint, pinned against the reference vectors by
    tests/test_triangulation.py): the pairs of the table are well conditioned, so the two agree far below the bound's floor."""
    for c in (x for x in rr.CASES if x.entry == "coma_dlt_score_f64" and x.P):
        d, ref = rr.data(c), rr.reference(c)
        for p in range(c.P):
            cam = d["cams"][int(d["cand_view"][p])]
            t = T.solve_dlt(d["ref_xy"], d["cams"][0], d["cand_xy"][p], cam)
            mine = ref["tri"].ref.reshape(c.P, c.J, 3)[p]
            assert float(np.abs(t - mine).max()) <= 1e-12 * float(np.abs(mine).max()), c.id
            rm = np.mean(np.sum((T.render(t.copy(), d["cams"][0]) - d["ref_xy"]) ** 2, axis=1))
            om = np.mean(np.sum((T.render(t.copy(), cam) - d["cand_xy"][p]) ** 2, axis=1))
            assert abs(rm - ref["ref_mse"].ref[p]) <= 1e-9 * ref["ref_mse"].norm[p] and abs(om - ref["other_mse"].ref[p]) <= 1e-9 * ref["other_mse"].norm[p]
            A = np.vstack([T.projection(d["cams"][0])[0][:2], T.projection(cam)[0][:2]])
            assert np.linalg.cond(A) < 10.0
    c = BY_ID["ransac-c127"]
    d, ref = rr.data(c), rr.reference(c)["mse"].ref.reshape(c.C, c.C)
    for a, b in ((0, 1), (5, 99), (126, 126)):
        ia, ib = int(d["sel"][a]), int(d["sel"][b])
        theirs = np.mean(np.sum((d["cand_xy"][ib] - T.render(d["tri"][ia].copy(), d["cams"][int(d["cand_view"][ib])])) ** 2, axis=1))
        assert abs(theirs - ref[a, b]) <= 1e-12 * max(ref[a, b], 1.0)


# ------------------------------------------------------------------------------------------------------------------ the emulation
@pytest.mark.parametrize("case", rr.CASES, ids=lambda c: c.id)
def test_the_emulation_passes_the_device_checks(case):
    """check() -- the assertions tests/test_coma_small_domain_gpu.py applies to the device -- on the emulation of the same case: the exact
    contracts bit for bit, the arithmetic within a bound that is max(4 e_emu, floor) with the floor stated beside the reference."""
    c = case
    fig = rr.check(c, rr.emulate(c))
    ref = rr.reference(c)
    for name, f in fig.items():
        print(f"REDUCE_YARD {c.id} out={name} e_emu={f.e_emu:.3e} floor={ref[name].floor:.3e} bound={f.bound:.3e}")
        assert f.bound == max(4 * f.e_emu, ref[name].floor) and f.err == f.e_emu
        assert f.e_emu <= 2 * ref[name].floor or c.entry in ("coma_dlt_score_f64",), (name, f)      # the count holds for the emulation itself
    ins, outs = rr.plan(c)
    for name, i in ins.items():
        buf = rr.pack(i.body, i.poison)
        assert buf.size == i.body.size + 2 * kit.GUARD and (bool(np.isnan(buf[:kit.GUARD]).all()) if buf.dtype.kind == "f" else bool((buf[:kit.GUARD] == i.poison).all()))
    for name, o in outs.items():
        assert o.init.size == o.must.size == o.finite.size and (o.must.all() or not o.must.any())


def test_a_stray_read_shows():
    # a mask guard byte read as a mask entry admits a NaN
    c = BY_ID["masked-max-5x65-one-which0"]
    d = rr.data(c)
    assert rr.plan(c)[0]["col_any"].poison == 1 and bool(np.isnan(d["contact"][:, d["col_any"] == 0]).all())
    col = d["col_any"].copy()
    col[0] = 1
    assert bool(np.isnan(d["contact"][:, col != 0].max(-1)).all()) and not np.isnan(rr.reference(c)["out"]).any()
    # a NaN vertex read from the guard wins under np.argmin's rule, with an index outside [0, V)
    c = BY_ID["nearest-2x255"]
    d = rr.data(c)
    ext = np.concatenate([d["verts"], np.full((1, 3), np.nan)])
    assert np.array_equal(orc.nearest_vertex(d["points"], ext), [255, 255])
    # outputs start as the sentinel; none of the table's results equals one
    for dt in (np.float32, np.float64, np.int64, np.int32, np.uint8):
        s = kit.sentinel(3, dt)
        assert s.dtype == dt and (np.isnan(s).all() if s.dtype.kind == "f" else (s < 0).all() or dt == np.uint8)
    assert kit.bits(kit.sentinel(1, np.float32))[0] == 0x7FC5A5A5


# mutation -> cases that have to notice it
MUTANTS = {
    "last-maximum": ("argmax-1x65-both-strided-p0", "argmax-1x65-idx-dense-p1", "nearest-3x5", "nearest-2x255", "nearest-3x257", "nearest-4x1000"),
    "max-ignores-nan": ("masked-max-3x64-random-which0", "masked-max-7x300-random-which1", "contact-select-5x65", "argmax-1x63-both-strided-p3"),
    "ge-to-gt": ("pairs-1x1-one", "pairs-4x257-one", "pairs-3x180-random"),
    "gt-to-ge": ("contact-select-3x64", "contact-select-130x3", "ransac-c2", "ransac-c129"),
    "round-half-away": ("entropy-2x8-nbin20",),
    "lane-stride-dropped": ("contact-map-5x65-contact", "entropy-9x250-nbin1000000", "pairs-5x65-one", "masked-max-3x180-one-which0", "contact-select-5x65",
                            "argmax-1x250-both-dense-p3", "nearest-2x257-on-the-last-vertex"),
    "last-partial-wave-dropped": ("contact-map-5x65-contact", "entropy-3x63-nbin20", "pairs-5x65-one", "masked-max-7x300-one-which0", "contact-select-7x300",
                                  "argmax-5x65-both-dense-p4", "normals-s1-v129-eps-1"),
    "eps-before-the-sum": ("contact-map-5x65-contact", "contact-map-9x250-normalise-only", "normals-s1-v4-eps1e-08", "normals-s3-v129-eps1e-08"),
    "masks-swapped": ("pairs-3x64-one", "masked-max-5x65-one-which0", "masked-max-5x65-one-which1", "masked-max-130x3-random-which1"),
    "col-offset-ignored": ("argmax-1x65-both-strided-p0", "argmax-5x64-both-strided-p3", "argmax-5x1-val-strided-p1"),
    "faces-reversed": ("normals-s1-v4-eps-1", "normals-s1-v127-eps-1", "normals-s3-v129-eps0"),
    "tie-by-thread": ("nearest-4x1000",),
    "nearest-skips-nan": ("nearest-3x257-nan-vertex-256", "nearest-4x1000-nan-vertices-321-65", "nearest-2x256-nan-vertices-255-254"),
}


@pytest.mark.parametrize("mut", rr.MUTATIONS)
def test_a_broken_kernel_fails_a_named_case(mut):
    """The emulation with one deliberate defect, put through check(): every case named for the mutation fails, and passes without it."""
    assert set(MUTANTS) == set(rr.MUTATIONS)
    for cid in MUTANTS[mut]:
        c = BY_ID[cid]
        with pytest.raises(AssertionError):
            rr.check(c, rr.emulate(c, mut))
        rr.check(c, rr.emulate(c))
    print(f"REDUCE_MUTANT {mut} caught by {' '.join(MUTANTS[mut])}")


# ------------------------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("entry", sorted(rr.REFUSALS), ids=str)
def test_every_refusal_gives_its_code_and_text_through_the_entry_point(entry, hip_lib):
    """(principle_vec is read on the host by coma_contact_map_f32, so the resolver gives it real host memory)"""
    base, rows = rr.REFUSALS[entry]
    assert len(rows) >= 6 and set(base) == set(_lib.PARAMS[entry][:-1])       # the header's own parameter names
    # the control: the base row passes every argument check and only fails where the launch needs a device
    kit.check_refusals(hip_lib, {entry: rr.REFUSALS[entry]}, kit.host_resolver(rr.HOST_ARGS), expect_control=not torch.cuda.is_available())


def test_empty_launches_return_ok_without_a_device(hip_lib):
    """P = 0 and C = 0 return COMA_OK before any HIP call"""
    resolve = kit.host_resolver(rr.HOST_ARGS)
    for entry, change in (("coma_nearest_vertex_i64", dict(P=0)), ("coma_dlt_score_f64", dict(P=0)), ("coma_ransac_mse_f64", dict(C=0))):
        assert kit.call(hip_lib, entry, {**rr.REFUSALS[entry][0], **change}, resolve) == 0, entry
    total = sum(len(rows) for _, rows in rr.REFUSALS.values())
    print(f"REDUCE_REFUSALS {total} rows over {len(rr.REFUSALS)} entry points")
    assert total >= 80


# ------------------------------------------------------------------------------------------------------------------ the host's index checks
def test_triangulate_refuses_an_index_outside_its_table_before_any_launch():
    """cand_view outside [0, n_views) and sel outside [0, P) raise ValueError while both are still host arrays: nothing has been uploaded
    or launched (device="cpu" would fail at the first upload with another error)."""
    from coma_amd import triangulate as tr
    views, ref_xy, cand_xy = np.zeros((3, tr.VIEW_DOUBLES)), np.zeros((4, 2)), np.zeros((2, 4, 2))
    for bad in ([0, 3], [-1, 0], [1, 1 << 31]):
        with pytest.raises(ValueError, match=r"dlt_score: cand_view\[\d\] = -?\d+ is outside \[0, n_views = 3\)"):
            tr.dlt_score(views, 0, ref_xy, bad, cand_xy, device="cpu")
    with pytest.raises(ValueError, match="must hold integers"):
        tr.dlt_score(views, 0, ref_xy, [0.5, 1.0], cand_xy, device="cpu")
    state = (torch.zeros(3, tr.VIEW_DOUBLES, dtype=torch.float64), torch.zeros(2, dtype=torch.int32), torch.zeros(2, 4, 2, dtype=torch.float64))
    tri = torch.zeros(2, 4, 3, dtype=torch.float64)
    for bad in ([0, 2], [1, -1], np.array([5], np.int64)):
        with pytest.raises(ValueError, match=r"ransac_matrix: sel\[\d\] = -?\d+ is outside \[0, P = 2\)"):
            tr.ransac_matrix(state, tri, bad, 200.0)
    assert tr._checked_indices([1, 0, 1], 2, "x", "n").dtype == np.int32 and tr._checked_indices([], 2, "x", "n").size == 0
