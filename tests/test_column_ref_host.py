"""CPU checks of tests/column_ref.py and of the argument checks of the rasteriser, column and shift-profile entry points: that the
tables reach every regime (counted from each case's own data), the three restatements against an independent dense reference (every
pixel x face pair decided with Python integers, no bounding boxes; every column swept by sorting plain tuples), the emulation through
the very assertions the device is held to, that each planted defect fails a named case, mesh_volume_shape against math.fsum within the
header's bound, and every refusal row through the REAL entry points with dummy non-null pointers (the argument checks run before any
HIP call).  `pytest -s tests/test_column_ref_host.py` prints the table."""
import math

import numpy as np
import pytest

from coma_amd import _lib
from tests import column_ref as cr
from tests import domain_kit as kit
from tests import raster_ref as RR
from tests import shift_ref as SR
from tests import volume_ref as VR


def _got(c, mut=None):
    e = cr.emulate(c.id, mut)
    return cr.pad_optimize(c, e) if c.kind == "optimize" else e


# ------------------------------------------------------------------------------------------------------------------ the tables
def test_the_tables_reach_every_regime():
    seen = set().union(*(cr.branches(c.id) for c in cr.CASES)) | cr.refusal_branches()
    assert seen == cr.REACHABLE, dict(unreached=sorted(cr.REACHABLE - seen), unlisted=sorted(seen - cr.REACHABLE))
    for c in cr.CASES:
        print(f"COLUMN_TABLE {c.id} {' '.join(sorted(cr.branches(c.id)))}")
    K = lambda kind: cr.KIND(kind)
    assert {(c.W, c.H) for c in K("raster")} >= {(1, 1), (16, 16), (17, 16), (50, 131), (8192, 49), (8192, 32), (8192, 1), (1, 8192)}
    assert {c.W * c.H for c in K("iou")} >= {1, 63, 64, 65, 255, 256, 257, 8192 * 33} and {c.K for c in K("iou")} >= {1, 7, 64}
    assert all(c.K <= 3 for c in K("iou") + K("columns") if c.W * c.H > 4096)
    assert {len(cr.data(c.id)["faces"]) for c in K("volume")} >= {1, 255, 256, 257, 65536, 65537}
    assert {(c.W, c.H) for c in K("columns")} >= {(1, 1), (32, 32), (33, 32), (8192, 32), (8192, 33), (8192, 49)} and {c.K for c in K("columns")} >= {1, 2, 3, 64}
    assert {c.N for c in K("optimize")} >= {0, 1, 255, 256, 257, 513} and {c.J for c in K("optimize")} >= {1, 25, 1024} and {c.E for c in K("optimize")} >= {1, 2, 20, 4096}
    assert {(c.w_mv != 0, c.w_col != 0) for c in K("optimize")} == {(True, True), (True, False), (False, True)}
    bad = [c for c in K("optimize") if c.bad]
    assert {(at == 0, v) for c in bad for at, v in c.bad} == {(True, "neg"), (True, "nv"), (False, "neg"), (False, "nv")} and all(c.bad[0][0] in (0, c.N - 1) for c in bad)
    # the cases the issue states in figures
    full = cr.emulate("r-64x64-hits-256")["stat"]
    assert full["max_hits"] == 256 and full["listed"] == full["on_tile_0"] == 260       # every listed triangle over tile 0: any 256 of them fill hits[]
    assert cr.emulate("r-8192x49-list-300")["stat"]["listed"] == 300 and cr.emulate("r-8192x32-list-600")["stat"]["listed"] == 600
    assert cr.emulate("c-8192x49-list-300")["stat"]["A"]["listed"] == 300 > 256 * cr.grid_slices(8192, 49)[1]
    assert cr.grid_slices(8192, 49) == (2048, 1) and cr.grid_slices(8192, 32) == (1024, 2) and cr.emulate("c-8192x33-sheets-k3")["stat"]["scan_blocks"] == 264
    assert (cr.reference("r-64x48-cover-2^25")["key"] != RR.EMPTY).all() and (cr.reference("r-16x16-scale-1.7e308")["key"] == RR.EMPTY).all()


def test_the_emulation_passes_the_assertions_the_device_is_held_to():
    for c in cr.CASES:
        n = cr.check(c, _got(c))
        print(f"COLUMN_EMU {c.id} compared={n}")


def test_the_status_3_contract_of_the_restatement():
    c = cr.BY_ID["o-badview-neg-last"]
    r = cr.reference(c.id)
    cols = cr.columns_ref(c.columns)
    assert r["status"] == 3 and r["epoch"] == 0 and len(r["traj"]) == 1 and r["traj"][0] == c.d0 and len(r["losses"]) == 0
    assert np.array_equal(r["Ltraj"], cols.profile([c.d0]))          # the profile ran before the step that met the entry
    p = cr.pad_optimize(c, r)
    assert (kit.bits(p["traj"][1:]) == kit.sentinel_bits(np.float64)).all() and (kit.bits(p["losses"]) == kit.sentinel_bits(np.float64)).all()


# ------------------------------------------------------------------------------------------------------------------ an independent reference
def _dense_cover(X, Y, Z, faces, W, H):
    """per face: [(i, j, z, sigma)] over ALL pixels, Python integers, no bounding box"""
    out = []
    for ia, ib, ic in np.asarray(faces).tolist():
        A, B, C = (X[ia], Y[ia], Z[ia]), (X[ib], Y[ib], Z[ib]), (X[ic], Y[ic], Z[ic])
        e = lambda P, Q, x, y: (Q[0] - P[0]) * (y - P[1]) - (Q[1] - P[1]) * (x - P[0])
        area = e(A, B, C[0], C[1])
        hits = []
        if area != 0:
            sigma = 1 if area > 0 else -1
            if area < 0:
                B, C, area = C, B, -area
            own = lambda P, Q: Q[1] < P[1] or (Q[1] == P[1] and Q[0] > P[0])
            for j in range(H):
                for i in range(W):
                    x, y = 256 * i + 128, 256 * j + 128
                    es = (e(B, C, x, y), e(C, A, x, y), e(A, B, x, y))
                    if all(v > 0 or (v == 0 and own(P, Q)) for v, (P, Q) in zip(es, ((B, C), (C, A), (A, B)))):
                        with np.errstate(all="ignore"):
                            z = ((np.float64(es[0]) * A[2] + np.float64(es[1]) * B[2]) + np.float64(es[2]) * C[2]) / np.float64(area)
                        hits.append((i, j, z, sigma))
        out.append(hits)
    return out


SMALL = lambda c: c.W <= 32 and c.H <= 32


def test_the_raster_restatement_against_dense_integers():
    n = 0
    for c in cr.KIND("raster"):
        d = cr.data(c.id)
        if not SMALL(c) or len(d["faces"]) > 64:
            continue
        X, Y, Z = RR.snap(d["verts"], d["R"], d["t"], d["scale"], c.W, c.H)
        key = np.full((c.H, c.W), RR.EMPTY, np.uint64)
        for hits in _dense_cover(X.tolist(), Y.tolist(), Z, d["faces"], c.W, c.H):
            for i, j, z, _ in hits:
                if z == z:
                    key[j, i] = min(int(key[j, i]), int(RR.depth_to_key(np.array([z]))[0]))
        assert np.array_equal(key, cr.reference(c.id)["key"]), c.id
        n += 1
    assert n >= 4


def _tuple_sweep(events, inside=lambda n: n != 0):
    """(L_AB, L_A, L_B) of one column from [(Z, mesh, sigma)]"""
    ev = sorted(events)
    na = nb = 0
    lab = la = lb = 0
    for k, (Z, mesh, sigma) in enumerate(ev):
        if k:
            ln = Z - ev[k - 1][0]
            la, lb, lab = la + ln * inside(na), lb + ln * inside(nb), lab + ln * (inside(na) and inside(nb))
        if mesh:
            nb -= sigma
        else:
            na -= sigma
    return lab, la, lb


def test_the_column_and_shift_restatements_against_tuples():
    n = 0
    for c in cr.KIND("columns"):
        d = cr.data(c.id)
        if not SMALL(c) or max(len(d["A"][1]), len(d["B"][1])) > 64:
            continue
        per = {}
        for mesh, (v, f) in enumerate((d["A"], d["B"])):
            X, Y, Zd = VR.snap(v, d["x0"], d["y0"], d["s"])
            for hits in _dense_cover(X.tolist(), Y.tolist(), Zd, f, c.W, c.H):
                for i, j, z, sigma in hits:
                    per.setdefault(j * c.W + i, []).append((int(math.floor((z * d["s"]) * 256.0 + 0.5)), mesh, sigma))
        ref = cr.reference(c.id)
        col_ab, sums = np.zeros(c.W * c.H, np.int64), [0, 0, 0]
        for col, ev in per.items():
            t = _tuple_sweep(ev)
            col_ab[col] = t[0]
            sums = [a + b for a, b in zip(sums, t)]
        assert sums == ref["sums"].tolist() and np.array_equal(col_ab.reshape(c.H, c.W), ref["col_ab"]), c.id
        assert np.array_equal(np.bincount(list(per) or [0], weights=[len(v) for v in per.values()] or [0], minlength=c.W * c.H).astype(np.int64).reshape(c.H, c.W), ref["counts"])
        for batch, L in zip(cr.shifts(c.id)[:2], ref["L"]):
            for dk, row in zip(batch.tolist(), L):
                delta = SR.shift_of(dk, d["s"])
                want = [sum(_tuple_sweep([(Z + (0 if m else delta + j), m, sg) for Z, m, sg in ev])[0] for ev in per.values()) for j in (-1, 0, 1)]
                assert want == row.tolist(), (c.id, dk)
        n += 1
    assert n >= 4


# ------------------------------------------------------------------------------------------------------------------ the volume's shape
def test_mesh_volume_shape_is_within_the_headers_bound_of_fsum():
    for c in cr.KIND("volume"):
        d = cr.data(c.id)
        got, det, ok = cr._volume_shape(d["verts"], d["faces"], None)
        if not ok.all():
            assert math.isnan(got), c.id
            continue
        exact, F = math.fsum(det.tolist()) / 6.0, len(det)
        bound = F * 2.0 ** -52 * math.fsum(np.abs(det).tolist()) / 6.0
        print(f"VOLUME_SHAPE {c.id} F={F} shape={got!r} fsum={exact!r} |difference|={abs(got - exact):.3e} bound={bound:.3e}")
        assert abs(got - exact) <= bound, c.id
        assert abs(got - VR.mesh_volume(d["verts"], d["faces"])[0]) <= bound
    assert cr.reference("v-cube")["out"] == 4.0 and cr.reference("v-cube-inward")["out"] == -4.0      # 2 x 0.5 x 4, dyadic: exact


# ------------------------------------------------------------------------------------------------------------------ planted defects
MUTANT_FAILS = {
    "n-hits-not-reset": ["r-8192x49-list-300", "c-8192x49-list-300"], "second-trip-dropped": ["r-8192x49-list-300", "c-8192x49-list-300"],
    "hits-capped-255": ["r-64x64-hits-256"], "small-max-ge": ["r-50x131-boxes-256-257", "r-8192x1-boxes-256-257", "r-1x8192-boxes-256-257"],
    "scan-chunk-1": ["c-8192x33-sheets-k3"], "iou-stride-dropped": ["i-8192x33-k1-nomask"], "profile-stride-dropped": ["c-8192x33-sheets-k3"],
    "volume-stride-dropped": ["v-f65537"], "top-left-wrong-edges": ["r-16x16-edges"], "iou-lt-to-le": ["i-n64-k64"],
    "unpack-truncates": ["c-1x1"], "sort-ignores-mesh": ["c-32x32-box"], "inside-n-positive": ["c-33x32-stacks-inward-k2"],
    "snap-limit-low": ["r-64x48-cover-2^25"], "z-limit-low": ["c-32x32-stacks-k64"], "volume-pad-wrong": ["v-f1", "v-f257"],
    "status-3-steps-anyway": ["o-badview-neg-first", "o-badview-nv-last"], "nan-shift-clamp-sign": ["c-32x32-stacks-k64"],
}
MUTANT_ACCEPTS = {"snap-limit-high": "range", "z-limit-high": "z-beyond"}          # a refusal row the broken limit lets through


@pytest.mark.parametrize("mut", cr.MUTATIONS)
def test_a_broken_kernel_fails_a_named_case(mut):
    if mut in MUTANT_ACCEPTS:
        for mesh in (0, 1):
            d = cr.refusal_data(MUTANT_ACCEPTS[mut], mesh)
            with pytest.raises(RR.Refused):
                cr.emulate_columns(d, 32, 32)
            cr.emulate_columns(d, 32, 32, mut)                    # accepted: the row that expects the refusal fails
        return
    for cid in MUTANT_FAILS[mut]:
        c = cr.BY_ID[cid]
        with pytest.raises((AssertionError, RR.Refused)):
            cr.check(c, _got(c, mut))
        cr.check(c, _got(c))


def test_every_defect_is_planted_or_shown_equivalent():
    assert set(MUTANT_FAILS) | set(MUTANT_ACCEPTS) == set(cr.MUTATIONS)
    # the one the issue names that changes no output: the merge's tie order.  Which clamp a NaN shift takes is NOT one: beyond the clamp
    # a closed pair overlaps nowhere, an open mesh (the stacks of 9 sheets) still does, and differently on the two sides
    cols, box = cr.columns_ref("c-32x32-stacks-k64"), cr.columns_ref("c-32x32-box")
    assert box.L_AB(cr.SHIFT) == box.L_AB(-cr.SHIFT) == 0 and 0 != cols.L_AB(cr.SHIFT) != cols.L_AB(-cr.SHIFT) != 0
    assert set(cr.EQUIVALENT) == {"merge-le-to-lt"}


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_the_restatement_refuses_every_device_row():
    assert cr.refusal_branches() >= {"snap-beyond-2^25", "Z-beyond-2^40", "Z-non-finite", "refused-capacity", "refused-scale-overflow"}
    d = cr.data("r-64x48-cover-2^25")
    out = d["verts"].copy()
    out[1, 0] += 1.0 / 256.0                                         # the covering triangle moved out by 1/256 pixel
    with pytest.raises(RR.Refused):
        RR.raster_depth(out, d["faces"], d["R"], d["t"], d["scale"], 64, 48)


def test_refusals_are_reported_before_any_launch():
    lib = _lib.lib()
    resolve = cr.with_host_arrays(kit.host_resolver())
    import torch
    n = kit.check_refusals(lib, cr.REFUSALS, resolve, expect_control=not torch.cuda.is_available())
    n += cr.run_plain_refusals(lib, resolve)
    covered, sites = cr.argument_check_sites()
    print(f"COLUMN_REFUSALS rows={n} sites covered={covered} of {sites}")
    assert covered == sites == 59 and n >= 150
