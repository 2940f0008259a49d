"""The ten oldest entry points -- coma_amd/csrc/reduce.hip (coma_contact_map_f32, coma_entropy_f32, coma_significant_pairs_u8,
coma_masked_max_f32, coma_row_argmax_i64, coma_contact_select_u8), nearest.hip (coma_nearest_vertex_i64), normals.hip
(coma_vertex_normals_f64) and triangulate.hip (coma_dlt_score_f64, coma_ransac_mse_f64) -- over the domain their argument checks accept.
CPU only: the table of launches (CASES), what each reaches (branches), its operands and first output contents (data, plan), the result in
float64 / np.longdouble NumPy written from the reference's formulas (reference; oracle/coma_oracle.py and oracle/triangulation_oracle.py
hold the same formulas and tests/test_reduce_ref_host.py compares), the kernel's own formula in its own precision and summation shape
(emulate: lane-strided partial sums, then the xor butterfly), the assertions the device is held to (check), and every argument check
(REFUSALS, written with tests/domain_kit.py's PTR; the guard width, the sentinels, pack_rows and the seeds are the kit's too).
tests/test_coma_small_domain_gpu.py launches the table; tests/test_reduce_ref_host.py checks the table itself.

The bound.  Bit for bit (NaN-ness compared for NaNs): pairs / col_any / row_any, the masked maximum (a maximum rounds nothing), idx and
val of the row argmax, contact_select (one correctly rounded f32 division per element, then comparisons), the nearest vertex (f64, no
contraction, the reference's order), the vertex normals (ascending face order, no contraction, correctly rounded f64 sqrt and /) and
ransac's counts against the device's own mse.  The arithmetic outputs -- normalised prob, contact, score, tri, ref_mse, other_mse, mse --
may differ from the float64 (triangulation: longdouble) reference by max(4 e_emu, floor) in units of `norm`: e_emu is what emulate() loses
on the same case, norm the sum of magnitudes of the formula's terms, floor the counted roundings of the formula (beside each Ref below)."""
import ctypes
import functools
import math
from typing import NamedTuple, Optional

import numpy as np

from coma_amd import _lib
from tests import domain_kit as kit
from tests.domain_kit import PTR, U32, bits, sentinel

f32, f64, i32, i64, u8 = np.float32, np.float64, np.int32, np.int64, np.uint8
U64 = 2.0 ** -53
WAVE, ROW_WAVES = 64, 4
NAN, INF = float("nan"), float("inf")
# what outputs are pre-filled with (the kit's sentinels): NaNs with a payload for the floats, 0xA5 bytes for the integers (no result of
# the table equals one)
SENTINEL = {np.dtype(t): sentinel(1, t)[0] for t in (f32, f64, i64, i32, u8)}


class Case:
    """one launch: `entry` with the parameters `kw` (shapes, modes, what the data holds)"""

    def __init__(self, id, entry, **kw):
        self.id, self.entry, self.kw = id, "coma_" + entry, kw

    def __getattr__(self, name):
        try:
            return self.kw[name]
        except KeyError:
            raise AttributeError(name)

    def __repr__(self):
        return self.id


# ------------------------------------------------------------------------------------------------------------------ the table
MN = ((1, 1), (3, 63), (4, 64), (5, 65), (9, 250), (6, 257))
HO = ((1, 1), (3, 64), (5, 65), (4, 257), (7, 300), (130, 3), (3, 180))
PV = ((1, 1), (3, 5), (2, 255), (2, 256), (3, 257), (4, 1000))
ARGMAX_PATTERNS = ("tie-next", "tie-64", "nan-first", "nan-after-larger", "all-ninf")


def _build_cases():
    cs = []
    # contact_map / entropy: every (M, N) with contact NULL and given, both n_bin; the N = 8 row of equal values on its own
    for k, (M, N) in enumerate(MN + ((2, 8),)):
        for with_contact in (0, 1):
            cs.append(Case(f"contact-map-{M}x{N}-{'contact' if with_contact else 'normalise-only'}", "contact_map_f32", M=M, N=N, with_contact=with_contact,
                           n_bin=(20.0, 1e6)[(k + with_contact) % 2], eps=1e-8))
        for n_bin in (20.0, 1e6):
            cs.append(Case(f"entropy-{M}x{N}-nbin{int(n_bin)}", "entropy_f32", M=M, N=N, n_bin=n_bin, eps=1e-8))
    # the masks: random (counts equal to the threshold, a NaN count), empty, one cell set (its column >= 64 / >= 256 and its row >= 4 where
    # the shape has them)
    for H, O in HO:
        for mask in ("random", "none", "one"):
            cs.append(Case(f"pairs-{H}x{O}-{mask}", "significant_pairs_u8", H=H, O=O, mask=mask))
            for which in (0, 1):
                cs.append(Case(f"masked-max-{H}x{O}-{mask}-which{which}", "masked_max_f32", H=H, O=O, mask=mask, which=which))
        cs.append(Case(f"contact-select-{H}x{O}", "contact_select_u8", H=H, O=O))
    # row_argmax: rows x n, the five row patterns rotated so that the single-row cases see every one of them
    k = 0
    for rows in (1, 5):
        for n in (1, 63, 64, 65, 250):
            for outs in (("both", "idx", "val") if n in (1, 65) else ("both",)):
                strided = k % 2 == 1
                cs.append(Case(f"argmax-{rows}x{n}-{outs}-{'strided' if strided else 'dense'}-p{k % 5}", "row_argmax_i64", rows=rows, n=n, outs=outs,
                               row_stride=n + (7 if strided else 0), col_offset=3 if strided else 0, first_pattern=k % 5))
                k += 1
    # nearest: per query a pattern; NaN vertices in cases of their own (a NaN vertex is every finite query's answer)
    nearest = {(1, 1): [("random",)], (3, 5): [("dup", 1, 2), ("far",), ("nan-point",)], (2, 255): [("dup", 100, 164), ("random",)],
               (2, 256): [("dup", 254, 255), ("far",)], (3, 257): [("dup", 0, 256), ("dup", 100, 101), ("random",)],
               (4, 1000): [("dup", 300, 556), ("dup", 255, 256), ("nan-point",), ("dup", 700, 764)]}
    for (P, V), q in nearest.items():
        cs.append(Case(f"nearest-{P}x{V}", "nearest_vertex_i64", P=P, V=V, queries=q, nan_verts=()))
    cs.append(Case("nearest-2x257-on-the-last-vertex", "nearest_vertex_i64", P=2, V=257, queries=[("at", 256), ("random",)], nan_verts=()))
    cs.append(Case("nearest-0x5-no-points", "nearest_vertex_i64", P=0, V=5, queries=[], nan_verts=()))
    cs.append(Case("nearest-3x257-nan-vertex-256", "nearest_vertex_i64", P=3, V=257, queries=[("random",), ("nan-point",), ("far",)], nan_verts=(256,)))
    cs.append(Case("nearest-4x1000-nan-vertices-321-65", "nearest_vertex_i64", P=4, V=1000, queries=[("random",), ("dup", 2, 3), ("far",), ("random",)], nan_verts=(321, 65)))
    cs.append(Case("nearest-2x256-nan-vertices-255-254", "nearest_vertex_i64", P=2, V=256, queries=[("random",), ("random",)], nan_verts=(255, 254)))
    # vertex normals
    k = 0
    for S in (1, 3):
        for V in (4, 127, 128, 129):
            for eps in ((-1.0, 0.0, 1e-8) if V in (4, 129) else ((-1.0, 0.0, 1e-8)[k % 3],)):
                cs.append(Case(f"normals-s{S}-v{V}-eps{eps:g}", "vertex_normals_f64", S=S, V=V, eps=eps, poison_others=0))
                k += 1
    cs.append(Case("normals-s3-v129-eps0-others-poisoned", "vertex_normals_f64", S=3, V=129, eps=0.0, poison_others=1))
    # triangulation
    for P, J in ((0, 17), (1, 1), (3, 17), (1, 127), (3, 128), (1, 129), (3, 300)):
        cs.append(Case(f"dlt-p{P}-j{J}", "dlt_score_f64", P=P, J=J))
    for C in (0, 1, 2, 127, 128, 129):
        cs.append(Case(f"ransac-c{C}", "ransac_mse_f64", C=C, J=17, P=40))
    return cs


CASES = _build_cases()
ENTRIES = sorted({c.entry for c in CASES})


def one_cell(H, O):
    """the cell of a `one` mask: the last row (>= 4 where H allows) and a column past the first lane stride / workgroup where O allows"""
    return H - 1, (O - 1 if O > 256 else 64 + (O - 65) // 2 if O > 64 else O - 1)


def branches(c):
    """names of the regimes the launch reaches"""
    e, b = c.entry[5:], set()
    b.add(e)
    if e in ("contact_map_f32", "entropy_f32"):
        b.add(f"{e}:contact-{'given' if c.kw.get('with_contact', 1) else 'null'}" if e == "contact_map_f32" else f"{e}:nbin{int(c.n_bin)}")
        b |= {f"{e}:lane-stride-{'many' if c.N > WAVE else 'once'}", f"{e}:{'ragged-last-block' if c.M % ROW_WAVES else 'full-blocks'}"}
        if c.N % WAVE:
            b.add(f"{e}:ragged-last-wave")
        if c.M > 1:
            b.add(f"{e}:zero-row")
    elif e in ("significant_pairs_u8", "masked_max_f32"):
        w = c.kw.get("which")
        tag = e if w is None else f"{e}:which{w}"
        b.add(tag)
        if c.mask == "none":
            b.add(f"{tag}:empty-mask")
        if c.mask == "random" and c.H * c.O > 1:
            b.add(f"{tag}:nan-path")
        if w in (None, 0) and c.O > WAVE:
            b.add(f"{tag}:lane-stride-many")
        if w in (None, 1) and c.O > 256:
            b.add(f"{tag}:second-workgroup")
        if w in (None, 0) and c.H > ROW_WAVES:
            b.add(f"{tag}:row-blocks")
        if w in (None, 0) and c.H % ROW_WAVES:
            b.add(f"{tag}:ragged-last-block")
        if w is None and c.H * c.O > 256:
            b.add(f"{tag}:pairs-second-workgroup")
        if c.mask == "one":
            h0, o0 = one_cell(c.H, c.O)
            b |= {f"{tag}:only-column-past-{t}" for t in (64, 256) if o0 >= t} | ({f"{tag}:only-row-past-4"} if h0 >= 4 else set())
    elif e == "contact_select_u8":
        b |= {f"{e}:threshold-equal", f"{e}:nan-path"} if c.H * c.O > 1 else set()
        b |= ({f"{e}:lane-stride-many"} if c.O > WAVE else set()) | ({f"{e}:row-blocks"} if c.H > ROW_WAVES else set())
        b |= ({f"{e}:ragged-last-block"} if c.H % ROW_WAVES else set()) | ({f"{e}:ragged-last-wave"} if c.O % WAVE else set())
    elif e == "row_argmax_i64":
        b |= {f"{e}:outs-{c.outs}", f"{e}:{'strided' if c.col_offset else 'dense'}"}
        b |= {f"{e}:{ARGMAX_PATTERNS[(c.first_pattern + r) % 5]}" for r in range(c.rows)} if c.n > 1 else set()
        pats = {ARGMAX_PATTERNS[(c.first_pattern + r) % 5] for r in range(c.rows)}
        if c.n > WAVE:
            b.add(f"{e}:lane-stride-many")
            if "tie-64" in pats:
                b.add(f"{e}:tie-across-strides")
        if c.n > 1 and "tie-next" in pats:
            b.add(f"{e}:tie-across-lanes")
        if c.n > 1 and pats & {"nan-first", "nan-after-larger"}:
            b.add(f"{e}:nan-path")
        b |= ({f"{e}:ragged-last-block"} if c.rows % ROW_WAVES else set()) | ({f"{e}:ragged-last-wave"} if c.n % WAVE else set())
    elif e == "nearest_vertex_i64":
        if c.P == 0:
            return b | {f"{e}:P==0"}
        b.add(f"{e}:{'idle-threads' if c.V < 256 else 'lane-stride-many' if c.V > 256 else 'one-stride'}")
        for q in c.queries:
            if q[0] == "dup":
                d = q[2] - q[1]
                b.add(f"{e}:tie-" + {1: "across-lanes", 64: "across-waves", 256: "across-strides"}[d])
                if q[1] % 256 > q[2] % 256:
                    b.add(f"{e}:tie-lower-index-on-higher-thread")
            else:
                b.add(f"{e}:{q[0]}")
        if c.nan_verts:
            b |= {f"{e}:nan-path", f"{e}:nan-vertex"}
        if ("nan-point",) in c.queries:
            b.add(f"{e}:nan-path")
    elif e == "vertex_normals_f64":
        b |= {f"{e}:{'eps>=0' if c.eps >= 0 else 'eps<0'}", f"{e}:S{c.S}", f"{e}:{'one-workgroup' if c.V <= 128 else 'second-workgroup'}"}
        b |= {f"{e}:ragged-last-wave"} if c.V % WAVE else set()
        if c.V > 4:
            b |= {f"{e}:zero-normal", f"{e}:isolated-vertex", f"{e}:zero-area-faces"}
        if c.poison_others:
            b.add(f"{e}:others-poisoned")
    elif e == "dlt_score_f64":
        if c.P == 0:
            return b | {f"{e}:P==0"}
        b.add(f"{e}:{'lane-stride-many' if c.J > 128 else 'one-stride'}")
        b |= ({f"{e}:ragged-last-wave"} if c.J % WAVE else set()) | ({f"{e}:idle-second-wave"} if c.J <= WAVE else set())
    else:
        if c.C == 0:
            return b | {f"{e}:C==0"}
        b.add(f"{e}:{'second-workgroup' if c.C > 128 else 'one-workgroup'}")
        b |= ({f"{e}:ragged-last-wave"} if c.C % WAVE else set()) | {f"{e}:threshold-equal", f"{e}:sel-out-of-order"} if c.C > 1 else set()
        b |= {f"{e}:sel-duplicates"} if c.C > 2 else set()
    return b


def _reachable():
    r = set()
    for e in ("contact_map_f32", "entropy_f32"):
        r |= {e, f"{e}:lane-stride-once", f"{e}:lane-stride-many", f"{e}:ragged-last-block", f"{e}:full-blocks", f"{e}:ragged-last-wave", f"{e}:zero-row"}
    r |= {"contact_map_f32:contact-given", "contact_map_f32:contact-null", "entropy_f32:nbin20", "entropy_f32:nbin1000000"}
    for tag, w in (("significant_pairs_u8", None), ("masked_max_f32:which0", 0), ("masked_max_f32:which1", 1)):
        r |= {tag.split(":")[0], tag, f"{tag}:empty-mask", f"{tag}:nan-path", f"{tag}:only-column-past-64", f"{tag}:only-column-past-256", f"{tag}:only-row-past-4"}
        r |= {f"{tag}:lane-stride-many", f"{tag}:row-blocks", f"{tag}:ragged-last-block"} if w in (None, 0) else set()
        r |= {f"{tag}:second-workgroup"} if w in (None, 1) else set()
    r.add("significant_pairs_u8:pairs-second-workgroup")
    e = "contact_select_u8"
    r |= {e} | {f"{e}:{t}" for t in ("threshold-equal", "nan-path", "lane-stride-many", "row-blocks", "ragged-last-block", "ragged-last-wave")}
    e = "row_argmax_i64"
    r |= {e} | {f"{e}:{t}" for t in ARGMAX_PATTERNS + ("outs-both", "outs-idx", "outs-val", "strided", "dense", "lane-stride-many", "tie-across-strides",
                                                       "tie-across-lanes", "nan-path", "ragged-last-block", "ragged-last-wave")}
    e = "nearest_vertex_i64"
    r |= {e} | {f"{e}:{t}" for t in ("P==0", "idle-threads", "one-stride", "lane-stride-many", "tie-across-lanes", "tie-across-waves", "tie-across-strides",
                                     "tie-lower-index-on-higher-thread", "random", "far", "at", "nan-point", "nan-path", "nan-vertex")}
    e = "vertex_normals_f64"
    r |= {e} | {f"{e}:{t}" for t in ("eps>=0", "eps<0", "S1", "S3", "one-workgroup", "second-workgroup", "ragged-last-wave", "zero-normal", "isolated-vertex",
                                     "zero-area-faces", "others-poisoned")}
    e = "dlt_score_f64"
    r |= {e} | {f"{e}:{t}" for t in ("P==0", "one-stride", "lane-stride-many", "ragged-last-wave", "idle-second-wave")}
    e = "ransac_mse_f64"
    r |= {e} | {f"{e}:{t}" for t in ("C==0", "one-workgroup", "second-workgroup", "ragged-last-wave", "threshold-equal", "sel-duplicates", "sel-out-of-order")}
    return r


REACHABLE = _reachable()


# ------------------------------------------------------------------------------------------------------------------ data
def fibonacci_sphere32(n):
    i = np.arange(n, dtype=f64)
    y = 1 - (i / max(n - 1, 1)) * 2
    r = np.sqrt(np.maximum(1 - y * y, 0))
    th = math.pi * (3.0 - math.sqrt(5.0)) * i
    return np.stack([np.cos(th) * r, y, np.sin(th) * r], -1).astype(f32)


def _histogram_rows(g, M, N, n_bin, tiny_row):
    """f32 [M, N] of non-negative rows whose normalised values v keep v * n_bin at least 0.15 away from every k + 1/2, so that no
    rounding of an f32 evaluation (relative error of v below 2^-18 at these sizes; v * n_bin <= 1e6) can move an element across a
    rounding boundary: targets t = k + f with integers k summing to n_bin - slack and fractions 0 <= f <= 0.35 summing to slack, the row
    is t times a scale.  Row 0 (M > 1) is all zero: sum + eps is the whole divisor.  With tiny_row the last row (M > 2) is of the order of
    eps = 1e-8, so that eps decides its result (contact_map only: such a row has no margin to its rounding boundaries)."""
    x = np.zeros((M, N), f64)
    for m in range(M):
        slack = min(0.17 * N, 0.75 * n_bin)
        K = int(math.ceil(n_bin - slack))
        slack = n_bin - K
        u = g.uniform(0.5, 1.0, N)
        fr = slack * u / u.sum()
        k = g.multinomial(K, g.dirichlet(np.full(N, 0.6))) if N > 1 else np.array([K])
        assert fr.max() <= 0.35
        x[m] = (k + fr) * (g.uniform(0.5, 40.0) / n_bin)
    if M > 1:
        x[0] = 0.0
    if M > 2 and tiny_row:
        x[M - 1] *= 1e-9 / x[M - 1].sum() * 7
    return x.astype(f32)


def _cameras(n):
    from coma_amd import triangulate as tr
    cams = []
    for v in range(n):
        ang = 2 * np.pi * v / n + 0.1
        eye = np.array([2.6 * np.cos(ang), 2.6 * np.sin(ang), 1.2 + 0.05 * v])
        f = (np.array([0, 0, 0.9]) - eye) / np.linalg.norm(np.array([0, 0, 0.9]) - eye)
        r = np.cross(f, [0.0, 0.0, 1.0])
        r /= np.linalg.norm(r)
        cams.append(dict(R=np.stack([r, np.cross(r, f), -f], axis=1), t=eye, resolution=(512, 384), scale=2.5))
    return cams, np.stack([tr.view_record(c) for c in cams])


def _icosphere():
    t = (1 + 5 ** 0.5) / 2
    v = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], f64)
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
         [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    v = list(v / np.linalg.norm(v[0]))
    mid, out = {}, []
    for a, b, c in f:
        m = []
        for p, q in ((a, b), (b, c), (c, a)):
            key = (min(p, q), max(p, q))
            if key not in mid:
                w = v[p] + v[q]
                mid[key] = len(v)
                v.append(w / np.linalg.norm(w))
            m.append(mid[key])
        out += [[a, m[0], m[2]], [b, m[1], m[0]], [c, m[2], m[1]], m]
    return np.array(v), np.array(out, i32)                      # 42 vertices, 80 faces


def _mesh(g, V):
    """V = 4: a tetrahedron.  Otherwise: the 42-vertex icosphere, then a soup over the next vertices -- random triangles, faces with a
    repeated index, faces on three collinear integer points (both kinds have a cross product of exactly zero; vertices 50 and 51 have
    only such faces: the zero normal) -- and isolated vertices: 60 and the last three."""
    if V == 4:
        return np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], f64) + g.normal(scale=0.01, size=(4, 3)), np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], i32)
    v0, f0 = _icosphere()
    v = np.concatenate([v0 * (1 + g.normal(scale=0.05, size=(42, 1))), g.normal(size=(V - 42, 3))])
    v[43:46] = [[0, 0, 0], [1, 1, 1], [2, 2, 2]]
    faces = [[43, 44, 45], [50, 51, 51], [51, 50, 50], [46, 46, 47], [45, 44, 43]]
    free = [i for i in range(42, V - 3) if i not in (50, 51, 60)]
    for _ in range(2 * V):
        faces.append([int(i) for i in g.choice(free, 3, replace=False)])
    f = np.concatenate([f0, np.array(faces, i32)])
    return v, f[g.permutation(len(f))].astype(i32)


def csr(faces, V):
    """vertex -> incident faces, ascending face index (a face naming a vertex twice is listed twice, as a per-face loop adds it twice)"""
    flat = faces.reshape(-1).astype(np.int64)
    fid = np.repeat(np.arange(len(faces)), 3)
    order = np.lexsort((fid, flat))
    off = np.zeros(V + 1, i32)
    np.add.at(off, flat + 1, 1)
    return np.cumsum(off).astype(i32), fid[order].astype(i32)


@functools.lru_cache(maxsize=None)
def _data(cid):
    c = BY_ID[cid]
    e, g = c.entry[5:], kit.rng(cid)
    if e in ("contact_map_f32", "entropy_f32"):
        prob = _histogram_rows(g, c.M, c.N, c.n_bin, e == "contact_map_f32")
        if (c.M, c.N) == (2, 8):
            prob[1] = 1.0                                       # n_bin = 20: v * n_bin = 2.5 exactly, half-to-even gives 2 (away gives 3)
        d = dict(prob=prob)
        if e == "contact_map_f32":
            nom, den = g.uniform(0.1, 3.0, c.M).astype(f32), g.integers(1, 9, c.M).astype(f32)
            if c.M > 3:
                den[1], nom[1] = 0.0, 0.0                       # 0 / 0: NaN
                den[2] = 0.0                                    # nom / 0: +inf
            pv = np.array([0.0, 0.6, 0.8], f32)
            d.update(grid=fibonacci_sphere32(c.N), pvec=pv, nom=nom, den=den)
        return d
    if e in ("significant_pairs_u8", "masked_max_f32"):
        H, O = c.H, c.O
        cnt = g.integers(0, 11, (H, O)).astype(f32)
        thr = f32(5.0)
        if c.mask == "none":
            cnt = np.minimum(cnt, 4).astype(f32)
        if c.mask == "one":
            cnt = np.minimum(cnt, 4).astype(f32)
            cnt[one_cell(H, O)] = thr                          # equal to the threshold: >= sets it
        if c.mask == "random" and H * O > 1:
            cnt[H // 2, O // 2] = NAN                           # NaN >= thr is false
            cnt[0, 0] = thr
        pairs = (cnt >= thr).astype(u8)
        d = dict(cnt=cnt, thr=thr, pairs=pairs, col_any=pairs.any(0).astype(u8), row_any=pairs.any(1).astype(u8))
        if e == "masked_max_f32":
            C = g.normal(size=(H, O)).astype(f32)
            C[g.random((H, O)) < 0.1] = -INF
            col, row = d["col_any"].astype(bool), d["row_any"].astype(bool)
            live = np.outer(np.ones(H, bool), col) if c.which == 0 else np.outer(row, np.ones(O, bool))
            if c.mask == "random" and H * O > 1:
                if c.which == 0:
                    C[H - 1, :] = -INF                          # an all -inf row: the maximum is -inf, not the 0 of an empty mask
                else:
                    C[:, O - 1] = -INF
                hh, oo = np.argwhere(live)[len(np.argwhere(live)) // 2]
                C[hh, oo] = NAN                                 # a NaN at a masked-in place: np.max gives NaN
            C[~live] = NAN                                      # poison: a read outside the mask turns the maximum into NaN
            d["contact"] = C
        return d
    if e == "contact_select_u8":
        H, O = c.H, c.O
        thr = f32(0.5)
        den = g.integers(1, 9, (H, O)).astype(f32)
        nom = (g.uniform(0.0, 0.45, (H, O)) * den).astype(f32)
        nom[g.random((H, O)) < 0.1] = -INF
        last = O - 1 if O % WAVE != 1 else O - 1
        for h in range(H):
            kind = h % 5
            if kind == 0:
                nom[h, last] = f32(0.75) * den[h, last]         # the only quotient above the threshold sits in the last column
            elif kind == 1 and O > 1:
                nom[h, O // 2], den[h, O // 2] = 2.0, 4.0       # the maximum EQUALS the threshold: strict > says no
            elif kind == 2 and O > 1:
                nom[h, O - 1], den[h, O - 1] = 0.0, 0.0         # NaN in the row: false, whatever else it holds
                nom[h, 0] = 3.0 * den[h, 0]
            elif kind == 3:
                nom[h, :] = -INF                                # all -inf: false
        return dict(nom=nom, den=den, thr=thr)
    if e == "row_argmax_i64":
        n, rs, co = c.n, c.row_stride, c.col_offset
        x = np.full((c.rows, rs + co), NAN, f32)                # (the last row's tail past row_stride belongs to the operand as well)
        body = g.normal(size=(c.rows, n)).astype(f32)
        for r in range(c.rows):
            pat = ARGMAX_PATTERNS[(c.first_pattern + r) % 5]
            row = body[r]
            k = int(g.integers(0, max(n - 65, 1))) if n > 65 else max(n // 2 - 1, 0)
            if pat == "tie-next" and n > 1:
                row[k] = row[k + 1] = 9.0
            elif pat == "tie-64" and n > 1:
                row[k] = row[k + 64 if k + 64 < n else n - 1] = 9.0
            elif pat == "nan-first" and n > 1:
                row[0], row[n - 1] = NAN, NAN
                row[n // 2] = 9.0
            elif pat == "nan-after-larger" and n > 1:
                row[0] = 9.0
                row[n - 1] = NAN                                # past the first lane stride where n > 64
            elif pat == "all-ninf":
                row[:] = -INF
        full = np.full(c.rows * rs + co + 8, NAN, f32)
        for r in range(c.rows):
            full[r * rs + co:r * rs + co + n] = body[r]
        return dict(x=full, body=body)
    if e == "nearest_vertex_i64":
        verts = g.normal(size=(c.V, 3))
        pts = np.zeros((c.P, 3))
        for p, q in enumerate(c.queries):
            if q[0] == "random":
                pts[p] = g.normal(size=3)
            elif q[0] == "dup":
                verts[q[2]] = verts[q[1]]
                pts[p] = verts[q[1]]                            # exactly on the pair: both distances are +0
            elif q[0] == "at":
                pts[p] = verts[q[1]]                            # the answer lies in the second stride of thread 0
            elif q[0] == "far":
                pts[p] = [1e200, -1e200, 1e200]                 # every squared distance overflows to +inf
            else:
                pts[p] = [0.5, NAN, 0.25]
        for v in c.nan_verts:
            verts[v, 1] = NAN
        return dict(points=pts, verts=verts)
    if e == "vertex_normals_f64":
        v, faces = _mesh(kit.rng(f"mesh-{c.V}"), c.V)
        gs = kit.rng(f"samples-{c.V}")                             # (the same samples for every eps and for the poisoned twin)
        verts = np.stack([v] + [v + gs.normal(scale=0.03, size=v.shape) for _ in range(c.S - 1)])
        if c.V > 4:
            verts[:, 43:46] = [[0, 0, 0], [1, 1, 1], [2, 2, 2]]
        if c.poison_others:
            verts[0], verts[2] = NAN, NAN
        off, vf = csr(faces, c.V)
        return dict(verts=verts, faces=faces, off=off, vf=vf)
    # triangulation: a ring of cameras, a skeleton seen by each with pixel noise
    P = c.P
    cams, views = _cameras(6)
    J = c.J
    skel = g.normal(scale=[0.25, 0.15, 0.45], size=(J, 3)) + np.array([0.0, 0.0, 0.9])
    from oracle import triangulation_oracle as T
    ref_xy = T.render(skel.copy(), cams[0]) + g.normal(scale=1.0, size=(J, 2))
    cand_view = np.array([1 + (3 * p) % 5 for p in range(P)], i32)
    cand_xy = np.stack([T.render(skel.copy(), cams[int(v)]) + g.normal(scale=1.0 + 0.5 * p, size=(J, 2)) for p, v in enumerate(cand_view)]) if P else np.zeros((0, J, 2))
    d = dict(views=views, cams=cams, ref_xy=ref_xy, cand_view=cand_view, cand_xy=cand_xy)
    if e == "ransac_mse_f64":
        d["tri"] = _dlt(d, np.float64, J)[0]
        sel = g.integers(0, P, c.C).astype(i32)                 # out of order, with duplicates
        if c.C > 2:
            sel[1] = sel[0]
        elif c.C == 2:
            sel[:] = [7, 3]
        d["sel"] = sel
        m = _ransac(d, c.C, J)
        d["thr"] = float(m[c.C // 2, c.C // 3]) if c.C else 200.0   # one entry of the emulation's own matrix: the strict < decides it
    return d


def data(c):
    return _data(c.id)


# ------------------------------------------------------------------------------------------------------------------ plan: operands and outputs
class In(NamedTuple):
    body: np.ndarray            # flat
    poison: object              # value of the guard elements


class Out(NamedTuple):
    init: np.ndarray            # flat first contents (the sentinel, or the data of an operand written in place)
    must: np.ndarray            # bool: elements the launch has to write
    finite: np.ndarray          # bool: elements that must come out finite


def pack(body, guard_value):
    return kit.pack_rows(body.reshape(-1), guard_value)


def _out(n, dtype, written=True, finite=True, init=None):
    init = sentinel(n, dtype) if init is None else np.ascontiguousarray(init).reshape(-1)
    return Out(init, np.full(n, bool(written)), np.broadcast_to(np.asarray(finite), (n,)).copy() if np.dtype(dtype).kind == "f" else np.zeros(n, bool))


def plan(c):
    """(name -> In, name -> Out).  Guards of float operands are NaN, of the masks 1 (a guard byte read as a mask entry admits a NaN of
    contact's guard or poison).  The index tables the kernels follow (faces, CSR, cand_view, sel) get 0: a guard must never send a
    kernel outside its buffers, so a stray read of those shows only through the values it then fetches."""
    e, d = c.entry[5:], data(c)
    if e == "contact_map_f32":
        ins = dict(grid=In(d["grid"].reshape(-1), NAN), nom=In(d["nom"], NAN), den=In(d["den"], NAN))
        ref = reference(c)
        outs = dict(prob=_out(c.M * c.N, f32, init=d["prob"]))
        outs["contact"] = _out(c.M, f32, written=bool(c.with_contact), finite=np.isfinite(ref["contact"].ref))
        return ins, outs
    if e == "entropy_f32":
        return {}, dict(prob=_out(c.M * c.N, f32, init=d["prob"]), score=_out(c.M, f32))
    if e == "significant_pairs_u8":
        return dict(cnt=In(d["cnt"].reshape(-1), NAN)), dict(pairs=_out(c.H * c.O, u8), col_any=_out(c.O, u8), row_any=_out(c.H, u8))
    if e == "masked_max_f32":
        ref = reference(c)["out"]
        return (dict(contact=In(d["contact"].reshape(-1), NAN), col_any=In(d["col_any"], u8(1)), row_any=In(d["row_any"], u8(1))),
                dict(out=_out(ref.size, f32, finite=np.isfinite(ref))))
    if e == "contact_select_u8":
        return dict(nom=In(d["nom"].reshape(-1), NAN), den=In(d["den"].reshape(-1), NAN)), dict(selected=_out(c.H, u8))
    if e == "row_argmax_i64":
        ref = reference(c)
        return dict(x=In(d["x"], NAN)), dict(idx=_out(c.rows, i64, written=c.outs != "val"), val=_out(c.rows, f32, written=c.outs != "idx", finite=np.isfinite(ref["val"])))
    if e == "nearest_vertex_i64":
        return dict(points=In(d["points"].reshape(-1), NAN), verts=In(d["verts"].reshape(-1), NAN)), dict(idx=_out(max(c.P, 1), i64, written=c.P > 0))
    if e == "vertex_normals_f64":
        big = i32(0)
        return (dict(verts=In(d["verts"].reshape(-1), NAN), faces=In(d["faces"].reshape(-1), big), off=In(d["off"], big), vf=In(d["vf"], big)),
                dict(normals=_out(c.S * c.V * 3, f64)))
    ins = dict(views=In(d["views"].reshape(-1), NAN), cand_view=In(d["cand_view"], i32(0)), cand_xy=In(d["cand_xy"].reshape(-1), NAN))
    if e == "dlt_score_f64":
        ins["ref_xy"] = In(d["ref_xy"].reshape(-1), NAN)
        w = c.P > 0
        return ins, dict(tri=_out(max(c.P, 1) * c.J * 3, f64, written=w), ref_mse=_out(max(c.P, 1), f64, written=w), other_mse=_out(max(c.P, 1), f64, written=w))
    ins.update(tri=In(d["tri"].reshape(-1), NAN), sel=In(d["sel"], i32(0)))
    w = c.C > 0
    return ins, dict(mse=_out(max(c.C * c.C, 1), f64, written=w), counts=_out(max(c.C, 1), i32, written=w))


_HOST_VEC = {}          # principle_vec is read on the HOST by the entry point: a real host array per case, kept alive here


def arguments(c, ptr):
    """keywords of the entry point in the header's parameter names; ptr: name of plan()'s operand / output -> address of its body"""
    e, d = c.entry[5:], data(c)
    if e == "contact_map_f32":
        pv = _HOST_VEC.setdefault(c.id, (ctypes.c_float * 3)(*[float(x) for x in d["pvec"]]))
        return dict(prob=ptr["prob"], sphere_grid=ptr["grid"], principle_vec=ctypes.addressof(pv), nom=ptr["nom"], den=ptr["den"], M=c.M, N=c.N, eps=c.eps,
                    contact=ptr["contact"] if c.with_contact else None)
    if e == "entropy_f32":
        return dict(prob=ptr["prob"], M=c.M, N=c.N, eps=c.eps, n_bin=c.n_bin, score=ptr["score"])
    if e == "significant_pairs_u8":
        return dict(cnt=ptr["cnt"], threshold=float(d["thr"]), H=c.H, O=c.O, pairs=ptr["pairs"], col_any=ptr["col_any"], row_any=ptr["row_any"])
    if e == "masked_max_f32":
        return dict(contact=ptr["contact"], col_any=ptr["col_any"], row_any=ptr["row_any"], H=c.H, O=c.O, which=c.which, out=ptr["out"])
    if e == "contact_select_u8":
        return dict(nom=ptr["nom"], den=ptr["den"], H=c.H, O=c.O, threshold=float(d["thr"]), selected=ptr["selected"])
    if e == "row_argmax_i64":
        return dict(x=ptr["x"], rows=c.rows, n=c.n, row_stride=c.row_stride, col_offset=c.col_offset, idx=ptr["idx"] if c.outs != "val" else None,
                    val=ptr["val"] if c.outs != "idx" else None)
    if e == "nearest_vertex_i64":
        return dict(points=ptr["points"], verts=ptr["verts"], P=c.P, V=c.V, idx=ptr["idx"])
    if e == "vertex_normals_f64":
        return dict(verts=ptr["verts"], faces=ptr["faces"], vf_offsets=ptr["off"], vf_faces=ptr["vf"], S=c.S, V=c.V, F=len(d["faces"]), eps=c.eps, normals=ptr["normals"])
    if e == "dlt_score_f64":
        return dict(views=ptr["views"], n_views=len(d["views"]), ref_view=0, ref_xy=ptr["ref_xy"], cand_view=ptr["cand_view"], cand_xy=ptr["cand_xy"], P=c.P, J=c.J,
                    tri=ptr["tri"], ref_mse=ptr["ref_mse"], other_mse=ptr["other_mse"])
    return dict(views=ptr["views"], tri=ptr["tri"], cand_view=ptr["cand_view"], cand_xy=ptr["cand_xy"], sel=ptr["sel"], C=c.C, J=c.J, threshold=d["thr"],
                mse=ptr["mse"], counts=ptr["counts"])


def launch(lib, c, ptr):
    return kit.call(lib, c.entry, arguments(c, ptr), None)


# ------------------------------------------------------------------------------------------------------------------ the kernels' summation shapes
def butterfly(v):
    """the xor butterfly over 64 lanes, in v's dtype: every lane ends with the same sum; lane 0's is returned.  v [..., 64]"""
    lane = np.arange(WAVE)
    for m in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ m]
    return v[..., 0]


def lane_sums(x, width=WAVE, drop_stride=False):
    """per-lane partial sums of x [..., n] in x's dtype: lane l adds x[l], x[l + width], ... in that order -> [..., width]"""
    n = x.shape[-1]
    acc = np.zeros(x.shape[:-1] + (width,), x.dtype)
    for k0 in range(0, n, width):
        if drop_stride and k0 >= width:
            break
        seg = x[..., k0:k0 + width]
        acc[..., :seg.shape[-1]] = acc[..., :seg.shape[-1]] + seg
    return acc


def wave_sum(x, **kw):
    return butterfly(lane_sums(x, **kw))


def block_sum_128(x):
    """triangulate.hip: 128 threads strided over x [..., n], a butterfly per wave, then the two partials"""
    acc = lane_sums(x, 128)
    return butterfly(acc[..., :64]) + butterfly(acc[..., 64:])


# ------------------------------------------------------------------------------------------------------------------ triangulation, in any float type
def _render(w, x, ft):
    """get_view2joints_render with the kernel's operation order; w: 28 numbers of type ft, x [..., 3] -> px, py"""
    mr, tmr, scale, maxres, hx, hy = w[12:21], w[21:24], w[24], w[25], w[26], w[27]
    cx = ((x[..., 0] * mr[0] + x[..., 1] * mr[3]) + x[..., 2] * mr[6]) - tmr[0]
    cy = ((x[..., 0] * mr[1] + x[..., 1] * mr[4]) + x[..., 2] * mr[7]) - tmr[1]
    return cx / scale * maxres + hx, cy / scale * maxres + hy


def _mse_norm(px, py, x, y):
    """what one joint's squared pixel error is sensitive to: d = p - x carries the roundings of the rendering relative to |p| + |x|, and
    d^2 moves by 2 |d| times that; the squares and their sums round relative to d^2 itself"""
    dx, dy = np.abs(px - x), np.abs(py - y)
    return 2 * (dx * (np.abs(px) + np.abs(x)) + dy * (np.abs(py) + np.abs(y))) + (dx * dx + dy * dy)


def _dlt(d, ft, J, sums=None):
    """tri [P, J, 3], ref_mse [P], other_mse [P] (and the norms of the two mses) by the normal equations with a cofactor inverse, every
    operation in ft and in the kernel's order; `sums` reduces the per-joint squared errors (the kernel's block_sum_128 by default)"""
    sums = sums or block_sum_128
    views, rxy, cxy = d["views"].astype(ft), d["ref_xy"].astype(ft), d["cand_xy"].astype(ft)
    P = len(d["cand_view"])
    tri, rm, om, nrm, nom_ = np.zeros((P, J, 3), ft), np.zeros(P, ft), np.zeros(P, ft), np.zeros(P, ft), np.zeros(P, ft)
    r = views[0]
    for p in range(P):
        o = views[int(d["cand_view"][p])]
        a = [r[0:3], r[3:6], o[0:3], o[3:6]]
        n = [[((a[0][i] * a[0][k] + a[1][i] * a[1][k]) + a[2][i] * a[2][k]) + a[3][i] * a[3][k] for k in range(3)] for i in range(3)]
        c00, c01, c02 = n[1][1] * n[2][2] - n[1][2] * n[2][1], n[1][2] * n[2][0] - n[1][0] * n[2][2], n[1][0] * n[2][1] - n[1][1] * n[2][0]
        det = n[0][0] * c00 + n[0][1] * c01 + n[0][2] * c02
        inv = [[c00 / det, (n[0][2] * n[2][1] - n[0][1] * n[2][2]) / det, (n[0][1] * n[1][2] - n[0][2] * n[1][1]) / det],
               [c01 / det, (n[0][0] * n[2][2] - n[0][2] * n[2][0]) / det, (n[0][2] * n[1][0] - n[0][0] * n[1][2]) / det],
               [c02 / det, (n[0][1] * n[2][0] - n[0][0] * n[2][1]) / det, (n[0][0] * n[1][1] - n[0][1] * n[1][0]) / det]]
        rx, ry, ox, oy = rxy[:, 0], rxy[:, 1], cxy[p, :, 0], cxy[p, :, 1]
        b = [(rx - r[26]) - r[9], (ry - r[27]) - r[10], (ox - o[26]) - o[9], (oy - o[27]) - o[10]]
        atb = [((a[0][i] * b[0] + a[1][i] * b[1]) + a[2][i] * b[2]) + a[3][i] * b[3] for i in range(3)]
        x = np.stack([(inv[i][0] * atb[0] + inv[i][1] * atb[1]) + inv[i][2] * atb[2] for i in range(3)], -1)
        tri[p] = x
        px, py = _render(r, x, ft)
        rm[p] = sums((px - rx) * (px - rx) + (py - ry) * (py - ry)) / ft(J)
        nrm[p] = _mse_norm(px, py, rx, ry).sum() / ft(J)
        px, py = _render(o, x, ft)
        om[p] = sums((px - ox) * (px - ox) + (py - oy) * (py - oy)) / ft(J)
        nom_[p] = _mse_norm(px, py, ox, oy).sum() / ft(J)
    return tri, rm, om, nrm, nom_


def _ransac(d, C, J, ft=np.float64, norms=False):
    """mse [C, C]: a sequential sum over the joints per (a, b), as the kernel's one thread per pair adds them"""
    views, tri, cxy, sel = d["views"].astype(ft), d["tri"].astype(ft), d["cand_xy"].astype(ft), d["sel"]
    mse, nm = np.zeros((C, C), ft), np.zeros((C, C), ft)
    for b in range(C):
        ib = int(sel[b])
        w = views[int(d["cand_view"][ib])]
        t = tri[sel.astype(np.int64)]                           # [C, J, 3]: every a at once
        px, py = _render(w, t, ft)
        dx, dy = cxy[ib, :, 0] - px, cxy[ib, :, 1] - py
        term = dx * dx + dy * dy
        e = np.zeros(C, ft)
        for j in range(J):
            e = e + term[:, j]
        mse[:, b] = e / ft(J)
        nm[:, b] = _mse_norm(px, py, cxy[ib, :, 0], cxy[ib, :, 1]).sum(-1) / ft(J)
    return (mse, nm) if norms else mse


# ------------------------------------------------------------------------------------------------------------------ the reference
class Ref(NamedTuple):
    ref: np.ndarray             # float64 (non-finite where the formula is: compared by class there)
    norm: np.ndarray            # what the error is divided by: the sum of magnitudes of the formula's terms
    floor: float                # counted roundings of the formula in the output's format


def _strides(n):
    return -(-n // WAVE)


def _np_argmin(d):
    return np.argmin(d, axis=-1)


@functools.lru_cache(maxsize=None)
def _reference(cid):
    c = BY_ID[cid]
    e, d = c.entry[5:], data(c)
    if e in ("contact_map_f32", "entropy_f32"):
        x = d["prob"].astype(f64)
        s = x.sum(-1, keepdims=True) + f64(f32(c.eps))
        v = x / s
        # prob: a sum of N non-negative terms in strides + 6 butterfly steps, + eps, one division: relative error (strides + 8) u
        out = dict(prob=Ref(v, np.where(v == 0, 1.0, v), (_strides(c.N) + 8) * U32))
        if e == "contact_map_f32":
            g, p = d["grid"].astype(f64), d["pvec"].astype(f64)
            w = (1.0 - (g * p).sum(-1)) / 2.0
            with np.errstate(divide="ignore", invalid="ignore"):
                prox = d["nom"].astype(f64) / d["den"].astype(f64)
                ref = (v * w).sum(-1) * prox
                norm = (v * ((1.0 + (np.abs(g) * np.abs(p)).sum(-1)) / 2.0)).sum(-1) * np.abs(prox)
            # contact: v as above (strides + 8), the weight 5 (three products, two sums, 1 - dot; the halving is exact), the product 1,
            # the sum strides + 6, nom / den 1, the last product 1
            out["contact"] = Ref(ref, np.where(np.isfinite(norm) & (norm > 0), norm, 1.0), (2 * _strides(c.N) + 22) * U32)
        else:
            nb = f64(f32(c.n_bin))
            q = np.rint(v * nb) / nb                            # (np.rint: half to even, as torch.round)
            with np.errstate(divide="ignore", invalid="ignore"):
                plogp = np.where(q == 0, 0.0, q * np.log(q))
            ln = f64(f32(math.log(c.n_bin)))
            # score: q = k / n_bin 1 (the data keeps k itself safe), log 2, product 1, its own error through q log q at most u in all
            # (sum q ~ 1) 1, the sum strides + 6, the division 1, ln(n_bin) in f32 1, + 1 1
            out["score"] = Ref(plogp.sum(-1) / ln + 1.0, 1.0 + np.abs(plogp).sum(-1) / ln, (_strides(c.N) + 14) * U32)
        return out
    if e == "significant_pairs_u8":
        pairs = d["cnt"] >= d["thr"]
        return dict(pairs=pairs.astype(u8).reshape(-1), col_any=pairs.any(0).astype(u8), row_any=pairs.any(1).astype(u8))
    if e == "masked_max_f32":
        C, col, row = d["contact"], d["col_any"].astype(bool), d["row_any"].astype(bool)
        if c.which == 0:
            return dict(out=C[:, col].max(-1) if col.any() else np.zeros(c.H, f32))
        return dict(out=C[row, :].max(0) if row.any() else np.zeros(c.O, f32))
    if e == "contact_select_u8":
        with np.errstate(divide="ignore", invalid="ignore"):
            return dict(selected=(np.max(d["nom"] / d["den"], axis=1) > d["thr"]).astype(u8))
    if e == "row_argmax_i64":
        return dict(idx=np.argmax(d["body"], axis=1).astype(i64), val=np.max(d["body"], axis=1).astype(f32))
    if e == "nearest_vertex_i64":
        with np.errstate(over="ignore", invalid="ignore"):
            q = np.square(d["points"][:, None, :] - d["verts"][None, :, :])
            return dict(idx=_np_argmin((q[..., 0] + q[..., 1]) + q[..., 2]).astype(i64) if c.P else np.zeros(0, i64))
    if e == "vertex_normals_f64":
        from oracle import coma_oracle as orc
        out = []
        for s in range(c.S):
            with np.errstate(invalid="ignore"):
                n = orc.vertex_normals(d["verts"][s], d["faces"])
                if c.eps >= 0:
                    n = n / (np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]) + c.eps)[:, None]
            out.append(n)
        return dict(normals=np.stack(out).reshape(-1))
    L = np.longdouble
    if e == "dlt_score_f64":
        tri, rm, om, nrm, nom_ = _dlt(d, L, c.J, sums=lambda t: t.sum(-1))
        top = np.abs(tri).reshape(c.P, -1).max(-1, keepdims=True) if c.P else np.zeros((0, 1))
        # tri: A^T A 7, cofactors 3, det 5, the quotient 1, b 2, A^T b 7, the product with the inverse 5: 30 roundings to first order, taken
        # twice for the higher orders; the conditioning of the pair multiplies all of it and is what 4 e_emu carries.
        # the mses: the rendering 8, the difference 1, squares and their sum 3, the sum over the joints in strides + 7, the division 1
        fl = (13 + -(-c.J // 128) + 7) * U64
        return dict(tri=Ref(tri.astype(f64).reshape(-1), np.repeat(top.astype(f64), c.J * 3), 64 * U64), ref_mse=Ref(rm.astype(f64), nrm.astype(f64), fl),
                    other_mse=Ref(om.astype(f64), nom_.astype(f64), fl))
    mse, nm = _ransac(d, c.C, c.J, L, norms=True)
    return dict(mse=Ref(mse.astype(f64).reshape(-1), nm.astype(f64).reshape(-1), (13 + c.J) * U64))    # the joints are added one after the other


def reference(c):
    return _reference(c.id)


# ------------------------------------------------------------------------------------------------------------------ the emulation
MUTATIONS = ("last-maximum", "max-ignores-nan", "ge-to-gt", "gt-to-ge", "round-half-away", "lane-stride-dropped", "last-partial-wave-dropped",
             "eps-before-the-sum", "masks-swapped", "col-offset-ignored", "faces-reversed", "tie-by-thread", "nearest-skips-nan")


def _first_best(v, index, mut, smallest=False):
    """index of the element np.argmax (np.argmin with `smallest`) picks among v -- NaN wins, the lowest `index` among equals -- or what a
    mutated reduction picks"""
    v, index = np.asarray(v), np.asarray(index)
    nan = np.isnan(v)
    if nan.any() and mut not in ("max-ignores-nan", "nearest-skips-nan"):
        cand = np.nonzero(nan)[0]
    else:
        w = np.where(nan, INF if smallest else -INF, v)
        cand = np.nonzero(w == (w.min() if smallest else w.max()))[0]
    if mut == "last-maximum":
        return int(cand[np.argmax(index[cand])])
    if mut == "tie-by-thread":
        return int(cand[np.lexsort((index[cand], index[cand] % 256))[0]])
    return int(cand[np.argmin(index[cand])])


def emulate(c, mut=None):
    """name -> the output bodies as the kernels leave them (what they do not write keeps plan()'s first contents), every operation in the
    kernel's precision and order; `mut` plants one defect."""
    e, d = c.entry[5:], data(c)
    out = {k: o.init.copy() for k, o in plan(c)[1].items()}
    drop = mut == "lane-stride-dropped"

    def rows_written(n):                                        # the last, partial block of four row waves is lost
        return n - n % ROW_WAVES if mut == "last-partial-wave-dropped" and n % ROW_WAVES else n

    if e in ("contact_map_f32", "entropy_f32"):
        x = d["prob"]
        M = rows_written(c.M)
        eps = f32(c.eps)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            if mut == "eps-before-the-sum":
                acc = lane_sums(x, drop_stride=drop) + eps      # every lane starts from eps
                s = butterfly(acc)
            else:
                s = wave_sum(x, drop_stride=drop) + eps
            v = (x / s[:, None]).astype(f32)
            out["prob"].reshape(c.M, c.N)[:M] = v[:M]
            if e == "contact_map_f32":
                g, p = d["grid"], d["pvec"]
                dot = (p[0] * g[:, 0] + p[1] * g[:, 1]) + p[2] * g[:, 2]
                w = (f32(1.0) - dot) / f32(2.0)
                if c.with_contact:
                    out["contact"][:M] = (wave_sum(v * w, drop_stride=drop) * (d["nom"] / d["den"]))[:M]
            else:
                nb = f32(c.n_bin)
                t = v * nb
                k = np.where(t - np.floor(t) == f32(0.5), np.floor(t) + 1, np.rint(t)).astype(f32) if mut == "round-half-away" else np.rint(t)
                q = (k / nb).astype(f32)
                lg = np.log(q.astype(f64)).astype(f32)          # logf through float64, rounded once
                term = np.where(q == 0, f32(0), q * lg).astype(f32)
                out["score"][:M] = (wave_sum(term, drop_stride=drop) / f32(math.log(c.n_bin)) + f32(1.0))[:M]
    elif e == "significant_pairs_u8":
        cnt = d["cnt"]
        pairs = (cnt > d["thr"]) if mut == "ge-to-gt" else (cnt >= d["thr"])
        out["pairs"][:] = pairs.reshape(-1)
        H = rows_written(c.H)
        out["col_any"][:] = pairs.any(0)
        out["row_any"][:H] = (pairs[:, :WAVE] if drop else pairs).any(1)[:H]
        if mut == "masks-swapped":
            out["col_any"][:], out["row_any"][:] = np.resize(pairs.any(1), c.O), np.resize(pairs.any(0), c.H)
    elif e == "masked_max_f32":
        C, col, row = d["contact"], d["col_any"].astype(bool), d["row_any"].astype(bool)
        if mut == "masks-swapped":
            col, row = np.resize(row, c.O), np.resize(col, c.H)
        mask = col if c.which == 0 else row
        A = C if c.which == 0 else C.T                          # [outputs, reduced axis]
        n_out = rows_written(A.shape[0]) if c.which == 0 else A.shape[0]
        for r in range(n_out):
            live = mask.copy()
            if drop and c.which == 0:
                live[WAVE:] = False
            vals = A[r][live]
            if not live.any():
                out["out"][r] = 0.0
            elif np.isnan(vals).any() and mut != "max-ignores-nan":
                out["out"][r] = NAN
            else:
                out["out"][r] = np.nanmax(vals) if not np.isnan(vals).all() else -INF
    elif e == "contact_select_u8":
        with np.errstate(divide="ignore", invalid="ignore"):
            q = (d["nom"] / d["den"]).astype(f32)
        if drop:
            q = q[:, :WAVE]
        nan = np.isnan(q).any(1) & (mut != "max-ignores-nan")
        mx = np.where(np.isnan(q), -INF, q).max(1)              # fmaxf drops NaNs; the flag carries them
        sel = (mx >= d["thr"]) if mut == "gt-to-ge" else (mx > d["thr"])
        H = rows_written(c.H)
        out["selected"][:H] = (~nan & sel)[:H]
    elif e == "row_argmax_i64":
        co = 0 if mut == "col-offset-ignored" else c.col_offset
        for r in range(rows_written(c.rows)):
            row = d["x"][r * c.row_stride + co:r * c.row_stride + co + c.n]
            if drop:
                row = row[:WAVE]
            k = _first_best(row, np.arange(row.size), None if mut == "nearest-skips-nan" else mut)
            if c.outs != "val":
                out["idx"][r] = k
            if c.outs != "idx":
                out["val"][r] = row[k]
    elif e == "nearest_vertex_i64":
        with np.errstate(over="ignore", invalid="ignore"):
            for p in range(c.P):
                dv = d["points"][p][None, :] - d["verts"][:256 if drop else None]
                dist = (dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1]) + dv[:, 2] * dv[:, 2]
                out["idx"][p] = _first_best(dist, np.arange(dist.size), mut, smallest=True)
    elif e == "vertex_normals_f64":
        faces, off, vf = d["faces"].astype(np.int64), d["off"], d["vf"]
        V = c.V - c.V % WAVE if mut == "last-partial-wave-dropped" and c.V % WAVE else c.V
        nrm = out["normals"].reshape(c.S, c.V, 3)
        with np.errstate(invalid="ignore", divide="ignore"):
            for s in range(c.S):
                P = d["verts"][s]
                a, b = P[faces[:, 1]] - P[faces[:, 0]], P[faces[:, 2]] - P[faces[:, 0]]
                tn = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], -1)
                for v in range(V):
                    n = np.zeros(3)
                    fs = vf[off[v]:off[v + 1]]
                    for f in (fs[::-1] if mut == "faces-reversed" else fs):
                        n = n + tn[f]
                    ln = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
                    n = n / ln if ln > 0 else np.array([0.0, 0.0, 1.0])
                    if c.eps >= 0:
                        ss = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
                        n = n / (np.sqrt(ss + c.eps) if mut == "eps-before-the-sum" else np.sqrt(ss) + c.eps)
                    nrm[s, v] = n
    elif e == "dlt_score_f64":
        if c.P:
            tri, rm, om, _, _ = _dlt(d, np.float64, c.J)
            out["tri"][:], out["ref_mse"][:], out["other_mse"][:] = tri.reshape(-1), rm, om
    elif c.C:
        mse = _ransac(d, c.C, c.J)
        out["mse"][:] = mse.reshape(-1)
        out["counts"][:] = ((mse <= d["thr"]) if mut == "gt-to-ge" else (mse < d["thr"])).sum(1)
    return out


# ------------------------------------------------------------------------------------------------------------------ the checks
class Figure(NamedTuple):
    e_emu: float
    bound: float
    err: float


def _err(got, r: Ref):
    """largest error in units of r.norm over the finite elements of the reference; the others must agree in class (NaN, +inf, -inf)"""
    got, fin = np.asarray(got, f64).reshape(r.ref.shape), np.isfinite(r.ref)
    assert np.array_equal(np.isnan(got), np.isnan(r.ref)), "NaN where the reference has none, or none where it has one"
    inf = np.isinf(r.ref)
    assert np.array_equal(got[inf], r.ref[inf]), "an infinite result differs"
    assert bool(np.isfinite(got[fin]).all()), "a non-finite value where the reference is finite"
    return float((np.abs(got[fin] - r.ref[fin]) / r.norm[fin]).max()) if fin.any() else 0.0


def same(a, b, what):
    """bit for bit; any NaN equals any NaN"""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype.kind == "f":
        both = np.isnan(a) & np.isnan(b)
        bad = np.nonzero((bits(a) != bits(b)) & ~both)[0]
    else:
        bad = np.nonzero(a != b)[0]
    assert bad.size == 0, f"{what}: {bad.size} of {a.size} elements differ, first at {int(bad[0])}: {a[bad[0]]!r} != {b[bad[0]]!r}"


@functools.lru_cache(maxsize=None)
def _yardstick(cid):
    c = BY_ID[cid]
    emu, out = emulate(c), {}
    for name, r in reference(c).items():
        if isinstance(r, Ref) and plan(c)[1][name].must.any():
            e = _err(emu[name], r)
            out[name] = (e, max(4 * e, r.floor))
    return out


def yardstick(c):
    """output name -> (e_emu, bound) of the arithmetic outputs the case writes"""
    return _yardstick(c.id)


def check(c, got):
    """Every assertion of case c on the output bodies `got` (name -> flat array, as emulate() returns them) -> name -> Figure."""
    ref, outs, y, fig = reference(c), plan(c)[1], yardstick(c), {}
    for name, o in outs.items():
        g = np.asarray(got[name]).reshape(-1)
        assert g.dtype == o.init.dtype and g.size == o.init.size, name
        same(g[~o.must], o.init[~o.must], f"{c.id}: `{name}` outside what the launch owns keeps its first contents")
        if not o.must.any():
            continue
        assert not bool((bits(g[o.must]) == bits(sentinel(1, g.dtype))[0]).any()), f"{c.id}: an element the launch owns of `{name}` still holds the sentinel"
        if g.dtype.kind == "f":
            assert bool(np.isfinite(g[o.must & o.finite]).all()), f"{c.id}: NaN / Inf in `{name}` where the case is finite"
        r = ref.get(name)
        if r is None:                                           # ransac's counts: against the given mse, below
            continue
        if isinstance(r, Ref):
            e_emu, bound = y[name]
            err = _err(g, r)
            fig[name] = Figure(e_emu, bound, err)
            assert err <= bound, f"{c.id}: `{name}` error {err:.3e} > {bound:.3e} (e_emu {e_emu:.3e})"
        else:
            same(g, r, f"{c.id}: `{name}`")
    if c.entry == "coma_ransac_mse_f64" and c.C:
        m = np.asarray(got["mse"]).reshape(c.C, c.C)
        same(np.asarray(got["counts"]), (m < data(c)["thr"]).sum(1).astype(i32), f"{c.id}: counts against the given mse")
    return fig


# ------------------------------------------------------------------------------------------------------------------ refusals
OUTPUT_ARGS = {"prob", "contact", "score", "pairs", "col_any", "row_any", "out", "idx", "val", "selected", "normals", "tri", "ref_mse", "other_mse", "mse", "counts"}
HOST_ARGS = {"principle_vec"}          # read on the host by the entry point: the tests put real host memory there


def _nulls(text, *names):
    return [(text, {n: None}) for n in names]


_CM = dict(prob=PTR, sphere_grid=PTR, principle_vec=PTR, nom=PTR, den=PTR, M=4, N=8, eps=1e-8, contact=PTR)
_SP = dict(cnt=PTR, threshold=1.0, H=2, O=4, pairs=PTR, col_any=PTR, row_any=PTR)
_MM = dict(contact=PTR, col_any=PTR, row_any=PTR, H=2, O=4, which=0, out=PTR)
_RA = dict(x=PTR, rows=2, n=8, row_stride=8, col_offset=0, idx=PTR, val=PTR)
_VN = dict(verts=PTR, faces=PTR, vf_offsets=PTR, vf_faces=PTR, S=1, V=4, F=4, eps=-1.0, normals=PTR)
_DL = dict(views=PTR, n_views=2, ref_view=0, ref_xy=PTR, cand_view=PTR, cand_xy=PTR, P=1, J=4, tri=PTR, ref_mse=PTR, other_mse=PTR)
_RM = dict(views=PTR, tri=PTR, cand_view=PTR, cand_xy=PTR, sel=PTR, C=2, J=4, threshold=1.0, mse=PTR, counts=PTR)

# entry point -> (accepted base, [(text of the refusal, change), ...]): every condition the argument checks state
REFUSALS = {
    "coma_contact_map_f32": (_CM, _nulls("null pointer", "prob", "sphere_grid", "principle_vec") + [
        ("nom/den required", dict(nom=None)), ("nom/den required", dict(den=None)), ("bad sizes", dict(M=0)), ("bad sizes", dict(M=-4)), ("bad sizes", dict(N=0)),
        ("bad sizes", dict(N=-1)), ("M too large", dict(M=4 * (2 ** 31 - 1) + 1)), ("M too large", dict(M=1 << 40, contact=None))]),
    "coma_entropy_f32": (dict(prob=PTR, M=4, N=8, eps=1e-8, n_bin=20.0, score=PTR), _nulls("null pointer", "prob", "score") + [
        ("bad sizes", dict(M=0)), ("bad sizes", dict(N=0)), ("bad sizes", dict(N=-8)), ("bad sizes", dict(n_bin=1.0)), ("bad sizes", dict(n_bin=0.0)),
        ("bad sizes", dict(n_bin=NAN)), ("M too large", dict(M=4 * (2 ** 31 - 1) + 1))]),
    "coma_significant_pairs_u8": (_SP, _nulls("null pointer", "cnt", "pairs", "col_any", "row_any") + [
        ("bad sizes", dict(H=0)), ("bad sizes", dict(O=0)), ("bad sizes", dict(H=-2)), ("bad sizes", dict(O=-4))]),
    "coma_masked_max_f32": (_MM, _nulls("null pointer", "contact", "col_any", "row_any", "out") + [
        ("bad args", dict(H=0)), ("bad args", dict(O=0)), ("bad args", dict(H=-1)), ("bad args", dict(which=2)), ("bad args", dict(which=-1))]),
    "coma_row_argmax_i64": (_RA, [("null pointer", dict(x=None)), ("null pointer", dict(idx=None, val=None)),
        ("bad sizes", dict(rows=0)), ("bad sizes", dict(rows=-1)), ("bad sizes", dict(n=0)), ("bad sizes", dict(row_stride=7)), ("bad sizes", dict(col_offset=-1)),
        ("rows too large", dict(rows=4 * (2 ** 31 - 1) + 1)), ("rows too large", dict(rows=1 << 40, val=None))]),
    "coma_contact_select_u8": (dict(nom=PTR, den=PTR, H=2, O=4, threshold=0.5, selected=PTR), _nulls("null pointer", "nom", "den", "selected") + [
        ("bad sizes", dict(H=0)), ("bad sizes", dict(O=0)), ("bad sizes", dict(H=-2)), ("bad sizes", dict(O=-4))]),
    "coma_nearest_vertex_i64": (dict(points=PTR, verts=PTR, P=2, V=4, idx=PTR), _nulls("null pointer", "points", "verts", "idx") + [
        ("bad sizes P=-1 V=4", dict(P=-1)), ("bad sizes P=2 V=0", dict(V=0)), ("bad sizes P=0 V=-3", dict(P=0, V=-3))]),
    "coma_vertex_normals_f64": (_VN, _nulls("null pointer", "verts", "faces", "vf_offsets", "vf_faces", "normals") + [
        ("bad sizes", dict(S=0)), ("bad sizes", dict(V=0)), ("bad sizes", dict(F=0)), ("bad sizes", dict(S=-1)),
        ("S = 65536 exceeds the grid limit 65535", dict(S=65536)), ("S = 2147483647 exceeds the grid limit 65535", dict(S=2 ** 31 - 1))]),
    "coma_dlt_score_f64": (_DL, _nulls("null pointer", "views", "ref_xy", "cand_view", "cand_xy", "tri", "ref_mse", "other_mse") + [
        ("bad sizes P=-1 J=4 views=2 ref=0", dict(P=-1)), ("bad sizes P=1 J=0", dict(J=0)), ("bad sizes P=1 J=4 views=0", dict(n_views=0)),
        ("views=2 ref=-1", dict(ref_view=-1)), ("views=2 ref=2", dict(ref_view=2)), ("bad sizes P=0 J=-1", dict(P=0, J=-1))]),
    "coma_ransac_mse_f64": (_RM, _nulls("null pointer", "views", "tri", "cand_view", "cand_xy", "sel", "mse", "counts") + [
        ("bad sizes C=-1 J=4", dict(C=-1)), ("bad sizes C=2 J=0", dict(J=0)), ("bad sizes C=0 J=0", dict(C=0, J=0)),
        ("C = 65536 exceeds the grid limit 65535", dict(C=65536)), ("C = 2147483647 exceeds the grid limit 65535", dict(C=2 ** 31 - 1))]),
}

BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES) and set(REFUSALS) == set(ENTRIES) <= set(_lib.PARAMS)
