"""The three occupancy entry points of coma_amd/csrc/occupancy.hip -- coma_occupancy_splat (K5), coma_occupancy_reduce (K6) and
coma_occupancy_fused (K5 + K6) -- over the domain their argument checks accept.  CPU only: the table of launches (CASES), the operands
(data), the dense reference (reference: sqrt(((cx-qx)^2 + (cy-qy)^2) + (cz-qz)^2) < thres in f64 over all R^3 centres), an emulation of
the fused pass's own decisions (emulate: candidate ranges, the f32 decision, the 2^-18 T2 band and the exact recount inside it, the
first-W-cells rule, plane buckets and rounds, 16-bit counter halves, quotient table below 256 and division above, group maxima), the
regimes a case reaches counted through that emulation (branches), the assertions the device is held to (check) and every argument check
(REFUSALS).  tests/test_coma_core_domain_gpu.py launches the table; tests/test_coma_core_ref_host.py checks the table itself.

The bound: none.  Counts, row sums, the normalised grid, the raw grid and the field match the reference in every bit on all three routes
(splat + reduce, fused with write_raw 0, fused with write_raw 1); NaN-ness is compared for NaNs.  Above a row sum of 2^24 (one case) the
contract is the fused route's alone: the row sum is the correctly rounded f32 of the exact integer and every quotient the correctly
rounded division by it; of the other route only the counts are compared there."""
import functools
import math

import numpy as np

from tests import domain_kit as kit
from tests.domain_kit import PTR, Off

f32, f64, u8 = np.float32, np.float64, np.uint8
NAN, INF = float("nan"), float("inf")
FAR = 50.0                                  # a position farther than any threshold from the whole grid: no candidate range
MAX_CELLS, LIST_CAP, RESIDENT = 20480, 512, 512          # kFusedMaxCells, kFusedListCap, kFusedResident of occupancy.hip
ROUTES = ("splat", "fused", "fused_raw")


class Case:
    def __init__(self, id, R, H, tol, rows, select="null", table="grid", window=None, big=False):
        self.id, self.R, self.H, self.tol, self.rows, self.select, self.table, self.big = id, R, H, tol, rows, select, table, big
        self._window = window

    def __repr__(self):
        return self.id


def window_needed(voxel, thres):
    """ComA_Occupancy._window and occ_window_needed of occupancy.hip: the same expression"""
    return int(np.ceil(2.0 * thres / voxel - 1e-9)) + 2


def pow2_window(w):
    return w if w <= 2 else 1 << (w - 1).bit_length()


def sqrt_cut(thres):
    """the smallest double whose square root is >= thres (ComA_Occupancy._sqrt_cut)"""
    y = f64(thres) * f64(thres)
    while np.sqrt(y) >= thres:
        y = np.nextafter(y, f64(0.0))
    while np.sqrt(y) < thres:
        y = np.nextafter(y, f64(np.inf))
    return float(y)


def axis_table(R, gridsize=2.4):
    """the per-axis centres as load_voxelgrid builds them: voxel * f32(index) is an f32 product, the additions are f64"""
    voxel = gridsize / R
    return (-gridsize / 2) + (f32(voxel) * np.arange(R, dtype=f32)).astype(f64) + voxel / 2, voxel


# a (dx, dy) offset in units of the hand-made table whose distance is irrational: thres = fl(sqrt(X)) with X = dx^2 + dy^2 exact, so that
# d == thres can be constructed with fl(thres * thres) != the cut (tests/test_coma_core_ref_host.py checks that it differs)
HAND_VOXEL = 0.25
HAND_OFFSETS = {"hand-equal": (0.5, 0.0, 0.0), "hand-cut": (0.5, 0.25, 0.0)}


@functools.lru_cache(maxsize=None)
def geometry(cid):
    """-> (cen [3, R] f64, voxel, thres, t2, window)"""
    c = BY_ID[cid]
    if c.table == "grid":
        ax, voxel = axis_table(c.R)
        thres = voxel * c.tol
    else:
        voxel = HAND_VOXEL
        ax = (np.arange(c.R, dtype=f64) - c.R / 2 + 0.5) * voxel
        o = HAND_OFFSETS[c.table]
        thres = float(np.sqrt(f64((o[0] * o[0] + o[1] * o[1]) + o[2] * o[2])))
    window = c._window if c._window is not None else window_needed(voxel, thres)
    return np.stack([ax, ax, ax]).copy(), float(voxel), float(thres), sqrt_cut(thres), window


# ------------------------------------------------------------------------------------------------------------------ positions
def _near(rng, cen, thres, t2, n, R, margin):
    """n positions whose squared distance to a chosen centre lies within 8 f32 ulps of T2, alternately on either side of the cut, along
    each axis (both senses) and along two diagonals: q = f32(c - u thres), then one coordinate stepped by f32 ulps"""
    dirs = [np.array(d, f64) for d in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
    dirs += [np.array((1, 1, 1), f64) / math.sqrt(3.0), np.array((-2, 1, -2), f64) / 3.0]
    ulp = float(np.spacing(f32(t2)))
    out = []
    for s in range(n):
        u = dirs[s % len(dirs)]
        idx = rng.integers(margin, R - margin, 3)
        ctr = np.array([cen[a][idx[a]] for a in range(3)])
        q0 = (ctr - u * thres).astype(f32)
        ax = int(np.argmax(np.abs(u)))
        found = {}
        for k in range(-48, 49):
            q = q0.copy()
            for _ in range(abs(k)):
                q[ax] = np.nextafter(q[ax], f32(INF if k > 0 else -INF))
            d = ctr - q.astype(f64)
            delta = float(((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) - t2) / ulp
            if abs(delta) <= 8:
                found.setdefault(delta < 0, []).append(q)
        side = found.get(s // len(dirs) % 2 == 0) or found.get(True) or found.get(False) or [q0]
        out.append(side[s % len(side)])
    return np.array(out, f32)


def _faces(rng, n, thres, half=1.2):
    """positions within thres of each face, edge and corner of the grid, some just outside it"""
    out = []
    for s in range(n):
        kind = (s % 26) + 1                                          # base-3 digits: -face, interior, +face per axis, never all interior
        p = []
        for a in range(3):
            sign = (0.0, -1.0, 1.0)[(kind // (1, 3, 9)[a]) % 3]
            p.append(rng.uniform(-1.0, 1.0) if sign == 0.0 else sign * (half + rng.uniform(-0.95, 0.95) * thres))
        out.append(p)
    return np.array(out, f32)


def _segment(rng, kind, n, cen, thres, t2, R, W):
    if kind == "interior":
        return rng.uniform(-1.0, 1.0, (n, 3)).astype(f32)
    if kind == "faces":
        return _faces(rng, n, thres)
    if kind == "outside":                                            # just outside the grid: a range exists, no centre is reached
        return np.array([[1.2 + thres * 1.5, 0.1, -0.2], [0.3, -1.2 - thres * 1.2, 0.0], [0.0, 0.5, 1.2 + thres * 1.01]] * n, f32)[:n]
    if kind == "far":
        return np.full((n, 3), FAR, f32)
    if kind == "nonfinite":
        pool = [(NAN, 0.1, 0.2), (0.1, NAN, 0.2), (0.1, 0.2, NAN), (INF, 0.0, 0.0), (0.0, -INF, 0.0), (0.3, 0.3, INF), (NAN, NAN, NAN), (-INF, INF, NAN)]
        a = np.array([pool[s % len(pool)] for s in range(n)], f32)
        neg = a.view(np.uint32).copy()                               # NaNs of both signs
        neg[1::2] |= np.where(np.isnan(a[1::2]), np.uint32(0x80000000), np.uint32(0))
        return neg.view(f32)
    if kind == "near":
        return _near(rng, cen, thres, t2, n, R, min(W, (R - 1) // 2))
    if kind.startswith("at:"):                                       # n copies of one position
        return np.tile(np.array([float(v) for v in kind[3:].split(",")], f32), (n, 1))
    if kind.startswith("x:"):                                        # x fixed (chooses the planes), y and z random interior
        p = rng.uniform(-0.8, 0.8, (n, 3)).astype(f32)
        p[:, 0] = f32(float(kind[2:]))
        return p
    if kind.startswith("sphere:"):                                   # the hand-made tables: d == thres exactly, and one step inside / outside
        o = HAND_OFFSETS[kind[7:]]
        out = []
        for s in range(n):
            ctr = np.array([cen[a][2 + (s + a) % (R - 4)] for a in range(3)])
            perm = [(0, 1, 2), (1, 2, 0), (2, 0, 1)][s % 3]
            off = np.zeros(3)
            for a in range(3):
                off[perm[a]] = o[a] * (1.0 if (s // 3) % 2 == 0 else -1.0)
            q = (ctr - off).astype(f32)
            assert np.array_equal(q.astype(f64), ctr - off)         # exactly representable
            step = (s // 6) % 3                                      # 0: exactly on the sphere, 1: one f32 ulp inside, 2: one outside
            if step:
                a = perm[0]
                toward = ctr[a] if step == 1 else q[a] - (ctr[a] - q[a])
                q[a] = np.nextafter(q[a], f32(toward))
            out.append(q)
        return np.array(out, f32)
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def data(cid):
    """-> dict(q [S, H, 3] f32, cen, voxel, thres, t2, window, W, select (u8 [H] or None))"""
    c = BY_ID[cid]
    cen, voxel, thres, t2, window = geometry(cid)
    W = pow2_window(window)
    rows = []
    for h in range(c.H):
        spec = c.rows[h] if h < len(c.rows) else c.rows[-1]
        rng = kit.rng(c.id, h)
        rows.append(np.concatenate([_segment(rng, kind, n, cen, thres, t2, c.R, W) for kind, n in spec]))
    S = max(len(r) for r in rows)
    q = np.full((S, c.H, 3), FAR, f32)
    for h, r in enumerate(rows):
        q[:len(r), h] = r
    if c.select == "null":
        sel = None
    elif c.select == "none":
        sel = np.zeros(c.H, u8)
    else:
        sel = (np.arange(c.H) % 2 == 0).astype(u8) if c.H > 1 else np.ones(1, u8)
        sel[0] = 1
    return dict(q=q, cen=cen, voxel=voxel, thres=thres, t2=t2, window=window, W=W, select=sel, S=S)


def _unique(Q):
    """distinct positions of a row (by bits) and how often each occurs: the predicate is a function of the position alone"""
    b = np.ascontiguousarray(Q).view(np.uint32).reshape(-1, 3)
    u, mult = np.unique(b, axis=0, return_counts=True)
    return u.view(f32).reshape(-1, 3), mult.astype(np.int64)


# ------------------------------------------------------------------------------------------------------------------ the reference
def _max_rows(norm, sel):
    """NaN-propagating maximum over the selected rows; -inf where nothing is selected"""
    pick = np.ones(len(norm), bool) if sel is None else sel.astype(bool)
    if not pick.any():
        return np.full(norm.shape[1], -INF, f32)
    with np.errstate(invalid="ignore"):
        return np.max(norm[pick], axis=0)                           # np.max propagates NaN


@functools.lru_cache(maxsize=None)
def reference(cid):
    """dense: every one of the R^3 centres against every position, f64, no contraction -> counts (int64 [H, R3]), rowsum_exact (int
    [H]), rowsum (f32), norm (f32 [H, R3]), field (f32 [R3])"""
    c, d = BY_ID[cid], data(cid)
    cen, thres, R = d["cen"], f64(d["thres"]), c.R
    counts = np.zeros((c.H, R ** 3), np.int64)
    for h in range(c.H):
        uq, mult = _unique(d["q"][:, h])
        for p, m in zip(uq.astype(f64), mult):
            with np.errstate(invalid="ignore", over="ignore"):
                dx2, dy2, dz2 = np.square(cen[0] - p[0]), np.square(cen[1] - p[1]), np.square(cen[2] - p[2])
                dist = np.sqrt((dx2[:, None, None] + dy2[None, :, None]) + dz2[None, None, :])
                counts[h] += m * (dist < thres).reshape(-1)
    exact = [int(v) for v in counts.sum(1)]
    rowsum = np.array([f32(v) for v in exact], f32)                  # int -> f64 (exact) -> f32: one rounding
    with np.errstate(invalid="ignore", divide="ignore"):
        norm = counts.astype(f32) / rowsum[:, None]
    return dict(counts=counts, rowsum_exact=exact, rowsum=rowsum, norm=norm, field=_max_rows(norm, d["select"]))


# ------------------------------------------------------------------------------------------------------------------ the emulation
MUTATIONS = ("lt-to-le", "band-dropped", "t2-is-thres-squared", "window-short", "last-slab-planes", "edge-mask-off-by-one", "counter-carry",
             "table-index-clamped", "group-max-not-sticky", "select-ignored", "raw-normalises")


def layout(R, H):
    P = MAX_CELLS // (R * R)
    slabs = -(-R // P)
    groups = min(H, -(-RESIDENT // slabs))
    return P, slabs, groups


def _ranges(qd, cen0, thres, inv, R):
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.floor((qd - thres - cen0) * inv - 0.01)
        b = np.ceil((qd + thres - cen0) * inv + 0.01)
    a = np.clip(np.nan_to_num(a, nan=0.0, posinf=2.0 ** 31 - 1, neginf=-2.0 ** 31), 0, None)
    b = np.clip(np.nan_to_num(b, nan=0.0, posinf=2.0 ** 31 - 1, neginf=-2.0 ** 31), None, R - 1)
    return a.astype(np.int64), (b - a + 1).astype(np.int64)


def emulate(cid, mut=None, write_raw=0):
    """the fused pass as the code decides -> dict(counts f32 [H * R3 + tail], rowsum f32 [H], out f32 [R3], stats)"""
    assert mut is None or mut in MUTATIONS
    c, d = BY_ID[cid], data(cid)
    R, H, W, cen = c.R, c.H, d["W"], d["cen"]
    RR, R3 = R * R, R ** 3
    thres, inv = f64(d["thres"]), f64(1.0) / f64(d["voxel"])
    t2 = f64(d["thres"]) * f64(d["thres"]) if mut == "t2-is-thres-squared" else f64(d["t2"])
    t2f, band = f32(t2), f32(t2 * 2.0 ** -18)
    pre_ok = 1e-30 < t2 < 1e30
    Wf = W - 1 if mut == "window-short" else W                      # the first-W-cells rule
    fast_prep, fast = W <= 8 and pre_ok, W == 8 and pre_ok
    Wx, Wc = W + 1, (8 if W <= 8 else W)
    P, slabs, groups = layout(R, H)
    SH = 12 if mut == "counter-carry" else 16
    st = dict(fast_hit=0, fast_miss=0, prep_recount=0, amb_hit=0, amb_miss=0, edge_items=0, shared_word=0, buckets=np.zeros((H, slabs), np.int64),
              w_last_x=0, w_last_yz=0)
    lt = (lambda x, y: x <= y) if mut == "lt-to-le" else (lambda x, y: x < y)
    cnt = np.zeros((H, R3), np.int64)
    rowsum = np.zeros(H, f32)
    for h in range(H):
        uq, mult = _unique(d["q"][:, h])
        keep = np.isfinite(uq).all(1)                                # a non-finite position has no candidate range
        uq, mult = uq[keep], mult[keep]
        hits_total = 0
        for i0 in range(0, len(uq), 128):
            Q, m = uq[i0:i0 + 128], mult[i0:i0 + 128]
            qd = Q.astype(f64)
            lo, n = zip(*(_ranges(qd[:, a], cen[a][0], thres, inv, R) for a in range(3)))
            ok = (n[0] > 0) & (n[1] > 0) & (n[2] > 0)
            Q, m, qd = Q[ok], m[ok], qd[ok]
            lo, n = [v[ok] for v in lo], [v[ok] for v in n]
            if not len(Q):
                continue
            ar = lambda a, w: lo[a][:, None] + np.arange(w)[None, :]                    # [s, w] cell indices, unclamped
            ix, iy, iz = ar(0, Wx), ar(1, Wc), ar(2, Wc)
            off = lambda a, i: cen[a][np.minimum(i, R - 1)] - qd[:, a, None]             # f64 offsets (clamped index, as the kernel reads)
            dx, dy, dz = off(0, ix), off(1, iy), off(2, iz)
            exact = lt(((dx * dx)[:, :, None, None] + (dy * dy)[:, None, :, None]) + (dz * dz)[:, None, None, :], t2)
            vx = (np.arange(Wx)[None, :] < n[0][:, None])
            rng_y = np.arange(Wc)[None, :] < np.minimum(n[1], Wf)[:, None]
            rng_z = np.arange(Wc)[None, :] < np.minimum(n[2], Wf)[:, None]
            full_y, full_z = np.arange(Wc)[None, :] < n[1][:, None], np.arange(Wc)[None, :] < n[2][:, None]
            if fast_prep or fast:
                dxf, dyf, dzf = dx.astype(f32), dy.astype(f32), dz.astype(f32)
                with np.errstate(invalid="ignore", over="ignore"):
                    dxy = (dxf * dxf)[:, :, None] + (dyf * dyf)[:, None, :]
                    dd = dxy[:, :, :, None] + (dzf * dzf - t2f)[:, None, None, :]       # fl(fl(dx2 + dy2) + fl(dz2 - fl(T2)))
                sign, inband = np.signbit(dd), (np.abs(dd) <= band) & (mut != "band-dropped")
            # ---- the preparation pass: the row sum
            if fast_prep:
                live = vx[:, :, None, None] & rng_y[:, None, :, None] & rng_z[:, None, None, :]
                amb_plane = (inband & live).any((2, 3))
                c32 = (sign & live).sum((2, 3))
                cex = (exact[:, :, :Wc, :Wc] & vx[:, :, None, None] & full_y[:, None, :, None] & full_z[:, None, None, :]).sum((2, 3))
                per = np.where(amb_plane, cex, c32) * vx
                st["prep_recount"] += int(amb_plane.sum())
            else:
                per = (exact & vx[:, :, None, None] & full_y[:, None, :, None] & full_z[:, None, None, :]).sum((2, 3))
            hits_total += int((per.sum(1) * m).sum())
            # ---- the incidences and the fused pass's candidate tests
            inc = np.arange(Wx)[None, :] < np.minimum(n[0], Wf)[:, None]               # planes that become incidences
            for sl in range(slabs):
                st["buckets"][h, sl] += int(((inc & (ix >= sl * P) & (ix < (sl + 1) * P)).sum(1) * m).sum())
            in_y = (iy < R) & (np.arange(Wc)[None, :] < (Wf if mut == "window-short" else Wc))
            edge = 1 if mut == "edge-mask-off-by-one" and fast else 0
            in_z = (iz < R + edge) & (np.arange(Wc)[None, :] < (Wf if mut == "window-short" else Wc))
            if not fast:
                in_y &= np.arange(Wc)[None, :] < W
                in_z &= np.arange(Wc)[None, :] < W
            live = inc[:, :, None, None] & in_y[:, None, :, None] & in_z[:, None, None, :]
            if fast:
                hit = np.where(inband, exact, sign) & live
                st["fast_hit"] += int((sign & ~inband & live).sum())
                st["fast_miss"] += int((~sign & ~inband & live).sum())
                st["amb_hit"] += int((inband & exact & live).sum())
                st["amb_miss"] += int((inband & ~exact & live).sum())
                st["edge_items"] += int((inc & ((lo[2] + 8 > R)[:, None])).sum())
            else:
                hit = exact & live
            flat = ix[:, :, None, None] * RR + iy[:, None, :, None] * R + iz[:, None, None, :]   # cell + k: an unmasked k past the edge spills on
            pair = hit[..., :-1] & hit[..., 1:] & ((flat[..., :-1] & 1) == 0)
            st["shared_word"] += int(pair.sum())
            st["w_last_x"] += int(hit[:, W - 1].sum()) if hit.shape[1] >= W else 0
            st["w_last_yz"] += int(hit[:, :, W - 1].sum() + hit[:, :, :, W - 1].sum())
            sel_flat = np.broadcast_to(flat, hit.shape)[hit]
            w = np.broadcast_to(m[:, None, None, None], hit.shape)[hit]
            inside = sel_flat < R3
            np.add.at(cnt[h], sel_flat[inside], w[inside])
        rowsum[h] = f32(hits_total)
    if SH != 16:                                                     # halves of SH bits: the low half carries into its neighbour
        lo_, hi_ = cnt[:, 0::2].copy(), cnt[:, 1::2].copy()
        cnt[:, 0::2], cnt[:, 1::2] = lo_ % (1 << SH), hi_ + lo_ // (1 << SH)
    # ---- the sweep: quotient table below 256, division above; per-group running maxima; the group maximum
    tail = P * RR
    counts = np.concatenate([np.zeros(H * R3, f32), kit.sentinel(tail, f32)])
    cf = cnt.astype(f32)
    with np.errstate(invalid="ignore", divide="ignore"):
        tab = np.arange(256, dtype=f32)[None, :] / rowsum[:, None]
        v = np.where(cnt < 256, np.take_along_axis(tab, np.minimum(cnt, 255), 1), tab[:, 255:256] if mut == "table-index-clamped" else cf / rowsum[:, None])
    store = v if (not write_raw or mut == "raw-normalises") else cf
    last_np = R - (slabs - 1) * P
    for h in range(H):
        counts[h * R3:(h + 1) * R3] = store[h]
        if mut == "last-slab-planes" and last_np < P and h == H - 1:   # the last slab stores P planes: past the row, past the buffer for the last row
            counts[H * R3:H * R3 + (P - last_np) * RR] = f32(0.0) / rowsum[h] if not write_raw else f32(0.0)
    sel = None if mut == "select-ignored" else d["select"]
    part = np.full((groups, R3), -INF, f32)
    for g in range(groups):
        for h in range(H * g // groups, H * (g + 1) // groups):
            if sel is None or sel[h]:
                with np.errstate(invalid="ignore"):
                    part[g] = np.where((v[h] > part[g]) | np.isnan(v[h]), v[h], part[g])
    with np.errstate(invalid="ignore"):
        out = np.fmax.reduce(part, 0) if mut == "group-max-not-sticky" else np.max(part, 0)
    st["max_count"], st["counts_set"] = int(cnt.max()), set(np.unique(cnt[(cnt >= 250) & (cnt <= 260)]).tolist())
    return dict(counts=counts, rowsum=rowsum, out=out.astype(f32), stats=st, tail=tail)


# ------------------------------------------------------------------------------------------------------------------ regimes
REACHABLE = {"f32-decision-hit", "f32-decision-miss", "prep-band-recount", "fused-amb-recount-hit", "fused-amb-recount-miss", "one-round", "multi-round",
             "round-hand-over-513", "overlap-hand-over", "non-overlap-hand-over", "sparse-then-crowded", "crowded-then-sparse", "partial-last-slab", "exact-fit-slabs",
             "one-slab", "edge-mask", "table-division-seam", "count-255", "count-256", "count-thousands", "shared-counter-word", "W4", "W8", "W16",
             "window-3", "window-4", "window-5", "window-6", "window-7", "window-8", "window-9", "window-16", "select-null", "select-some", "select-none", "nan-row",
             "nonfinite-row", "H-above-groups", "H-equals-groups", "H-1", "rowsum-above-2^24", "hit-in-last-window-cell-x", "hit-in-last-window-cell-yz",
             "d-equals-thres", "P-1", "P-2"}


@functools.lru_cache(maxsize=None)
def branches(cid):
    c, d = BY_ID[cid], data(cid)
    e = emulate(cid)
    st, ref = e["stats"], reference(cid)
    P, slabs, groups = layout(c.R, c.H)
    b = {f"W{d['W']}", f"window-{d['window']}", f"select-{c.select}"}
    for name, key in (("f32-decision-hit", "fast_hit"), ("f32-decision-miss", "fast_miss"), ("prep-band-recount", "prep_recount"), ("fused-amb-recount-hit", "amb_hit"),
                      ("fused-amb-recount-miss", "amb_miss"), ("edge-mask", "edge_items"), ("shared-counter-word", "shared_word"),
                      ("hit-in-last-window-cell-x", "w_last_x"), ("hit-in-last-window-cell-yz", "w_last_yz")):
        if st[key]:
            b.add(name)
    bk = st["buckets"]
    for g in range(groups):
        hs = list(range(c.H * g // groups, c.H * (g + 1) // groups))
        for sl in range(slabs):
            first = int(bk[hs[0], sl])
            if 0 < first <= LIST_CAP:
                b.add("one-round")
            if first > 2 * LIST_CAP:
                b.add("multi-round")
            if first == LIST_CAP + 1:
                b.add("round-hand-over-513")
            for prev, nxt in zip(hs, hs[1:]):
                over = int(bk[nxt, sl]) <= LIST_CAP
                b.add("overlap-hand-over" if over else "non-overlap-hand-over")
                if int(bk[prev, sl]) <= 64 and not over:
                    b.add("sparse-then-crowded")
                if int(bk[prev, sl]) > LIST_CAP and int(bk[nxt, sl]) <= 64:
                    b.add("crowded-then-sparse")
    b.add("one-slab" if slabs == 1 else "partial-last-slab" if c.R % P else "exact-fit-slabs")
    if P <= 2:
        b.add(f"P-{P}")
    if st["max_count"] >= 256 and (ref["counts"] > 0).any() and ((ref["counts"] > 0) & (ref["counts"] < 256)).any():
        b.add("table-division-seam")
    b |= {f"count-{k}" for k in (255, 256) if k in st["counts_set"]}
    if st["max_count"] >= 2000:
        b.add("count-thousands")
    if any(v == 0 for v in ref["rowsum_exact"]):
        b.add("nan-row")
    if any(not np.isfinite(d["q"][:, h]).all() for h in range(c.H)):
        b.add("nonfinite-row")
    b.add("H-1" if c.H == 1 else "H-above-groups" if c.H > groups else "H-equals-groups")
    if max(ref["rowsum_exact"]) > 2 ** 24:
        b.add("rowsum-above-2^24")
    if c.table != "grid":
        b.add("d-equals-thres")
    return b


# ------------------------------------------------------------------------------------------------------------------ the assertions
def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN where the reference has none, or the reverse"
    bad = kit.bits(got)[~nan] != kit.bits(want)[~nan]
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {int(np.flatnonzero(bad.reshape(-1))[0]) if nan.sum() == 0 else '?'}"


def compared_routes(c):
    return ("fused", "fused_raw") if c.big else ROUTES


def check(c, got):
    """got: route -> dict(counts [H * R3] (+ an optional tail that must still hold the sentinel), rowsum [H], out [R3]); for the splat route
    `counts` is the normalised grid after the reducer and `raw` the counts the splat left.  -> the number of elements compared"""
    ref = reference(c.id)
    H, R3 = c.H, c.R ** 3
    raw, n = ref["counts"].astype(f32), 0
    for route in compared_routes(c):
        g = got[route]
        body, tail = g["counts"][:H * R3].reshape(H, R3), g["counts"][H * R3:]
        assert bool((kit.bits(tail) == kit.sentinel_bits(f32)).all()), f"{c.id} {route}: counts written past the last row"
        same(g["rowsum"], ref["rowsum"], f"{c.id} {route} rowsum")
        same(body, raw if route == "fused_raw" else ref["norm"], f"{c.id} {route} counts")
        same(g["out"], ref["field"], f"{c.id} {route} out")
        if route == "splat":
            same(g["raw"].reshape(H, R3), raw, f"{c.id} splat raw counts")
        n += body.size + H + R3
    if c.big:                                                        # of the other route only the counts
        same(got["splat"]["raw"].reshape(H, R3), raw, f"{c.id} splat raw counts")
    return n


# ------------------------------------------------------------------------------------------------------------------ the table
def _build_cases():
    I, F = "interior", "faces"
    cs = [
        Case("occ-r2-w3", 2, 1, 0.5, [[(I, 7), ("outside", 2)]]),
        Case("occ-r6-w7-edges", 6, 2, 2.5, [[(F, 52)], [(I, 20), ("outside", 3)]]),
        Case("occ-r8-w4", 8, 5, 1.0, [[(I, 17)], [(F, 52)], [("far", 3)], [("nonfinite", 16), (I, 5)], [("near", 48)]]),
        Case("occ-r8-w3-some", 8, 2, 0.5, [[(I, 30), (F, 26)], [(I, 9)]], select="some"),
        Case("occ-r30-w8-near", 30, 2, 3.0, [[("near", 192)], [(I, 12), (F, 26)]]),
        Case("occ-r30-w8-tol-below-3", 30, 1, float(np.nextafter(3.0, 0.0)), [[("near", 128), (I, 4)]]),
        Case("occ-r30-w8-tol-above-3", 30, 1, float(np.nextafter(3.0, 4.0)), [[("near", 128), (I, 4)]]),
        Case("occ-r30-w5-none", 30, 2, 1.5, [[("near", 96), (F, 26)], [(I, 9)]], select="none"),
        Case("occ-r30-w7", 30, 2, 2.5, [[("near", 96)], [(F, 52), ("nonfinite", 8)]]),
        Case("occ-r30-w9", 30, 2, 3.5, [[("near", 64), (F, 26)], [(I, 9)]]),
        Case("occ-r16-w16-near", 16, 2, 7.0, [[("near", 64), (F, 26)], [(I, 9)]], select="some"),
        Case("occ-r64-13-slabs", 64, 5, 3.0, [[(I, 20)], [(F, 52)], [("near", 96)], [("far", 2)], [("nonfinite", 8), (I, 3)]], select="some"),
        Case("occ-r100-p2", 100, 2, 3.0, [[(F, 26), (I, 6)], [("near", 32)]]),
        Case("occ-r102-p1-h7", 102, 7, 3.0, [[(I, 6)], [(F, 26)], [("near", 16)], [(I, 2)], [("far", 1)], [(I, 3)], [(F, 8)]], select="some"),
        Case("occ-r142-p1-h4", 142, 4, 3.0, [[(I, 4)], [(F, 8)], [("near", 8)], [("outside", 2), (I, 1)]]),
        Case("occ-hand-equal", 8, 1, None, [[("sphere:hand-equal", 36), (I, 4)]], table="hand-equal"),
        Case("occ-hand-cut", 8, 1, None, [[("sphere:hand-cut", 36), (I, 4)]], table="hand-cut"),
        # buckets of (row, slab 1) at R = 30: x = 0.92 -> planes 22 .. 29, all eight in slab 1; x = 1.47 -> plane 29 alone
        Case("occ-crowd-rounds", 30, 3, 3.0, [[("x:0.92", 64)], [("x:0.92", 64), ("x:1.47", 1)], [("x:0.92", 130)]]),
        Case("occ-crowd-hand-over", 30, 260, 3.0, [[(I, 2)]] * 63 + [[(I, 3)], [("x:0.92", 130)]] + [[(I, 2)]] * 63 + [[("x:0.92", 131)], [(I, 3)]]
             + [[(I, 2)]] * 63 + [[("x:0.92", 64)], [("x:0.92", 64), ("x:1.47", 1)]] + [[(I, 2)]] * 63 + [[(I, 3)], [(F, 5)]]),
        Case("occ-cell-255-256-5000", 30, 3, 3.0, [[("at:0.1,-0.3,0.52", 255), (I, 5)], [("at:0.1,-0.3,0.52", 256), (I, 5)], [("at:-0.41,0.2,0.77", 5000), (I, 40)]]),
        Case("occ-rowsum-above-2^24", 16, 1, 7.0, [[("at:0.07,-0.11,0.02", 12000), (I, 30)]], big=True),
    ]
    return cs


CASES = _build_cases()
BY_ID = {c.id: c for c in CASES}
NEAR_CASES = tuple(c.id for c in CASES if any(k == "near" for spec in c.rows for k, _ in spec) and pow2_window(geometry(c.id)[4]) == 8)


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def workspace_bytes(lib, c):
    d = data(c.id)
    return int(lib.coma_occupancy_fused_workspace_bytes(d["S"], c.H, c.R, d["window"]))


OUTPUT_ARGS = ("counts", "rowsum", "out", "workspace")
_T = 2.4 / 30 * 3.0
_FUSED = dict(q=PTR, S=4, H=2, R=30, centers=PTR, voxel=2.4 / 30, thres=_T, thres_sq_cut=sqrt_cut(_T), window=8, select=PTR, write_raw=0, counts=PTR,
              rowsum=PTR, out=PTR, workspace=PTR, workspace_bytes=1 << 18)
REFUSALS = {
    "coma_occupancy_fused": (_FUSED, [
        ("null pointer", dict(q=0)), ("null pointer", dict(centers=0)), ("null pointer", dict(counts=0)), ("null pointer", dict(rowsum=0)),
        ("null pointer", dict(out=0)), ("null pointer", dict(workspace=0)),
        ("bad sizes", dict(S=0)), ("bad sizes", dict(S=-1)), ("bad sizes", dict(H=0)), ("bad sizes", dict(R=0)), ("bad sizes", dict(R=256)), ("bad sizes", dict(R=31)), ("bad sizes", dict(R=-2)), ("bad sizes", dict(H=-1)),
        ("bad sizes", dict(voxel=0.0)), ("bad sizes", dict(voxel=NAN)), ("bad sizes", dict(thres=0.0)), ("bad sizes", dict(thres=NAN)),
        ("bad sizes", dict(window=1)), ("bad sizes", dict(window=17)),
        ("too large for an LDS-resident plane", dict(R=144)),
        ("workspace", dict(workspace_bytes=1024)),
        ("S=65536", dict(S=65536, workspace_bytes=1 << 40)),
        ("window=4", dict(window=4)), ("window=4", dict(window=3)), ("window=2", dict(window=2)),
        ("window=8", dict(thres=_T * 1.2, thres_sq_cut=sqrt_cut(_T * 1.2))),
        ("window=16", dict(window=16, thres=_T * 40, thres_sq_cut=sqrt_cut(_T * 40))),
        ("thres_sq_cut", dict(thres_sq_cut=float(np.nextafter(sqrt_cut(_T), 0.0)))), ("thres_sq_cut", dict(thres_sq_cut=float(np.nextafter(sqrt_cut(_T), 1.0)))),
        ("thres_sq_cut", dict(thres_sq_cut=0.0)), ("thres_sq_cut", dict(thres_sq_cut=NAN)), ("thres_sq_cut", dict(thres_sq_cut=_T)),
        ("counts must be 16-byte aligned", dict(counts=Off(4))), ("counts must be 16-byte aligned", dict(counts=Off(8))),
        ("out must be 16-byte aligned", dict(out=Off(4))), ("workspace must be 16-byte aligned", dict(workspace=Off(8))),
        ("workspace must be 16-byte aligned", dict(workspace=Off(1))),
    ]),
    "coma_occupancy_splat": (dict(q=PTR, S=4, H=2, R=30, centers=PTR, voxel=2.4 / 30, thres=_T, counts=PTR), [
        ("null pointer", dict(q=0)), ("null pointer", dict(centers=0)), ("null pointer", dict(counts=0)),
        ("bad sizes", dict(S=-1)), ("bad sizes", dict(H=0)), ("bad sizes", dict(R=0)), ("bad sizes", dict(voxel=0.0)), ("bad sizes", dict(thres=-1.0)),
        ("bad sizes", dict(thres=NAN)),
    ]),
    "coma_occupancy_reduce": (dict(counts=PTR, select=PTR, H=2, R3=27000, rowsum=PTR, out=PTR), [
        ("null pointer", dict(counts=0)), ("null pointer", dict(rowsum=0)), ("null pointer", dict(out=0)),
        ("bad sizes", dict(H=0)), ("bad sizes", dict(R3=0)), ("bad sizes", dict(R3=-4)),
        ("more than 2^31 - 1 workgroups", dict(R3=(1 << 31) * 1024)), ("more than 2^31 - 1 workgroups", dict(R3=(1 << 31) * 256 + 1)),
    ]),
}
