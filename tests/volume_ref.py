"""NumPy restatement of the column rule set of include/coma_hip.h (coma_intersection_columns, coma_mesh_volume_f64): the yardstick
the device kernels are compared with sum for sum and column for column.  Snapping, coverage and depth are the rasteriser's rules,
written with the helpers of tests/raster_ref.py; every step after the depth is int64.  Vectorised over each triangle's bounding
box and over the sweep; the loop over triangles is plain Python."""
import numpy as np

from tests import raster_ref as RR

Refused = RR.Refused
Z_LIMIT = 2 ** 40
_R = np.diag([1.0, -1.0, -1.0])


def snap(verts, x0, y0, s):
    """Integer 1/256-cell coordinates and depth of every vertex: u = (x - x0) s, v = (y - y0) s, depth = z."""
    p = np.asarray(verts, dtype=np.float64)
    with np.errstate(all="ignore"):
        cx, cy, cz = RR.camera_space(p, _R, (x0, y0, 0.0))
        su = np.floor((cx * s + 0.0) * 256.0 + 0.5)
        sv = np.floor((cy * s + 0.0) * 256.0 + 0.5)
    if not (np.isfinite(p).all() and np.isfinite(cz).all()):
        raise Refused("non-finite vertex")
    if not ((np.abs(su) <= RR.SNAP_LIMIT).all() and (np.abs(sv) <= RR.SNAP_LIMIT).all()):
        raise Refused("a snapped coordinate exceeds +-2^25")
    return su.astype(np.int64), sv.astype(np.int64), cz


def crossings(verts, faces, x0, y0, s, W, H):
    """(column index i64 [n], Z i64 [n], sigma i64 [n]) of one mesh, in no particular order."""
    X, Y, Zd = snap(verts, x0, y0, s)
    faces = np.asarray(faces, dtype=np.int64)
    if faces.size and (faces.min() < 0 or faces.max() >= len(X)):
        raise Refused("face index outside [0, V)")
    X, Y = X.tolist(), Y.tolist()
    cols, zs, sg = [], [], []
    for ia, ib, ic in faces.tolist():
        ax, ay, bx, by, cx, cy = X[ia], Y[ia], X[ib], Y[ib], X[ic], Y[ic]
        za, zb, zc = Zd[ia], Zd[ib], Zd[ic]
        area = RR.edge(ax, ay, bx, by, cx, cy)
        if area == 0:
            continue
        sigma = 1 if area > 0 else -1
        if area < 0:
            bx, by, zb, cx, cy, zc, area = cx, cy, zc, bx, by, zb, -area
        i0, i1 = max(0, (min(ax, bx, cx) + 127) >> 8), min(W - 1, (max(ax, bx, cx) - 128) >> 8)
        j0, j1 = max(0, (min(ay, by, cy) + 127) >> 8), min(H - 1, (max(ay, by, cy) - 128) >> 8)
        if i0 > i1 or j0 > j1:
            continue
        px = (256 * np.arange(i0, i1 + 1, dtype=np.int64) + 128)[None, :]
        py = (256 * np.arange(j0, j1 + 1, dtype=np.int64) + 128)[:, None]
        e0, e1, e2 = RR.edge(bx, by, cx, cy, px, py), RR.edge(cx, cy, ax, ay, px, py), RR.edge(ax, ay, bx, by, px, py)
        t0, t1, t2 = RR.owns_ties(bx, by, cx, cy), RR.owns_ties(cx, cy, ax, ay), RR.owns_ties(ax, ay, bx, by)
        inside = ((e0 > 0) | ((e0 == 0) & t0)) & ((e1 > 0) | ((e1 == 0) & t1)) & ((e2 > 0) | ((e2 == 0) & t2))
        if not inside.any():
            continue
        jj, ii = np.nonzero(inside)
        with np.errstate(all="ignore"):
            z = ((e0[jj, ii].astype(np.float64) * za + e1[jj, ii].astype(np.float64) * zb) + e2[jj, ii].astype(np.float64) * zc) / float(area)
            q = np.floor((z * s) * 256.0 + 0.5)
        if not (np.abs(q) <= float(Z_LIMIT)).all():            # NaN and infinities fail the comparison too
            raise Refused("a crossing's depth is non-finite or beyond +-2^40")
        cols.append((jj + j0) * W + (ii + i0)), zs.append(q.astype(np.int64)), sg.append(np.full(len(jj), sigma, dtype=np.int64))
    if not cols:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(cols), np.concatenate(zs), np.concatenate(sg)


def sweep(ca, cb, W, H):
    """(sums i64 [3] = L_AB, L_A, L_B; col_ab i64 [H,W]; crossings per column i64 [H,W]) from the crossings of A and of B."""
    col = np.concatenate([ca[0], cb[0]])
    Z = np.concatenate([ca[1], cb[1]])
    sa = np.concatenate([ca[2], np.zeros(len(cb[0]), np.int64)])
    sb = np.concatenate([np.zeros(len(ca[0]), np.int64), cb[2]])
    order = np.lexsort((Z, col))
    col, Z, sa, sb = col[order], Z[order], sa[order], sb[order]
    counts = np.bincount(col, minlength=W * H).astype(np.int64)
    if len(col) == 0:
        return np.zeros(3, np.int64), np.zeros((H, W), np.int64), counts.reshape(H, W)
    first = np.concatenate([[True], col[1:] != col[:-1]])
    start = np.maximum.accumulate(np.where(first, np.arange(len(col)), 0))

    def winding(sig):                                           # n after event k, counted from the start of its column
        c = np.cumsum(sig)
        return -(c - (c - sig)[start])
    na, nb = winding(sa), winding(sb)
    same = ~first[1:]                                           # event k and k + 1 lie in one column
    length = np.where(same, Z[1:] - Z[:-1], 0)
    in_a, in_b = na[:-1] != 0, nb[:-1] != 0
    sums = np.array([length[in_a & in_b].sum(), length[in_a].sum(), length[in_b].sum()], dtype=np.int64)
    col_ab = np.zeros(W * H, np.int64)
    np.add.at(col_ab, col[:-1][in_a & in_b], length[in_a & in_b])
    return sums, col_ab.reshape(H, W), counts.reshape(H, W)


def intersection_columns(vertsA, facesA, vertsB, facesB, x0, y0, s, W, H):
    """(sums, col_ab, crossings per column) of coma_intersection_columns."""
    return sweep(crossings(vertsA, facesA, x0, y0, s, W, H), crossings(vertsB, facesB, x0, y0, s, W, H), W, H)


def volumes(sums, s):
    """(V_AB, V_A, V_B) in world units: L / (256 s^3)."""
    return tuple(float(v) / (256.0 * s * s * s) for v in sums)


def mesh_volume(verts, faces):
    """Signed volume, sum of det[a b c] / 6 in the header's order of operations; also the sum of |det| / 6 for error bounds."""
    v, f = np.asarray(verts, dtype=np.float64), np.asarray(faces, dtype=np.int64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    det = (a[:, 0] * (b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1]) - a[:, 1] * (b[:, 0] * c[:, 2] - b[:, 2] * c[:, 0])) + a[:, 2] * (b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0])
    return float(det.sum() / 6.0), float(np.abs(det).sum() / 6.0)
