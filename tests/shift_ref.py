"""NumPy restatement of the depth-optimisation rule set of include/coma_hip.h (coma_shift_columns_prepare, coma_shift_profile,
coma_depth_optimize_f64), built on tests/volume_ref.py: the shift profile is the column sweep with Delta added to every crossing of
mesh A; the multiview term and Adam are written operation for operation, with the device's summation shapes, so the trajectory can be
compared bit for bit."""
import numpy as np

from tests import volume_ref as VR

SHIFT_LIMIT = 2 ** 42
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8


def camera_frame(verts, R):
    """p' = p R in f64: the camera's front vector R[:, 2] becomes +z."""
    return np.asarray(verts, dtype=np.float64) @ np.asarray(R, dtype=np.float64)


def shift_of(d, s):
    """Delta of a displacement d: floor((d s) 256 + 0.5), clamped to +-2^42; a NaN counts as beyond the clamp."""
    with np.errstate(all="ignore"):
        q = np.floor((np.float64(d) * np.float64(s)) * 256.0 + 0.5)
    if not abs(q) <= float(SHIFT_LIMIT):
        return -SHIFT_LIMIT if q < 0.0 else SHIFT_LIMIT
    return int(q)


class Columns:
    """The crossings of A (the human) and of B on one grid, and the two lengths that do not depend on the shift."""

    def __init__(self, vertsA, facesA, vertsB, facesB, x0, y0, s, W, H):
        self.s, self.W, self.H = float(s), W, H
        self.ca = VR.crossings(vertsA, facesA, x0, y0, s, W, H)
        self.cb = VR.crossings(vertsB, facesB, x0, y0, s, W, H)
        _, _, counts = VR.sweep(self.ca, self.cb, W, H)
        # "the sweep's, for one mesh at a time": each mesh walked alone.  For a closed mesh these are sums[1] and sums[2] of the joint
        # sweep; an OPEN mesh is still inside after its last crossing, and the joint sweep counts that up to the other mesh's next one.
        none = (np.zeros(0, np.int64),) * 3
        self.L_A, self.L_B = int(VR.sweep(self.ca, none, W, H)[0][1]), int(VR.sweep(none, self.cb, W, H)[0][2])
        self.counts = counts
        self._lab = {}

    def L_AB(self, delta):
        if delta not in self._lab:                  # one sweep per distinct shift: neighbouring shifts share two of their three
            self._lab[delta] = int(VR.sweep((self.ca[0], self.ca[1] + np.int64(delta), self.ca[2]), self.cb, self.W, self.H)[0][0])
        return self._lab[delta]

    def profile(self, d):
        """i64 [K,3]: L_AB at Delta - 1, Delta, Delta + 1 for every displacement of d."""
        out = np.zeros((len(d), 3), np.int64)
        for k, dk in enumerate(d):
            delta = shift_of(dk, self.s)
            out[k] = [self.L_AB(delta - 1), self.L_AB(delta), self.L_AB(delta + 1)]
        return out


def _tree_256(per_view):
    """The device's sum over the views: partial t adds the views t, t + 256, ... in ascending order, then lds[t] + lds[t + h]."""
    part = np.zeros(256, np.float64)
    for base in range(0, len(per_view), 256):
        chunk = per_view[base:base + 256]
        part[:len(chunk)] = part[:len(chunk)] + chunk
    h = 128
    while h > 0:
        part[:h] = part[:h] + part[h:2 * h]
        h //= 2
    return part[0]


def multiview(d, views, joints0, front, cand_view, cand_xy):
    """(loss, d loss / dd) of the multiview joint term at displacement d; views [n_views,28] in the view_record layout."""
    N, J = cand_xy.shape[0], joints0.shape[0]
    if N == 0:
        return 0.0, 0.0
    d = np.float64(d)
    f0, f1, f2 = (np.float64(x) for x in front)
    w = views[np.asarray(cand_view)]
    mr, tmr, scale, maxres, hx, hy = w[:, 12:21], w[:, 21:24], w[:, 24], w[:, 25], w[:, 26], w[:, 27]
    ax = ((f0 * mr[:, 0] + f1 * mr[:, 3]) + f2 * mr[:, 6]) / scale * maxres
    ay = ((f0 * mr[:, 1] + f1 * mr[:, 4]) + f2 * mr[:, 7]) / scale * maxres
    ox, oy, oz = d * f0, d * f1, d * f2
    sq, gr = np.zeros(N), np.zeros(N)
    for j in range(J):
        x, y, z = joints0[j, 0] + ox, joints0[j, 1] + oy, joints0[j, 2] + oz
        cx = ((x * mr[:, 0] + y * mr[:, 3]) + z * mr[:, 6]) - tmr[:, 0]
        cy = ((x * mr[:, 1] + y * mr[:, 4]) + z * mr[:, 7]) - tmr[:, 1]
        rx = (cx / scale * maxres + hx) - cand_xy[:, j, 0]
        ry = (cy / scale * maxres + hy) - cand_xy[:, j, 1]
        sq = sq + (rx * rx + ry * ry)
        gr = gr + (rx * ax + ry * ay)
    return float(_tree_256(0.5 * sq) / np.float64(N)), float(_tree_256(gr) / np.float64(N))


def optimize(columns, views, joints0, front, cand_view, cand_xy, d0, lr, w_multiview, w_collision, E):
    """dict(d, traj f64 [E+1], Ltraj i64 [E,3], losses f64 [E,2]) of coma_depth_optimize_f64.  columns: a Columns, or None."""
    views, joints0, cand_xy = (np.asarray(a, dtype=np.float64) for a in (views, joints0, cand_xy))
    lr, w_mv, w_col = np.float64(lr), np.float64(w_multiview), np.float64(w_collision)
    collide = columns is not None and w_collision != 0.0
    traj, Ltraj, losses = np.zeros(E + 1), np.zeros((E, 3), np.int64), np.zeros((E, 2))
    d, m, v, p1, p2 = np.float64(d0), np.float64(0.0), np.float64(0.0), np.float64(1.0), np.float64(1.0)
    b1, b2 = np.float64(BETA1), np.float64(BETA2)
    traj[0] = d
    cv = np.asarray(cand_view, dtype=np.int64).reshape(-1)
    if len(cv) and (cv.min() < 0 or cv.max() >= len(views)):
        # the cand_view contract: the entry is not followed; epoch 0 stops with status 3 before it writes losses[0] or traj[1], the
        # Adam state stays at its start.  The profile at traj[0] ran before the step: Ltraj[0] holds it when the collision term is on.
        if collide:
            Ltraj[0] = columns.profile([d])[0]
        return dict(d=float(d), traj=traj[:1], Ltraj=Ltraj[:1], losses=losses[:0], status=3, epoch=0)
    with np.errstate(all="ignore"):
        for e in range(E):
            loss, g_mv = multiview(d, views, joints0, front, cand_view, cand_xy)
            ratio, slope = np.float64(0.0), np.float64(0.0)
            if collide:
                Ltraj[e] = columns.profile([d])[0]
                if columns.L_A != 0:
                    la = np.float64(columns.L_A)
                    ratio = np.float64(int(Ltraj[e, 1])) / la
                    slope = (np.float64(int(Ltraj[e, 2] - Ltraj[e, 0])) * (np.float64(256.0) * np.float64(columns.s))) / (np.float64(2.0) * la)
            losses[e] = [loss, ratio]
            g = w_mv * np.float64(g_mv) + w_col * slope
            m = b1 * m + (np.float64(1.0) - b1) * g
            v = b2 * v + (np.float64(1.0) - b2) * g * g
            p1, p2 = p1 * b1, p2 * b2
            d = d - (lr / (np.float64(1.0) - p1)) * m / (np.sqrt(v) / np.sqrt(np.float64(1.0) - p2) + np.float64(EPS))
            traj[e + 1] = d
            if not np.isfinite(d):
                traj, Ltraj, losses = traj[:e + 2], Ltraj[:e + 1], losses[:e + 1]
                break
    return dict(d=float(traj[-1]), traj=traj, Ltraj=Ltraj, losses=losses)


def breakpoint_shifts(cols):
    """EVERY shift at which a face of A meets a face of B (the breakpoints of the profile: all differences of a Z of B and a Z of
    A), each with its two neighbours; 0 and +-1; and one far outside the overlap."""
    diffs = np.unique(np.subtract.outer(np.unique(cols.cb[1]), np.unique(cols.ca[1])))
    near = sorted({int(d) + k for d in diffs for k in (-1, 0, 1)} | {-1, 0, 1})
    return near, int(diffs.max()) + 4096


def box_pair_closed_form(a_lo, a_hi, b_lo, b_hi, delta):
    """L_AB(Delta) of two axis-aligned boxes given in grid units (xy in whole cells, z in 1/256-cell units): the number of shared
    columns times the overlap of the two z intervals after the shift."""
    cols = max(0, min(a_hi[0], b_hi[0]) - max(a_lo[0], b_lo[0])) * max(0, min(a_hi[1], b_hi[1]) - max(a_lo[1], b_lo[1]))
    return cols * max(0, min(a_hi[2] + delta, b_hi[2]) - max(a_lo[2] + delta, b_lo[2]))
