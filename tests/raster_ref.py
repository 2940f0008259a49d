"""NumPy restatement of the rasteriser rule set of include/coma_hip.h (coma_raster_depth_f64, coma_silhouette_iou): the yardstick
the device kernels are compared with key for key.  Every f64 step is one elementwise NumPy operation in the order the header
states (explicit products and sums, never `@` or np.dot: a BLAS may fuse a multiply-add), every coverage step is int64.
Vectorised over each triangle's bounding box; the loop over triangles is plain Python."""
import numpy as np

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
SNAP_LIMIT = 2.0 ** 25
_SIGN = np.uint64(1 << 63)


class Refused(ValueError):
    """The call the device refuses with COMA_E_INVALID."""


def depth_to_key(z):
    b = np.ascontiguousarray(z, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63) != 0, ~b, b | _SIGN)


def key_to_depth(k):
    k = np.ascontiguousarray(k, dtype=np.uint64)
    return np.where(k >> np.uint64(63) != 0, k & ~_SIGN, ~k).view(np.float64)


def camera_space(verts, R, t):
    """c = diag(1,-1,-1) R^T (p - t), columns written out."""
    p = np.asarray(verts, dtype=np.float64)
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    t = np.asarray(t, dtype=np.float64).reshape(3)
    d0, d1, d2 = p[:, 0] - t[0], p[:, 1] - t[1], p[:, 2] - t[2]
    cx = (R[0, 0] * d0 + R[1, 0] * d1) + R[2, 0] * d2
    cy = -((R[0, 1] * d0 + R[1, 1] * d1) + R[2, 1] * d2)
    cz = -((R[0, 2] * d0 + R[1, 2] * d1) + R[2, 2] * d2)
    return cx, cy, cz


def snap(verts, R, t, scale, W, H):
    """Integer 1/256-pixel coordinates and depth of every vertex; raises Refused where the device refuses."""
    p = np.asarray(verts, dtype=np.float64)
    with np.errstate(all="ignore"):
        cx, cy, cz = camera_space(p, R, t)
        s = float(max(W, H)) / float(scale)
        su = np.floor((cx * s + W * 0.5) * 256.0 + 0.5)
        sv = np.floor((cy * s + H * 0.5) * 256.0 + 0.5)
    if not (np.isfinite(p).all() and np.isfinite(cz).all()):
        raise Refused("non-finite vertex")
    if not ((np.abs(su) <= SNAP_LIMIT).all() and (np.abs(sv) <= SNAP_LIMIT).all()):
        raise Refused("a snapped coordinate exceeds +-2^25")
    return su.astype(np.int64), sv.astype(np.int64), cz


def edge(Px, Py, Qx, Qy, x, y):
    return (Qx - Px) * (y - Py) - (Qy - Py) * (x - Px)


def owns_ties(Px, Py, Qx, Qy):
    dx, dy = Qx - Px, Qy - Py
    return dy < 0 or (dy == 0 and dx > 0)


def raster_depth(verts, faces, R, t, scale, W, H):
    """u64 [H,W] nearest-depth key map of one mesh."""
    X, Y, Z = snap(verts, R, t, scale, W, H)
    faces = np.asarray(faces, dtype=np.int64)
    if faces.size and (faces.min() < 0 or faces.max() >= len(X)):
        raise Refused("face index outside [0, V)")
    X, Y = X.tolist(), Y.tolist()          # Python integers: exact
    key = np.full((H, W), EMPTY, dtype=np.uint64)
    for ia, ib, ic in faces.tolist():
        ax, ay, bx, by, cx, cy = X[ia], Y[ia], X[ib], Y[ib], X[ic], Y[ic]
        za, zb, zc = Z[ia], Z[ib], Z[ic]
        area = edge(ax, ay, bx, by, cx, cy)
        if area == 0:
            continue
        if area < 0:
            bx, by, zb, cx, cy, zc, area = cx, cy, zc, bx, by, zb, -area
        x0, x1 = max(0, (min(ax, bx, cx) + 127) >> 8), min(W - 1, (max(ax, bx, cx) - 128) >> 8)
        y0, y1 = max(0, (min(ay, by, cy) + 127) >> 8), min(H - 1, (max(ay, by, cy) - 128) >> 8)
        if x0 > x1 or y0 > y1:
            continue
        px = (256 * np.arange(x0, x1 + 1, dtype=np.int64) + 128)[None, :]
        py = (256 * np.arange(y0, y1 + 1, dtype=np.int64) + 128)[:, None]
        e0, e1, e2 = edge(bx, by, cx, cy, px, py), edge(cx, cy, ax, ay, px, py), edge(ax, ay, bx, by, px, py)
        t0, t1, t2 = owns_ties(bx, by, cx, cy), owns_ties(cx, cy, ax, ay), owns_ties(ax, ay, bx, by)
        inside = ((e0 > 0) | ((e0 == 0) & t0)) & ((e1 > 0) | ((e1 == 0) & t1)) & ((e2 > 0) | ((e2 == 0) & t2))
        if not inside.any():
            continue
        with np.errstate(all="ignore"):
            z = ((e0.astype(np.float64) * za + e1.astype(np.float64) * zb) + e2.astype(np.float64) * zc) / float(area)
        k = np.where(inside & (z == z), depth_to_key(z), EMPTY)
        sub = key[y0:y1 + 1, x0:x1 + 1]
        np.minimum(sub, k, out=sub)
    return key


def silhouette_iou(human_key, asset_key, offsets, gt, want_masks=True):
    """(visible, inter, uni) i64 [K] and masks u8 [K,H,W] (or None) of coma_silhouette_iou."""
    human = human_key != EMPTY
    zh = key_to_depth(human_key)
    if asset_key is None:
        bare, za = np.ones_like(human), np.zeros_like(zh)
    else:
        bare, za = asset_key == EMPTY, key_to_depth(asset_key)
    g = np.asarray(gt) != 0
    vis, inter, uni, masks = [], [], [], []
    with np.errstate(all="ignore"):
        for off in np.asarray(offsets, dtype=np.float64).tolist():
            v = human & (bare | (zh + off < za))
            vis.append(int(v.sum())), inter.append(int((v & g).sum())), uni.append(int((v | g).sum()))
            masks.append(np.where(v, 255, 0).astype(np.uint8))
    out = [np.array(a, dtype=np.int64) for a in (vis, inter, uni)]
    return out[0], out[1], out[2], (np.stack(masks) if want_masks else None)


def segmap(meshes, R, t, scale, W, H):
    """Instance map of several meshes (1-based index of the front-most mesh, 0 = background); on an exact depth tie the EARLIER
    mesh wins, so with the asset listed first this is the strict test of coma_silhouette_iou."""
    best = np.full((H, W), EMPTY, dtype=np.uint64)
    seg = np.zeros((H, W), dtype=np.uint8)
    for i, (v, f) in enumerate(meshes):
        k = raster_depth(v, f, R, t, scale, W, H)
        with np.errstate(all="ignore"):
            front = (k != EMPTY) & ((best == EMPTY) | (key_to_depth(k) < key_to_depth(best)))
        seg[front] = i + 1
        best = np.where(front, k, best)
    return seg


# ---- meshes ----
def icosphere(subdivisions, radius=1.0, center=(0.0, 0.0, 0.0)):
    """Subdivided icosahedron: 20 * 4^n faces (n = 5: 20 480, the size of SMPL-X)."""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v) * radius + np.asarray(center, dtype=np.float64), np.array(f, dtype=np.int32)


def box(lo, hi):
    """12-face axis-aligned box."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    v = np.array([[(hi if (i >> k) & 1 else lo)[k] for k in range(3)] for i in range(8)])
    f = np.array([(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4), (1, 5, 7), (1, 7, 3)],
                 dtype=np.int32)
    return v, f


def look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)):
    """Camera-to-world rotation whose columns are the camera's axes (Blender / OpenGL: the camera looks down -z)."""
    eye, target = np.asarray(eye, dtype=np.float64), np.asarray(target, dtype=np.float64)
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right)
    return np.stack([right, np.cross(right, fwd), -fwd], axis=1)
