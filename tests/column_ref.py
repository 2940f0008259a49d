"""The rasteriser, column and shift-profile kernels of coma_amd/csrc/raster.hip, mesh_volume.hip and depth_opt.hip over the domain their
entry points accept.  CPU only: the table of launches (CASES, by kind: raster, iou, volume, columns, optimize), the operands (data, from
a crc32 seed), the references (reference: tests/raster_ref.py, tests/volume_ref.py, tests/shift_ref.py -- the three restatements --
and mesh_volume_shape, the fixed summation shape of coma_mesh_volume_f64), an emulation of the kernels' own decisions (emulate: lane or
work list, list slot -> slice and trip, hits per tile and step, scan chunk, grid strides, packed crossings) in which a defect can be
planted (MUTATIONS), the regimes a case reaches counted from its own data (branches), the assertions the device is held to (check),
the data refusals the device takes (DEVICE_REFUSALS) and every argument check (REFUSALS).  tests/test_coma_column_domain_gpu.py launches
the tables; tests/test_column_ref_host.py checks the tables themselves.

The bound: none.  Keys, counts, masks, sums, per-column maps, lengths, profiles and whole Adam trajectories are compared bit for bit;
the volume is compared bit for bit with mesh_volume_shape, and mesh_volume_shape is held on the CPU to the header's own bound against
math.fsum.  A list length is compared too (the work list's length in the workspace header): it is the one place where the kSmallMax
boundary shows, since a triangle gives the same samples on either path."""
import functools
import math

import numpy as np

from tests import domain_kit as kit
from tests import raster_ref as RR
from tests import shift_ref as SR
from tests import volume_ref as VR
from tests.domain_kit import PTR, Off

f64, i32, i64, u8, u64 = np.float64, np.int32, np.int64, np.uint8, np.uint64
NAN, INF = float("nan"), float("inf")
EMPTY = RR.EMPTY
SMALL_MAX, SORT_MAX, TILE, SCAN_BLOCK = 256, 16, 16, 1024           # kSmallMax, kSortMax, kTile, kScanBlock
IOU_BLOCKS, PROFILE_BLOCKS, VOLUME_BLOCKS = 1024, 1024, 256         # fixed grids of iou_count, shift_profile, volume_partial
SNAP, ZLIM, SHIFT = 2 ** 25, 2 ** 40, 2 ** 42
IDENT = (np.eye(3), np.zeros(3))


class Case:
    def __init__(self, id, kind, **kw):
        self.id, self.kind = id, kind
        self.__dict__.update(kw)

    def __repr__(self):
        return self.id


def grid_slices(W, H):
    """(tiles, slices) of the work-list kernels' grid"""
    tiles = -(-W // TILE) * -(-H // TILE)
    return tiles, (1 if tiles >= 2048 else min(32, 2048 // tiles))


# ------------------------------------------------------------------------------------------------------------------ meshes in snapped units
def raster_world(U, V, depth, W, H):
    """vertices that the identity camera with scale = max(W, H) snaps to (U, V) (1/256 pixel; .5 allowed: a half-way snap) at `depth`"""
    U, V, depth = (np.asarray(a, f64) for a in (U, V, depth))
    return np.stack([U / 256.0 - W * 0.5, -(V / 256.0 - H * 0.5), -depth], 1)


def column_world(U, V, Z):
    """vertices that the grid x0 = y0 = 0, s = 1 snaps to (U, V) with crossings at Z (1/256 cell)"""
    U, V, Z = (np.asarray(a, f64) for a in (U, V, Z))
    return np.stack([U / 256.0, V / 256.0, Z / 256.0], 1)


class Soup:
    """triangles in snapped units, three vertices of its own each"""

    def __init__(self):
        self.p, self.f = [], []

    def tri(self, pts, z, flip=False):
        n = len(self.p)
        z = [z] * 3 if np.isscalar(z) else list(z)
        self.p += [(pts[k][0], pts[k][1], z[k]) for k in range(3)]
        self.f.append((n, n + 2, n + 1) if flip else (n, n + 1, n + 2))

    def box_tri(self, rng, i0, j0, w, h, z, flip=False):
        """a right triangle whose clipped box holds exactly w x h pixel centres from (i0, j0): corners within 100/256 outside the
        outermost centres"""
        a, b, c, d = (int(v) for v in rng.integers(0, 101, 4))
        xl, xr, yt, yb = 256 * i0 + 128 - a, 256 * (i0 + w - 1) + 128 + b, 256 * j0 + 128 - c, 256 * (j0 + h - 1) + 128 + d
        self.tri([(xl, yt), (xr, yt), (xl, yb)], z, flip)

    def sheet(self, i0, i1, j0, j1, Z, up):
        """the cells [i0, i1) x [j0, j1) at height Z: two triangles whose shared edge runs through pixel centres when the sheet is square"""
        P = [(256 * i0, 256 * j0), (256 * i1, 256 * j0), (256 * i1, 256 * j1), (256 * i0, 256 * j1)]
        self.tri([P[0], P[1], P[2]], Z, flip=not up)
        self.tri([P[0], P[2], P[3]], Z, flip=not up)

    def stack(self, i0, i1, j0, j1, Zs, inward=False):
        for k, Z in enumerate(Zs):
            self.sheet(i0, i1, j0, j1, Z, up=(k % 2 == 1) != inward)

    def arrays(self):
        p = np.array(self.p, f64).reshape(-1, 3)
        return p[:, 0], p[:, 1], p[:, 2], np.array(self.f, i32).reshape(-1, 3)


def _pool_soup(rng, W, H, nV, nF):
    """nF faces over a pool of nV vertices scattered up to two pixels outside the screen, depths in quarters"""
    U, V = rng.integers(-512, W * 256 + 513, nV), rng.integers(-512, H * 256 + 513, nV)
    depth = rng.integers(-40, 41, nV) / 4.0
    return raster_world(U, V, depth, W, H), rng.integers(0, nV, (nF, 3)).astype(i32)


# ------------------------------------------------------------------------------------------------------------------ raster data
def _raster(rng, c):
    W, H, s = c.W, c.H, Soup()
    R, t, scale = IDENT[0], IDENT[1], float(max(W, H))
    if c.mesh == "one":
        s.tri([(0, 0), (512, 0), (0, 512)], [1.0, 2.0, 3.0])
    elif c.mesh == "pool":
        v, f = _pool_soup(rng, W, H, c.V, c.F)
        return dict(verts=v, faces=f, R=R, t=t, scale=c.scale or scale)
    elif c.mesh == "boxes":                                       # both sides of kSmallMax, both windings, off-screen and zero-area faces
        for k in range(c.n):
            w, h = c.boxes[k % len(c.boxes)]
            s.box_tri(rng, int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h, float(rng.integers(-40, 41)) / 4.0, flip=k % 2 == 1)
        s.tri([(-4000, 0), (-3000, 0), (-3500, 700)], 1.0)
        s.tri([(0, 0), (256, 256), (512, 512)], 1.0)
    elif c.mesh == "crowd":                                       # `crowd` large triangles that all cover pixel (6, 6) of tile 0, the nearest LAST; then scattered ones
        for k in range(c.crowd):
            s.box_tri(rng, int(rng.integers(0, 4)), int(rng.integers(0, 3)), 17, 16, 1000.0 - k, flip=k % 2 == 1)
        for k in range(c.scattered):
            s.box_tri(rng, int(rng.integers(20, W - 17)), int(rng.integers(0, H - 16 + 1)), 17, 16, float(rng.integers(-400, 401)) / 4.0, flip=k % 2 == 1)
        for k in range(30):
            s.box_tri(rng, int(rng.integers(0, W - 5)), int(rng.integers(0, H - 5)), 5, 5, float(rng.integers(-400, 401)) / 4.0)
    elif c.mesh == "cover":                                       # corners at exactly +-2^25, one winding each
        P = [(-SNAP, -SNAP), (SNAP, -SNAP), (0, SNAP)]
        s.tri(P, [1.0, 2.0, 3.0])
        s.tri(P, [3.0, 2.0, 1.0], flip=True)
    elif c.mesh == "edges":
        c0 = 128
        s.tri([(c0, c0), (c0 + 1024, c0), (c0, c0 + 1024)], 2.0)                        # corners on pixel centres
        s.tri([(c0 + 1024, c0), (c0 + 1024, c0 + 1024), (c0, c0 + 1024)], 3.0)          # shares the edge through the centres of its diagonal
        s.tri([(0, 0), (300, 300), (900, 900)], 1.0)                                    # zero area
        s.tri([(700, 700), (700, 700), (900, 100)], 1.0)
        s.tri([(-3000, 100), (-2000, 100), (-2500, 900)], 1.0)                          # off the screen
        s.tri([(10, 10), (100, 10), (10, 100)], 1.0)                                    # no centre inside its box
        s.tri([(1500.5, 300.5), (2900.5, 310.5), (1510.5, 1700.5)], -7.25)              # half-way snaps, positive
        s.tri([(-300.5, 2000.5), (900.5, 2100.5), (-200.5, 3300.5)], [-1.0, -2.5, -4.0], flip=True)   # and negative; negative depths
        s.tri([(1400, 2000), (2600, 2000), (1400, 3200)], 0.0)                          # +0.0 against -0.0 at the same pixels
        s.tri([(1400, 2000), (2600, 2000), (1400, 3200)], -0.0, flip=True)
        s.tri([(2700, 2000), (3900, 2000), (2700, 3200)], 2.5)                          # equal depths from two faces
        s.tri([(2650, 1900), (3900, 1950), (2700, 3300)], 2.5)
        s.tri([(3000, 100), (3900, 100), (3000, 1000)], 1e305)                          # e z overflows: +inf, drawn
        s.tri([(3000, 1100), (3900, 1100), (3000, 1900)], [1e305, -1e305, 1e305])       # inf - inf: NaN, not drawn
    elif c.mesh == "sphere":
        v, f = RR.icosphere(2, 0.8)
        eye = np.array([1.5, -2.0, 1.1])
        return dict(verts=v, faces=f, R=RR.look_at(eye), t=eye, scale=2.4)
    U, V, Z, f = s.arrays()
    return dict(verts=raster_world(U, V, Z, W, H), faces=f, R=R, t=t, scale=c.scale or scale)


# ------------------------------------------------------------------------------------------------------------------ iou data
OFFSET_POOL = [0.0, 1.0, -1.0, 0.5, INF, -INF, NAN, 3.0, -2.0, 1e300]


def _iou(rng, c):
    N = c.W * c.H
    def keys(p_empty):
        z = rng.integers(-4, 5, N).astype(f64)
        z[rng.random(N) < 0.1] = -0.0
        return np.where(rng.random(N) < p_empty, EMPTY, RR.depth_to_key(z))
    human, asset = keys(0.3), (keys(0.4) if c.asset else None)
    if N >= 128:
        human[64:128] = EMPTY                                     # a wave without a human pixel
    gt = rng.choice(np.array([0, 1, 255], u8), N)
    off = np.array([OFFSET_POOL[k % len(OFFSET_POOL)] if k < len(OFFSET_POOL) else float(rng.integers(-5, 6)) for k in range(c.K)], f64)
    return dict(human=human.reshape(c.H, c.W), asset=None if asset is None else asset.reshape(c.H, c.W), offsets=off, gt=gt.reshape(c.H, c.W))


# ------------------------------------------------------------------------------------------------------------------ volume data
def _volume(rng, c):
    if c.mesh in ("cube", "cube-inward"):
        v, f = RR.box((-0.5, 0.25, 1.0), (1.5, 0.75, 5.0))          # 2 x 0.5 x 4
        return dict(verts=v, faces=f if c.mesh == "cube-inward" else np.ascontiguousarray(f[:, ::-1]))      # RR.box winds inwards for this sum
    V = c.V
    verts = rng.normal(size=(V, 3))
    faces = rng.integers(0, V, (c.F, 3)).astype(i32) if c.F > 1 else np.array([[0, 1, 2]], i32)
    for at, value in c.bad:
        faces[at, int(rng.integers(0, 3))] = V if value == "V" else -1
    return dict(verts=verts, faces=faces)


def mesh_volume_shape(verts, faces):
    """coma_mesh_volume_f64 in its own summation shape, f64: thread t of block b adds its faces b 256 + t, + gridDim 256, ... in
    ascending order from +0.0 (a face index outside [0, V) makes the thread's sum NaN); lds[t] + lds[t + h] for h = 128 ... 1; a second
    such tree over the partials padded with +0.0; one division by 6."""
    return _volume_shape(verts, faces, None)


def _tree(a):
    a = a.copy()
    h = a.shape[-1] // 2
    while h:
        a[..., :h] = a[..., :h] + a[..., h:2 * h]
        h //= 2
    return a[..., 0]


def _volume_shape(verts, faces, mut):
    v, f = np.asarray(verts, f64), np.asarray(faces, i64)
    F, V = len(f), len(v)
    ok = ((f >= 0) & (f < V)).all(1)
    g = np.where(ok[:, None], f, 0)
    a, b, c = v[g[:, 0]], v[g[:, 1]], v[g[:, 2]]
    with np.errstate(all="ignore"):
        det = (a[:, 0] * (b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1]) - a[:, 1] * (b[:, 0] * c[:, 2] - b[:, 2] * c[:, 0])) + a[:, 2] * (b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0])
        nb = min(-(-F // 256), VOLUME_BLOCKS)
        acc = np.zeros(nb * 256)
        for base in range(0, F, nb * 256):
            n = min(nb * 256, F - base)
            acc[:n] = np.where(ok[base:base + n], acc[:n] + det[base:base + n], NAN)
            if mut == "volume-stride-dropped":
                break
        partial = np.zeros(256)
        partial[:nb] = _tree(acc.reshape(nb, 256))
        if mut == "volume-pad-wrong":
            partial[nb:] = partial[0]
        return float(_tree(partial) / 6.0), det, ok


# ------------------------------------------------------------------------------------------------------------------ column data
def _lattice(n, base, step=1000):
    return [base + step * k for k in range(n)]


def _stacks(A, B, x, y0, y1, yb0, inward):
    """the stacks of the small grids, four cells wide each from x: columns of exactly 1, 2, 16, 17 and 82 crossings, B alone,
    coincident faces, negative Z and +-2^40.  B's sheets start at row yb0."""
    st = lambda s, k, Zs, j0: s.stack(x + 4 * k, x + 4 * k + 4, j0, y1, Zs, inward=inward and s is A)
    st(A, 0, [1003], y0)
    st(A, 1, [-2997, 1003], y0)
    st(A, 2, _lattice(8, 3), y0), st(B, 2, _lattice(8, 503), yb0)
    st(A, 3, _lattice(9, 3), y0), st(B, 3, _lattice(8, 503), yb0)
    st(A, 4, _lattice(41, 3), y0), st(B, 4, _lattice(41, 503), yb0)
    st(B, 5, [503, 4503], yb0)
    st(A, 6, [2003, 2003, 8003, 12003], y0), st(B, 6, [2003, 8003, 8003, 15503], yb0)     # equal Z within a mesh and across the meshes
    st(A, 7, [-ZLIM, -4997], y0), st(B, 7, [-1497, ZLIM], yb0)


def _columns(rng, c):
    W, H, A, B = c.W, c.H, Soup(), Soup()
    m = c.mesh
    if m == "one":
        A.stack(0, 1, 0, 1, [-300, 500]), B.stack(0, 1, 0, 1, [-700, 100])
    elif m == "stacks":
        _stacks(A, B, 0, 0, H, c.yb0, c.inward)
        if W > 32:
            A.stack(32, W, 0, H, [10, 20])
    elif m == "box":
        A.stack(10, 22, 10, 22, [200, 2000]), B.stack(4, 28, 4, 28, [1500, 5000])
    elif m == "disjoint":
        A.stack(0, 10, 0, H, [0, 500]), B.stack(20, 30, 0, H, [0, 500])
    elif m == "a-empty":
        A.stack(W + 8, W + 18, 0, H, [0, 500]), B.stack(4, 28, 4, 28, [100, 900])
    elif m == "sheets":                                           # whole-grid sheets: large triangles through the work list; stacks of 17 and 16 at the far end
        A.stack(0, W, 0, H, [-1000, 4000]), B.stack(0, W, 0, H, [1000, 9000])
        A.stack(W - 40, W - 8, H - 9, H - 1, _lattice(7, 100, 300)), B.stack(W - 40, W - 8, H - 9, H - 1, _lattice(6, 250, 300))
        A.stack(8, 40, 1, 9, _lattice(6, 100, 300)), B.stack(8, 40, 1, 9, _lattice(6, 250, 300))
    elif m == "list":                                             # more listed triangles of A than 256 x slices, small ones too; B two sheets over a part
        for k in range(c.large):
            A.box_tri(rng, int(rng.integers(0, W - 17)), int(rng.integers(0, H - 16 + 1)), 17, 16, float(rng.integers(-4000, 4001)), flip=k % 2 == 1)
        for k in range(60):
            A.box_tri(rng, int(rng.integers(0, W - 6)), int(rng.integers(0, H - 6)), 6, 6, float(rng.integers(-4000, 4001)), flip=k % 2 == 1)
        B.stack(0, 4096, 0, H, [-2000, 2000])
        for k in range(300):
            B.box_tri(rng, int(rng.integers(0, W - 17)), int(rng.integers(0, H - 16 + 1)), 16, 16, float(rng.integers(-4000, 4001)), flip=k % 2 == 1)
    meshes = []
    for s in (A, B):
        U, V, Z, f = s.arrays()
        meshes.append((column_world(U, V, Z), f))
    return dict(A=meshes[0], B=meshes[1], x0=0.0, y0=0.0, s=1.0)


def to_d(delta):
    """the displacement whose shift is `delta` on a grid with s = 1"""
    d = float(delta) / 256.0
    assert SR.shift_of(d, 1.0) == max(-SHIFT, min(SHIFT, delta))
    return d


@functools.lru_cache(maxsize=None)
def columns_ref(cid):
    d = data(cid)
    return SR.Columns(d["A"][0], d["A"][1], d["B"][0], d["B"][1], d["x0"], d["y0"], d["s"], BY_ID[cid].W, BY_ID[cid].H)


SPECIAL_D = [to_d(SHIFT), to_d(SHIFT + 1), to_d(-SHIFT), to_d(-SHIFT - 1), 1e30, -1e30, INF, -INF, NAN, -NAN]


@functools.lru_cache(maxsize=None)
def shifts(cid):
    """the launches of coma_shift_profile of a column case: a list of f64 arrays of at most K displacements.  Small grids: every
    breakpoint with its two neighbours (a crossing of A exactly on one of B, and one step to either side), one far outside on either
    side, the clamp and beyond, +-inf and NaN.  Big grids: ONE launch of K <= 3."""
    c, cols = BY_ID[cid], columns_ref(cid)
    if len(cols.ca[1]) and len(cols.cb[1]):
        near, far = SR.breakpoint_shifts(cols)
    else:
        near, far = [-1, 0, 1], 4096
    if c.W * c.H > 4096:
        d = ([to_d(near[len(near) // 2]), NAN, to_d(SHIFT + 1)])[:c.K]
        return [np.array(d, f64)]
    d = SPECIAL_D + [to_d(far), to_d(-far)] + [to_d(k) for k in near[::c.every]]
    return [np.array(d[i:i + c.K], f64) for i in range(0, len(d), c.K)]


# ------------------------------------------------------------------------------------------------------------------ optimize data
def _optimize(rng, c):
    N, J, nv = c.N, c.J, c.n_views
    views = np.zeros((nv, 28))
    views[:, 12:21], views[:, 21:24] = rng.normal(size=(nv, 9)), rng.normal(size=(nv, 3))
    views[:, 24], views[:, 25], views[:, 26], views[:, 27] = 2.4, 512.0, 256.0, 256.0
    cand_view = rng.integers(0, max(nv, 1), N).astype(i32)
    for at, value in c.bad:
        cand_view[at] = nv if value == "nv" else -1
    return dict(views=views, joints0=rng.normal(scale=0.3, size=(J, 3)), front=np.array([0.125, -0.25, 0.96]), cand_view=cand_view,
                cand_xy=256.0 + rng.normal(scale=50.0, size=(N, J, 2)))


_BUILD = dict(raster=_raster, iou=_iou, volume=_volume, columns=_columns, optimize=_optimize)


@functools.lru_cache(maxsize=None)
def data(cid):
    c = BY_ID[cid]
    return _BUILD[c.kind](kit.rng(cid), c)


# ------------------------------------------------------------------------------------------------------------------ the emulation
MUTATIONS = ("n-hits-not-reset", "second-trip-dropped", "hits-capped-255", "small-max-ge", "scan-chunk-1", "iou-stride-dropped", "profile-stride-dropped",
             "volume-stride-dropped", "top-left-wrong-edges", "iou-lt-to-le", "unpack-truncates", "sort-ignores-mesh", "inside-n-positive", "snap-limit-low",
             "snap-limit-high", "z-limit-low", "z-limit-high", "volume-pad-wrong", "status-3-steps-anyway", "nan-shift-clamp-sign")
# One defect the issue names changes no output, so no case can fail it: `<=` -> `<` in the merge -- the events that change
# order have equal Z, and the interval between them is empty.  (The clamp sign of a NaN shift looks like another, since beyond the clamp
# nothing overlaps; that holds for closed meshes only.  An open mesh -- a stack with an odd number of sheets -- stays "inside" to the end
# of its column, L_AB(+2^42) and L_AB(-2^42) differ, and the stacks cases catch it.)
EQUIVALENT = ("merge-le-to-lt",)


def _snap(verts, R, t, s, hw, hh, limit):
    """RR.snap / VR.snap with the limit as a parameter"""
    p = np.asarray(verts, f64)
    with np.errstate(all="ignore"):
        cx, cy, cz = RR.camera_space(p, R, t)
        su, sv = np.floor((cx * s + hw) * 256.0 + 0.5), np.floor((cy * s + hh) * 256.0 + 0.5)
    if not (np.isfinite(p).all() and np.isfinite(cz).all()):
        raise RR.Refused("non-finite vertex")
    if not ((np.abs(su) <= limit).all() and (np.abs(sv) <= limit).all()):
        raise RR.Refused("a snapped coordinate exceeds +-2^25")
    return su.astype(i64).tolist(), sv.astype(i64).tolist(), cz


def _walk(verts, faces, cam, W, H, mut, draw):
    """The bin and tile kernels' decisions for one mesh, faces in index order (the device appends in the order of arrival; any order
    gives the same samples): draw(x0, x1, y0, y1, jj, ii, z, sigma, times) for every box or box-and-tile piece -> dict(listed, trips,
    max_hits)."""
    limit = SNAP - 1 if mut == "snap-limit-low" else SNAP + 1 if mut == "snap-limit-high" else SNAP
    X, Y, Zd = _snap(verts, *cam, limit)
    faces = np.asarray(faces, i64)
    if faces.size and (faces.min() < 0 or faces.max() >= len(X)):
        raise RR.Refused("face index outside [0, V)")
    tiles_x = -(-W // TILE)
    _, slices = grid_slices(W, H)
    listed, hits, pieces, again = 0, {}, {}, 0
    stat = dict(listed=0, trips=0, max_hits=0, small_max=0, zero_area=0, flipped=0, ties=0, on_tile_0=0)
    for ia, ib, ic in faces.tolist():
        ax, ay, bx, by, cx, cy, za, zb, zc = X[ia], Y[ia], X[ib], Y[ib], X[ic], Y[ic], Zd[ia], Zd[ib], Zd[ic]
        area = RR.edge(ax, ay, bx, by, cx, cy)
        if area == 0:
            stat["zero_area"] += 1
            continue
        sigma = 1 if area > 0 else -1
        if area < 0:
            bx, by, zb, cx, cy, zc, area = cx, cy, zc, bx, by, zb, -area
            stat["flipped"] += 1
        x0, x1 = max(0, (min(ax, bx, cx) + 127) >> 8), min(W - 1, (max(ax, bx, cx) - 128) >> 8)
        y0, y1 = max(0, (min(ay, by, cy) + 127) >> 8), min(H - 1, (max(ay, by, cy) - 128) >> 8)
        if x0 > x1 or y0 > y1:
            continue
        px, py = (256 * np.arange(x0, x1 + 1, dtype=i64) + 128)[None, :], (256 * np.arange(y0, y1 + 1, dtype=i64) + 128)[:, None]
        e0, e1, e2 = RR.edge(bx, by, cx, cy, px, py), RR.edge(cx, cy, ax, ay, px, py), RR.edge(ax, ay, bx, by, px, py)
        t0, t1, t2 = RR.owns_ties(bx, by, cx, cy), RR.owns_ties(cx, cy, ax, ay), RR.owns_ties(ax, ay, bx, by)
        if mut == "top-left-wrong-edges":
            t0, t1, t2 = not t0, not t1, not t2
        inside = ((e0 > 0) | ((e0 == 0) & t0)) & ((e1 > 0) | ((e1 == 0) & t1)) & ((e2 > 0) | ((e2 == 0) & t2))
        stat["ties"] += int((inside & ((e0 == 0) | (e1 == 0) | (e2 == 0))).sum())
        with np.errstate(all="ignore"):
            z = ((e0.astype(f64) * za + e1.astype(f64) * zb) + e2.astype(f64) * zc) / float(area)
        centres = (x1 - x0 + 1) * (y1 - y0 + 1)
        stat["small_max"] = max(stat["small_max"], centres if centres <= SMALL_MAX else 0)
        if not (centres >= SMALL_MAX if mut == "small-max-ge" else centres > SMALL_MAX):
            jj, ii = np.nonzero(inside)
            draw(jj + y0, ii + x0, z[jj, ii], sigma, 1)
            continue
        step, listed = listed // 256, listed + 1
        stat["on_tile_0"] += x0 < TILE and y0 < TILE
        sl, trip = step % slices, step // slices
        stat["trips"] = max(stat["trips"], trip + 1)
        for ty in range(y0 // TILE, y1 // TILE + 1):
            for tx in range(x0 // TILE, x1 // TILE + 1):
                tile = ty * tiles_x + tx
                rank = hits.get((step, tile), 0)
                hits[(step, tile)] = rank + 1
                stat["max_hits"] = max(stat["max_hits"], rank + 1)
                times = 1
                if mut == "second-trip-dropped" and trip > 0:
                    times = 0
                if mut == "hits-capped-255" and rank >= 255:
                    times = 0
                if mut == "n-hits-not-reset" and trip > 0:       # the count goes on from the trip before: what is stored past hits[255] is lost,
                    before = sum(hits.get((s2, tile), 0) for s2 in range(sl, step, slices))
                    times = 0 if before + rank >= 256 else 1
                    if rank == 0:                                # and the earlier hits are walked again
                        for s2 in range(sl, step, slices):
                            for piece in pieces.get((s2, tile), ()):
                                draw(*piece, 1)
                                again += 1
                if times:
                    sub = inside[max(ty * TILE, y0) - y0:min(ty * TILE + TILE - 1, y1) - y0 + 1, max(tx * TILE, x0) - x0:min(tx * TILE + TILE - 1, x1) - x0 + 1]
                    jj, ii = np.nonzero(sub)
                    jj, ii = jj + max(ty * TILE, y0), ii + max(tx * TILE, x0)
                    draw(jj, ii, z[jj - y0, ii - x0], sigma, times)
                    if mut == "n-hits-not-reset":
                        pieces.setdefault((step, tile), []).append((jj, ii, z[jj - y0, ii - x0], sigma))
    stat["listed"], stat["walked_again"] = listed, again
    return stat


def emulate_raster(d, W, H, mut=None):
    """-> dict(key u64 [H, W], stat)"""
    key = np.full((H, W), EMPTY, u64)
    inf_drawn, nan_skipped = [0], [0]

    def draw(jj, ii, z, sigma, times):
        k = np.where(z == z, RR.depth_to_key(z), EMPTY)
        inf_drawn[0] += int(np.isinf(z).sum())
        nan_skipped[0] += int((z != z).sum())
        np.minimum.at(key, (jj, ii), k)
    s = float(max(W, H)) / float(d["scale"])
    stat = _walk(d["verts"], d["faces"], (d["R"], d["t"], s, W * 0.5, H * 0.5), W, H, mut, draw)
    stat.update(inf_drawn=inf_drawn[0], nan_skipped=nan_skipped[0])
    return dict(key=key, stat=stat)


def _unpack(p, mut):
    if mut == "unpack-truncates":
        return np.where(p < 0, -((-p) // 4), p // 4)
    return p >> 2


def _sweep_packed(col, packed, mesh, W, H, mut, delta=0):
    """VR.sweep on the words the device stores (Z * 4 + mesh * 2 + (sigma > 0)), `delta` added to every Z of A
    -> (sums, col_ab, counts)"""
    Z = _unpack(packed, mut) + np.where(mesh == 0, i64(delta), i64(0))
    sg = np.where(packed & 1, 1, -1).astype(i64)
    order = np.lexsort((Z, col))
    col, Z, sg, mesh = col[order], Z[order], sg[order], mesh[order]
    counts = np.bincount(col, minlength=W * H).astype(i64)
    if len(col) == 0:
        return np.zeros(3, i64), np.zeros((H, W), i64), counts.reshape(H, W)
    first = np.concatenate([[True], col[1:] != col[:-1]])
    start = np.maximum.accumulate(np.where(first, np.arange(len(col)), 0))

    def winding(sig):
        c = np.cumsum(sig)
        return -(c - (c - sig)[start])
    na, nb = winding(np.where(mesh == 0, sg, 0)), winding(np.where(mesh == 1, sg, 0))
    same = ~first[1:]
    length = np.where(same, Z[1:] - Z[:-1], 0)
    inside = (lambda n: n > 0) if mut == "inside-n-positive" else (lambda n: n != 0)
    in_a, in_b = inside(na[:-1]), inside(nb[:-1])
    sums = np.array([length[in_a & in_b].sum(), length[in_a].sum(), length[in_b].sum()], i64)
    col_ab = np.zeros(W * H, i64)
    np.add.at(col_ab, col[:-1][in_a & in_b], length[in_a & in_b])
    return sums, col_ab.reshape(H, W), counts.reshape(H, W)


def emulate_columns(d, W, H, mut=None, batches=()):
    """-> dict(sums, col_ab, counts, lengths, L (one [k, 3] per batch), stat) of coma_intersection_columns and of
    coma_shift_columns_prepare + coma_shift_profile as the kernels decide"""
    zlim = ZLIM - 1 if mut == "z-limit-low" else ZLIM + 1 if mut == "z-limit-high" else ZLIM
    s = float(d["s"])
    cam = (VR._R, (d["x0"], d["y0"], 0.0), s, 0.0, 0.0)
    cols, packed, meshes, stats = [], [], [], []
    for m, (v, f) in enumerate((d["A"], d["B"])):
        def draw(jj, ii, z, sigma, times):
            with np.errstate(all="ignore"):
                q = np.floor((z * s) * 256.0 + 0.5)
            if not (np.abs(q) <= float(zlim)).all():
                raise RR.Refused("a crossing's depth is non-finite or beyond +-2^40")
            for _ in range(times):
                cols.append(jj * W + ii), packed.append(q.astype(i64) * 4 + (m << 1) + (1 if sigma > 0 else 0)), meshes.append(np.full(len(jj), m, i64))
        stats.append(_walk(v, f, cam, W, H, mut, draw))
    cat = lambda a: np.concatenate(a) if a else np.zeros(0, i64)
    col, pk, mesh = cat(cols), cat(packed), cat(meshes)
    needed = len(col)
    scan_blocks = -(-W * H // SCAN_BLOCK)
    if mut == "scan-chunk-1" and scan_blocks > 256:               # the scan blocks past the 256th keep their sums instead of their offsets:
        keep = col < 256 * SCAN_BLOCK                              # their columns' crossings land elsewhere; here: they are lost
        col, pk, mesh = col[keep], pk[keep], mesh[keep]
    sums, col_ab, counts = _sweep_packed(col, pk, mesh, W, H, mut)
    pmesh = mesh
    if mut == "sort-ignores-mesh":                                # sorted by Z alone: A's part ends at the first crossing of B, the rest counts as B
        order = np.lexsort((pk, col))
        c2, m2 = col[order], mesh[order]
        first = np.concatenate([[True], c2[1:] != c2[:-1]]) if len(c2) else np.zeros(0, bool)
        start = np.maximum.accumulate(np.where(first, np.arange(len(c2)), 0))
        seen = np.cumsum(m2)
        after = (seen - (seen - m2)[start]) > 0
        pmesh = np.empty_like(mesh)
        pmesh[order] = np.where(after, 1, 0)
    alone = lambda m: _sweep_packed(col[pmesh == m], pk[pmesh == m], pmesh[pmesh == m], W, H, mut)[0][1 + m]      # each list walked by itself
    lengths = np.array([alone(0), alone(1)], i64)
    pcol, ppk = col, pk
    if mut == "profile-stride-dropped":
        keep = col < PROFILE_BLOCKS * 256
        pcol, ppk, pmesh = col[keep], pk[keep], pmesh[keep]
    L, seen = [], {}
    for batch in batches:
        out = np.zeros((len(batch), 3), i64)
        for k, dk in enumerate(batch):
            delta = SR.shift_of(dk, s)
            if mut == "nan-shift-clamp-sign" and dk != dk:
                delta = -delta
            for j in (-1, 0, 1):
                if delta + j not in seen:
                    seen[delta + j] = int(_sweep_packed(pcol, ppk, pmesh, W, H, mut, delta + j)[0][0])
                out[k, j + 1] = seen[delta + j]
        L.append(out)
    stat = dict(A=stats[0], B=stats[1], needed=needed, scan_blocks=scan_blocks)
    return dict(sums=sums, col_ab=col_ab, counts=counts, lengths=lengths, L=L, needed=needed, stat=stat)


def emulate_iou(d, K, want_masks, mut=None):
    hk, ak, gt = d["human"].reshape(-1), None if d["asset"] is None else d["asset"].reshape(-1), d["gt"].reshape(-1)
    N = len(hk)
    live = np.ones(N, bool)
    if mut == "iou-stride-dropped":
        live[IOU_BLOCKS * 256:] = False
    human, zh = (hk != EMPTY) & live, RR.key_to_depth(hk)
    bare, za = (np.ones(N, bool), np.zeros(N)) if ak is None else (ak == EMPTY, RR.key_to_depth(ak))
    g = (gt != 0) & live
    vis, inter, uni, masks = [], [], [], []
    with np.errstate(all="ignore"):
        for off in d["offsets"][:K].tolist():
            v = human & (bare | ((zh + off <= za) if mut == "iou-lt-to-le" else (zh + off < za)))
            vis.append(int(v.sum())), inter.append(int((v & g).sum())), uni.append(int((v | g).sum()))
            m = np.where(v, 255, 0).astype(u8)
            if mut == "iou-stride-dropped":
                m[~live] = 0xA5                                    # never written
            masks.append(m)
    return dict(visible=np.array(vis, i64), inter=np.array(inter, i64), uni=np.array(uni, i64),
                masks=np.stack(masks).reshape(K, *d["human"].shape) if want_masks else None)


def emulate_optimize(c, d, mut=None):
    """SR.optimize; with the planted defect, the step as the kernel took it before the contract was decided: the bad inlier skipped,
    the sums still divided by N, losses[0] and traj[1] written"""
    cols = columns_ref(c.columns) if c.columns else None
    cv = d["cand_view"]
    if mut == "status-3-steps-anyway" and c.bad:
        ok = (cv >= 0) & (cv < c.n_views)
        views, xy = d["views"], np.where(ok[:, None, None], d["cand_xy"], 0.0)
        cv2 = np.where(ok, cv, 0)
        # (loss, gradient) with the bad inliers' terms zeroed: one epoch, then status 3
        out = SR.optimize(cols if c.ws else None, views, d["joints0"], d["front"], cv2, xy, c.d0, c.lr, c.w_mv, c.w_col, 1)
        return dict(out, traj=out["traj"][:2], status=3, epoch=0)
    return SR.optimize(cols if c.ws else None, d["views"], d["joints0"], d["front"], cv, d["cand_xy"], c.d0, c.lr, c.w_mv, c.w_col, c.E)


def emulate(cid, mut=None):
    """the case as the kernels decide, with the defect `mut` planted; computed once per (case, defect), shared, never changed"""
    return _emulate(cid, mut)


@functools.lru_cache(maxsize=None)
def _emulate(cid, mut):
    assert mut is None or mut in MUTATIONS
    c, d = BY_ID[cid], data(cid)
    if c.kind == "raster":
        return emulate_raster(d, c.W, c.H, mut)
    if c.kind == "iou":
        return emulate_iou(d, c.K, c.masks, mut)
    if c.kind == "volume":
        return dict(out=_volume_shape(d["verts"], d["faces"], mut)[0])
    if c.kind == "columns":
        return emulate_columns(d, c.W, c.H, mut, shifts(cid))
    return emulate_optimize(c, d, mut)


# ------------------------------------------------------------------------------------------------------------------ the references
@functools.lru_cache(maxsize=None)
def reference(cid):
    """what the three restatements give, unchanged; for a volume case mesh_volume_shape"""
    c, d = BY_ID[cid], data(cid)
    if c.kind == "raster":
        return dict(key=RR.raster_depth(d["verts"], d["faces"], d["R"], d["t"], d["scale"], c.W, c.H))
    if c.kind == "iou":
        v, i, u, m = RR.silhouette_iou(d["human"], d["asset"], d["offsets"], d["gt"], want_masks=c.masks)
        return dict(visible=v, inter=i, uni=u, masks=m)
    if c.kind == "volume":
        return dict(out=mesh_volume_shape(d["verts"], d["faces"])[0])
    if c.kind == "columns":
        sums, col_ab, counts = VR.intersection_columns(d["A"][0], d["A"][1], d["B"][0], d["B"][1], d["x0"], d["y0"], d["s"], c.W, c.H)
        cols = columns_ref(cid)
        return dict(sums=sums, col_ab=col_ab, counts=counts, needed=int(counts.sum()), lengths=np.array([cols.L_A, cols.L_B], i64),
                    L=[cols.profile(b.tolist()) for b in shifts(cid)])
    cols = columns_ref(c.columns) if (c.columns and c.ws) else None
    r = SR.optimize(cols, d["views"], d["joints0"], d["front"], d["cand_view"], d["cand_xy"], c.d0, c.lr, c.w_mv, c.w_col, c.E)
    return r


def optimize_status(c, r):
    """(status, epoch) coma_depth_optimize_status reports for a trajectory of SR.optimize"""
    if r.get("status") == 3:
        return 3, r["epoch"]
    if not np.isfinite(r["traj"][-1]):
        return 1, len(r["traj"]) - 1
    return 0, 0


# ------------------------------------------------------------------------------------------------------------------ the assertions
def tile_0_hits(big, n):
    """hits of tile 0 in each step of 256 slots of a work list as the device left it (int32 [n, 4]: face, x0 | y0 << 16, x1 | y1 << 16, 0)"""
    big = np.asarray(big).reshape(-1, 4)[:n]
    on = ((big[:, 1] & 0xffff) < TILE) & ((big[:, 1] >> 16) < TILE)
    return [int(on[s:s + 256].sum()) for s in range(0, n, 256)]


def same(got, want, what, nan_at=()):
    """every bit; at the flat positions `nan_at` a NaN for a NaN"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = kit.bits(got) != kit.bits(want)
    for i in nan_at:                                                # IEEE 754 leaves the sign and payload of an invalid operation's NaN open:
        if np.isnan(got.flat[i]) and np.isnan(want.flat[i]):        # inf - inf is 0xFFF8... on the host and 0x7FF8... on the device
            bad.flat[i] = False
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {int(np.flatnonzero(bad.reshape(-1))[0])}"


def check(c, got):
    """got: what the launches of the case left (or what emulate gives) -> the number of elements compared.  Everything in every bit."""
    ref = reference(c.id)
    if c.kind == "raster":
        same(got["key"], ref["key"], f"{c.id} depth_key")
        assert got["stat"]["listed"] == emulate(c.id)["stat"]["listed"], f"{c.id}: {got['stat']['listed']} triangles on the work list"
        return ref["key"].size
    if c.kind == "iou":
        for k in ("visible", "inter", "uni"):
            same(got[k], ref[k], f"{c.id} {k}")
        if c.masks:
            same(got["masks"], ref["masks"], f"{c.id} masks")
        return 3 * c.K + (ref["masks"].size if c.masks else 0)
    if c.kind == "volume":
        a, b = np.array([got["out"]], f64), np.array([ref["out"]], f64)
        assert (np.isnan(a[0]) and np.isnan(b[0])) or kit.bits(a)[0] == kit.bits(b)[0], f"{c.id}: {got['out']!r}, the summation shape gives {ref['out']!r}"
        return 1
    if c.kind == "columns":
        same(got["sums"], ref["sums"], f"{c.id} sums")
        if c.col_ab:
            same(got["col_ab"], ref["col_ab"], f"{c.id} col_ab")
        assert got["needed"] == ref["needed"], f"{c.id}: {got['needed']} crossings counted, {ref['needed']} in the restatement"
        if c.lengths:
            same(got["lengths"], ref["lengths"], f"{c.id} lengths")
        assert len(got["L"]) == len(ref["L"])
        for k, (a, b) in enumerate(zip(got["L"], ref["L"])):
            same(a, b, f"{c.id} L of launch {k}")
        emu = emulate(c.id)["stat"]
        for m in "AB":
            assert got["stat"][m]["listed"] == emu[m]["listed"], f"{c.id}: {got['stat'][m]['listed']} triangles of {m} on the work list"
        return 3 + ref["col_ab"].size * bool(c.col_ab) + sum(a.size for a in ref["L"]) + 3
    status, epoch = optimize_status(c, ref)
    assert (got["status"], got["epoch"]) == (status, epoch), f"{c.id}: status {got['status']} in epoch {got['epoch']}, the restatement {status} in {epoch}"
    collide = bool(c.columns and c.ws and c.w_col != 0.0)
    for k in ("traj", "Ltraj", "losses"):
        n = len(ref[k]) if (k != "Ltraj" or collide) else 0
        same(got[k][:n], ref[k][:n], f"{c.id} {k}", nan_at=(n - 1,) if k == "traj" and status == 1 else ())     # the d that left the finite range
        rest = kit.bits(np.ascontiguousarray(got[k][n:]))
        if k == "Ltraj" and collide:
            assert not rest.any(), f"{c.id}: Ltraj behind the stopping epoch is not the zero the init kernel wrote"
        else:
            assert (rest == kit.sentinel_bits(got[k].dtype)).all(), f"{c.id}: {k} was written behind the stopping epoch"
    return sum(ref[k].size for k in ("traj", "Ltraj", "losses"))


def pad_optimize(c, r):
    """a result of SR.optimize as the device's buffers would hold it: full length, the sentinel behind what was written (Ltraj: zero
    when the collision term is on), with the status and the epoch"""
    collide = bool(c.columns and c.ws and c.w_col != 0.0)
    status, epoch = optimize_status(c, r)
    out = dict(status=status, epoch=epoch)
    for k, shape in (("traj", (c.E + 1,)), ("Ltraj", (c.E, 3)), ("losses", (c.E, 2))):
        a = np.zeros(shape, r[k].dtype) if (k == "Ltraj" and collide) else kit.sentinel(int(np.prod(shape)), r[k].dtype).reshape(shape)
        if k != "Ltraj" or collide:
            a[:len(r[k])] = r[k]
        out[k] = a
    return out


def written(c):
    """how many leading elements of traj, Ltraj, losses the contract says the case writes (everything behind keeps its sentinel);
    Ltraj is zeroed as a whole by the init kernel when the collision term is on"""
    ref = reference(c.id)
    collide = bool(c.columns and c.ws and c.w_col != 0.0)
    return dict(traj=len(ref["traj"]), Ltraj=3 * c.E if collide else 0, losses=2 * len(ref["losses"]))


# ------------------------------------------------------------------------------------------------------------------ regimes
REACHABLE = {
    "raster-trip-2", "raster-hits-full", "raster-slices-1", "raster-slices-2", "raster-slices-32", "box-256-by-lane", "box-257-listed", "snap-at-2^25",
    "depth-inf-drawn", "depth-nan-not-drawn", "winding-flipped", "zero-area", "sample-on-edge", "map-all-empty",
    "iou-stride-2", "iou-wave-without-human", "iou-exact-tie", "iou-masks", "iou-no-masks", "iou-no-asset", "iou-K-64",
    "volume-stride-2", "volume-bad-index", "volume-partials-padded", "volume-256-blocks",
    "count-trip-2", "fill-trip-2", "scan-chunk-1", "scan-chunk-2", "scan-one-block", "column-16-in-lds", "column-17-in-place", "column-82", "column-1", "column-2",
    "Z-negative", "Z-at-2^40", "coincident-Z", "col_ab-null", "lengths-null", "inward", "LA-zero", "disjoint",
    "profile-stride-2", "shift-at-2^42", "shift-beyond-2^42", "shift-nan", "shift-inf", "wave-without-both", "profile-K-64", "A-on-B",
    "opt-N-0", "opt-N-above-256", "opt-status-3", "opt-nonfinite-epoch-0", "opt-nonfinite-later", "opt-LA-zero-collision", "opt-lr-0", "opt-E-4096",
    "opt-ws-given-w-0", "opt-ws-null-w-nonzero",
    "snap-beyond-2^25", "Z-beyond-2^40", "Z-non-finite", "refused-nonfinite-vertex", "refused-face-index", "refused-capacity", "refused-scale-overflow",
}


@functools.lru_cache(maxsize=None)
def branches(cid):
    c, d, b = BY_ID[cid], data(cid), set()
    if c.kind == "raster":
        e = emulate(cid)
        st, key = e["stat"], e["key"]
        _, slices = grid_slices(c.W, c.H)
        if slices in (1, 2, 32):
            b.add(f"raster-slices-{slices}")
        full = st["listed"] >= 256 and st["on_tile_0"] == st["listed"]       # whatever the order of arrival, the first step holds 256 hits of tile 0
        for name, on in (("raster-trip-2", st["trips"] >= 2), ("raster-hits-full", full), ("box-256-by-lane", st["small_max"] == SMALL_MAX),
                         ("box-257-listed", st["listed"] > 0), ("depth-inf-drawn", st["inf_drawn"]), ("depth-nan-not-drawn", st["nan_skipped"]),
                         ("winding-flipped", st["flipped"]), ("zero-area", st["zero_area"]), ("sample-on-edge", st["ties"]), ("map-all-empty", (key == EMPTY).all())):
            if on:
                b.add(name)
        X, Y, _ = RR.snap(d["verts"], d["R"], d["t"], d["scale"], c.W, c.H)
        if max(np.abs(X).max(), np.abs(Y).max()) == SNAP:
            b.add("snap-at-2^25")
    elif c.kind == "iou":
        N = c.W * c.H
        human = (d["human"] != EMPTY).reshape(-1)
        if N > IOU_BLOCKS * 256:
            b.add("iou-stride-2")
        if any(not human[w:w + 64].any() for w in range(0, N, 64)):
            b.add("iou-wave-without-human")
        if d["asset"] is None:
            b.add("iou-no-asset")
        else:
            both = human & (d["asset"] != EMPTY).reshape(-1)
            zh, za = RR.key_to_depth(d["human"].reshape(-1)), RR.key_to_depth(d["asset"].reshape(-1))
            if any(((zh + off == za) & both).any() for off in d["offsets"][np.isfinite(d["offsets"])]):
                b.add("iou-exact-tie")
        b.add("iou-masks" if c.masks else "iou-no-masks")
        if c.K == 64:
            b.add("iou-K-64")
    elif c.kind == "volume":
        F, V = len(d["faces"]), len(d["verts"])
        if F > VOLUME_BLOCKS * 256:
            b.add("volume-stride-2")
        if ((d["faces"] < 0) | (d["faces"] >= V)).any():
            b.add("volume-bad-index")
        b.add("volume-partials-padded" if -(-F // 256) < VOLUME_BLOCKS else "volume-256-blocks")
    elif c.kind == "columns":
        e, ref = emulate(cid), reference(cid)
        st, counts = e["stat"], ref["counts"]
        if max(st["A"]["trips"], st["B"]["trips"]) >= 2:
            b |= {"count-trip-2", "fill-trip-2"}                   # one template, the same list: both kernels go round twice
        nb = st["scan_blocks"]
        b.add("scan-one-block" if nb == 1 else "scan-chunk-1" if nb <= 256 else "scan-chunk-2")
        for n, name in ((1, "column-1"), (2, "column-2"), (16, "column-16-in-lds"), (17, "column-17-in-place"), (82, "column-82")):
            if (counts == n).any():
                b.add(name)
        cols = columns_ref(cid)
        Z = np.concatenate([cols.ca[1], cols.cb[1]])
        if (Z < 0).any():
            b.add("Z-negative")
        if len(Z) and np.abs(Z).max() == ZLIM:
            b.add("Z-at-2^40")
        cz = (np.concatenate([cols.ca[0], cols.cb[0]]) << 42) + (Z + ZLIM)     # (column, Z) as one word: 19 + 42 bits
        if len(np.unique(cz)) < len(cz):
            b.add("coincident-Z")
        for name, on in (("col_ab-null", not c.col_ab), ("lengths-null", not c.lengths), ("inward", getattr(c, "inward", False)), ("LA-zero", cols.L_A == 0),
                         ("disjoint", len(cols.ca[0]) and len(cols.cb[0]) and not np.intersect1d(cols.ca[0], cols.cb[0]).size)):
            if on:
                b.add(name)
        ha, hb = np.bincount(cols.ca[0], minlength=c.W * c.H) > 0, np.bincount(cols.cb[0], minlength=c.W * c.H) > 0
        both = ha & hb
        if both[PROFILE_BLOCKS * 256:].any():
            b.add("profile-stride-2")
        waves = [both[w:w + 64].any() for w in range(0, c.W * c.H, 64)]
        if any(x != y for x, y in zip(waves, waves[1:])):
            b.add("wave-without-both")
        near = set(np.unique(np.subtract.outer(np.unique(cols.cb[1]), np.unique(cols.ca[1]))).tolist())
        for batch in shifts(cid):
            if len(batch) == 64:
                b.add("profile-K-64")
            for dk in batch.tolist():
                with np.errstate(all="ignore"):
                    q = np.floor((f64(dk) * f64(d["s"])) * 256.0 + 0.5)
                b |= {"shift-nan"} if q != q else {"shift-inf"} if np.isinf(q) else {"shift-at-2^42"} if abs(q) == SHIFT else {"shift-beyond-2^42"} if abs(q) > SHIFT else set()
                if q == q and abs(q) < SHIFT and int(q) in near and both.any():
                    b.add("A-on-B")
    else:
        ref = reference(cid)
        status, epoch = optimize_status(c, ref)
        collide = bool(c.columns and c.ws and c.w_col != 0.0)
        for name, on in (("opt-N-0", c.N == 0), ("opt-N-above-256", c.N > 256), ("opt-status-3", status == 3), ("opt-nonfinite-epoch-0", status == 1 and epoch == 1),
                         ("opt-nonfinite-later", status == 1 and epoch > 1), ("opt-LA-zero-collision", collide and columns_ref(c.columns).L_A == 0),
                         ("opt-lr-0", c.lr == 0.0), ("opt-E-4096", c.E == 4096), ("opt-ws-given-w-0", c.ws and c.w_col == 0.0),
                         ("opt-ws-null-w-nonzero", not c.ws and c.w_col != 0.0)):
            if on:
                b.add(name)
    return frozenset(b)


# ------------------------------------------------------------------------------------------------------------------ the tables
def _cases():
    R = lambda id, W, H, mesh, **kw: Case(id, "raster", W=W, H=H, mesh=mesh, **{**dict(scale=None), **kw})
    I = lambda id, W, H, K, asset=True, masks=True: Case(id, "iou", W=W, H=H, K=K, asset=asset, masks=masks)
    Vo = lambda id, mesh="soup", V=40, F=1, bad=(): Case(id, "volume", mesh=mesh, V=V, F=F, bad=bad)
    Co = lambda id, W, H, mesh, K, **kw: Case(id, "columns", W=W, H=H, mesh=mesh, K=K, **{**dict(col_ab=True, lengths=True, inward=False, yb0=0, every=1), **kw})
    O = lambda id, N, J, E, w, **kw: Case(id, "optimize", N=N, J=J, E=E, w_mv=w[0], w_col=w[1],
                                          **{**dict(n_views=3, columns="c-32x32-box", ws=True, d0=0.0, lr=0.01, bad=()), **kw})
    both, mv, col = (1e-3, 0.4), (1e-3, 0.0), (0.0, 0.4)
    return [
        R("r-1x1-one-face", 1, 1, "one"),
        R("r-16x16-v255", 16, 16, "pool", V=255, F=85),
        R("r-16x16-v256-f255", 16, 16, "pool", V=256, F=255),
        R("r-17x16-v257-f256", 17, 16, "pool", V=257, F=256),
        R("r-17x16-f257", 17, 16, "pool", V=100, F=257),
        R("r-17x16-v30-f64", 17, 16, "pool", V=30, F=64),
        R("r-50x131-boxes-256-257", 50, 131, "boxes", n=60, boxes=[(16, 16), (17, 16), (16, 17), (2, 128), (2, 129), (1, 131), (8, 32), (3, 86)]),
        R("r-8192x1-boxes-256-257", 8192, 1, "boxes", n=24, boxes=[(256, 1), (257, 1), (255, 1)]),
        R("r-1x8192-boxes-256-257", 1, 8192, "boxes", n=24, boxes=[(1, 256), (1, 257), (1, 255)]),
        R("r-8192x49-list-300", 8192, 49, "crowd", crowd=260, scattered=40),
        R("r-8192x32-list-600", 8192, 32, "crowd", crowd=8, scattered=592),
        R("r-64x64-hits-256", 64, 64, "crowd", crowd=260, scattered=0),
        R("r-64x48-cover-2^25", 64, 48, "cover"),
        R("r-16x16-edges", 16, 16, "edges"),
        R("r-50x131-rotated-sphere", 50, 131, "sphere"),
        R("r-16x16-scale-1.7e308", 16, 16, "pool", V=60, F=40, scale=1.7e308),
        I("i-n1-k1", 1, 1, 1), I("i-n63-k7-bare", 63, 1, 7, asset=False, masks=False), I("i-n64-k64", 64, 1, 64), I("i-n65-k7", 65, 1, 7),
        I("i-n255-k1-nomask", 255, 1, 1, masks=False), I("i-n256-k7-bare", 256, 1, 7, asset=False), I("i-n257-k64", 1, 257, 64),
        I("i-8192x33-k3", 8192, 33, 3), I("i-8192x33-k1-nomask", 8192, 33, 1, masks=False),
        Vo("v-f1", F=1, V=3), Vo("v-f255", F=255), Vo("v-f256", F=256), Vo("v-f257", F=257), Vo("v-f65536", F=65536, V=999), Vo("v-f65537", F=65537, V=999),
        Vo("v-bad-V-first-block", F=65536, V=999, bad=((0, "V"),)), Vo("v-bad-neg-first-block", F=65537, V=999, bad=((65536, "neg"),)),
        Vo("v-bad-V-last-block", F=65536, V=999, bad=((65535, "V"),)), Vo("v-bad-neg-last-block", F=65537, V=999, bad=((65300, "neg"),)),
        Vo("v-cube", "cube"), Vo("v-cube-inward", "cube-inward"),
        Co("c-1x1", 1, 1, "one", 1),
        Co("c-32x32-stacks-k64", 32, 32, "stacks", 64),
        Co("c-33x32-stacks-inward-k2", 33, 32, "stacks", 2, inward=True, yb0=4, col_ab=False, lengths=False),
        Co("c-32x32-box", 32, 32, "box", 1),
        Co("c-32x32-disjoint", 32, 32, "disjoint", 1),
        Co("c-32x32-a-empty", 32, 32, "a-empty", 2),
        Co("c-8192x32-sheets-k1", 8192, 32, "sheets", 1, col_ab=False),
        Co("c-8192x33-sheets-k3", 8192, 33, "sheets", 3),
        Co("c-8192x49-list-300", 8192, 49, "list", 1, large=300, col_ab=False),
        O("o-n0-e2-collision", 0, 25, 2, col, n_views=0),
        O("o-n1-j1-e4096-multiview", 1, 1, 4096, mv, n_views=1, columns=None, ws=False),
        O("o-n255-j25-e20-both", 255, 25, 20, both),
        O("o-n256-j25-e1-ws-given-w0", 256, 25, 1, mv),
        O("o-n257-j25-e20-both", 257, 25, 20, both),
        O("o-n513-j1-e2-both", 513, 1, 2, both),
        O("o-n2-j1024-e2-ws-null", 2, 1024, 2, both, ws=False),
        O("o-la0-e2-both", 1, 25, 2, both, columns="c-32x32-a-empty"),
        O("o-lr0-e2-both", 7, 25, 2, both, lr=0.0),
        O("o-nonfinite-epoch-0", 1, 25, 5, (1.0, 0.0), d0=1e306, columns=None, ws=False),
        O("o-nonfinite-later", 1, 25, 5, (1e-6, 0.4), lr=1e304),         # d1 ~ 1e304 is finite; at it the residuals overflow, and d2 is NaN
        O("o-badview-neg-first", 257, 25, 3, both, bad=((0, "neg"),)),
        O("o-badview-nv-first", 257, 25, 3, both, bad=((0, "nv"),)),
        O("o-badview-neg-last", 257, 25, 3, both, bad=((256, "neg"),)),
        O("o-badview-nv-last", 257, 25, 3, mv, bad=((256, "nv"),), columns=None, ws=False),
    ]


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
KIND = lambda kind: [c for c in CASES if c.kind == kind]


# ------------------------------------------------------------------------------------------------------------------ refusals on the device
# One row per refusal the device takes, for mesh A and for mesh B: (id, what is changed, the status text, the regime).  A row runs through
# every entry point that can raise it.  The data comes from the accepted case c-32x32-box (the rasteriser sees mesh A of it under the
# identity camera); every bad index is tested by raster_setup_kernel before any kernel follows it, a refused depth never becomes an index.
REFUSAL_BASE = "c-32x32-box"
DEVICE_REFUSALS = [
    ("nan-vertex", "non-finite vertex", "refused-nonfinite-vertex", ("raster", "columns", "prepare")),
    ("inf-vertex", "non-finite vertex", "refused-nonfinite-vertex", ("raster", "columns", "prepare")),
    ("range", "a snapped coordinate exceeds +-2^25", "snap-beyond-2^25", ("raster", "columns", "prepare")),
    ("scale-overflow", "a snapped coordinate exceeds +-2^25", "refused-scale-overflow", ("raster",)),
    ("face-V", "face index outside [0, V)", "refused-face-index", ("raster", "columns", "prepare")),
    ("face-neg", "face index outside [0, V)", "refused-face-index", ("raster", "columns", "prepare")),
    ("z-nonfinite", "a crossing's depth is non-finite or beyond +-2^40", "Z-non-finite", ("columns", "prepare")),
    ("z-beyond", "a crossing's depth is non-finite or beyond +-2^40", "Z-beyond-2^40", ("columns", "prepare")),
    ("capacity", "capacity exceeded", "refused-capacity", ("columns", "prepare")),
    ("nan-and-range", "non-finite vertex", "refused-nonfinite-vertex", ("raster", "columns", "prepare")),          # two bits: the first the status function tests
    ("range-and-face", "a snapped coordinate exceeds +-2^25", "snap-beyond-2^25", ("raster", "columns", "prepare")),
    ("face-and-capacity", "face index outside [0, V)", "refused-face-index", ("columns", "prepare")),
]


def refusal_data(kind, mesh):
    """the operands of REFUSAL_BASE with one thing changed in mesh `mesh` (0: A, 1: B) -> dict(A, B, x0, y0, s, capacity, scale)"""
    d = data(REFUSAL_BASE)
    m = [(d["A"][0].copy(), d["A"][1].copy()), (d["B"][0].copy(), d["B"][1].copy())]
    v, f = m[mesh]
    capacity, scale = reference(REFUSAL_BASE)["needed"], 32.0
    if kind in ("nan-vertex", "nan-and-range"):
        v[3, 1] = NAN
    if kind == "inf-vertex":
        v[len(v) - 1, 2] = -INF
    if kind in ("range", "nan-and-range", "range-and-face"):
        v[0, 0] = (SNAP + 1) / 256.0                                # one 1/256 cell beyond (the rasteriser's camera adds W / 2: farther still)
    if kind in ("face-V", "range-and-face", "face-and-capacity"):
        f[len(f) - 1, 2] = len(v)
    if kind == "face-neg":
        f[0, 0] = -1
    if kind == "z-nonfinite":
        v[f[0], 2] = [1e305, -1e305, 1e305]                         # finite vertices, inf - inf at the samples
    if kind == "z-beyond":
        v[f[0], 2] = (ZLIM + 1) / 256.0
    if kind in ("capacity", "face-and-capacity"):
        capacity -= 1
    if kind == "scale-overflow":
        scale = 1e-308                                              # s = 32 / 1e-308 overflows: u is inf or NaN
    return dict(A=m[0], B=m[1], x0=d["x0"], y0=d["y0"], s=d["s"], capacity=capacity, scale=scale)


def refusal_reached(kind, mesh, entry):
    """what the restatement says of a refusal row: the text it refuses with (capacity: the count it would need)"""
    d = refusal_data(kind, mesh)
    try:
        if entry == "raster":
            v, f = d["A"] if mesh == 0 else d["B"]
            RR.raster_depth(v, f, IDENT[0], IDENT[1], d["scale"], 32, 32)
        else:
            _, _, counts = VR.intersection_columns(d["A"][0], d["A"][1], d["B"][0], d["B"][1], d["x0"], d["y0"], d["s"], 32, 32)
            if int(counts.sum()) > d["capacity"]:
                return "capacity exceeded"
    except RR.Refused as e:
        return str(e)
    return None


# ------------------------------------------------------------------------------------------------------------------ the argument checks
OUTPUT_ARGS = ("depth_key", "visible", "inter", "uni", "masks", "out", "sums", "col_ab", "lengths", "L", "traj", "Ltraj", "losses", "Ctraj", "state")
HOST_ARGS = ("R", "t", "front")
_RAST = dict(verts=PTR, V=8, faces=PTR, F=12, R=PTR, t=PTR, scale=2.4, W=64, H=48, workspace=PTR, depth_key=PTR)
_IOU = dict(human_key=PTR, asset_key=PTR, offsets=PTR, K=7, gt=PTR, W=64, H=48, visible=PTR, inter=PTR, uni=PTR, masks=PTR)
_VOL = dict(verts=PTR, V=8, faces=PTR, F=12, out=PTR, workspace=PTR)
_COL = dict(vertsA=PTR, VA=8, facesA=PTR, FA=12, vertsB=PTR, VB=8, facesB=PTR, FB=12, x0=0.0, y0=0.0, s=32.0, W=32, H=32, capacity=4096, workspace=PTR)
_OPT = dict(workspace=PTR, views=PTR, n_views=3, joints0=PTR, front=PTR, cand_view=PTR, cand_xy=PTR, N=4, J=25, d0=0.0, lr=0.01, w_multiview=1e-3,
            w_collision=0.4, E=3, traj=PTR, Ltraj=PTR, losses=PTR, state=PTR)
_COAP = dict(weights=PTR, weights_floats=1 << 40, code=PTR, K=1, points=PTR, T=16, filter_threshold=0.5, coap_workspace=PTR, coap_workspace_bytes=1 << 40,
             **{k: v for k, v in _OPT.items() if k not in ("workspace", "Ltraj")}, Ctraj=PTR)
_BIG = (1 << 24) + 1
_sizes = lambda: [("outside", dict(VA=0)), ("outside", dict(FA=0)), ("outside", dict(VB=_BIG)), ("outside", dict(FB=-1)), ("outside", dict(W=0)), ("outside", dict(W=8193)),
                  ("outside", dict(H=0)), ("outside", dict(H=8193)), ("outside", dict(capacity=0)), ("outside", dict(capacity=1 << 31))]
_grid = lambda: [("must be positive and finite", dict(s=0.0)), ("must be positive and finite", dict(s=-1.0)), ("must be positive and finite", dict(s=NAN)),
                 ("must be positive and finite", dict(s=INF)), ("must be positive and finite", dict(x0=NAN)), ("must be positive and finite", dict(y0=INF))]
_optrows = lambda: [("null pointer", dict(front=0)), ("null pointer", dict(traj=0)), ("null pointer", dict(losses=0)), ("null pointer", dict(state=0)),
                    ("outside [1, 4096]", dict(E=0)), ("outside [1, 4096]", dict(E=4097)), ("outside [0, 65536]", dict(N=-1)), ("outside [0, 65536]", dict(N=65537)),
                    ("outside [0, 65536]", dict(J=0)), ("outside [0, 65536]", dict(J=1025)), ("outside [0, 65536]", dict(n_views=-1)),
                    ("are read when N > 0", dict(views=0)), ("are read when N > 0", dict(joints0=0)), ("are read when N > 0", dict(cand_view=0)),
                    ("are read when N > 0", dict(cand_xy=0)), ("are read when N > 0", dict(n_views=0)),
                    ("must be finite", dict(d0=NAN)), ("must be finite", dict(lr=INF)), ("must be finite", dict(w_multiview=NAN)), ("must be finite", dict(w_collision=-INF)),
                    ("must be finite", dict(lr=NAN))]       # the rows above are one check function's: the same words after either name
REFUSALS = {
    "coma_raster_depth_f64": (_RAST, [
        ("null pointer", dict(verts=0)), ("null pointer", dict(faces=0)), ("null pointer", dict(R=0)), ("null pointer", dict(t=0)), ("null pointer", dict(workspace=0)),
        ("null pointer", dict(depth_key=0)), ("outside [1, 16777216]", dict(V=0)), ("outside [1, 16777216]", dict(V=_BIG)), ("outside [1, 16777216]", dict(F=0)), ("outside [1, 16777216]", dict(F=_BIG)),
        ("outside [1, 8192]", dict(W=0)), ("outside [1, 8192]", dict(W=8193)), ("outside [1, 8192]", dict(H=0)), ("outside [1, 8192]", dict(H=8193)),
        ("must be positive and finite", dict(scale=0.0)), ("must be positive and finite", dict(scale=-2.0)), ("must be positive and finite", dict(scale=NAN)),
        ("must be positive and finite", dict(scale=INF)), ("workspace must be 16-byte aligned", dict(workspace=Off(8))),
    ]),
    "coma_silhouette_iou": (_IOU, [
        ("null pointer", dict(human_key=0)), ("null pointer", dict(offsets=0)), ("null pointer", dict(gt=0)), ("null pointer", dict(visible=0)),
        ("null pointer", dict(inter=0)), ("null pointer", dict(uni=0)), ("outside [1, 64]", dict(K=0)), ("outside [1, 64]", dict(K=65)),
        ("outside [1, 8192]", dict(W=0)), ("outside [1, 8192]", dict(W=8193)), ("outside [1, 8192]", dict(H=0)), ("outside [1, 8192]", dict(H=8193)),
    ]),
    "coma_mesh_volume_f64": (_VOL, [
        ("null pointer", dict(verts=0)), ("null pointer", dict(faces=0)), ("null pointer", dict(out=0)), ("null pointer", dict(workspace=0)),
        ("outside [1, 16777216]", dict(V=0)), ("outside [1, 16777216]", dict(V=_BIG)), ("outside [1, 16777216]", dict(F=0)), ("outside [1, 16777216]", dict(F=_BIG)), ("workspace must be 8-byte aligned", dict(workspace=Off(4))),
    ]),
    "coma_intersection_columns": (dict(_COL, sums=PTR, col_ab=PTR), [
        ("null pointer", dict(vertsA=0)), ("null pointer", dict(facesA=0)), ("null pointer", dict(vertsB=0)), ("null pointer", dict(facesB=0)),
        ("null pointer", dict(workspace=0)), ("null pointer", dict(sums=0)), *_sizes(), *_grid(), ("workspace must be 16-byte aligned", dict(workspace=Off(8))),
    ]),
    "coma_shift_columns_prepare": (dict(_COL, lengths=PTR), [
        ("null pointer", dict(vertsA=0)), ("null pointer", dict(facesA=0)), ("null pointer", dict(vertsB=0)), ("null pointer", dict(facesB=0)),
        ("null pointer", dict(workspace=0)), *_sizes(), *_grid(), ("workspace must be 16-byte aligned", dict(workspace=Off(4))),
    ]),
    "coma_shift_profile": (dict(workspace=PTR, d=PTR, K=3, L=PTR), [
        ("null pointer", dict(workspace=0)), ("null pointer", dict(d=0)), ("null pointer", dict(L=0)), ("outside [1, 64]", dict(K=0)), ("outside [1, 64]", dict(K=65)),
        ("workspace must be 16-byte aligned", dict(workspace=Off(8))),
    ]),
    "coma_depth_optimize_f64": (_OPT, [
        *_optrows(), ("Ltraj is written", dict(Ltraj=0)), ("workspace 16-byte, state 8-byte", dict(workspace=Off(8))), ("workspace 16-byte, state 8-byte", dict(state=Off(4))),
    ]),
    "coma_depth_optimize_coap_f64": (_COAP, [
        *_optrows(), ("Ctraj is written", dict(Ctraj=0)), ("weights of 3 floats", dict(weights_floats=3)), ("Ctraj 8-byte, the weights 16-byte", dict(Ctraj=Off(4))),
        ("Ctraj 8-byte, the weights 16-byte", dict(weights=Off(4))), ("state must be 8-byte aligned", dict(state=Off(4))),
    ]),
}
# the entry points whose last parameter is not the stream (kit.call does not take them) and the size functions: (call, arguments, text or 0)
STATUS_REFUSALS = [
    ("coma_raster_status", (0, None), "coma_raster_status: null pointer"),
    ("coma_intersection_status", (0, None, None), "coma_intersection_status: null pointer"),
    ("coma_shift_columns_status", (0, None, None), "coma_shift_columns_status: null pointer"),
    ("coma_depth_optimize_status", (0, None, None), "coma_depth_optimize_status: null pointer"),
]
SIZE_REFUSALS = [
    ("coma_raster_workspace_bytes", (0, 1)), ("coma_raster_workspace_bytes", (1, 0)), ("coma_mesh_volume_workspace_bytes", (0,)),
    ("coma_column_crossings_workspace_bytes", (8, 12, 8, 12, 32, 32, 0)), ("coma_column_crossings_workspace_bytes", (8, 12, 8, 12, 8193, 32, 10)),
    ("coma_column_crossings_workspace_bytes", (0, 12, 8, 12, 32, 32, 10)), ("coma_shift_columns_workspace_bytes", (8, 12, 8, 12, 32, 32, 0)),
    ("coma_shift_columns_workspace_bytes", (8, 12, 8, 12, 32, 0, 10)), ("coma_shift_columns_workspace_bytes", (8, _BIG, 8, 12, 32, 32, 10)),
]
# the texts the status functions report after a refusal on the device: one fail(COMA_E_INVALID site each
STATUS_TEXTS = {
    "coma_raster_status": ["non-finite vertex (depth map untouched)", "a snapped coordinate exceeds +-2^25 (1/256-pixel units; depth map untouched)",
                           "face index outside [0, V) (depth map untouched)"],
    "coma_intersection_status": ["non-finite vertex (sums untouched)", "a snapped coordinate exceeds +-2^25 (1/256-cell units; sums untouched)",
                                 "face index outside [0, V) (sums untouched)", "non-finite or beyond +-2^40 (1/256-cell units; sums untouched)",
                                 "capacity exceeded, %d crossings needed (sums untouched)"],
    "coma_shift_columns_status": ["non-finite vertex (nothing written)", "a snapped coordinate exceeds +-2^25 (1/256-cell units; nothing written)",
                                  "face index outside [0, V) (nothing written)", "non-finite or beyond +-2^40 (1/256-cell units; nothing written)",
                                  "capacity exceeded, %d crossings needed (nothing written)"],
    "coma_depth_optimize_status": ["cand_view holds an index outside [0, n_views) (met in epoch %d; nothing written for it, later epochs not run)",
                                   "the columns workspace holds a refused call (nothing written)", "d is not finite after epoch %d (later epochs not run)"],
}


CAMERA_ROWS = 1           # coma_raster_depth_f64's "non-finite camera": R and t are host memory, the tests run that row with a NaN in R


def argument_check_sites():
    """(sites the rows above cover: distinct (entry point, text) pairs, every row of one site carries the same text;
    fail(COMA_E_INVALID sites in the three files)"""
    import os
    import re
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "coma_amd", "csrc")
    sites = sum(len(re.findall(r"fail\(COMA_E_INVALID", open(os.path.join(root, f)).read())) for f in ("raster.hip", "mesh_volume.hip", "depth_opt.hip"))
    # the two depth optimisers share one check function that takes their name: each of its sites is one site of either entry point
    depth = open(os.path.join(root, "depth_opt.hip")).read()
    shared = re.search(r"\nstatic int depth_optimize_check\(.*?\n}\n", depth, re.S).group(0)
    sites += (len(re.findall(r"depth_optimize_check\(who,", depth)) - 1) * len(re.findall(r"fail\(COMA_E_INVALID", shared))
    host = {(e, t) for e, (_, rows) in REFUSALS.items() for t, _ in rows}
    return len(host) + CAMERA_ROWS + len(STATUS_REFUSALS) + sum(len(v) for v in STATUS_TEXTS.values()), sites


def refusal_branches():
    """the regimes the DEVICE_REFUSALS rows reach, from what the restatement says of each row's own data"""
    b = set()
    for kind, text, _, entries in DEVICE_REFUSALS:
        for mesh in (0, 1):
            for entry in entries:
                said = refusal_reached(kind, mesh, entry)
                assert said is not None and (text in said or said in text), (kind, mesh, entry, said)
                d = refusal_data(kind, mesh)
                if "non-finite vertex" in said:
                    b.add("refused-nonfinite-vertex")
                elif "snapped" in said:
                    b.add("refused-scale-overflow" if not np.isfinite(32.0 / d["scale"]) else "snap-beyond-2^25")
                elif "face index" in said:
                    b.add("refused-face-index")
                elif "capacity" in said:
                    b.add("refused-capacity")
                else:
                    z = (d["A"], d["B"])[mesh][0][:, 2]
                    b.add("Z-beyond-2^40" if np.abs(z * 256.0).max() == ZLIM + 1 else "Z-non-finite")
    return b


def with_host_arrays(resolve, nan=False):
    """R, t and front are read on the host: real memory for them (the identity's first nine doubles serve all three), `nan`: a NaN in it"""
    import ctypes
    arr = (ctypes.c_double * 9)(1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, NAN if nan else 1.0)
    out = lambda name: ctypes.addressof(arr) if name in HOST_ARGS else resolve(name)
    out.keep = (arr, resolve)
    return out


def run_plain_refusals(lib, resolve):
    """the rows kit.check_refusals does not take: the camera row, the status functions' null pointer, the size functions' 0 -> their number"""
    rc = kit.call(lib, "coma_raster_depth_f64", dict(_RAST), with_host_arrays(resolve, nan=True))
    assert rc == kit.COMA_E_INVALID and "non-finite camera" in lib.coma_last_error().decode()
    for entry, args, text in STATUS_REFUSALS:
        assert getattr(lib, entry)(*args) == kit.COMA_E_INVALID and text in lib.coma_last_error().decode(), entry
    for entry, args in SIZE_REFUSALS:
        assert getattr(lib, entry)(*args) == 0, (entry, args)
    assert lib.coma_raster_workspace_bytes(8, 12) == 64 + 8 * 16 + 12 * 16 and lib.coma_mesh_volume_workspace_bytes(65537) == 256 * 8
    return CAMERA_ROWS + len(STATUS_REFUSALS) + len(SIZE_REFUSALS)
