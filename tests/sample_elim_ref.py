"""NumPy f64 restatement of weighted sample elimination as coma_sample_eliminate_f64 defines it (include/coma_hip.h); the device
result must equal this one index for index.  Like tests/clip_ref.py and tests/rowtile_ref.py it shares no code with the package.

    d_ij = sqrt(((xi-xj)^2 + (yi-yj)^2) + (zi-zj)^2)          pairs with d_ij >= r_max contribute nothing
    w_ij = ((t*t)^2)^2,  t = 1 - max(d_ij, r_min)/r_max       (alpha = 8)
    w_i  = sum of w_ij over j != i, in ASCENDING j            (a sequential sum: np.cumsum, never np.sum, which sums pairwise)
    until n_keep points are alive: the alive point of largest w goes (np.argmax: the first maximum = the lowest index) and every
    alive neighbour j of it gets one  w_j -= w_ij.

w_ij is a function of the pair alone, so the matrix rows computed for the initial sum are kept (sparse) and reused by the loop.
Above DENSE_MAX_M points the [M,M] matrix is not formed: a k-d tree lists, per point, a SUPERSET of its neighbours (radius
r_max (1 + 1e-9)), and the same exact expressions and the same `d < r_max` test run on that list in ascending j -- a pair outside
the list has d >= r_max and contributes nothing either way (tests/test_sample_elim_host.py compares the two routes bit for bit).

Also here, shared by the CPU and the GPU tests: the radii as the host computes them, the three test meshes, the candidate draw.
"""
import numpy as np

DENSE_MAX_M = 16384


def pair_weights(p, q, r_max, r_min):
    """w_ij for points p [A,3] against q [B,3] -> ([A,B] f64 weights, [A,B] bool `d < r_max`); 0 where the pair contributes nothing."""
    dx, dy, dz = (p[:, None, k] - q[None, :, k] for k in range(3))
    d = np.sqrt(((dx * dx) + (dy * dy)) + (dz * dz))
    near = d < r_max
    t = 1.0 - np.maximum(d, r_min) / r_max
    t2 = t * t
    t4 = t2 * t2
    return np.where(near, t4 * t4, 0.0), near


def sample_eliminate(points, n_keep, r_max, r_min, alpha=8.0, return_weights=False, dense=None):
    points = np.ascontiguousarray(points, dtype=np.float64)
    M = len(points)
    assert alpha == 8 and 1 <= n_keep <= M and r_max > 0 and 0 <= r_min < r_max
    if n_keep == M:
        return np.arange(M, dtype=np.int64)
    w = np.zeros(M)
    nbr_idx, nbr_w = [None] * M, [None] * M
    rows = max(1, (1 << 22) // M)
    if dense is None:
        dense = M <= DENSE_MAX_M
    if not dense:
        from scipy.spatial import cKDTree
        lists = cKDTree(points).query_ball_point(points, r_max * (1.0 + 1e-9), return_sorted=True)
        for i in range(M):
            j = np.asarray(lists[i], dtype=np.int64)
            j = j[j != i]
            wij, near = pair_weights(points[i:i + 1], points[j], r_max, r_min)
            nbr_idx[i], nbr_w[i] = j[near[0]], wij[0][near[0]]
            w[i] = np.cumsum(nbr_w[i])[-1] if len(nbr_w[i]) else 0.0
    for i0 in range(0, M if dense else 0, rows):
        blk, near = pair_weights(points[i0:i0 + rows], points, r_max, r_min)
        for r in range(len(blk)):
            blk[r, i0 + r], near[r, i0 + r] = 0.0, False            # j != i; adding 0.0 for a pair that contributes nothing changes no sum
            nbr_idx[i0 + r] = np.flatnonzero(near[r])
            nbr_w[i0 + r] = blk[r, nbr_idx[i0 + r]]
        w[i0:i0 + rows] = np.cumsum(blk, axis=1)[:, -1]             # sequential, ascending j
    w0 = w.copy()
    alive = np.ones(M, dtype=bool)
    for _ in range(M - n_keep):
        i = int(np.argmax(np.where(alive, w, -np.inf)))
        alive[i] = False
        j = nbr_idx[i]
        m = alive[j]
        w[j[m]] -= nbr_w[i][m]                                      # one subtraction per alive neighbour (indices are distinct)
    keep = np.flatnonzero(alive).astype(np.int64)
    return (keep, w0) if return_weights else keep


def mean_nn_distance(points):
    """Mean distance of each point to its nearest other point."""
    from scipy.spatial import cKDTree
    d, _ = cKDTree(points).query(points, k=2)
    return float(d[:, 1].mean())


# ---------------------------------------------------------------------------------------------- shared test material
def radii(area, n, m, beta=0.5, gamma=1.5):
    """r_max, r_min as the host computes them ([3rd-party, from memory of open3d's source, unpinned])."""
    r_max = 2.0 * float(np.sqrt((area / n) / (2.0 * np.sqrt(3.0))))
    return r_max, r_max * beta * (1.0 - (n / m) ** gamma)


def mesh_area(verts, faces):
    a, b, c = (verts[faces[:, k]] for k in range(3))
    return float((0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)).sum())


def grid_box(n=9):
    """The closed box of tests/test_cli_gpu.py: six n x n vertex grids, two triangles per cell."""
    g = np.linspace(-0.5, 0.5, n)
    verts, faces = [], []
    for axis in range(3):
        for val in (0.5, -0.5):
            base = len(verts)
            ax = [i for i in range(3) if i != axis]
            for a in g:
                for b in g:
                    p = [0.0, 0.0, 0.0]
                    p[axis], p[ax[0]], p[ax[1]] = val, a, b
                    verts.append(p)
            for i in range(n - 1):
                for j in range(n - 1):
                    q = base + i * n + j
                    tri = [[q, q + 1, q + n + 1], [q, q + n + 1, q + n]]
                    faces.extend(tri if val > 0 else [t[::-1] for t in tri])
    return np.array(verts, dtype=np.float64), np.array(faces, dtype=np.int64)


def uv_sphere(rings=12, segs=20, radius=0.7):
    verts = [[0.0, 0.0, radius]]
    for r in range(1, rings):
        th = np.pi * r / rings
        verts += [[radius * np.sin(th) * np.cos(2 * np.pi * s / segs), radius * np.sin(th) * np.sin(2 * np.pi * s / segs), radius * np.cos(th)]
                  for s in range(segs)]
    verts.append([0.0, 0.0, -radius])
    faces = [[0, 1 + s, 1 + (s + 1) % segs] for s in range(segs)]
    for r in range(rings - 2):
        a, b = 1 + r * segs, 1 + (r + 1) * segs
        for s in range(segs):
            t = (s + 1) % segs
            faces += [[a + s, b + s, b + t], [a + s, b + t, a + t]]
    last, b = len(verts) - 1, 1 + (rings - 2) * segs
    faces += [[last, b + (s + 1) % segs, b + s] for s in range(segs)]
    return np.array(verts, dtype=np.float64), np.array(faces, dtype=np.int64)


def big_face_with_slivers(slivers=40):
    """One triangle that holds almost all of the area, and a fan of long thin triangles hanging off one of its edges."""
    verts = [[0.0, 0.0, 0.0], [4.0, 0.0, 0.0], [0.0, 4.0, 0.0]]
    faces = [[0, 1, 2]]
    for k in range(slivers):
        x = 4.0 * (k + 0.5) / slivers
        base = len(verts)
        verts += [[x, 0.0, 0.0], [x + 1e-3, 0.0, 0.0], [x, -0.3, 1.0 + 0.01 * k]]
        faces.append([base, base + 2, base + 1])
    return np.array(verts, dtype=np.float64), np.array(faces, dtype=np.int64)


MESHES = {"grid_box": grid_box, "uv_sphere": uv_sphere, "big_face_slivers": big_face_with_slivers}


def uniform_points(verts, faces, count, seed):
    """Seeded area-weighted uniform surface points (the draw of coma_amd.downsample.sample_uniform, restated)."""
    rng = np.random.default_rng(seed)
    a, b, c = (verts[faces[:, k]] for k in range(3))
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    f = rng.choice(len(faces), size=count, p=area / area.sum())
    r1, r2 = np.sqrt(rng.random(count)), rng.random(count)
    w = np.stack([1 - r1, r1 * (1 - r2), r1 * r2], axis=1)
    return (w[:, :, None] * verts[faces[f]]).sum(1)


def case(mesh, n, seed, init_factor=5):
    """(candidates [5n,3], r_max, r_min) of one test case."""
    verts, faces = MESHES[mesh]()
    m = init_factor * n
    return (uniform_points(verts, faces, m, seed),) + radii(mesh_area(verts, faces), n, m)
