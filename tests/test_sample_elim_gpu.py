"""GPU: coma_sample_eliminate_f64 through the C ABI against the NumPy restatement (tests/sample_elim_ref.py) -- every index equal,
no tolerance -- its refusals, and the opt-in device sampler of the two down-sampling writers end to end."""
import ctypes as C
import functools
import pickle
import types

import numpy as np
import pytest

from tests import sample_elim_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEEDS = (0, 1, 2)
SENTINEL = -7


def _call(lib, points, n_keep, r_max, r_min, alpha=8.0, keep_len=None):
    """One call through the ctypes table; returns (rc, keep_idx as NumPy).  keep_idx is pre-filled with SENTINEL."""
    import torch
    from coma_amd import _lib
    pts = torch.tensor(np.ascontiguousarray(points, dtype=np.float64), device=DEV)
    M = pts.shape[0]
    ws = torch.empty([max(1, lib.coma_sample_eliminate_workspace_bytes(M) // 8)], dtype=torch.float64, device=DEV)
    keep = torch.full([keep_len if keep_len is not None else n_keep], SENTINEL, dtype=torch.int64, device=DEV)
    rc = lib.coma_sample_eliminate_f64(_lib.ptr(pts), M, n_keep, r_max, r_min, alpha, _lib.ptr(ws), _lib.ptr(keep), _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    return rc, keep.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _reference(mesh, n, seed):
    """The restatement of one (mesh, N, seed) case, computed once per module (M = 10 240 takes seconds on the host)."""
    pts, r_max, r_min = R.case(mesh, n, seed)
    return pts, r_max, r_min, R.sample_eliminate(pts, n, r_max, r_min)


@pytest.mark.parametrize("n", [40, 500, 2048])
@pytest.mark.parametrize("mesh", sorted(R.MESHES))
def test_exact_against_the_restatement(hip_lib, mesh, n):
    for seed in SEEDS:
        pts, r_max, r_min, ref = _reference(mesh, n, seed)
        rc, got = _call(hip_lib, pts, n, r_max, r_min)
        assert rc == 0, hip_lib.coma_last_error()
        mism = int((got != ref).sum())
        print(f"{mesh} N={n} M={len(pts)} seed={seed}: {mism} of {n} indices differ")
        assert np.array_equal(got, ref), f"{mesh} N={n} seed={seed}: {mism} of {n} indices differ from the restatement"


def test_ties_duplicates_and_equal_weights(hip_lib):
    rng = np.random.default_rng(4)
    base = rng.random((300, 3))
    pts = np.concatenate([base, base[:120], base[:40]])[rng.permutation(460)]          # exact duplicates and triplicates
    for n_keep in (300, 100, 7):
        rc, got = _call(hip_lib, pts, n_keep, 0.2, 0.05)
        assert rc == 0 and np.array_equal(got, R.sample_eliminate(pts, n_keep, 0.2, 0.05))
    iso = np.array([[10.0 * (k % 17), 10.0 * (k // 17), 0.0] for k in range(200)])      # isolated points: every weight 0, every step a tie
    rc, got = _call(hip_lib, iso, 50, 1.0, 0.25)
    assert rc == 0 and got.tolist() == list(range(150, 200)) == R.sample_eliminate(iso, 50, 1.0, 0.25).tolist()
    same = np.tile(np.array([[0.25, -1.5, 3.0]]), (130, 1))                             # all points equal: all weights equal
    rc, got = _call(hip_lib, same, 9, 1.0, 0.5)
    assert rc == 0 and np.array_equal(got, R.sample_eliminate(same, 9, 1.0, 0.5))


@pytest.mark.parametrize("M", [1, 63, 1037, 2500])
def test_sizes_off_the_wave_and_workgroup_grid_and_the_two_ends(hip_lib, M):
    pts = np.random.default_rng(M).random((M, 3))
    r_max = 1.5 * (1.0 / M) ** (1.0 / 3.0)
    for n_keep in sorted({1, max(1, M // 5), M}):
        rc, got = _call(hip_lib, pts, n_keep, r_max, 0.3 * r_max)
        assert rc == 0, hip_lib.coma_last_error()
        assert np.array_equal(got, R.sample_eliminate(pts, n_keep, r_max, 0.3 * r_max)), (M, n_keep)
        if n_keep == M:
            assert got.tolist() == list(range(M))


def test_largest_accepted_m(hip_lib):
    M = 65536
    pts = np.random.default_rng(11).random((M, 3))
    rc, got = _call(hip_lib, pts, M - 3, 0.035, 0.01)
    assert rc == 0, hip_lib.coma_last_error()
    assert np.array_equal(got, R.sample_eliminate(pts, M - 3, 0.035, 0.01))


def test_refusals_leave_keep_idx_untouched(hip_lib):
    pts = np.random.default_rng(0).random((100, 3))
    big = np.zeros((65537, 3))
    for what, args, word in (("M > 65536", (big, 10, 0.5, 0.1, 8.0), b"M="),
                             ("n_keep > M", (pts, 101, 0.5, 0.1, 8.0), b"n_keep"),
                             ("n_keep < 1", (pts, 0, 0.5, 0.1, 8.0), b"n_keep"),
                             ("alpha != 8", (pts, 10, 0.5, 0.1, 4.0), b"alpha"),
                             ("r_max <= 0", (pts, 10, 0.0, 0.0, 8.0), b"r_max"),
                             ("r_max < 0", (pts, 10, -1.0, 0.0, 8.0), b"r_max"),
                             ("r_min >= r_max", (pts, 10, 0.5, 0.5, 8.0), b"r_min")):
        rc, keep = _call(hip_lib, *args, keep_len=128)
        assert rc == -1, what
        assert word in hip_lib.coma_last_error(), (what, hip_lib.coma_last_error())
        assert (keep == SENTINEL).all(), what
    assert hip_lib.coma_sample_eliminate_f64(None, 10, 5, 0.5, 0.1, 8.0, None, None, None) == -1
    assert b"null pointer" in hip_lib.coma_last_error()
    assert hip_lib.coma_sample_eliminate_workspace_bytes(1000) >= 8 * 1000 and hip_lib.coma_sample_eliminate_workspace_bytes(0) == 0


def test_two_runs_give_the_same_bytes(hip_lib):
    pts, r_max, r_min, _ = _reference("uv_sphere", 500, 0)
    a, b = _call(hip_lib, pts, 500, r_max, r_min), _call(hip_lib, pts, 500, r_max, r_min)
    assert a[0] == 0 == b[0] and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("mesh", sorted(R.MESHES))
def test_device_sampler_spreads_points_wider_than_uniform(hip_lib, mesh):
    """A condition, not a tolerance: same mesh, same N, mean nearest-neighbour distance strictly larger than the uniform draw's."""
    from coma_amd.downsample import sample_poisson_disk, sample_uniform
    verts, faces = R.MESHES[mesh]()
    nrm = np.ones_like(verts)
    for seed in SEEDS:
        p, pn = sample_poisson_disk(verts, faces, nrm, 500, seed, DEV)
        u, _ = sample_uniform(verts, faces, nrm, 500, seed)
        assert p.shape == (500, 3) == pn.shape
        ref_pts, _, _, ref_keep = _reference(mesh, 500, seed)
        assert np.array_equal(p, ref_pts[ref_keep])                       # kept candidates, ascending candidate order
        dp, du = R.mean_nn_distance(p), R.mean_nn_distance(u)
        print(f"{mesh} seed={seed}: mean nearest-neighbour distance device {dp:.5f} uniform {du:.5f} ratio {dp / du:.3f}")
        assert dp > du


HUMAN_KEYS = {"vertices", "faces", "V", "F", "N", "N_raw", "downsample_indices", "downsampled_pcd_points_raw", "downsampled_pcd_normal_raw"}
OBJECT_KEYS = {"supercategory", "category", "asset_id", "V", "F", "N", "N_raw", "downsample_indices", "downsampled_pcd_points_raw",
               "downsampled_pcd_normal_raw", "obj_vertices_original", "obj_faces_original", "obj_vertex_normals_original"}


def test_writers_end_to_end_with_the_device_sampler(tmp_path, hip_lib):
    from oracle import coma_oracle as orc
    from coma_amd.downsample import downsample_object
    from src.coma import downsample_human as dh, downsample_objects as do
    verts, faces = R.grid_box()
    # object writer, called directly
    N = 180
    o = downsample_object("BEHAVE", "backpack", "behave_asset", verts, faces, N, simplify_method="poisson_disk", seed=3, device=DEV, sampler="device")
    assert set(o) == OBJECT_KEYS
    cand, r_max, r_min = R.case("grid_box", N, 3)
    pts = cand[R.sample_eliminate(cand, N, r_max, r_min)]
    zero = int((o["downsampled_pcd_normal_raw"].sum(1) == 0).sum())
    assert zero == 0 and o["N"] == N and o["N_raw"] == N - zero == len(o["downsampled_pcd_points_raw"])
    assert np.array_equal(o["downsampled_pcd_points_raw"], pts)
    assert o["downsample_indices"] == [int(i) for i in orc.nearest_vertex(o["downsampled_pcd_points_raw"], verts)]
    # object CLI: the namespace carries the flag; without it the same call is still refused
    with open(tmp_path / "box.obj", "w") as h:
        h.writelines(f"v {x} {y} {z}\n" for x, y, z in verts)
        h.writelines(f"f {a + 1} {b + 1} {c + 1}\n" for a, b, c in faces)
    a = types.SimpleNamespace(supercategory="BEHAVE", category="backpack", asset_id="behave_asset", obj_pth=str(tmp_path / "box.obj"),
                              asset_downsample_dir=str(tmp_path / "ads"), num_object_downsample_points_list=[60], simplify_method="poisson_disk",
                              points_pth=None, skip_done=False, debug=False, seed=1, sampler="device")
    out = do.main(a)
    oc = pickle.load(open(out[0], "rb"))
    assert set(oc) == OBJECT_KEYS and oc["N"] == 60 and oc["N_raw"] == 60 - int((oc["downsampled_pcd_normal_raw"].sum(1) == 0).sum())
    a.sampler = "supplied"
    with pytest.raises(NotImplementedError):
        do.main(a)
    # human writer through its CLI function
    with open(tmp_path / "star.pickle", "wb") as h:
        pickle.dump({"vertices": verts.astype(np.float32), "faces": faces}, h)
    args = types.SimpleNamespace(mesh_pth=str(tmp_path / "star.pickle"), points_pth=None, simplify_method="poisson_disk", seed=5, skip_done=False,
                                 save_dir=str(tmp_path / "mesh"), num_human_downsample_points=100, sampler="device")
    d = pickle.load(open(dh.downsample_smplx(args, device=DEV), "rb"))
    assert set(d) == HUMAN_KEYS and d["N_raw"] == 100 and d["N"] == len(d["downsample_indices"]) <= 100
    v64 = verts.astype(np.float32).astype(np.float64)
    assert d["downsample_indices"] == [int(i) for i in orc.nearest_vertex(d["downsampled_pcd_points_raw"], v64)]
    assert len(np.unique(d["downsampled_pcd_points_raw"], axis=0)) == 100
    assert np.allclose(np.linalg.norm(d["downsampled_pcd_normal_raw"], axis=1), 1.0)
