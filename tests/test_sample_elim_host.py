"""CPU: the NumPy restatement of weighted sample elimination (tests/sample_elim_ref.py) on cases worked by hand, and the host
surface of the opt-in device sampler (parser flags, the `sampler` keyword).  No kernel is launched here."""
import numpy as np
import pytest

from tests import sample_elim_ref as R


def _w(d, r_max, r_min):
    t = 1.0 - max(d, r_min) / r_max
    return ((t * t) ** 2) ** 2


def test_four_collinear_points_by_hand():
    """x = 0, 1, 2, 4 with r_max 2.5, r_min 0.5.  Pairs inside the radius: (0,1) (1,2) at d 1, (0,2) (2,3) at d 2; d 3 and 4 are out.
    With a = w(1) = 0.6^8, b = w(2) = 0.2^8:  w = [a+b, 2a, a+2b, b]  ->  point 1 goes first (2a is the largest);
    then w = [b, -, 2b, b] up to rounding  ->  point 2 goes;  survivors 0 and 3."""
    pts = np.array([[0.0, 0, 0], [1.0, 0, 0], [2.0, 0, 0], [4.0, 0, 0]])
    r_max, r_min = 2.5, 0.5
    a, b = _w(1.0, r_max, r_min), _w(2.0, r_max, r_min)
    keep, w0 = R.sample_eliminate(pts, 2, r_max, r_min, return_weights=True)
    assert w0.tolist() == [a + b, a + a, (a + b) + b, b]          # ascending j: point 2 sums (0,2), (1,2), (2,3) in that order
    assert keep.tolist() == [0, 3] and keep.dtype == np.int64
    assert R.sample_eliminate(pts, 3, r_max, r_min).tolist() == [0, 2, 3]


def test_last_tie_goes_to_the_lowest_index():
    """Isolated points: every w is 0 and stays 0, so each step is a tie and removes the lowest alive index."""
    pts = np.array([[10.0 * k, 0, 0] for k in range(6)])
    assert R.sample_eliminate(pts, 2, 1.0, 0.25).tolist() == [4, 5]


def test_ties_and_r_min_clamp_on_duplicates():
    """Three copies of one point and one point far away: d = 0 is clamped to r_min, so each copy weighs 2 (1 - r_min/r_max)^8 and the
    three tie; the lowest index goes first, then the next."""
    pts = np.array([[1.0, 2, 3], [1.0, 2, 3], [9.0, 9, 9], [1.0, 2, 3]])
    r_max, r_min = 1.0, 0.5
    keep, w0 = R.sample_eliminate(pts, 3, r_max, r_min, return_weights=True)
    c = _w(0.0, r_max, r_min)
    assert c == 0.5 ** 8 and w0.tolist() == [c + c, c + c, 0.0, c + c]
    assert keep.tolist() == [1, 2, 3]
    assert R.sample_eliminate(pts, 2, r_max, r_min).tolist() == [2, 3]     # w = [-, c, 0, c] -> index 1 goes
    # without the clamp the copies would weigh 2 each: the clamp is what keeps a duplicate from dominating
    assert R.sample_eliminate(pts, 3, r_max, 0.0, return_weights=True)[1].tolist() == [2.0, 2.0, 0.0, 2.0]


def test_n_keep_equals_m():
    pts = np.random.default_rng(0).random((17, 3))
    assert R.sample_eliminate(pts, 17, 0.3, 0.1).tolist() == list(range(17))


def test_pair_at_exactly_r_max_contributes_nothing():
    pts = np.array([[0.0, 0, 0], [2.0, 0, 0], [3.5, 0, 0]])
    assert R.sample_eliminate(pts, 3 - 1, 2.0, 0.5, return_weights=True)[1].tolist() == [0.0, _w(1.5, 2.0, 0.5), _w(1.5, 2.0, 0.5)]


def test_kdtree_route_equals_dense_route():
    pts = np.random.default_rng(3).random((1500, 3))
    a = R.sample_eliminate(pts, 300, 0.11, 0.04, return_weights=True, dense=True)
    b = R.sample_eliminate(pts, 300, 0.11, 0.04, return_weights=True, dense=False)
    assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("mesh", sorted(R.MESHES))
def test_restatement_spreads_points_wider_than_uniform(mesh):
    """The condition of the GPU quality test, on the restatement alone: same mesh, same N, mean nearest-neighbour distance strictly
    larger than that of the uniform draw."""
    verts, faces = R.MESHES[mesh]()
    for seed in (0, 1, 2):
        pts, r_max, r_min = R.case(mesh, 200, seed)
        keep = R.sample_eliminate(pts, 200, r_max, r_min)
        assert R.mean_nn_distance(pts[keep]) > R.mean_nn_distance(R.uniform_points(verts, faces, 200, seed))


def test_host_radii_and_candidate_draw_match_the_restatement():
    from coma_amd import downsample as ds
    verts, faces = R.grid_box()
    assert ds.poisson_radii(R.mesh_area(verts, faces), 100, 500) == R.radii(R.mesh_area(verts, faces), 100, 500)
    assert np.array_equal(ds.sample_uniform(verts, faces, np.ones_like(verts), 64, 7)[0], R.uniform_points(verts, faces, 64, 7))
    assert (ds.POISSON_INIT_FACTOR, ds.POISSON_ALPHA, ds.POISSON_BETA, ds.POISSON_GAMMA) == (5, 8.0, 0.5, 1.5)


def test_parsers_accept_sampler_and_default_to_supplied():
    from src.coma import downsample_human as dh, downsample_objects as do
    assert dh.build_parser().parse_args([]).sampler == "supplied"
    assert dh.build_parser().parse_args(["--sampler", "device"]).sampler == "device"
    req = ["--supercategory", "S", "--category", "C", "--asset_id", "a", "--obj_pth", "x.obj"]
    assert do.build_parser().parse_args(req).sampler == "supplied"
    assert do.build_parser().parse_args(req + ["--sampler", "device"]).sampler == "device"
    with pytest.raises(SystemExit):
        dh.build_parser().parse_args(["--sampler", "open3d"])


def test_supplied_sampler_still_refuses_poisson_disk_without_points():
    from coma_amd.downsample import _points
    verts, faces = R.grid_box(3)
    with pytest.raises(NotImplementedError):
        _points(verts, faces, np.ones_like(verts), 10, None, None, simplify_method="poisson_disk", seed=0, sampler="supplied")
    with pytest.raises(NotImplementedError):
        _points(verts, faces, np.ones_like(verts), 10, None, None, "poisson_disk", 0)          # the default is "supplied"
    p, n = _points(verts, faces, np.ones_like(verts), 10, np.zeros((4, 3)), np.ones((4, 3)), "poisson_disk", 0, sampler="device")
    assert p.shape == (4, 3) and n.shape == (4, 3)                                              # supplied points win
    with pytest.raises(AssertionError):
        _points(verts, faces, np.ones_like(verts), 10, None, None, "poisson_disk", 0, sampler="open3d")
