"""CPU: depth initialisation's host arithmetic against the values recorded from the reference's own functions
(tests/golden/depth_init_golden.npz, written by tests/golden/make_golden_depth_init.py), the selection rule driven by the recorded
integer counts, and the properties of the rasteriser rule set on its NumPy restatement (tests/raster_ref.py)."""
import os

import numpy as np
import pytest

from tests import raster_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(ROOT, "tests", "golden", "depth_init_golden.npz"), allow_pickle=False)


def _cases(fx):
    return [str(t) for t in fx["cases"]]


def camera_of(fx, t):
    return dict(R=fx[f"{t}_cam_R"], t=fx[f"{t}_cam_t"], scale=float(fx[f"{t}_cam_scale"]), resolution=tuple(int(x) for x in fx[f"{t}_cam_resolution"]),
                obj_R=fx[f"{t}_cam_obj_R"], obj_t=fx[f"{t}_cam_obj_t"])


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def test_fixture_holds_the_cases_the_selection_rule_needs(fx):
    tied, none, skipped = False, False, False
    for t in _cases(fx):
        vis, inter, uni = fx[f"{t}_visible"], fx[f"{t}_inter"], fx[f"{t}_uni"]
        if f"{t}_saved" in fx:
            none |= int(vis.sum()) == 0
            continue
        iou = [int(i) / int(u) for i, u, v in zip(inter, uni, vis) if v > 0]
        tied |= sorted(iou)[-1] == sorted(iou)[-2]
        skipped |= bool((vis == 0).any())
    assert tied and none and skipped
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "depth_init_golden.npz")) < (1 << 20)


def test_host_functions_equal_the_reference_bit_for_bit(fx):
    from coma_amd import depth_init as D
    for t in _cases(fx):
        direction = fx[f"{t}_direction"]
        size = D.compute_directional_size(mesh_verts=fx[f"{t}_size_verts"], direction=direction)
        assert same_bits(size, fx[f"{t}_directional_size"]), t
        nearest, distance = D.compute_nearest_point(asset_verts=fx[f"{t}_asset_verts"], point=fx[f"{t}_pelvis"], direction=direction)
        assert nearest.shape == (3, 1) and same_bits(nearest, fx[f"{t}_nearest_point"]), t
        assert isinstance(distance, float) and same_bits(distance, fx[f"{t}_distance_from_point"]), t
        ratio, rng = float(fx[f"{t}_params"][0]), int(fx[f"{t}_params"][1])
        disp = D.candidate_displacements(distance, size * ratio, rng)
        assert len(disp) == 2 * rng + 1 and same_bits(disp, fx[f"{t}_displacements"]), t
        cands = D.extract_candidates(fx[f"{t}_human_verts"], fx[f"{t}_human_faces"], fx[f"{t}_asset_verts"], fx[f"{t}_asset_faces"], disp, direction, 9, 1000)
        assert same_bits(np.stack([c["verts"] for c in cands]), fx[f"{t}_cand_verts"]), t
        assert same_bits(np.stack([c["displacement"] for c in cands]), fx[f"{t}_cand_disp"]), t
        assert all(c["faces"] is cands[0]["faces"] for c in cands) and cands[0]["displacement"].shape == (1, 3)
    with pytest.raises(NotImplementedError):
        D.extract_candidates(np.zeros((3, 3)), np.zeros((1, 3), int), np.zeros((3, 3)), np.zeros((1, 3), int), [0.0], np.ones(3), 9, 1000, filter_out=True)


def test_cli_transforms_equal_the_reference_bit_for_bit(fx):
    from src.generation import initialize_depth as cli
    from constants.generation.assets import CATEGORY2DATASET_TYPE
    for t in _cases(fx):
        cam = camera_of(fx, t)
        verts, pelvis = cli.human_world(fx[f"{t}_pred_verts"], fx[f"{t}_pred_pelvis"], cam, cam["resolution"])
        assert same_bits(verts, fx[f"{t}_human_verts"]) and same_bits(pelvis, fx[f"{t}_pelvis"]), t
        sc, c, _ = (str(x) for x in fx[f"{t}_category"])
        assert same_bits(cli.asset_world(fx[f"{t}_asset_co"], cam, CATEGORY2DATASET_TYPE[(sc, c)]), fx[f"{t}_asset_verts"]), t
    # the OBJ file's vertices enter the chain unchanged (as in optimize_depth.py:639-659): y up becomes z up ONCE, in asset_world
    cam = dict(obj_R=np.eye(3), obj_t=np.zeros((3, 1)))
    assert cli.asset_world(np.array([[1.0, 2.0, 3.0], [0.0, 0.0, 0.0]]), cam, "3D-FUTURE").tolist() == [[1.0, -3.0, 2.0], [0.0, 0.0, 0.0]]
    assert not hasattr(cli, "blender_obj_import")


def test_selection_rule_on_the_recorded_counts(fx):
    from coma_amd import depth_init as D
    for t in _cases(fx):
        vis, inter, uni = fx[f"{t}_visible"], fx[f"{t}_inter"], fx[f"{t}_uni"]
        K = len(vis)
        cands = [dict(idx=k, IoU=int(inter[k]) / int(uni[k]), interval_from_center=np.abs(k - K)) for k in range(K) if vis[k] > 0]
        got = D.choose(cands)
        if f"{t}_saved" in fx:
            assert got is None and str(fx[f"{t}_saved"]) == "ERRONEOUS SAMPLE DUE TO TOO SMALL HUMAN", t
        else:
            assert got["idx"] == int(fx[f"{t}_sel_idx"]) and got["IoU"] == float(fx[f"{t}_sel_IoU"]), t
            assert got["interval_from_center"] == int(fx[f"{t}_sel_interval"]) == K - got["idx"], t      # len, not len // 2


def test_restatement_reproduces_the_recorded_renders(fx):
    """The fixture's counts come from K two-mesh renders of the shifted copies; one human map, one asset map and K offsets give the same."""
    from coma_amd import depth_init as D
    for t in _cases(fx):
        cam = camera_of(fx, t)
        W, H = cam["resolution"]
        cands = [dict(displacement=d) for d in fx[f"{t}_cand_disp"]]
        hk = RR.raster_depth(fx[f"{t}_cand_verts"][0], fx[f"{t}_human_faces"], cam["R"], cam["t"], cam["scale"], W, H)
        ak = RR.raster_depth(fx[f"{t}_asset_verts"], fx[f"{t}_asset_faces"], cam["R"], cam["t"], cam["scale"], W, H)
        vis, inter, uni, masks = RR.silhouette_iou(hk, ak, D.depth_offsets(cands, cam), D.person_mask(fx[f"{t}_gt"]))
        assert vis.tolist() == fx[f"{t}_visible"].tolist(), t
        seen = vis > 0
        assert inter[seen].tolist() == fx[f"{t}_inter"][seen].tolist() and uni[seen].tolist() == fx[f"{t}_uni"][seen].tolist(), t
        if f"{t}_saved" not in fx:
            assert np.array_equal(masks[int(fx[f"{t}_sel_idx"])], fx[f"{t}_sel_segmentation"]), t


def test_person_mask_conversion():
    from coma_amd import depth_init as D
    assert D.person_mask(np.array([[True, False]])).tolist() == [[1, 0]]
    assert D.person_mask(np.array([[255, 254, 1, 0]], dtype=np.uint8)).tolist() == [[1, 0, 0, 0]]


# ---- the rule set, on the restatement ----
EYE = dict(R=np.diag([1.0, -1.0, -1.0]), t=np.zeros(3))      # camera space == world space: x right, y down, z away


def _draw(verts, faces, W=32, H=32, scale=32.0, cam=EYE):
    return RR.raster_depth(np.asarray(verts, dtype=np.float64), np.asarray(faces), cam["R"], cam["t"], scale, W, H)


def test_quad_split_along_either_diagonal_covers_what_the_rectangle_covers():
    rng = np.random.default_rng(0)
    for _ in range(40):
        x0, y0 = rng.integers(-20 * 256, 10 * 256, 2) / 256.0
        x1, y1 = x0 + rng.integers(1, 30 * 256) / 256.0, y0 + rng.integers(1, 30 * 256) / 256.0
        if rng.random() < 0.5:                                 # corners on pixel centres: the tie rule decides
            x0, y0, x1, y1 = np.floor(x0) + 0.5, np.floor(y0) + 0.5, np.floor(x1) + 0.5, np.floor(y1) + 0.5
        v = [[x0, y0, 1.0], [x1, y0, 1.0], [x1, y1, 1.0], [x0, y1, 1.0]]
        a = _draw(v, [[0, 1, 2], [0, 2, 3]]) != RR.EMPTY
        b = _draw(v, [[0, 1, 3], [1, 2, 3]]) != RR.EMPTY
        # pixel centres i + 0.5 (screen = world + 16) with x0 <= centre < x1: left and top edges own their samples
        cx = np.arange(32) + 0.5 - 16.0
        want = ((cx >= y0) & (cx < y1))[:, None] & ((cx >= x0) & (cx < x1))[None, :]
        assert np.array_equal(a, want) and np.array_equal(b, want)


def test_shared_edges_are_hit_exactly_once():
    """A 5 x 5 patch of 6-pixel cells whose inner vertices are moved by up to a pixel in half-pixel steps (so that edges and
    vertices fall ON pixel centres), every cell split along a random diagonal: each centre of the patch is hit exactly once."""
    rng = np.random.default_rng(1)
    for _ in range(10):
        gy, gx = np.mgrid[0:6, 0:6]
        p = np.stack([gx * 6.0 - 14.5, gy * 6.0 - 14.5], axis=-1)
        p[1:5, 1:5] += rng.integers(-2, 3, (4, 4, 2)) * 0.5
        v = np.concatenate([p.reshape(-1, 2), np.ones((36, 1))], axis=1)
        faces = []
        for j in range(5):
            for i in range(5):
                a, b, c, d = j * 6 + i, j * 6 + i + 1, (j + 1) * 6 + i + 1, (j + 1) * 6 + i
                faces += [[a, b, c], [a, c, d]] if rng.random() < 0.5 else [[a, b, d], [d, c, b]]      # mixed windings too
        hits = sum((_draw(v, [f]) != RR.EMPTY).astype(int) for f in faces)
        want = np.zeros((32, 32), int)
        want[1:31, 1:31] = 1                                   # centres i + 0.5 - 16 in [-14.5, 15.5): the left / top edge owns its samples
        assert np.array_equal(hits, want)


def test_mirrored_winding_gives_identical_output():
    v, f = RR.icosphere(2, 0.31, (0.02, -0.05, 1.0))
    cam = dict(R=RR.look_at((1.0, -2.0, 1.5), (0.0, 0.0, 1.0)), t=np.array([1.0, -2.0, 1.5]))
    a = RR.raster_depth(v, f, cam["R"], cam["t"], 1.0, 48, 40)
    b = RR.raster_depth(v, f[:, [0, 2, 1]], cam["R"], cam["t"], 1.0, 48, 40)      # the swap the rule undoes: the same keys
    assert (a != RR.EMPTY).sum() > 100 and np.array_equal(a, b)
    c = RR.raster_depth(v, f[:, ::-1], cam["R"], cam["t"], 1.0, 48, 40)           # reversed: another order of the depth sum, same coverage
    assert np.array_equal(a != RR.EMPTY, c != RR.EMPTY)
    assert np.abs(RR.key_to_depth(a[a != RR.EMPTY]) - RR.key_to_depth(c[a != RR.EMPTY])).max() < 1e-14


def test_known_vertex_lands_in_the_known_pixel_x_right_y_down():
    eye = np.array([0.0, -5.0, 0.0])
    R = RR.look_at(eye, (0.0, 0.0, 0.0))                       # looks along +y; world x is to the right, world z is up
    s = 0.01

    def dot(p):
        p = np.asarray(p, dtype=np.float64)
        return np.array([p + [-s, 0, -s], p + [s, 0, -s], p + [0, 0, s]]), np.array([[0, 1, 2]])
    for p, (col, row) in (((0.0, 0.0, 0.0), (32, 32)), ((1.0, 0.0, 0.0), (48, 32)), ((0.0, 0.0, 1.0), (32, 16)), ((-1.5, 3.0, -0.5), (8, 40))):
        v, f = dot(np.array(p) + [s * 3.125, 0, -s * 3.125])     # a small triangle around the centre of pixel (col, row)
        k = RR.raster_depth(v, f, R, eye, 4.0, 64, 64)          # 16 pixels per world unit
        ys, xs = np.nonzero(k != RR.EMPTY)
        assert (xs.tolist(), ys.tolist()) == ([col], [row]), (p, xs, ys)
        assert abs(float(RR.key_to_depth(k[row, col])[0]) - (5.0 + p[1])) < 1e-12           # depth = distance along the view, larger is farther
    # non-square image: the scale spans the larger side
    v, f = dot(np.array((1.0, 0.0, 0.5)) + [s * 3.125, 0, -s * 3.125])
    ys, xs = np.nonzero(RR.raster_depth(v, f, R, eye, 4.0, 64, 32) != RR.EMPTY)
    assert (xs.tolist(), ys.tolist()) == ([48], [8])


def test_icosphere_pixel_count_is_within_one_perimeter_of_the_disc():
    for r_px, sub in ((20.3, 3), (57.7, 4), (9.1, 2)):
        v, f = RR.icosphere(sub, r_px / 128.0 * 2.0, (0.013, 0.021, 3.0))
        n = int((_draw(v, f, 128, 128, 2.0) != RR.EMPTY).sum())
        # the faceted silhouette lies inside the circle by at most r (1 - cos(pi / n_edge)) < one pixel at these subdivisions
        assert abs(n - np.pi * r_px ** 2) <= 2 * np.pi * r_px, (r_px, n, np.pi * r_px ** 2)


def test_key_order_and_refusals():
    z = np.array([-np.inf, -3.5, -0.0, 0.0, 1e-300, 2.0, np.inf])
    k = RR.depth_to_key(z)
    assert (np.diff(k.astype(object)) > 0).all() and (k != RR.EMPTY).all() and RR.key_to_depth(k).tobytes() == z.tobytes()
    tri = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 1.0], [0.0, 1.0, 1.0]])
    for bad in (np.nan, np.inf):
        v = tri.copy()
        v[1, 2] = bad
        with pytest.raises(RR.Refused, match="non-finite"):
            _draw(v, [[0, 1, 2]])
    v = tri.copy()
    v[2, 0] = 2.0 ** 25 / 256.0 + 1.0
    with pytest.raises(RR.Refused, match="exceeds"):
        _draw(v, [[0, 1, 2]])
    with pytest.raises(RR.Refused, match="face index"):
        _draw(tri, [[0, 1, 3]])
    assert (_draw(tri, [[0, 1, 1], [2, 2, 2]]) == RR.EMPTY).all()            # zero area: skipped


def test_silhouette_counts_front_to_back_null_asset_and_exact_tie():
    human = RR.icosphere(2, 6.0, (0.0, 0.0, 20.0))
    wall = (np.array([[-40.0, -40.0, 20.0], [40.0, -40.0, 20.0], [40.0, 40.0, 20.0], [-40.0, 40.0, 20.0]]), np.array([[0, 1, 2], [0, 2, 3]]))
    hk, ak = _draw(*human), _draw(*wall)
    gt = np.zeros((32, 32), np.uint8)
    gt[10:20, 8:30] = 1
    off = np.linspace(-7.0, 7.0, 7)
    vis, inter, uni, masks = RR.silhouette_iou(hk, ak, off, gt)
    full = int((hk != RR.EMPTY).sum())
    assert vis[0] == full and vis[-1] == 0 and (np.diff(vis) <= 0).all() and 0 < vis[4] < full
    assert all(uni[k] == int(gt.sum()) + vis[k] - inter[k] for k in range(7)) and masks.shape == (7, 32, 32) and set(np.unique(masks)) == {0, 255}
    v0, i0, u0, _ = RR.silhouette_iou(hk, None, off, gt)
    assert (v0 == full).all() and (i0 == i0[0]).all() and (u0 == u0[0]).all()
    v1, _, _, _ = RR.silhouette_iou(hk, hk, [0.0, -1e-9], gt)     # the human against itself: an exact tie goes to the asset
    assert v1.tolist() == [0, full]
