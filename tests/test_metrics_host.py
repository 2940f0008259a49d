"""CPU: the column rule set of the intersection volume (tests/volume_ref.py, the restatement the device is held against) checked
against exact volumes and its integer identities, and the host code of coma_amd.metrics, src/generation/compute_metrics.py and
src/coma/filter.py against values recorded from the reference's own modules (tests/golden/metrics_golden.npz)."""
import json
import os

import numpy as np
import pytest

from tests import metrics_common as MC
from tests import raster_ref as RR
from tests import volume_ref as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Relative error of the restatement's V_AB against the exact intersection volume (SciPy HalfspaceIntersection + ConvexHull.volume),
# measured once on the fixtures of metrics_common.convex_pairs() (DESIGN 9 carries the same table):
#            32^2      64^2      128^2
#   cubes    3.344e-4  3.642e-6  3.238e-5
#   cube_tet 6.822e-5  2.620e-5  3.478e-5
#   spheres  1.625e-3  3.775e-6  2.629e-5
# The bound per resolution is twice the largest entry of its column.  The inputs are deterministic: the margin only guards later
# edits of the fixtures.
RECORDED_WORST = {32: 1.625e-3, 64: 2.620e-5, 128: 3.478e-5}


@pytest.fixture(scope="module")
def golden_metrics():
    return np.load(os.path.join(ROOT, "tests", "golden", "metrics_golden.npz"), allow_pickle=False)


def _exact_convex_intersection(va, vb):
    from scipy.optimize import linprog
    from scipy.spatial import ConvexHull, HalfspaceIntersection
    hs = np.concatenate([ConvexHull(va).equations, ConvexHull(vb).equations])
    A, b = hs[:, :3], -hs[:, 3]
    # Chebyshev centre: an interior point for HalfspaceIntersection
    res = linprog([0, 0, 0, -1], A_ub=np.hstack([A, np.linalg.norm(A, axis=1)[:, None]]), b_ub=b, bounds=[(None, None)] * 3 + [(0, None)])
    assert res.status == 0 and res.x[3] > 1e-9
    return ConvexHull(HalfspaceIntersection(hs, res.x[:3]).intersections).volume


def _columns(A, B, resolution):
    from coma_amd.metrics import overlap_grid
    x0, y0, s, W, H = overlap_grid(A[0], B[0], resolution)
    sums, col_ab, counts = VR.intersection_columns(A[0], A[1], B[0], B[1], x0, y0, s, W, H)
    return sums, col_ab, counts, s


@pytest.mark.parametrize("name", ["cubes", "cube_tet", "spheres"])
def test_restatement_against_exact_convex_intersection(name):
    A, B = MC.convex_pairs()[name]
    exact = _exact_convex_intersection(A[0], B[0])
    err = {}
    for res in (32, 64, 128):
        sums, _, _, s = _columns(A, B, res)
        v_ab, v_a, _ = VR.volumes(sums, s)
        err[res] = abs(v_ab - exact) / exact
        print(f"{name} at {res}^2: V_AB {v_ab:.9f}, exact {exact:.9f}, relative error {err[res]:.3e}")
        assert err[res] <= 2.0 * RECORDED_WORST[res]
    assert err[128] <= err[32]


def test_integer_identities():
    A, B = MC.convex_pairs()["spheres"]
    from coma_amd.metrics import overlap_grid
    x0, y0, s, W, H = overlap_grid(A[0], B[0], 48)

    def run(P, Q):
        return VR.intersection_columns(P[0], P[1], Q[0], Q[1], x0, y0, s, W, H)[0]
    ab, ba, aa = run(A, B), run(B, A), run(A, A)
    assert ab[0] > 0
    assert aa[0] == aa[1] == aa[2] == ab[1]                              # L_AB(A, A) == L_A
    assert ab[0] == ba[0] and ab[1] == ba[2] and ab[2] == ba[1]          # symmetric
    assert ab[0] <= min(ab[1], ab[2])
    assert np.array_equal(run(A, MC.flipped(B)), ab)                     # either orientation
    assert np.array_equal(run(MC.flipped(A), B), ab)
    far = (B[0] + np.array([0.0, 0.0, 5.0]), B[1])                      # overlaps in xy, not in z
    assert run(A, far)[0] == 0
    inner, outer = RR.icosphere(2, 0.3, (0.05, 0.02, -0.03)), RR.box((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))
    g = overlap_grid(inner[0], outer[0], 40)
    sums = VR.intersection_columns(inner[0], inner[1], outer[0], outer[1], *g)[0]
    assert sums[0] == sums[1] > 0 and sums[2] > sums[1]                  # B contains A


def test_disjoint_boxes_need_no_grid():
    from coma_amd.metrics import overlap_grid
    a, b = RR.box((0, 0, 0), (1, 1, 1)), RR.box((2, 0, 0), (3, 1, 1))
    assert overlap_grid(a[0], b[0], 64) is None
    assert overlap_grid(a[0], a[0] + np.array([0.0, 0.0, 1.5]), 64) is None
    x0, y0, s, W, H = overlap_grid(a[0], RR.box((0.5, 0.25, 0.5), (3.0, 0.75, 2.0))[0], 64)
    assert (x0, y0, s, W, H) == (0.5, 0.25, 128.0, 64, 64)
    assert overlap_grid(RR.box((0, 0, 0), (1.0, 0.3, 1))[0], a[0], 10)[3:] == (10, 3)     # ceil of the shorter side


def test_grazing_bounding_boxes_stay_in_coordinate_range():
    from coma_amd.metrics import MAX_REACH_CELLS, overlap_grid
    A, B = MC.grazing_pair()
    x0, y0, s, W, H = overlap_grid(A[0], B[0], 512)
    assert s < 512 / 0.005 and 1 <= W <= 512 and 1 <= H <= 512                     # capped: the plain rule would give 1.02e5
    reach = max(np.abs(m[0][:, :2] - [x0, y0]).max() for m in (A, B))
    assert reach * s <= MAX_REACH_CELLS and W >= 0.005 * s - 1 and H >= 0.003 * s - 1     # in range, and the grid still spans the overlap
    sums, _, counts = VR.intersection_columns(A[0], A[1], B[0], B[1], x0, y0, s, W, H)    # not Refused
    assert counts.sum() > 0 and sums[0] == 0 and sums[2] > 0                        # the box's corner lies outside the sphere
    A, B = MC.grazing_boxes()
    x0, y0, s, W, H = overlap_grid(A[0], B[0], 512)
    assert s < 512 / 0.004
    v = VR.volumes(VR.intersection_columns(A[0], A[1], B[0], B[1], x0, y0, s, W, H)[0], s)[0]
    # the covered width along each axis is a whole number of cells within one cell of the true width; depth is exact to 1/256 cell
    bound = (1.0 + 1.0 / (0.004 * s)) * (1.0 + 1.0 / (0.003 * s)) - 1.0
    print(f"grazing boxes: s {s:.1f}, {W} x {H}, V_AB {v:.6e} against 7.2e-6, relative bound {bound:.3e}")
    assert abs(v - 7.2e-6) <= bound * 7.2e-6


def test_edges_through_sample_centres_give_two_crossings_per_column():
    # grid cells of size 1, samples at i + 0.5: every vertical face of this cube passes exactly through sample centres
    cube = RR.box((1.5, 2.5, 0.25), (5.5, 6.5, 2.0))
    other = RR.box((0.0, 0.0, 1.0), (8.0, 8.0, 3.0))
    sums, col_ab, counts = VR.intersection_columns(cube[0], cube[1], cube[0], cube[1], 0.0, 0.0, 1.0, 8, 8)
    assert set(np.unique(counts).tolist()) == {0, 4}                     # A and B are the same cube: 2 + 2
    cnt = VR.sweep(VR.crossings(cube[0], cube[1], 0.0, 0.0, 1.0, 8, 8), (np.zeros(0, np.int64),) * 3, 8, 8)[2]
    assert set(np.unique(cnt).tolist()) == {0, 2} and int((cnt == 2).sum()) == 16        # the top-left rule: 4 x 4 columns, once each
    assert sums[0] == 16 * int(1.75 * 256)
    s2 = VR.intersection_columns(cube[0], cube[1], other[0], other[1], 0.0, 0.0, 1.0, 8, 8)[0]
    assert s2[0] == 16 * 256 and s2[2] == 64 * 2 * 256


def test_refusals_of_the_restatement():
    v, f = RR.box((0, 0, 0), (1, 1, 1))
    bad = v.copy()
    bad[3, 1] = np.nan
    with pytest.raises(VR.Refused):
        VR.crossings(bad, f, 0.0, 0.0, 8.0, 8, 8)
    with pytest.raises(VR.Refused):
        VR.crossings(v, f + 1, 0.0, 0.0, 8.0, 8, 8)
    with pytest.raises(VR.Refused):
        VR.crossings(v * np.array([1.0, 1.0, 2.0 ** 31]), f, 0.0, 0.0, 8.0, 8, 8)       # |Z| beyond 2^40


def test_mesh_volume_closed_forms():
    v, f = RR.box((-1.0, 0.5, 2.0), (0.0, 2.5, 5.0))
    vol, _ = VR.mesh_volume(v, f)
    assert abs(abs(vol) - 6.0) <= 6.0 * 1e-12
    assert VR.mesh_volume(v, f[:, ::-1])[0] == -vol
    tet = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    assert abs(VR.mesh_volume(tet, np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]]))[0] - 1.0 / 6.0) <= 1e-12 / 6.0
    r = 0.7
    v, f = RR.icosphere(0, r, (0.3, -0.2, 0.1))
    edge = 4.0 * r / np.sqrt(10.0 + 2.0 * np.sqrt(5.0))
    closed = 5.0 / 12.0 * (3.0 + np.sqrt(5.0)) * edge ** 3
    assert abs(VR.mesh_volume(v, f)[0] - closed) <= closed * 1e-12


# ---- host code recorded from the reference ----
def test_get_asset_info_per_dataset_type(golden_metrics, tmp_path):
    from coma_amd import metrics as M
    from src.generation.initialize_depth import asset_obj_path
    g = golden_metrics
    root = str(tmp_path / "data")
    os.makedirs(f"{root}/ShapeNetCore.v2")
    with open(f"{root}/ShapeNetCore.v2/taxonomy.json", "w") as fh:
        json.dump([dict(name="chair", synsetId="03001627"), dict(name="motorcycle,bike", synsetId="03790512")], fh)
    for kind in g["asset_types"].tolist():
        sc, c, asset = g[f"asset_{kind}_names"].tolist()
        recorded = str(g[f"asset_{kind}_path"])
        assert asset_obj_path(root, sc, c, asset, False) == root + recorded[len("data"):]
        MC.write_obj(root + recorded[len("data"):], g[f"asset_{kind}_obj_verts"], g[f"asset_{kind}_obj_faces"])
        cam = dict(obj_R=g[f"asset_{kind}_obj_R"], obj_t=g[f"asset_{kind}_obj_t"])
        M.ASSET_INFO.clear()
        info = M.get_asset_info(sc, c, asset, "view:00000", cam, False, asset_obj_root=root)
        assert np.array_equal(info["verts"], g[f"asset_{kind}_verts"]), kind
        assert np.array_equal(info["faces"], g[f"asset_{kind}_faces"]) and info["z_min"] == float(g[f"asset_{kind}_z_min"])
        assert M.get_asset_info(sc, c, asset, "view:00000", None, False, asset_obj_root="/nonexistent") is info       # cached per (asset, view)
    M.ASSET_INFO.clear()
    with pytest.raises(NotImplementedError):
        M.get_asset_info("cart", "cart", "x", "view:00000", None, False, asset_obj_root=root)


def test_frame_change_and_asset_transform(golden_metrics):
    from coma_amd import metrics as M
    g = golden_metrics
    cam = dict(obj_R=g["frame_obj_R"], obj_t=g["frame_obj_t"])
    _, z_min = M.asset_transform(g["frame_obj_verts"], cam, "BEHAVE")
    assert z_min == float(g["frame_saved_z_min"])
    assert np.array_equal(M.to_object_frame(g["frame_human_verts"], z_min, cam), g["frame_saved_verts"])
    assert g["frame_saved_keys"].tolist() == sorted(["verts", "faces", "num_inliers", "IoU", "interscetion_ratio", "z_min"])


def test_slice_rule_and_sentinel_pass_through(golden_metrics, tmp_path):
    import pickle
    from src.generation import compute_metrics as cli
    g = golden_metrics
    src = str(tmp_path / "in")
    for rel in g["slice_inputs"].tolist():
        MC.write_pickle(f"{src}/{rel}", "NO HUMANS")
    for num, idx in g["slices"].tolist():
        dst = str(tmp_path / f"out_{num}_{idx}")
        done = cli.save_human(None, None, None, src, "unused", "unused", dst, False, True, False, idx, num)
        assert MC.relative_files(dst, ".pickle") == g[f"slice_{num}_{idx}"].tolist(), (num, idx)
        for pth in done:
            with open(pth, "rb") as fh:
                assert pickle.load(fh) == "NO HUMANS"
    dst = str(tmp_path / "out_1_0")
    assert cli.save_human(None, None, None, src, "unused", "unused", dst, False, True, True, 0, 1) == []       # --skip_done
    assert cli.save_human(None, ["nothing"], None, src, "unused", "unused", dst, False, True, False, 0, 1) == []


def test_cli_flags_match_the_reference():
    from src.coma import filter as flt
    from src.generation import compute_metrics as cli
    a = cli.build_parser().parse_args([])
    assert (a.camera_dir, a.human_after_opt_dir, a.human_pred_dir, a.save_dir) == ("results/generation/cameras", "results/generation/human_after_opt",
                                                                                  "results/generation/human_preds", "results/generation/human_sample")
    assert a.disable_lowres_switch_for_behave is True and (a.parallel_num, a.parallel_idx, a.volume_resolution, a.asset_obj_root) == (1, 0, 512, "data")
    b = flt.build_parser().parse_args([])
    assert (b.human_sample_dir, b.save_dir) == ("results/generation/human_sample", "results/coma/human_postfilterings")
    assert (b.IoU_threshold_min, b.intersection_volume_ratio_threshold_max, b.inlier_num_threshold_min) == (0.7, 0.05, 1)


@pytest.mark.parametrize("mode", ["plain", "total"])
def test_filter_json_and_counters(golden_metrics, tmp_path, capsys, mode):
    from src.coma import filter as flt
    g = golden_metrics
    src, dst = str(tmp_path / "in"), str(tmp_path / "out")
    for rel, payload in zip(g["filter_tree_paths"].tolist(), g["filter_tree_payloads"].tolist()):
        MC.write_pickle(f"{src}/{rel}", json.loads(payload))
    capsys.readouterr()
    r = flt.run_post_filtering(None, None, None, src, dst, enable_aggregate_total_prompts=(mode == "total"), **json.loads(str(g["filter_kw"])))
    printed = capsys.readouterr().out.replace(dst, "SAVE_DIR")
    assert printed == str(g[f"filter_{mode}_stdout"])
    files = MC.relative_files(dst, ".json")
    assert files == g[f"filter_{mode}_files"].tolist()
    for rel, text in zip(files, g[f"filter_{mode}_json"].tolist()):
        assert open(f"{dst}/{rel}").read() == text, rel
    assert r["NUM_MESH"] - (r["REJECTED_FROM_IoU"] + r["REJECTED_FROM_INTERSECTION"] + r["REJECTED_FROM_INLIERS"]) == sum(len(v) for v in r["to_save"].values())
