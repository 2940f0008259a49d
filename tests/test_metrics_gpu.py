"""GPU: coma_intersection_columns and coma_mesh_volume_f64 through the C ABI against the NumPy restatement (tests/volume_ref.py) -- the
three sums and the per-column map bit for bit, no tolerance -- their device-side refusals, and src/generation/compute_metrics.py +
src/coma/filter.py end to end on a synthetic tree."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest

from tests import metrics_common as MC
from tests import raster_ref as RR
from tests import volume_ref as VR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x0123456789ABCDEF


def _call(lib, A, B, grid, capacity):
    """One call through the ctypes table: (rc of the launch, rc of the status call, crossings reported, sums i64 [3], col_ab i64 [H,W]);
    sums and col_ab are pre-filled with a sentinel."""
    import torch
    from coma_amd import _lib
    x0, y0, s, W, H = grid
    t = [torch.tensor(np.ascontiguousarray(m[0], dtype=np.float64), device=DEV) for m in (A, B)]
    f = [torch.tensor(np.ascontiguousarray(np.asarray(m[1]), dtype=np.int32), device=DEV) for m in (A, B)]
    nbytes = lib.coma_column_crossings_workspace_bytes(t[0].shape[0], f[0].shape[0], t[1].shape[0], f[1].shape[0], W, H, capacity)
    assert nbytes > 0
    ws = torch.empty([nbytes // 16 + 1, 2], dtype=torch.int64, device=DEV)
    sums = torch.full([3], SENTINEL, dtype=torch.int64, device=DEV)
    col = torch.full([H, W], SENTINEL, dtype=torch.int64, device=DEV)
    needed = C.c_int64(-1)
    st = _lib.stream_ptr(DEV)
    rc = lib.coma_intersection_columns(_lib.ptr(t[0]), t[0].shape[0], _lib.ptr(f[0]), f[0].shape[0], _lib.ptr(t[1]), t[1].shape[0], _lib.ptr(f[1]),
                                       f[1].shape[0], float(x0), float(y0), float(s), W, H, capacity, _lib.ptr(ws), _lib.ptr(sums), _lib.ptr(col), st)
    rs = lib.coma_intersection_status(_lib.ptr(ws), st, C.byref(needed)) if rc == 0 else None
    torch.cuda.synchronize()
    return rc, rs, needed.value, sums.cpu().numpy(), col.cpu().numpy()


def _exact(lib, A, B, grid, what, capacity=None):
    ref_sums, ref_col, counts = VR.intersection_columns(A[0], A[1], B[0], B[1], *grid)
    total = int(counts.sum())
    rc, rs, needed, sums, col = _call(lib, A, B, grid, capacity if capacity is not None else max(1, total))
    assert rc == 0 and rs == 0, lib.coma_last_error()
    print(f"{what}: {grid[3]}x{grid[4]}, {len(A[1])}+{len(B[1])} faces, {total} crossings (longest column {int(counts.max())}), "
          f"sums {sums.tolist()} vs {ref_sums.tolist()}, {int((col != ref_col).sum())} columns differ")
    assert needed == total
    assert np.array_equal(sums, ref_sums), what
    assert np.array_equal(col, ref_col), what
    return ref_sums, counts


def _grid(A, B, resolution):
    from coma_amd.metrics import overlap_grid
    return overlap_grid(A[0], B[0], resolution)


def test_icospheres_small_triangle_path(hip_lib):
    A, B = RR.icosphere(3, 0.8), RR.icosphere(3, 0.7, (0.45, 0.3, -0.25))
    sums, _ = _exact(hip_lib, A, B, _grid(A, B, 64), "icospheres 64^2")
    assert sums[0] > 0
    _exact(hip_lib, A, B, (-0.85, -0.3, 50.0, 96, 40), "icospheres 96x40")          # W != H, the grid cuts both meshes


def test_boxes_filling_the_grid_tile_path(hip_lib):
    A, B = RR.box((-1.0, -1.0, -0.5), (1.0, 1.0, 0.5)), RR.box((-1.0, -1.0, 0.1), (1.0, 1.0, 0.9))
    A = (A[0] @ MC.rot((0.1, 0.2, 1.0), 0.05).T, A[1])                                # slightly turned: slanted faces, not only constant depth
    sums, counts = _exact(hip_lib, A, B, (-1.0, -1.0, 64.0, 128, 128), "boxes 128^2")
    assert sums[0] > 0 and counts.max() >= 4


def test_box_and_icosphere_both_paths(hip_lib):
    A, B = RR.icosphere(3, 0.6, (0.1, 0.0, 0.2)), RR.box((-0.3, -0.8, -0.4), (0.9, 0.5, 0.5))
    sums, _ = _exact(hip_lib, A, B, _grid(A, B, 96), "icosphere and box 96")
    assert sums[0] > 0
    _exact(hip_lib, A, MC.flipped(B), _grid(A, B, 96), "icosphere and outward box 96")


def test_edges_through_sample_centres(hip_lib):
    cube, other = RR.box((1.5, 2.5, 0.25), (5.5, 6.5, 2.0)), RR.box((0.0, 0.0, 1.0), (8.0, 8.0, 3.0))
    sums, counts = _exact(hip_lib, cube, other, (0.0, 0.0, 1.0, 8, 8), "cube on sample centres")
    assert sums.tolist() == [16 * 256, 16 * 448, 64 * 512] and int((counts == 4).sum()) == 16


def test_coincident_faces_tie_in_z(hip_lib):
    A, B = RR.box((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), RR.box((0.25, 0.25, 0.5), (1.5, 1.5, 1.0))      # the two top faces coincide
    sums, _ = _exact(hip_lib, A, B, (0.0, 0.0, 16.0, 24, 24), "coincident top faces")
    assert sums[0] == 12 * 12 * 8 * 256
    _exact(hip_lib, A, A, (0.0, 0.0, 16.0, 24, 24), "a mesh against itself")                         # every crossing tied


def test_long_columns_sorted_in_the_workspace(hip_lib):
    A = RR.box((0.0, 0.0, 0.0), (1.0, 1.0, 4.5))
    B = MC.slab_stack(40, (0.1, 0.1), (0.9, 0.7), 0.05, 0.1, 0.04)
    sums, counts = _exact(hip_lib, A, B, (0.0, 0.0, 20.0, 20, 20), "40 slabs in a tall box")
    assert counts.max() >= 82 and sums[0] == sums[2] > 0


def test_inward_mesh_and_no_overlap_in_z(hip_lib):
    A, B = RR.icosphere(2, 0.8), RR.icosphere(2, 0.7, (0.45, 0.3, -0.25))
    g = _grid(A, B, 48)
    ref, _ = _exact(hip_lib, A, MC.flipped(B), g, "inward B")
    assert np.array_equal(ref, VR.intersection_columns(A[0], A[1], B[0], B[1], *g)[0])
    far = (B[0] + np.array([0.0, 0.0, 5.0]), B[1])
    sums, _ = _exact(hip_lib, A, far, g, "apart in z")
    assert sums[0] == 0 and sums[1] > 0 and sums[2] > 0


def test_grazing_bounding_boxes(hip_lib):
    from coma_amd import metrics as M
    A, B = MC.grazing_pair()
    g = M.overlap_grid(A[0], B[0], 128)                                             # 128 x 77 cells of 39 um; at 512 the scale is capped
    assert g[3] <= 128 and g[4] <= 128
    sums, _ = _exact(hip_lib, A, B, g, "grazing boxes")
    assert sums[0] == 0 and sums[2] > 0
    assert M.intersection_volume(A[0], A[1], B[0], B[1], 512, device=DEV) == 0.0   # launched, not refused
    A, B = MC.grazing_boxes()                                                       # capped at 512: 262 x 196 cells
    g = M.overlap_grid(A[0], B[0], 512)
    ref, _ = _exact(hip_lib, A, B, g, "grazing boxes with a common corner")
    assert ref[0] > 0 and M.intersection_volume(A[0], A[1], B[0], B[1], 512, device=DEV) == float(int(ref[0])) / (256.0 * g[2] ** 3)


def test_device_side_refusals(hip_lib):
    from coma_amd import _lib, metrics as M
    A, B = RR.icosphere(2, 0.8), RR.icosphere(2, 0.7, (0.45, 0.3, -0.25))
    g = _grid(A, B, 32)
    ref_sums, ref_col, counts = VR.intersection_columns(A[0], A[1], B[0], B[1], *g)
    total = int(counts.sum())
    untouched = [SENTINEL] * 3

    bad = A[0].copy()
    bad[7, 2] = np.nan
    rc, rs, needed, sums, col = _call(hip_lib, (bad, A[1]), B, g, total)
    assert rc == 0 and rs == -1 and b"non-finite vertex" in hip_lib.coma_last_error()
    assert sums.tolist() == untouched and (col == SENTINEL).all()

    faces = B[1].copy()
    faces[5, 1] = len(B[0])
    rc, rs, needed, sums, col = _call(hip_lib, A, (B[0], faces), g, total)
    assert rc == 0 and rs == -1 and b"face index" in hip_lib.coma_last_error()
    assert sums.tolist() == untouched and (col == SENTINEL).all()

    tall = (A[0] * np.array([1.0, 1.0, 2.0 ** 33]), A[1])
    rc, rs, needed, sums, col = _call(hip_lib, tall, B, g, total)
    assert rc == 0 and rs == -1 and b"2^40" in hip_lib.coma_last_error()
    assert sums.tolist() == untouched

    rc, rs, needed, sums, col = _call(hip_lib, A, B, g, total - 1)                 # one entry short
    assert rc == 0 and rs == -1 and b"capacity exceeded" in hip_lib.coma_last_error() and needed == total
    assert sums.tolist() == untouched and (col == SENTINEL).all()
    rc, rs, needed, sums, col = _call(hip_lib, A, B, g, total)                     # exactly enough
    assert rc == 0 and rs == 0 and np.array_equal(sums, ref_sums)

    got, got_col = M.intersection_columns(A[0], A[1], B[0], B[1], *g, capacity=7, want_columns=True, device=DEV)     # the wrapper's one retry
    assert np.array_equal(got, ref_sums) and np.array_equal(got_col, ref_col)
    with pytest.raises(_lib.ComaHipError, match="non-finite"):
        M.intersection_columns(bad, A[1], B[0], B[1], *g, device=DEV)

    one = C.c_void_p(16)   # never dereferenced: argument validation fails first
    assert hip_lib.coma_intersection_columns(one, 1, one, 1, one, 1, one, 1, 0.0, 0.0, 1.0, 9000, 8, 1, one, one, None, None) == -1
    assert hip_lib.coma_intersection_columns(one, 1, one, 1, one, 1, one, 1, 0.0, 0.0, 0.0, 8, 8, 1, one, one, None, None) == -1
    assert hip_lib.coma_column_crossings_workspace_bytes(1, 1, 1, 1, 8, 8, 0) == 0


def test_wrapper_volume_and_ratio(hip_lib):
    from coma_amd import metrics as M
    A, B = RR.icosphere(2, 0.8), RR.icosphere(2, 0.7, (0.45, 0.3, -0.25))
    x0, y0, s, W, H = M.overlap_grid(A[0], B[0], 64)
    ref = VR.intersection_columns(A[0], A[1], B[0], B[1], x0, y0, s, W, H)[0]
    assert M.intersection_volume(A[0], A[1], B[0], B[1], 64, device=DEV) == float(int(ref[0])) / (256.0 * s * s * s)
    ratio = M.compute_instersection_ratio(A[0], A[1], B[0], B[1], 64, device=DEV)
    assert abs(ratio - VR.volumes(ref, s)[0] / VR.mesh_volume(*A)[0]) <= 1e-12
    assert M.intersection_volume(A[0], A[1], B[0] + np.array([3.0, 0.0, 0.0]), B[1], 64, device=DEV) == 0.0      # no launch


def test_mesh_volume_against_numpy_and_run_to_run(hip_lib):
    import torch
    from coma_amd import _lib
    for v, f in (RR.icosphere(4, 0.9, (2.0, -1.5, 0.7)), RR.box((-1.0, 0.5, 2.0), (0.0, 2.5, 5.0)), RR.icosphere(5, 1.3, (0.1, 0.2, -4.0))):
        ref, ref_abs = VR.mesh_volume(v, f)
        tv, tf = torch.tensor(v, device=DEV), torch.tensor(np.ascontiguousarray(f, dtype=np.int32), device=DEV)
        ws = torch.empty([hip_lib.coma_mesh_volume_workspace_bytes(len(f)) // 8 + 1], dtype=torch.int64, device=DEV)
        outs = []
        for _ in range(2):
            out = torch.full([1], float("nan"), dtype=torch.float64, device=DEV)
            rc = hip_lib.coma_mesh_volume_f64(_lib.ptr(tv), len(v), _lib.ptr(tf), len(f), _lib.ptr(out), _lib.ptr(ws), _lib.stream_ptr(DEV))
            assert rc == 0, hip_lib.coma_last_error()
            outs.append(out.cpu().numpy().view(np.uint64)[0])
        got = float(np.array(outs[0], dtype=np.uint64).view(np.float64))
        bound = len(f) * 2.0 ** -52 * ref_abs / abs(ref)          # worst case of a reordered f64 sum, relative
        print(f"{len(f)} faces: device {got!r}, NumPy {ref!r}, relative difference {abs(got - ref) / abs(ref):.3e}, bound {bound:.3e}")
        assert abs(got - ref) / abs(ref) <= bound
        assert outs[0] == outs[1]
    bad = torch.tensor(np.array([[0, 1, 8]], dtype=np.int32), device=DEV)        # an index past V is not followed
    out = torch.zeros([1], dtype=torch.float64, device=DEV)
    assert hip_lib.coma_mesh_volume_f64(_lib.ptr(tv), 8, _lib.ptr(bad), 1, _lib.ptr(out), _lib.ptr(ws), _lib.stream_ptr(DEV)) == 0
    assert np.isnan(out.item())


def test_cli_end_to_end(hip_lib, tmp_path):
    from coma_amd import metrics as M
    from src.coma import filter as flt
    from src.generation import compute_metrics as cli
    root = str(tmp_path)
    sc, c, asset, view, mask, prompt = "BEHAVE", "backpack", "behave_asset", "view:00000", "mask:000", "sitting on the backpack, full body"
    box = RR.box((-0.5, 0.0, -0.5), (0.5, 1.0, 0.5))                              # OBJ frame: y is up
    MC.write_obj(f"{root}/data/BEHAVE/objects/{c}/{c}.obj", *box)
    eye = np.array([0.0, -3.0, 0.5])
    cam = dict(R=RR.look_at(eye, (0.0, 0.0, 0.5)), t=eye, scale=2.4, resolution=(64, 64), obj_R=np.eye(3), obj_t=np.zeros((3, 1)))
    MC.write_pickle(f"{root}/cam/{sc}/{c}/{asset}/{view}.pickle", cam)
    M.ASSET_INFO.clear()
    world = M.get_asset_info(sc, c, asset, view, cam, True, asset_obj_root=f"{root}/data")
    M.ASSET_INFO.clear()
    assert np.allclose(world["verts"].min(axis=0), [-0.5, -0.5, 0.0]) and np.allclose(world["verts"].max(axis=0), [0.5, 0.5, 1.0])
    humans = {"00000": RR.icosphere(2, 0.3, (0.0, -0.75, 0.5)),                   # dips 0.05 into the front face: about 2 % of its volume
              "00001": RR.icosphere(2, 0.3, (0.0, -0.55, 0.5))}                   # 0.25 deep: about 40 %
    expected = {}
    for iid, (v, f) in humans.items():
        seg = RR.segmap([(world["verts"], world["faces"].astype(np.int32)), (v, f)], cam["R"], cam["t"], cam["scale"], 64, 64)
        MC.write_pickle(f"{root}/pred/{sc}/{c}/{asset}/{view}/{mask}/{prompt}/{iid}.pickle", dict(kps_aux=dict(mask_person_list=[seg == 2])))
        MC.write_pickle(f"{root}/opt/{sc}/{c}/{asset}/{view}/{mask}/{prompt}/{iid}.pickle", dict(verts=v.copy(), faces=f.astype(np.int64), num_inliers=3))
        x0, y0, s, W, H = M.overlap_grid(v, world["verts"], 64)
        sums = VR.intersection_columns(v, f, world["verts"], world["faces"], x0, y0, s, W, H)[0]
        expected[iid] = abs(VR.volumes(sums, s)[0] / VR.mesh_volume(v, f)[0])
    MC.write_pickle(f"{root}/opt/{sc}/{c}/{asset}/{view}/{mask}/{prompt}/00002.pickle", "NO HUMANS")
    args = cli.build_parser().parse_args(["--camera_dir", f"{root}/cam", "--human_after_opt_dir", f"{root}/opt", "--human_pred_dir", f"{root}/pred",
                                          "--save_dir", f"{root}/sample", "--asset_obj_root", f"{root}/data", "--volume_resolution", "64"])
    assert len(cli.main(args)) == 3
    for iid, (v, f) in humans.items():
        with open(f"{root}/sample/{sc}/{c}/{asset}/{view}/{mask}/{prompt}/{iid}.pickle", "rb") as fh:
            saved = pickle.load(fh)
        assert sorted(saved) == sorted(["verts", "faces", "num_inliers", "IoU", "interscetion_ratio", "z_min"])
        print(f"sample {iid}: IoU {saved['IoU']}, interscetion_ratio {saved['interscetion_ratio']} (restatement {expected[iid]})")
        assert saved["IoU"] == 1.0 and abs(saved["interscetion_ratio"] - expected[iid]) <= 1e-12
        assert np.array_equal(saved["verts"], M.to_object_frame(v, world["z_min"], cam)) and saved["z_min"] == world["z_min"]
    assert expected["00000"] < 0.05 < expected["00001"]
    with open(f"{root}/sample/{sc}/{c}/{asset}/{view}/{mask}/{prompt}/00002.pickle", "rb") as fh:
        assert pickle.load(fh) == "NO HUMANS"
    M.ASSET_INFO.clear()
    r = flt.main(flt.build_parser().parse_args(["--human_sample_dir", f"{root}/sample", "--save_dir", f"{root}/post"]))
    assert (r["NUM_MESH"], r["REJECTED_FROM_IoU"], r["REJECTED_FROM_INTERSECTION"], r["REJECTED_FROM_INLIERS"]) == (2, 0, 1, 0)
    import json
    with open(f"{root}/post/{sc}/{c}/{asset}/sitting on the backpack.json") as fh:
        assert json.load(fh) == [[view, mask, prompt, "00000"]]
