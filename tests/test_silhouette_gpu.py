"""GPU: coma_raster_depth_f64 and coma_silhouette_iou through the C ABI against the NumPy restatement (tests/raster_ref.py) -- key for
key and count for count, no tolerance -- their refusals, coma_amd.depth_init.select_human against the values recorded from the
reference (tests/golden/depth_init_golden.npz), and the CLI end to end."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest

from tests import raster_ref as RR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x0123456789ABCDEF


def _depth(lib, verts, faces, R, t, scale, W, H):
    """One call through the ctypes table: (rc of the launch, rc of the status call, key map u64 [H,W]); the map is pre-filled."""
    import torch
    from coma_amd import _lib
    v = torch.tensor(np.ascontiguousarray(verts, dtype=np.float64), device=DEV)
    f = torch.tensor(np.ascontiguousarray(np.asarray(faces), dtype=np.int32), device=DEV)
    ws = torch.empty([lib.coma_raster_workspace_bytes(v.shape[0], f.shape[0]) // 8 + 2], dtype=torch.int64, device=DEV)
    key = torch.full([H, W], SENTINEL, dtype=torch.int64, device=DEV)
    Rh, th = np.ascontiguousarray(R, dtype=np.float64).reshape(9), np.ascontiguousarray(t, dtype=np.float64).reshape(3)
    dp = C.POINTER(C.c_double)
    st = _lib.stream_ptr(DEV)
    rc = lib.coma_raster_depth_f64(_lib.ptr(v), v.shape[0], _lib.ptr(f), f.shape[0], Rh.ctypes.data_as(dp), th.ctypes.data_as(dp), float(scale), W, H,
                                   _lib.ptr(ws), _lib.ptr(key), st)
    rs = lib.coma_raster_status(_lib.ptr(ws), st) if rc == 0 else None
    torch.cuda.synchronize()
    return rc, rs, key.cpu().numpy().view(np.uint64), key


def _exact(lib, verts, faces, R, t, scale, W, H, what):
    rc, rs, got, dev = _depth(lib, verts, faces, R, t, scale, W, H)
    assert rc == 0 and rs == 0, lib.coma_last_error()
    ref = RR.raster_depth(verts, faces, R, t, scale, W, H)
    diff = int((got != ref).sum())
    print(f"{what}: {W}x{H}, {len(faces)} faces, {int((ref != RR.EMPTY).sum())} covered pixels, {diff} keys differ")
    assert np.array_equal(got, ref), f"{what}: {diff} of {W * H} keys differ from the restatement"
    return dev, ref


def _camera(eye, target):
    return RR.look_at(eye, target), np.asarray(eye, dtype=np.float64)


def test_icosphere_at_several_radii_and_poses(hip_lib):
    for n, (sub, radius, eye, target, scale, W) in enumerate(((3, 0.4, (2.0, -1.0, 1.0), (0.0, 0.0, 0.1), 2.0, 128), (4, 0.93, (0.0, -3.0, 0.0), (0.0, 0.0, 0.0), 2.0, 256),
                                                              (5, 0.7, (-1.0, 2.0, 3.0), (0.1, 0.0, 0.0), 2.2, 256), (2, 1.6, (0.5, 0.5, 4.0), (0.0, 0.1, 0.0), 2.0, 96))):
        v, f = RR.icosphere(sub, radius)
        R, t = _camera(eye, target)
        _exact(hip_lib, v, f, R, t, scale, W, W, f"icosphere case {n}")


def test_icosphere_at_512(hip_lib):
    v, f = RR.icosphere(5, 0.8)
    R, t = _camera((2.0, -2.0, 1.5), (0.0, 0.0, 0.0))
    _exact(hip_lib, v, f, R, t, 2.5, 512, 512, "SMPL-X-sized icosphere")


def _soup(rng, n, W, H):
    """Triangles of every kind in pixel units, drawn with the identity camera of the host tests (scale = max(W, H))."""
    c = rng.uniform([-0.3 * W, -0.3 * H], [1.3 * W, 1.3 * H], (n, 1, 2))
    size = np.exp(rng.uniform(np.log(0.05), np.log(0.6 * max(W, H)), (n, 1, 1)))
    p = c + rng.normal(size=(n, 3, 2)) * size
    kind = rng.integers(0, 8, n)
    p[kind == 0, 2] = p[kind == 0, 0] + (p[kind == 0, 1] - p[kind == 0, 0]) * 0.5 + rng.normal(size=((kind == 0).sum(), 2)) * 1e-3    # slivers
    p[kind == 1, 2] = p[kind == 1, 1]                                                                                               # zero area
    p[kind == 2] = np.round(p[kind == 2] - 0.5) + 0.5                                                                               # corners ON pixel centres
    p[kind == 3] += np.array([3.0 * W, 0.0])                                                                                        # wholly off-screen
    z = rng.uniform(1.0, 9.0, (n, 3, 1))
    verts = np.concatenate([p - np.array([W / 2, H / 2]), z], axis=2).reshape(-1, 3)
    return verts, np.arange(3 * n, dtype=np.int32).reshape(n, 3)


@pytest.mark.parametrize("W,H", [(160, 160), (200, 72), (50, 131)])
def test_triangle_soup_square_and_not(hip_lib, W, H):
    rng = np.random.default_rng(W * 1000 + H)
    verts, faces = _soup(rng, 1500, W, H)
    faces[::7] = faces[::7, ::-1]
    _exact(hip_lib, verts, faces, np.diag([1.0, -1.0, -1.0]), np.zeros(3), float(max(W, H)), W, H, "triangle soup")


def test_full_screen_quad_and_large_triangles(hip_lib):
    W = H = 256
    quad = np.array([[-300.0, -300.0, 2.0], [300.0, -300.0, 3.0], [300.0, 300.0, 5.0], [-300.0, 300.0, 4.0]])
    I, o = np.diag([1.0, -1.0, -1.0]), np.zeros(3)
    _, ref = _exact(hip_lib, quad, [[0, 1, 2], [0, 2, 3]], I, o, float(W), W, H, "two-triangle full-screen quad")
    assert (ref != RR.EMPTY).all()
    v, f = RR.box((-90.0, -70.0, 3.0), (100.0, 60.0, 40.0))                  # 12 faces, most of the image, seen at an angle
    R, t = _camera((150.0, -220.0, -400.0), (0.0, 0.0, 20.0))
    _exact(hip_lib, v, f, R, t, float(W), W, H, "12-face box")
    rng = np.random.default_rng(5)                                           # a few hundred overlapping mid-sized and large triangles
    p = rng.uniform(-160, 160, (300, 3, 2))
    p[100:] = p[100:, :1] + rng.normal(size=(200, 3, 2)) * 14.0
    soup = np.concatenate([p, rng.uniform(1.0, 9.0, (300, 3, 1))], axis=2).reshape(-1, 3)
    _exact(hip_lib, soup, np.arange(900).reshape(300, 3), I, o, float(W), W, H, "large overlapping triangles")


def test_two_runs_give_the_same_bytes(hip_lib):
    v, f = RR.icosphere(4, 0.9)
    R, t = _camera((1.0, -2.0, 0.5), (0.0, 0.0, 0.0))
    a, b = _depth(hip_lib, v, f, R, t, 2.0, 200, 200), _depth(hip_lib, v, f, R, t, 2.0, 200, 200)
    assert a[0] == 0 == b[0] and a[1] == 0 == b[1] and a[2].tobytes() == b[2].tobytes() and (a[2] != RR.EMPTY).sum() > 1000


def _iou(lib, hk, ak, offsets, gt, want_masks=True, K=None):
    import torch
    from coma_amd import _lib
    off = torch.tensor(np.asarray(offsets, dtype=np.float64), device=DEV)
    K = len(offsets) if K is None else K
    H, W = hk.shape
    g = torch.tensor(np.ascontiguousarray(gt, dtype=np.uint8), device=DEV)
    counts = torch.full([3, 64], -5, dtype=torch.int64, device=DEV)
    masks = torch.full([max(1, len(offsets)), H, W], 7, dtype=torch.uint8, device=DEV) if want_masks else None
    rc = lib.coma_silhouette_iou(_lib.ptr(hk), _lib.ptr(ak), _lib.ptr(off), K, _lib.ptr(g), W, H, _lib.ptr(counts[0]), _lib.ptr(counts[1]),
                                 _lib.ptr(counts[2]), _lib.ptr(masks), _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    return rc, counts.cpu().numpy(), (masks.cpu().numpy() if want_masks else None)


def test_counts_and_masks_front_to_back_null_asset_and_exact_tie(hip_lib):
    W, H = 144, 120
    R, t = _camera((0.0, -6.0, 0.3), (0.0, 0.0, 0.0))
    human, wall = RR.icosphere(4, 0.8), RR.box((-1.1, -0.05, -1.2), (1.0, 0.05, 0.9))
    hk_dev, hk = _exact(hip_lib, *human, R, t, 3.0, W, H, "human")
    ak_dev, ak = _exact(hip_lib, *wall, R, t, 3.0, W, H, "wall")
    yy, xx = np.mgrid[0:H, 0:W]
    gt = (((xx - 80) ** 2 + (yy - 50) ** 2) < 30 ** 2).astype(np.uint8) * 3
    off = np.linspace(-2.0, 2.0, 7)                      # wholly in front of the wall ... wholly behind it
    rc, counts, masks = _iou(hip_lib, hk_dev, ak_dev, off, gt)
    assert rc == 0, hip_lib.coma_last_error()
    vis, inter, uni, ref_masks = RR.silhouette_iou(hk, ak, off, gt)
    print(f"visible {counts[0, :7].tolist()} inter {counts[1, :7].tolist()} union {counts[2, :7].tolist()}")
    assert counts[0, :7].tolist() == vis.tolist() and counts[1, :7].tolist() == inter.tolist() and counts[2, :7].tolist() == uni.tolist()
    assert (counts[:, 7:] == -5).all() and np.array_equal(masks, ref_masks)
    both = (hk != RR.EMPTY) & (ak != RR.EMPTY)
    assert (np.diff(vis) <= 0).all() and vis[0] == (hk != RR.EMPTY).sum() == both.sum() > 500 and 0 < vis[3] < vis[0] and vis[-1] == 0
    rc, counts, masks = _iou(hip_lib, hk_dev, hk_dev, [-2.0, 0.0, 2.0], gt)      # an asset that hides the whole footprint
    assert rc == 0 and counts[0, :3].tolist() == [int((hk != RR.EMPTY).sum()), 0, 0] and (masks[1:] == 0).all()   # exact tie: the asset wins
    rc, counts, masks = _iou(hip_lib, hk_dev, None, off, gt)                                              # no asset
    v0, i0, u0, m0 = RR.silhouette_iou(hk, None, off, gt)
    assert rc == 0 and counts[0, :7].tolist() == v0.tolist() and counts[1, :7].tolist() == i0.tolist() and counts[2, :7].tolist() == u0.tolist()
    assert np.array_equal(masks, m0)
    rc, counts, none = _iou(hip_lib, hk_dev, ak_dev, off, gt, want_masks=False)                          # counts only
    assert rc == 0 and none is None and counts[0, :7].tolist() == vis.tolist() and counts[2, :7].tolist() == uni.tolist()


def _fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "depth_init_golden.npz"), allow_pickle=False)


def _fixture_case(fx, t):
    cam = dict(R=fx[f"{t}_cam_R"], t=fx[f"{t}_cam_t"], scale=float(fx[f"{t}_cam_scale"]), resolution=tuple(int(x) for x in fx[f"{t}_cam_resolution"]),
               obj_R=fx[f"{t}_cam_obj_R"], obj_t=fx[f"{t}_cam_obj_t"], obj_euler=(0.0, 0.0, 0.0), obj_location=(0.0, 0.0, 0.0))
    cands = [dict(verts=v, faces=fx[f"{t}_human_faces"], displacement=d) for v, d in zip(fx[f"{t}_cand_verts"], fx[f"{t}_cand_disp"])]
    return cam, cands


def test_select_human_against_the_reference_record(hip_lib):
    from coma_amd import depth_init as D
    fx = _fixture()
    for t in (str(x) for x in fx["cases"]):
        cam, cands = _fixture_case(fx, t)
        got = D.select_human(cands, cam, fx[f"{t}_gt"], fx[f"{t}_asset_verts"], fx[f"{t}_asset_faces"], device=DEV)
        if f"{t}_saved" in fx:
            assert got is None, t
            assert D.render_human_segmap(cands[0]["verts"], cands[0]["faces"], fx[f"{t}_asset_verts"], fx[f"{t}_asset_faces"], cam, DEV) is None
            assert D.compute_IoU(fx[f"{t}_gt"], cands[0]["verts"], cands[0]["faces"], fx[f"{t}_asset_verts"], fx[f"{t}_asset_faces"], cam, DEV) == 0.0
            continue
        assert set(got) == {"idx", "verts", "faces", "IoU", "human_segmentation", "interval_from_center", "displacement"}
        print(f"case {t}: idx {got['idx']} IoU {got['IoU']!r} (recorded {int(fx[f'{t}_sel_idx'])}, {float(fx[f'{t}_sel_IoU'])!r})")
        assert got["idx"] == int(fx[f"{t}_sel_idx"]) and isinstance(got["IoU"], float) and got["IoU"] == float(fx[f"{t}_sel_IoU"]), t
        assert got["human_segmentation"].dtype == np.uint8 and np.array_equal(got["human_segmentation"], fx[f"{t}_sel_segmentation"]), t
        assert got["interval_from_center"] == int(fx[f"{t}_sel_interval"]) and np.array_equal(got["displacement"], fx[f"{t}_sel_displacement"])
        assert np.array_equal(got["verts"], fx[f"{t}_sel_verts"]), t
        # the metric of compute_metrics.py on the selected human: the same render, the same ratio
        seg = D.render_human_segmap(got["verts"], got["faces"], fx[f"{t}_asset_verts"], fx[f"{t}_asset_faces"], cam, DEV)
        assert np.array_equal(seg, fx[f"{t}_sel_segmentation"]), t
        assert D.compute_IoU(fx[f"{t}_gt"], got["verts"], got["faces"], fx[f"{t}_asset_verts"], fx[f"{t}_asset_faces"], cam, DEV) == got["IoU"], t


def test_refusals_leave_the_outputs_untouched(hip_lib):
    from coma_amd import depth_init as D, _lib
    tri = np.array([[0.0, 0.0, 1.0], [9.0, 0.0, 1.0], [0.0, 9.0, 1.0], [3.0, 3.0, 2.0]])
    faces = [[0, 1, 2], [0, 1, 3]]
    I, o = np.diag([1.0, -1.0, -1.0]), np.zeros(3)
    rc, rs, key, _ = _depth(hip_lib, tri, faces, I, o, 32.0, 32, 32)
    assert rc == 0 and rs == 0 and (key != SENTINEL).all()
    # data the host cannot see: refused on the device, reported by the status call, the map never written
    for what, v, f, word in (("NaN vertex", np.where(np.arange(12).reshape(4, 3) == 4, np.nan, tri), faces, b"non-finite"),
                             ("infinite vertex", np.where(np.arange(12).reshape(4, 3) == 11, np.inf, tri), faces, b"non-finite"),
                             ("coordinate beyond 2^25", np.where(np.arange(12).reshape(4, 3) == 3, 2.0 ** 25 / 256 + 17.0, tri), faces, b"exceeds"),
                             ("negative coordinate beyond 2^25", np.where(np.arange(12).reshape(4, 3) == 7, -(2.0 ** 25) / 256 - 17.0, tri), faces, b"exceeds"),
                             ("face index past V", tri, [[0, 1, 2], [0, 1, 4]], b"face index"),
                             ("negative face index", tri, [[0, -1, 2]], b"face index")):
        rc, rs, key, _ = _depth(hip_lib, v, f, I, o, 32.0, 32, 32)
        assert rc == 0 and rs == -1, what
        assert word in hip_lib.coma_last_error(), (what, hip_lib.coma_last_error())
        assert (key == SENTINEL).all(), what
        with pytest.raises(_lib.ComaHipError, match=word.decode()):
            D.raster_depth(v, f, dict(R=I, t=o, scale=32.0, resolution=(32, 32)), DEV)
    # arguments the host can see: refused before any launch
    for kw, word in ((dict(W=0), b"W="), (dict(H=8193), b"W="), (dict(scale=0.0), b"scale"), (dict(scale=np.nan), b"scale"), (dict(R=I * np.inf), b"camera")):
        a = dict(R=I, t=o, scale=32.0, W=32, H=32)
        a.update(kw)
        import torch
        v = torch.tensor(tri, device=DEV)
        f = torch.tensor(np.asarray(faces, dtype=np.int32), device=DEV)
        ws = torch.empty([64], dtype=torch.int64, device=DEV)
        out = torch.full([32, 32], SENTINEL, dtype=torch.int64, device=DEV)
        Rh, th = np.ascontiguousarray(a["R"], dtype=np.float64).reshape(9), np.ascontiguousarray(a["t"], dtype=np.float64)
        dp = C.POINTER(C.c_double)
        rc = hip_lib.coma_raster_depth_f64(_lib.ptr(v), 4, _lib.ptr(f), 2, Rh.ctypes.data_as(dp), th.ctypes.data_as(dp), float(a["scale"]), a["W"], a["H"],
                                           _lib.ptr(ws), _lib.ptr(out), None)
        torch.cuda.synchronize()
        assert rc == -1 and word in hip_lib.coma_last_error(), (kw, hip_lib.coma_last_error())
        assert (out == SENTINEL).all()
    assert hip_lib.coma_raster_depth_f64(None, 4, None, 2, None, None, 1.0, 8, 8, None, None, None) == -1 and b"null pointer" in hip_lib.coma_last_error()
    assert hip_lib.coma_raster_status(None, None) == -1 and b"null pointer" in hip_lib.coma_last_error()
    assert hip_lib.coma_raster_workspace_bytes(1000, 2000) >= 16 * 3000 and hip_lib.coma_raster_workspace_bytes(0, 5) == 0
    # the count pass
    _, _, _, hk = _depth(hip_lib, tri, faces, I, o, 32.0, 32, 32)
    gt = np.ones((32, 32), np.uint8)
    for K in (0, -3, 65):
        rc, counts, masks = _iou(hip_lib, hk, None, [0.0], gt, K=K)
        assert rc == -1 and b"K=" in hip_lib.coma_last_error(), K
        assert (counts == -5).all() and (masks == 7).all()
    assert hip_lib.coma_silhouette_iou(None, None, None, 1, None, 32, 32, None, None, None, None, None) == -1
    assert b"null pointer" in hip_lib.coma_last_error()


def _write_obj(pth, co, polygons):
    """The asset as a Wavefront OBJ: the file's vertices are the `vertex.co` the reference reads back."""
    os.makedirs(os.path.dirname(pth), exist_ok=True)
    with open(pth, "w") as h:
        h.writelines(f"v {float(x)!r} {float(y)!r} {float(z)!r}\n" for x, y, z in co)
        h.writelines(f"f {a + 1} {b + 1} {c + 1}\n" for a, b, c in polygons)


def test_cli_on_a_three_item_tree(tmp_path, hip_lib):
    from PIL import Image
    from coma_amd import depth_init as D
    from src.generation import initialize_depth as cli
    fx = _fixture()
    root = str(tmp_path)
    sc, c, asset_id = "BEHAVE", "backpack", "behave_asset"
    view, mask, prompt = "view:00000", "mask:000", "a person, full body"
    # item 00000: fixture case a (a box in front of part of the human); 00001: a "NO HUMANS" prediction; 00002: the human BEHIND the box
    cam, _ = _fixture_case(fx, "a")
    _write_obj(f"{root}/data/BEHAVE/objects/backpack/backpack_canon_lowres_in_gen_coord.obj", fx["a_asset_co"], fx["a_asset_polygons"])
    os.makedirs(f"{root}/cam/{sc}/{c}/{asset_id}")
    with open(f"{root}/cam/{sc}/{c}/{asset_id}/{view}.pickle", "wb") as h:
        pickle.dump(cam, h)
    ys, xs = np.nonzero(RR.raster_depth(fx["a_asset_verts"], fx["a_asset_faces"], cam["R"], cam["t"], cam["scale"], 64, 64) != RR.EMPTY)
    cx, cy = float(xs.mean()) + 0.5, float(ys.mean()) + 0.5
    behind = fx["a_pred_verts"].copy()
    behind[:, :2] = (behind[:, :2] - [30.0, 33.0]) * 0.2 + [cx, cy]             # small enough to fit inside the box's footprint
    preds = {"00000": dict(verts=fx["a_pred_verts"], faces=fx["a_pred_faces"], pelvis=fx["a_pred_pelvis"], kps_aux=dict(mask_person_list=[fx["a_gt"]])),
             "00001": "NO HUMANS",
             "00002": dict(verts=behind, faces=fx["a_pred_faces"], pelvis=np.array([cx, cy, 0.0]), kps_aux=dict(mask_person_list=[fx["a_gt"]]))}
    for iid, pred in preds.items():
        os.makedirs(f"{root}/inpaint/{sc}/{c}/{asset_id}/{view}/{mask}/{prompt}", exist_ok=True)
        Image.new("RGB", (64, 64)).save(f"{root}/inpaint/{sc}/{c}/{asset_id}/{view}/{mask}/{prompt}/{iid}.png")
        os.makedirs(f"{root}/pred/{sc}/{c}/{asset_id}/{view}/{mask}/{prompt}", exist_ok=True)
        with open(f"{root}/pred/{sc}/{c}/{asset_id}/{view}/{mask}/{prompt}/{iid}.pickle", "wb") as h:
            pickle.dump(pred, h)
    args = cli.build_parser().parse_args(["--inpaint_dir", f"{root}/inpaint", "--camera_dir", f"{root}/cam", "--human_pred_dir", f"{root}/pred",
                                          "--save_dir", f"{root}/save", "--asset_obj_root", f"{root}/data", "--supercategories", "BEHAVE"])
    done = cli.main(args)
    out = {iid: pickle.load(open(f"{root}/save/{sc}/{c}/{asset_id}/{view}/{mask}/{prompt}/{iid}.pickle", "rb")) for iid in preds}
    assert len(done) == 2 and out["00001"] == "NO HUMANS"
    # item 00000 is the fixture's case: the reference's own pickle, field by field
    a = out["00000"]
    assert set(a) == {"idx", "verts", "faces", "IoU", "human_segmentation", "interval_from_center", "displacement"}
    assert a["idx"] == int(fx["a_sel_idx"]) and a["IoU"] == float(fx["a_sel_IoU"]) and np.array_equal(a["human_segmentation"], fx["a_sel_segmentation"])
    assert np.array_equal(a["verts"], fx["a_sel_verts"]) and np.array_equal(a["displacement"], fx["a_sel_displacement"])
    # item 00002 against select_human on the same inputs; the candidates behind the box are invisible
    p = preds["00002"]
    hv, pelvis = cli.human_world(p["verts"], p["pelvis"], cam, cam["resolution"])
    front = cam["R"][:, 2].reshape((3, 1))
    av, af = fx["a_asset_verts"], fx["a_asset_faces"]
    _, dist = D.compute_nearest_point(asset_verts=av, point=pelvis, direction=front)
    cands = D.extract_candidates(hv, p["faces"], av, af, D.candidate_displacements(dist, D.compute_directional_size(mesh_verts=hv, direction=front) * 0.3, 3), front)
    want = D.select_human(cands, cam, fx["a_gt"], av, af, device=DEV)
    hk = D.raster_depth(cands[0]["verts"], p["faces"], cam, DEV)
    vis, _, _, _ = D.silhouette_counts(hk, D.raster_depth(av, af, cam, DEV), D.depth_offsets(cands, cam), D.person_mask(fx["a_gt"]), want_masks=False)
    print(f"item 00002: visible pixels per candidate {vis.tolist()}")
    assert vis[0] == 0 and vis[-1] > 0
    b = out["00002"]
    assert isinstance(b, dict) and b["idx"] == want["idx"] and b["IoU"] == want["IoU"] and b["interval_from_center"] == want["interval_from_center"]
    for k in ("verts", "faces", "human_segmentation", "displacement"):
        assert np.array_equal(b[k], want[k]), k
