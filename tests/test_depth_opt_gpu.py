"""GPU: coma_shift_columns_prepare / coma_shift_profile / coma_depth_optimize_f64 through the C ABI and coma_amd.depth_opt against the
NumPy restatement (tests/shift_ref.py) -- the profile, the two lengths and the whole Adam trajectory bit for bit, no tolerance -- the
device-side refusals, and src/generation/optimize_depth.py end to end on a synthetic tree with a stand-in body model."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest

from tests import metrics_common as MC
from tests import raster_ref as RR
from tests import shift_ref as SR
from tests import volume_ref as VR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x0123456789ABCDEF


def u_shape():
    """A closed C-shaped prism: the outline below in the (x, z) plane, extruded along y.  A column through the two arms is inside the
    mesh twice."""
    outline = [(0.2, 0.1), (0.8, 0.1), (0.8, 0.3), (0.4, 0.3), (0.4, 0.6), (0.8, 0.6), (0.8, 0.8), (0.2, 0.8)]
    caps = [(0, 1, 2), (0, 2, 3), (0, 3, 4), (0, 4, 7), (4, 5, 6), (4, 6, 7)]
    y0, y1, n = 0.25, 0.75, len(outline)
    verts = np.array([(x, y0, z) for x, z in outline] + [(x, y1, z) for x, z in outline])
    faces = [(a, b, c) for a, b, c in caps] + [(a + n, c + n, b + n) for a, b, c in caps]
    for i in range(n):
        j = (i + 1) % n
        faces += [(i, i + n, j + n), (i, j + n, j)]
    faces = np.array(faces, dtype=np.int32)
    vol = VR.mesh_volume(verts, faces)[0]
    assert abs(abs(vol) - 0.30 * 0.5) < 1e-12, vol          # consistently oriented: outline area 0.30 times the depth
    return (verts, faces if vol > 0 else np.ascontiguousarray(faces[:, ::-1]))


def _tet():
    v, f = MC.convex_pairs()["cube_tet"][1]
    return v * 0.4 + np.array([0.5, 0.5, 0.5]), f


PAIRS = {
    "box_in_box": (RR.box((0.3, 0.3, 0.2), (0.7, 0.7, 0.5)), RR.box((0.1, 0.1, 0.0), (0.9, 0.9, 1.0))),
    "tet_box": (_tet(), RR.box((0.2, 0.1, 0.3), (0.9, 0.8, 0.6))),
    "u_shape": (u_shape(), RR.box((0.1, 0.2, 0.35), (0.9, 0.8, 0.55))),
    "inward": (MC.flipped(RR.box((0.3, 0.3, 0.2), (0.7, 0.7, 0.5))), RR.box((0.1, 0.1, 0.0), (0.9, 0.9, 1.0))),
    "slabs": (RR.box((0.2, 0.2, 0.0), (0.8, 0.8, 1.0)), MC.slab_stack(40, (0.1, 0.1), (0.9, 0.7), 0.05, 0.1, 0.04)),
}
_COLUMNS = {}


def ref_columns(name, res):
    """The restatement's crossings of a pair on the res x res grid over the unit square: computed once, shared, never changed."""
    if (name, res) not in _COLUMNS:
        A, B = PAIRS[name]
        _COLUMNS[(name, res)] = SR.Columns(A[0], A[1], B[0], B[1], 0.0, 0.0, float(res), res, res)
    return _COLUMNS[(name, res)]


breakpoint_shifts = SR.breakpoint_shifts


def to_d(delta, s):
    d = float(delta) / (256.0 * s)
    assert SR.shift_of(d, s) == delta
    return d


@pytest.mark.parametrize("res", [16, 32])
@pytest.mark.parametrize("name", sorted(PAIRS))
def test_profile_bit_exact(hip_lib, name, res):
    from coma_amd import depth_opt as D, metrics as M
    A, B = PAIRS[name]
    ref = ref_columns(name, res)
    cols = D.prepare_columns(A[0], A[1], B[0], B[1], 0.0, 0.0, float(res), res, res, capacity=int(ref.counts.sum()), device=DEV)
    assert (cols.L_A, cols.L_B, cols.crossings) == (ref.L_A, ref.L_B, int(ref.counts.sum()))
    sums, _ = M.intersection_columns(A[0], A[1], B[0], B[1], 0.0, 0.0, float(res), res, res, device=DEV)
    centre = D.shift_profile(cols, [0.0])                                            # K = 1
    assert centre.shape == (1, 3) and np.array_equal(centre, ref.profile([0.0]))
    assert [int(centre[0, 1]), cols.L_A, cols.L_B] == sums.tolist()                  # the same numbers as coma_intersection_columns
    near, far = breakpoint_shifts(ref)
    d = [to_d(k, ref.s) for k in near] + [to_d(far, ref.s), to_d(-far, ref.s), 1e6, -1e30, 1e300]
    want = ref.profile(d)
    got = np.concatenate([D.shift_profile(cols, d[i:i + 64]) for i in range(0, len(d), 64)])     # K = 64, and a shorter tail
    print(f"{name} {res}^2: {cols.crossings} crossings (longest column {int(ref.counts.max())}), L_A {cols.L_A}, L_B {cols.L_B}, {len(d)} shifts, "
          f"L_AB(0) {int(centre[0, 1])}, largest L_AB {int(want.max())}, {int((got != want).any(axis=1).sum())} shifts differ")
    assert len(d) > 64 or name not in ("slabs", "tet_box")                           # these two also go through K = 64
    assert np.array_equal(got, want)
    assert not want[-5:].any() and want.max() > 0                                    # far outside the overlap: nothing
    if name == "slabs":
        assert ref.counts.max() >= 82                                                # longer than the LDS sort holds
    if name == "u_shape":
        assert np.bincount(ref.ca[0]).max() == 4                                     # two intervals of A in the columns through its arms
    if name == "inward":
        assert np.array_equal(want, ref_columns("box_in_box", res).profile(d))       # n != 0, not n > 0


def _raw_prepare(lib, A, B, res, capacity):
    import torch
    from coma_amd import _lib
    t = [torch.tensor(np.ascontiguousarray(m[0], dtype=np.float64), device=DEV) for m in (A, B)]
    f = [torch.tensor(np.ascontiguousarray(np.asarray(m[1]), dtype=np.int32), device=DEV) for m in (A, B)]
    nbytes = lib.coma_shift_columns_workspace_bytes(t[0].shape[0], f[0].shape[0], t[1].shape[0], f[1].shape[0], res, res, capacity)
    assert nbytes > 0
    ws = torch.zeros([nbytes // 16 + 1, 2], dtype=torch.int64, device=DEV)
    lengths = torch.full([2], SENTINEL, dtype=torch.int64, device=DEV)
    needed = C.c_int64(-1)
    st = _lib.stream_ptr(DEV)
    rc = lib.coma_shift_columns_prepare(_lib.ptr(t[0]), t[0].shape[0], _lib.ptr(f[0]), f[0].shape[0], _lib.ptr(t[1]), t[1].shape[0], _lib.ptr(f[1]),
                                        f[1].shape[0], 0.0, 0.0, float(res), res, res, capacity, _lib.ptr(ws), _lib.ptr(lengths), st)
    rs = lib.coma_shift_columns_status(_lib.ptr(ws), st, C.byref(needed)) if rc == 0 else None
    return rc, rs, needed.value, lengths.cpu().numpy(), ws


def test_capacity_refusal_and_retry(hip_lib):
    import torch
    from coma_amd import _lib, depth_opt as D
    A, B = PAIRS["u_shape"]
    ref = ref_columns("u_shape", 16)
    total = int(ref.counts.sum())
    rc, rs, needed, lengths, ws = _raw_prepare(hip_lib, A, B, 16, total - 1)       # one entry short
    assert rc == 0 and rs == -1 and b"capacity exceeded" in hip_lib.coma_last_error() and needed == total
    assert lengths.tolist() == [SENTINEL] * 2
    # everything that is given the refused workspace idles: the outputs keep what they held
    st = _lib.stream_ptr(DEV)
    d = torch.zeros([2], dtype=torch.float64, device=DEV)
    L = torch.full([2, 3], SENTINEL, dtype=torch.int64, device=DEV)
    assert hip_lib.coma_shift_profile(_lib.ptr(ws), _lib.ptr(d), 2, _lib.ptr(L), st) == 0
    traj = torch.full([4], 7.5, dtype=torch.float64, device=DEV)
    Lt = torch.full([3, 3], SENTINEL, dtype=torch.int64, device=DEV)
    losses = torch.full([3, 2], 7.5, dtype=torch.float64, device=DEV)
    state = torch.zeros([hip_lib.coma_depth_optimize_state_bytes() // 8], dtype=torch.int64, device=DEV)
    front = (C.c_double * 3)(0.0, 0.0, 1.0)
    assert hip_lib.coma_depth_optimize_f64(_lib.ptr(ws), None, 0, None, front, None, None, 0, 25, 0.0, 0.01, 0.0, 0.4, 3, _lib.ptr(traj), _lib.ptr(Lt),
                                           _lib.ptr(losses), _lib.ptr(state), st) == 0
    assert hip_lib.coma_depth_optimize_status(_lib.ptr(state), st, None) == -1 and b"refused" in hip_lib.coma_last_error()
    assert (L.cpu().numpy() == SENTINEL).all() and (Lt.cpu().numpy() == SENTINEL).all()
    assert (traj.cpu().numpy() == 7.5).all() and (losses.cpu().numpy() == 7.5).all()
    rc, rs, needed, lengths, ws = _raw_prepare(hip_lib, A, B, 16, total)           # exactly enough
    assert rc == 0 and rs == 0 and needed == total and lengths.tolist() == [ref.L_A, ref.L_B]
    cols = D.prepare_columns(A[0], A[1], B[0], B[1], 0.0, 0.0, 16.0, 16, 16, capacity=7, device=DEV)      # the wrapper's one retry
    assert (cols.L_A, cols.L_B, cols.crossings) == (ref.L_A, ref.L_B, total)
    assert np.array_equal(D.shift_profile(cols, [0.0, 0.05]), ref.profile([0.0, 0.05]))
    bad = A[0].copy()
    bad[3, 2] = np.nan
    with pytest.raises(_lib.ComaHipError, match="non-finite"):
        D.prepare_columns(bad, A[1], B[0], B[1], 0.0, 0.0, 16.0, 16, 16, device=DEV)
    one = C.c_void_p(16)   # never dereferenced: argument validation fails first
    assert hip_lib.coma_shift_profile(one, one, 65, one, None) == -1 and hip_lib.coma_shift_profile(one, one, 0, one, None) == -1
    assert hip_lib.coma_depth_optimize_f64(None, None, 0, None, front, None, None, 0, 25, 0.0, 0.01, 0.0, 0.0, 4097, one, one, one, one, None) == -1
    assert hip_lib.coma_shift_columns_workspace_bytes(1, 1, 1, 1, 8, 8, 0) == 0


def _multiview_inputs(copies):
    """The golden "converge" case; with copies > 1 every view is repeated with jittered joints, so that one partial sum of the step
    kernel holds more than one view (N > 256)."""
    from tests.test_depth_opt_host import _golden_case
    g = np.load(os.path.join(ROOT, "tests", "golden", "depth_opt_golden.npz"), allow_pickle=False)
    c = _golden_case(g, "converge")
    if copies > 1:
        rng = np.random.default_rng(3)
        c["cand_view"] = np.tile(c["cand_view"], copies)
        c["cand_xy"] = np.tile(c["cand_xy"], (copies, 1, 1)) + rng.normal(scale=2.0, size=(copies * len(c["views"]), 25, 2))
    return c


@pytest.mark.parametrize("setting", ["both", "multiview", "collision"])
def test_loop_bit_identical(hip_lib, setting):
    from coma_amd import depth_opt as D
    E = 20
    A, B = RR.box((0.3, 0.3, 0.2), (0.7, 0.7, 0.5)), RR.box((0.1, 0.1, 0.4), (0.9, 0.9, 1.0))      # A pushed 0.1 into B from below
    ref_cols = SR.Columns(A[0], A[1], B[0], B[1], 0.0, 0.0, 32.0, 32, 32)
    c = _multiview_inputs(70 if setting == "both" else 1)
    w_mv, w_col = dict(both=(1e-3, 0.4), multiview=(1e-3, 0.0), collision=(0.0, 0.4))[setting]
    cols = D.prepare_columns(A[0], A[1], B[0], B[1], 0.0, 0.0, 32.0, 32, 32, device=DEV) if setting != "multiview" else None
    want = SR.optimize(ref_cols if cols is not None else None, c["views"], c["joints0"], c["front"], c["cand_view"], c["cand_xy"], 0.0, 0.01, w_mv, w_col, E)
    got = D.optimize_displacement(cols, c["views"], c["joints0"], c["front"], c["cand_view"], c["cand_xy"], 0.0, 0.01, w_mv, w_col, E, device=DEV)
    print(f"{setting}: N {len(c['cand_view'])}, d {got['d']!r} vs {want['d']!r}, max |traj difference| {np.abs(got['traj'] - want['traj']).max():.3e}, "
          f"L_AB {got['Ltraj'][0, 1]} -> {got['Ltraj'][-1, 1]}, losses[0] {got['losses'][0].tolist()} vs {want['losses'][0].tolist()}")
    assert np.array_equal(got["Ltraj"], want["Ltraj"])
    assert np.array_equal(got["losses"].view(np.uint64), want["losses"].view(np.uint64))
    assert np.array_equal(got["traj"].view(np.uint64), want["traj"].view(np.uint64)) and got["d"] == want["d"]
    assert got["traj"][0] == 0.0 and (np.diff(got["traj"]) != 0.0).all()
    if setting == "collision":
        assert got["Ltraj"][0, 1] == 144 * 819 > got["Ltraj"][-1, 1] and got["d"] < 0.0   # 12 x 12 columns, 0.1 deep at 32 x 256 per unit
    if setting == "multiview":
        assert not got["Ltraj"].any() and not got["losses"][:, 1].any()


def test_loop_stops_when_d_is_not_finite(hip_lib):
    from coma_amd import _lib, depth_opt as D
    c = _multiview_inputs(1)
    want = SR.optimize(None, c["views"], c["joints0"], c["front"], c["cand_view"], c["cand_xy"], 1e306, 0.01, 1.0, 0.0, 5)
    assert len(want["traj"]) == 2 and not np.isfinite(want["traj"][1])              # the squares overflow in the first epoch
    with pytest.raises(_lib.ComaHipError, match="not finite after epoch 1"):
        D.optimize_displacement(None, c["views"], c["joints0"], c["front"], c["cand_view"], c["cand_xy"], 1e306, 0.01, 1.0, 0.0, 5, device=DEV)


def test_cli_end_to_end(hip_lib, tmp_path):
    from PIL import Image
    from coma_amd import depth_opt as D, metrics as M
    from oracle import triangulation_oracle as T
    from src.generation import optimize_depth as cli
    from src.generation.initialize_depth import asset_world
    root = str(tmp_path)
    sc, c, asset, mask, prompt = "BEHAVE", "backpack", "behave_asset", "mask:000", "sitting on the backpack, full body"
    box = RR.box((-0.5, 0.0, -0.5), (0.5, 1.0, 0.5))                              # OBJ frame: y is up
    MC.write_obj(f"{root}/data/BEHAVE/objects/{c}/{c}_canon_lowres_in_gen_coord.obj", *box)
    centre = np.array([0.0, 0.0, 0.5])
    eyes = [np.array([0.0, -3.0, 0.5]), np.array([2.5, -1.5, 0.9]), np.array([-2.2, -2.0, 1.4]), np.array([1.0, -2.8, 1.8])]
    cams = [dict(R=RR.look_at(e, centre), t=e, scale=2.4, resolution=(64, 64), obj_R=np.eye(3), obj_t=np.zeros((3, 1))) for e in eyes]
    for v, cam in enumerate(cams):
        MC.write_pickle(f"{root}/cam/{sc}/{c}/{asset}/view:{v:05}.pickle", cam)
    front = cams[0]["R"][:, 2]
    conv = dict(focals=(80.0, 80.0), princpt=(32.0, 32.0), z_mean=4.0)
    transl = np.array([[0.0, 0.0, 4.0]], dtype=np.float32)
    sphere = RR.icosphere(2, 0.3)

    def body_model(smplx_data, smplx_path):
        rng = np.random.default_rng(smplx_data["seed"])
        return sphere[0].astype(np.float32), rng.normal(scale=0.3, size=(137, 3)).astype(np.float32)
    probe = D.convert_cam2real(np.zeros((1, 3), np.float32), transl, (64, 64), cams[0], conv).astype(np.float64)
    placed = (np.array([0.0, -0.62, 0.5]) - probe)                                 # where the depth initialisation left the human: 0.1 deep in the asset
    true_d = {"0": -0.08, "1": 0.05}
    for iid in ("0", "1", "2"):
        below = f"{sc}/{c}/{asset}/view:00000/{mask}/{prompt}"
        os.makedirs(f"{root}/inpaint/{below}", exist_ok=True)
        Image.new("RGB", (64, 64)).save(f"{root}/inpaint/{below}/{iid}.png")
        if iid == "2":
            MC.write_pickle(f"{root}/init/{below}/{int(iid):06}.pickle", "NO HUMANS")
            continue
        MC.write_pickle(f"{root}/init/{below}/{int(iid):06}.pickle", dict(faces=sphere[1].astype(np.int64), displacement=placed))
        smplx_data = dict(transl=transl, seed=int(iid))
        J0 = D.convert_cam2real(body_model(smplx_data, None)[1], transl, (64, 64), cams[0], conv).astype(np.float64) + placed
        MC.write_pickle(f"{root}/pred/{below}/{int(iid):06}.pickle",
                        dict(smplx_data=smplx_data, convert_data=conv, joints_proj=T.render(J0.copy(), cams[0]).astype(np.float32)))
        for v in (1, 2, 3):                                                        # the other views saw the human at J0 + true_d front
            MC.write_pickle(f"{root}/pred/{sc}/{c}/{asset}/view:{v:05}/{mask}/{prompt}/{int(iid):06}.pickle",
                            dict(joints_proj=T.render(J0 + true_d[iid] * front, cams[v]).astype(np.float32)))
    args = cli.build_parser().parse_args(["--inpaint_dir", f"{root}/inpaint", "--camera_dir", f"{root}/cam", "--human_preds_dir", f"{root}/pred",
                                          "--human_initial_dir", f"{root}/init", "--save_dir", f"{root}/opt", "--asset_obj_root", f"{root}/data",
                                          "--num_epoch", "20", "--volume_resolution", "32", "--w_multiview", "1e-4",
                                          "--ransac_threshold", "2"])   # in px^2: the other item's predictions share the prompt directory and stay out
    done = cli.main(args, body_model=body_model)
    out = f"{root}/opt/{sc}/{c}/{asset}/view:00000/{mask}/{prompt}"
    assert [os.path.basename(p) for p in done] == ["000000.pickle", "000001.pickle"]
    with open(f"{out}/000002.pickle", "rb") as fh:
        assert pickle.load(fh) == "NO HUMANS"
    world = asset_world(box[0], cams[0], "BEHAVE")
    for iid in ("0", "1"):
        with open(f"{out}/{int(iid):06}.pickle", "rb") as fh:
            saved = pickle.load(fh)
        with open(f"{root}/pred/{sc}/{c}/{asset}/view:00000/{mask}/{prompt}/{int(iid):06}.pickle", "rb") as fh:
            pred = pickle.load(fh)
        v_cam, j_cam = body_model(pred["smplx_data"], None)
        V0, J0 = (D.convert_cam2real(x, transl, (64, 64), cams[0], conv).astype(np.float64) + placed for x in (v_cam, j_cam))
        item = dict(inpaint_pth=f"{root}/inpaint/{sc}/{c}/{asset}/view:00000/{mask}/{prompt}/{iid}.png")
        inliers = cli.find_inliers(pred["joints_proj"], item, f"{root}/pred", f"{root}/cam", 400, 2, 100, False, ["original", "full body"], None, "cuda")
        views, cand_view, cand_xy = D.inlier_views(inliers)
        a, b = SR.camera_frame(V0, cams[0]["R"]), SR.camera_frame(world, cams[0]["R"])
        grid = M.overlap_grid_xy(a, b, 32)
        ref_cols = SR.Columns(a, sphere[1], b, box[1], *grid)
        want = SR.optimize(ref_cols, views, J0[D.BODY_INDICES], front, cand_view, cand_xy, 0.0, 0.01, 1e-4, 0.4, 20)
        print(f"item {iid}: {len(inliers)} inliers, d {want['d']!r}, ratio {want['losses'][0, 1]:.4f} -> {want['losses'][-1, 1]:.4f}, "
              f"multiview loss {want['losses'][0, 0]:.3f} -> {want['losses'][-1, 0]:.3f}")
        assert saved["num_inliers"] == len(inliers) == 3 and want["losses"][0, 1] > 0.0 and want["d"] != 0.0
        assert saved["verts"].dtype == np.float32 and saved["faces"].dtype == np.uint32
        assert np.array_equal(saved["verts"], (V0 + want["d"] * front.reshape((1, 3))).astype(np.float32))
