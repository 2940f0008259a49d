"""CPU: the depth-optimisation rule set as restated in tests/shift_ref.py -- the shift profile against a closed form, the multiview
term and Adam against the reference's own trajectory (tests/golden/depth_opt_golden.npz) -- the host mirrors of coma_amd/depth_opt.py,
and the work list, sentinels, directories and pickles of src/generation/optimize_depth.py with the device calls replaced."""
import os
import pickle

import numpy as np
import pytest

from tests import metrics_common as MC
from tests import raster_ref as RR
from tests import shift_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# max |d_ref - d_restated| over the 201 displacements, measured by tests/golden/make_golden_depth_opt.py (f32 autograd against the f64
# restatement over 200 steps): far 7.369e-07, converge 7.509e-08.  Four times that is allowed.
MEASURED = dict(far=7.369e-07, converge=7.509e-08)


@pytest.fixture(scope="module")
def golden_opt():
    return np.load(os.path.join(ROOT, "tests", "golden", "depth_opt_golden.npz"), allow_pickle=False)


def test_box_profile_matches_closed_form_over_the_full_slide():
    # grid of 8 x 8 unit cells: A covers columns [1, 5) x [2, 6), z in [0.25, 2.0); B covers [3, 8) x [0, 4), z in [1.0, 3.0)
    A, B = RR.box((1.0, 2.0, 0.25), (5.0, 6.0, 2.0)), RR.box((3.0, 0.0, 1.0), (8.0, 4.0, 3.0))
    cols = SR.Columns(A[0], A[1], B[0], B[1], 0.0, 0.0, 1.0, 8, 8)
    assert cols.L_A == 16 * 448 and cols.L_B == 20 * 512
    a_lo, a_hi, b_lo, b_hi = (1, 2, 64), (5, 6, 512), (3, 0, 256), (8, 4, 768)
    seen = set()
    for delta in range(-300, 760):                            # from no overlap below, through full containment, to no overlap above
        want = SR.box_pair_closed_form(a_lo, a_hi, b_lo, b_hi, delta)
        assert cols.L_AB(delta) == want, delta
        seen.add(want)
    assert 0 in seen and 4 * 448 in seen                      # 2 x 2 shared columns; A's 448 fit inside B's 512
    assert cols.L_AB(-300) == 0 and cols.L_AB(759) == 0
    prof = cols.profile([0.0, 1.0, -50.0])
    assert prof[0].tolist() == [SR.box_pair_closed_form(a_lo, a_hi, b_lo, b_hi, k) for k in (-1, 0, 1)]
    assert prof[1].tolist() == [SR.box_pair_closed_form(a_lo, a_hi, b_lo, b_hi, k) for k in (255, 256, 257)]
    assert prof[2].tolist() == [0, 0, 0]


def test_shift_rounding_and_clamp():
    assert SR.shift_of(0.0, 3.0) == 0 and SR.shift_of(1.0 / 512, 1.0) == 1 and SR.shift_of(-1.0 / 512, 1.0) == 0
    assert SR.shift_of(1e300, 1.0) == 2 ** 42 and SR.shift_of(-1e300, 1.0) == -2 ** 42
    assert SR.shift_of(float("nan"), 1.0) == 2 ** 42 and SR.shift_of(float("inf"), 1.0) == 2 ** 42


def _golden_case(g, tag):
    from coma_amd.triangulate import view_record
    idx = g["body_indices"]
    views = np.stack([view_record(dict(R=R.astype(np.float64), t=t.astype(np.float64), scale=float(s), resolution=tuple(int(r) for r in res)))
                      for R, t, s, res in zip(g[f"{tag}_cam_R"], g[f"{tag}_cam_t"], g[f"{tag}_cam_scale"], g[f"{tag}_cam_res"])])
    lr, w = g[f"{tag}_params"]
    return dict(views=views, joints0=g[f"{tag}_joints0"].astype(np.float64)[idx], front=g[f"{tag}_front"].astype(np.float64),
                cand_view=np.arange(len(views)), cand_xy=g[f"{tag}_xy"].astype(np.float64)[:, idx], lr=float(lr), w=float(w))


@pytest.mark.parametrize("tag", ["far", "converge"])
def test_restatement_follows_the_reference_trajectory(golden_opt, tag):
    from coma_amd import depth_opt as D
    assert np.array_equal(golden_opt["body_indices"], D.BODY_INDICES) and len(D.BODY_INDICES) == 25
    c = _golden_case(golden_opt, tag)
    ref_traj, ref_loss = golden_opt[f"{tag}_traj"], golden_opt[f"{tag}_losses"]
    E = len(ref_loss)
    assert E == 200
    got = SR.optimize(None, c["views"], c["joints0"], c["front"], c["cand_view"], c["cand_xy"], 0.0, c["lr"], c["w"], 0.0, E)
    err = float(np.abs(got["traj"] - ref_traj).max())
    loss_err = float(np.abs(got["losses"][:, 0] / ref_loss - 1.0).max())
    print(f"{tag}: d ends at {got['d']!r} (reference {ref_traj[-1]!r}), max |d_ref - d_restated| {err:.3e} (measured {MEASURED[tag]:.3e}), "
          f"max relative loss difference {loss_err:.3e}")
    assert err <= 4.0 * MEASURED[tag]
    assert loss_err <= 1e-4                                   # f32 sums of 50 squares of a few hundred pixels: ~1e-6 observed
    steps = np.diff(got["traj"])
    if tag == "far":                                          # the optimum (5.0) is farther than lr * E = 2: every step goes the same way
        assert (steps > 0).all() and got["d"] < c["lr"] * E
    else:
        assert abs(got["d"] - 0.3) < 0.01 and (steps < 0).any()
    assert not got["Ltraj"].any() and not got["losses"][:, 1].any()


def test_multiview_gradient_is_the_derivative_of_the_loss(golden_opt):
    c = _golden_case(golden_opt, "converge")
    args = (c["views"], c["joints0"], c["front"], c["cand_view"], c["cand_xy"])
    for d in (-0.7, 0.0, 0.25):
        h = 1e-5
        num = (SR.multiview(d + h, *args)[0] - SR.multiview(d - h, *args)[0]) / (2 * h)
        assert abs(SR.multiview(d, *args)[1] - num) <= 1e-6 * max(1.0, abs(num))      # the loss is a quadratic in d


def test_overlap_grid_xy_ignores_z():
    from coma_amd import metrics as M
    A, B = RR.box((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), RR.box((0.5, 0.25, 7.0), (2.0, 2.0, 9.0))
    assert M.overlap_grid(A[0], B[0], 32) is None                                      # apart in z
    x0, y0, s, W, H = M.overlap_grid_xy(A[0], B[0], 32)
    near = (B[0] - np.array([0.0, 0.0, 6.5]), B[1])
    assert (x0, y0, s, W, H) == M.overlap_grid(A[0], near[0], 32) == (0.5, 0.25, 32 / 0.75, 22, 32)
    assert M.overlap_grid_xy(A[0], B[0] + np.array([1.0, 0.0, 0.0]), 32) is None       # apart in x
    assert M.overlap_grid_xy(A[0], B[0] + np.array([0.5, 0.0, 0.0]), 32) is None       # only touching
    G = MC.grazing_pair()
    assert M.overlap_grid_xy(G[0][0], G[1][0], 512) == M.overlap_grid(G[0][0], G[1][0], 512)   # the same cap on the scale


def test_convert_cam2real_ends_in_the_pixel_to_world_chain():
    from coma_amd import depth_opt as D
    from src.generation.initialize_depth import human_world
    rng = np.random.default_rng(5)
    verts = rng.normal(size=(40, 3)).astype(np.float32)
    transl = np.array([[0.1, -0.2, 4.0]], dtype=np.float32)
    eye = np.array([0.0, -3.0, 0.5])
    cam = dict(R=RR.look_at(eye, (0.0, 0.0, 0.5)), t=eye, scale=2.4)
    conv = dict(focals=(5000.0, 4800.0), princpt=(250.0, 260.0), z_mean=4.1)
    res = (512, 384)
    keep = verts.copy()
    got = D.convert_cam2real(verts, transl, res, cam, conv)
    assert got.dtype == np.float32 and got.shape == (40, 3) and np.array_equal(verts, keep)
    pix = (verts.astype(np.float64) + transl.astype(np.float64)) * np.array([5000.0, 4800.0, 4900.0]) / 4.1
    pix += np.array([250.0, 260.0, 500.0 - pix[:, 2].mean()])
    want, _ = human_world(pix, np.zeros(3), cam, res)
    assert abs(pix[:, 2].mean() - 500.0) < 1e-9 and np.abs(got - want).max() <= 2e-5 * np.abs(want).max()


# ---- the CLI, device calls replaced ----
SC, C_, ASSET, VIEW, MASK = "BEHAVE", "backpack", "behave_asset", "view:00000", "mask:000"
PROMPT = "sitting on the backpack, full body"


def _tree(root, items, prompt=PROMPT, initial_dir="init"):
    """items: {inpaint id: what the depth initialisation left (dict or sentinel)}"""
    from PIL import Image
    eye = np.array([0.0, -3.0, 0.5])
    cam = dict(R=RR.look_at(eye, (0.0, 0.0, 0.5)), t=eye, scale=2.4, resolution=(64, 64), obj_R=np.eye(3), obj_t=np.zeros((3, 1)))
    MC.write_pickle(f"{root}/cam/{SC}/{C_}/{ASSET}/{VIEW}.pickle", cam)
    MC.write_obj(f"{root}/data/BEHAVE/objects/{C_}/{C_}_canon_lowres_in_gen_coord.obj", *RR.box((-0.5, 0.0, -0.5), (0.5, 1.0, 0.5)))
    for iid, initial in items.items():
        below = f"{SC}/{C_}/{ASSET}/{VIEW}/{MASK}/{prompt}"
        os.makedirs(f"{root}/inpaint/{below}", exist_ok=True)
        Image.new("RGB", (64, 64)).save(f"{root}/inpaint/{below}/{iid}.png")
        if initial is not None:
            MC.write_pickle(f"{root}/{initial_dir}/{below}/{int(iid):06}.pickle", initial)
        MC.write_pickle(f"{root}/pred/{below}/{int(iid):06}.pickle",
                        dict(smplx_data=dict(transl=np.array([[0.0, 0.0, 4.0]], dtype=np.float32), seed=int(iid)),
                             joints_proj=np.zeros((137, 2), dtype=np.float32),
                             convert_data=dict(focals=(5000.0, 5000.0), princpt=(32.0, 32.0), z_mean=4.0)))
    return cam


def _body_model(smplx_data, smplx_path):
    rng = np.random.default_rng(smplx_data["seed"])
    v, _ = RR.icosphere(1, 0.3)
    return v.astype(np.float32), rng.normal(scale=0.2, size=(137, 3)).astype(np.float32)


def _args(cli, root, *extra):
    return cli.build_parser().parse_args(["--inpaint_dir", f"{root}/inpaint", "--camera_dir", f"{root}/cam", "--human_preds_dir", f"{root}/pred",
                                          "--human_initial_dir", f"{root}/init", "--save_dir", f"{root}/opt", "--asset_obj_root", f"{root}/data",
                                          "--smplx_path", "unused", *extra])


def _load(pth):
    with open(pth, "rb") as fh:
        return pickle.load(fh)


@pytest.fixture
def patched_cli(monkeypatch):
    from src.generation import optimize_depth as cli
    calls = []

    def inliers(joints_proj, item, *a):
        n = int(os.path.basename(item["save_path"]).split(".")[0])
        return [dict(joints_MSE=1.0)] * (n % 3)                # 000000: none, 000001: one, 000002: two

    def solve(human_verts, human_faces, asset_verts, asset_faces, cam_R, joints, found, lr, w_multiview, w_collision, num_epoch, *a):
        calls.append(dict(w_collision=w_collision, asset=asset_verts, n=len(found), lr=lr, num_epoch=num_epoch, joints=joints))
        return 0.125 * len(found)
    monkeypatch.setattr(cli, "find_inliers", inliers)
    monkeypatch.setattr(cli, "solve_displacement", solve)
    return cli, calls


def test_cli_defaults_are_the_references():
    from src.generation import optimize_depth as cli
    a = cli.build_parser().parse_args([])
    assert (a.maximum_candidates, a.ransac_threshold, a.triangulation_threshold, a.num_epoch, a.minimum_inliers) == (400, 200, 100, 200, 1)
    assert (a.lr, a.w_collision, a.w_multiview, a.w_refview) == (0.01, 0.4, 1e-3, 0.0)
    assert a.allowed_viewpoint_prompts == ["original", "full body"] and a.human_initial_dir.endswith("human_before_opt")
    assert a.save_dir.endswith("human_after_opt") and a.smplx_path.endswith("human_model_files/") and a.parallel_num == 1
    with pytest.raises(RuntimeError, match="smplx"):
        cli.default_body_model(dict(), "nowhere")


def test_cli_sentinels_pickles_and_skip_done(tmp_path, patched_cli):
    from coma_amd import depth_opt as D
    cli, calls = patched_cli
    root = str(tmp_path)
    faces = RR.icosphere(1, 0.3)[1].astype(np.int64)
    moved = np.array([[0.0, 0.5, 0.0]])
    items = {"0": dict(faces=faces, displacement=moved), "1": dict(faces=faces, displacement=moved), "2": dict(faces=faces, displacement=None),
             "3": "NO HUMANS", "4": "MORE THAN 2 HUMANS", "5": "LARGELY PENETRATED HUMAN", "6": "ERRONEOUS SAMPLE DUE TO TOO SMALL HUMAN", "7": None}
    cam = _tree(root, items)
    _tree(root, {"8": dict(faces=faces, displacement=moved)}, prompt="sitting on the backpack, from above")
    done = cli.main(_args(cli, root, "--lr", "0.02", "--num_epoch", "7"), body_model=_body_model)
    out = f"{root}/opt/{SC}/{C_}/{ASSET}/{VIEW}/{MASK}/{PROMPT}"
    assert [os.path.basename(p) for p in done] == ["000000.pickle", "000001.pickle", "000002.pickle"]
    assert sorted(os.listdir(out)) == [f"{k:06}.pickle" for k in range(7)]           # 7 has no initial human: skipped without a trace
    assert _load(f"{out}/000000.pickle") == "TOO LITTLE INLIERS"
    for k in (3, 4, 5, 6):
        assert _load(f"{out}/{k:06}.pickle") == items[str(k)]
    assert _load(f"{root}/opt/{SC}/{C_}/{ASSET}/{VIEW}/{MASK}/sitting on the backpack, from above/000008.pickle") == "NOT ALLOWED VIEWPOINT PROMPTS"
    assert [c["n"] for c in calls] == [1, 2] and all(c["w_collision"] == 0.4 and c["lr"] == 0.02 and c["num_epoch"] == 7 for c in calls)
    assert all(c["asset"] is not None and np.allclose(c["asset"].min(axis=0), [-0.5, -0.5, 0.0]) for c in calls)
    front = cam["R"][:, 2].reshape((1, 3))
    for k, placed in ((1, moved), (2, np.zeros((1, 3)))):
        saved = _load(f"{out}/{k:06}.pickle")
        assert sorted(saved) == ["faces", "num_inliers", "verts"] and saved["num_inliers"] == k
        assert saved["verts"].dtype == np.float32 and saved["faces"].dtype == np.uint32 and np.array_equal(saved["faces"], faces)
        pred = _load(f"{root}/pred/{SC}/{C_}/{ASSET}/{VIEW}/{MASK}/{PROMPT}/{k:06}.pickle")
        v_cam, j_cam = _body_model(pred["smplx_data"], None)
        V0 = D.convert_cam2real(v_cam, pred["smplx_data"]["transl"], cam["resolution"], cam, pred["convert_data"]).astype(np.float64) + placed
        assert np.array_equal(saved["verts"], (V0 + 0.125 * k * front).astype(np.float32))
        J0 = D.convert_cam2real(j_cam, pred["smplx_data"]["transl"], cam["resolution"], cam, pred["convert_data"]).astype(np.float64) + placed
        assert np.array_equal(calls[k - 1]["joints"], J0)
    # --skip_done: nothing is recomputed, the files stay as they are
    before = {f: os.path.getmtime(f"{out}/{f}") for f in os.listdir(out)}
    n_calls = len(calls)
    assert cli.main(_args(cli, root, "--skip_done"), body_model=_body_model) == [] and len(calls) == n_calls
    assert before == {f: os.path.getmtime(f"{out}/{f}") for f in os.listdir(out)}
    os.remove(f"{out}/000002.pickle")
    assert [os.path.basename(p) for p in cli.main(_args(cli, root, "--skip_done"), body_model=_body_model)] == ["000002.pickle"]


def test_cli_suffix_directories_total_prompts_and_slices(tmp_path, patched_cli):
    cli, calls = patched_cli
    root = str(tmp_path)
    faces = RR.icosphere(1, 0.3)[1].astype(np.int64)
    items = {str(k): dict(faces=faces, displacement=None) for k in (1, 2, 4, 5, 7)}
    _tree(root, items, initial_dir="init_no_initialize")
    _tree(root, {}, initial_dir="init")
    # --no_initialize reads {initial}_no_initialize and writes {save}_no_initialize; --no_collision appends its own suffix and zeroes the weight
    done = cli.main(_args(cli, root, "--no_initialize", "--no_collision", "--enable_aggregate_total_prompts"), body_model=_body_model)
    out = f"{root}/opt_no_initialize_no_collision/{SC}/{C_}/{ASSET}/{VIEW}/{MASK}/total:{PROMPT}"
    assert [p for p in done] == [f"{out}/{k:06}.pickle" for k in (1, 2, 4, 5, 7)]
    assert all(c["w_collision"] == 0.0 and c["asset"] is None for c in calls) and not os.path.exists(f"{root}/opt")
    assert cli.main(_args(cli, root), body_model=_body_model) == []                  # the plain directory holds no initial humans
    # slices of len // n + 1 = 5 // 2 + 1 = 3 items of the list sorted by save path; a slice past the end is empty
    got = [[os.path.basename(p) for p in cli.main(_args(cli, root, "--no_initialize", "--save_dir", f"{root}/s", "--parallel_num", "2", "--parallel_idx", str(i)),
                                                  body_model=_body_model)] for i in range(2)]
    assert got == [["000001.pickle", "000002.pickle", "000004.pickle"], ["000005.pickle", "000007.pickle"]]
    assert cli.main(_args(cli, root, "--no_initialize", "--save_dir", f"{root}/s5", "--parallel_num", "5", "--parallel_idx", "3"), body_model=_body_model) == []


def test_exports_validate_their_arguments_before_any_launch(hip_lib):
    import ctypes as C
    one = C.c_void_p(16)   # never dereferenced: argument validation fails first
    front = (C.c_double * 3)(0.0, 0.0, 1.0)
    assert hip_lib.coma_shift_columns_workspace_bytes(1, 1, 1, 1, 8, 8, 0) == 0
    plain, shift = (fn(8, 12, 8, 12, 20, 10, 1000) for fn in (hip_lib.coma_column_crossings_workspace_bytes, hip_lib.coma_shift_columns_workspace_bytes))
    assert shift == 64 + (plain + 15) // 16 * 16 + 4 * 200          # the parameter block, the columns workspace, one split per column
    assert hip_lib.coma_shift_columns_prepare(one, 1, one, 1, one, 1, one, 1, 0.0, 0.0, 0.0, 8, 8, 1, one, None, None) == -1
    assert b"positive and finite" in hip_lib.coma_last_error()
    assert hip_lib.coma_shift_columns_prepare(one, 1, one, 1, one, 1, one, 1, 0.0, 0.0, 1.0, 9000, 8, 1, one, None, None) == -1
    assert hip_lib.coma_shift_columns_prepare(one, 1, one, 1, one, 1, one, 1, 0.0, 0.0, 1.0, 8, 8, 1, C.c_void_p(8), None, None) == -1
    assert b"16-byte aligned" in hip_lib.coma_last_error()
    for K in (0, 65):
        assert hip_lib.coma_shift_profile(one, one, K, one, None) == -1 and b"outside [1, 64]" in hip_lib.coma_last_error()
    assert hip_lib.coma_shift_profile(None, one, 1, one, None) == -1 and hip_lib.coma_shift_columns_status(None, None, None) == -1

    def optimize(E=10, N=0, J=25, d0=0.0, lr=0.01, views=None, state=one):
        return hip_lib.coma_depth_optimize_f64(None, views, 1, views, front, views, views, N, J, d0, lr, 1e-3, 0.0, E, one, one, one, state, None)
    for bad in (dict(E=0), dict(E=4097), dict(N=-1), dict(N=65537), dict(J=0), dict(J=1025), dict(d0=float("nan")), dict(lr=float("inf")),
                dict(N=3), dict(state=None), dict(state=C.c_void_p(12))):
        assert optimize(**bad) == -1, bad
    assert hip_lib.coma_depth_optimize_state_bytes() == 64 and hip_lib.coma_depth_optimize_status(None, None, None) == -1
