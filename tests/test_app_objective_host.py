"""CPU: the optimisation app's ComA objective -- the restatement tests/app_ref.py pinned against the reference's own functions
(R64 of tests/golden/app_objective_golden.npz), the argument refusals of the new export (which return before any launch), the CLI
mirror's flag set, and the host halves of coma_amd.app."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest

from coma_amd import _lib
from tests import app_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fixture():
    return app_ref.load_golden()


@pytest.mark.parametrize("name", app_ref.CASES)
def test_restatement_agrees_with_the_reference_in_f64(fixture, name):
    g, meta = fixture
    c = app_ref.golden_case(g, meta, name)
    mine = app_ref.evaluate(c["verts"], c["faces"], c["gt"], c["obj_normal"], c["p"], c["sub_p"], c["eps"], c["sel"], c["targets"])
    dev = app_ref.deviations(mine, c)
    print(name, dev)
    assert all(v <= 1e-12 for v in dev.values()), dev
    # the isolated vertex (the last one) has no gradient, in the reference and in the restatement
    assert not c["r64_grad_orientation"][-1].any() and not mine["grad_orientation"][-1].any()


def test_fixture_covers_the_branches_and_is_small(fixture):
    g, meta = fixture
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "app_objective_golden.npz")) < 600_000
    assert set(app_ref.CASES) <= set(meta)
    assert meta["opposite_replacer"]["replacer"] and not meta["opposite"]["replacer"] and not meta["near"]["replacer"]
    assert meta["near"]["eps"] < meta["near"]["one_plus_b_dot_p"] < 5 * meta["near"]["eps"]
    assert sorted(m["k"] for n, m in meta.items() if n.startswith("small_k")) == [1, 7, 20, 25, 60]
    assert sorted(m["k"] for n, m in meta.items() if n.startswith("large_k")) == [300, 1000]
    for q in app_ref.QUANTITIES:
        assert 0 < float(g[f"e_reg_{q}"]) <= float(g[f"e_ref_{q}"]) < 0.05
    for name in app_ref.CASES:
        assert not any(np.isnan(g[f"{name}__r32_{key}"]).any() for key in ("terms", "grad_orientation", "grad_contact"))


def _call(lib, nulls=(), V=8, F=4, k=2, ws_bytes=1 << 20, eps=1e-6):
    one = C.c_void_p(16)          # never dereferenced: validation fails first
    args = dict(verts=one, faces=one, off=one, vf=one, gt=one, b=_lib.vec3([0, 0, 1]), p=_lib.vec3([0, 0, 1]), s=_lib.vec3([0, 1, 0]), sel=one,
                targets=one, terms=one, g_o=one, g_c=one, ws=one)
    for n in nulls:
        args[n] = None
    a = args
    return lib.coma_app_objective_f32(a["verts"], a["faces"], a["off"], a["vf"], V, F, a["gt"], a["b"], a["p"], a["s"], eps, a["sel"], a["targets"], k,
                                      a["terms"], a["g_o"], a["g_c"], a["ws"], ws_bytes, None)


def test_export_refuses_bad_arguments_before_any_launch(hip_lib):
    for name in ("verts", "faces", "off", "vf", "gt", "b", "p", "s", "sel", "targets", "terms", "g_o", "g_c", "ws"):
        assert _call(hip_lib, nulls=(name,)) == -1 and b"null pointer" in hip_lib.coma_last_error(), name
    for kw in (dict(V=0), dict(V=-3), dict(F=0), dict(F=-1)):
        assert _call(hip_lib, **kw) == -1 and b"bad sizes" in hip_lib.coma_last_error(), kw
    for kw in (dict(k=-1), dict(k=9)):
        assert _call(hip_lib, **kw) == -1 and b"outside [0, V" in hip_lib.coma_last_error(), kw
    assert _call(hip_lib, eps=-1.0) == -1 and b"eps" in hip_lib.coma_last_error()
    assert _call(hip_lib, ws_bytes=8) == -1 and b"workspace" in hip_lib.coma_last_error()
    need = hip_lib.coma_app_objective_workspace_bytes
    assert need(0, 4, 0) == 0 and need(8, 0, 0) == 0 and need(8, 4, -1) == 0 and need(8, 4, 9) == 0
    assert need(8, 4, 0) >= 8 * 3 * 8 and need(10475, 20908, 5000) > need(10475, 20908, 500) > need(10475, 20908, 0)


def test_cli_flag_set_and_defaults():
    from src.application import optimize as app
    parser = app.build_parser()
    args = parser.parse_args([])
    assert vars(args) == dict(supercategory=None, category=None, coma_path=None, save_dir="output/", asset_downsample_pth=None, eps=1e-6, lr=1e-2,
                              body_pose_weight=10000, bending_prior_weight=31700, pprior_weight=1e-6, orientation_weight=1e12,
                              contact_weight=2.6e11, contact_threshold=0.3, scale_factor=0.84, use_collision=False, num_iters=2000)
    with pytest.raises(SystemExit):
        parser.parse_args(["--no_such_flag", "1"])
    with pytest.raises(SystemExit):
        parser.parse_args(["--contact", "1"])          # no abbreviations either


def test_use_collision_is_refused():
    from src.application import optimize as app
    args = app.build_parser().parse_args(["--use_collision"])
    with pytest.raises(SystemExit, match="COAP"):
        app.main(args)
    kw = dict(supercategory="s", category="c", coma_path={}, asset_downsample_pth={}, eps=1e-6, principle_vec=[0, 0, 1], sub_principle_vec=[0, 1, 0],
              reference_object_vertex_index=0, lr=1e-2, body_pose_weight=1.0, bending_prior_weight=1.0, pprior_weight=1.0, orientation_weight=1.0,
              contact_weight=1.0, contact_threshold=0.3, scale_factor=1.0)
    with pytest.raises(NotImplementedError, match="COAP"):
        app.optimize_smpl(use_collision=True, **kw)


def test_missing_third_party_hooks_say_so():
    from src.application import optimize as app
    with pytest.raises(RuntimeError, match="VPoser"):
        app.default_pose_decoder("cpu")
    with pytest.raises(RuntimeError, match="angle prior"):
        app.default_angle_prior("cpu")


def test_obj_writer_round_trips(tmp_path):
    from coma_amd.downsample import load_obj
    from src.application.optimize import write_obj
    verts, faces = app_ref.grid_mesh(5, seed=3)
    pth = str(tmp_path / "optimized.obj")
    write_obj(pth, verts, faces)
    v, f = load_obj(pth)
    assert np.array_equal(v.astype(np.float32), verts) and np.array_equal(f, faces)
    lines = open(pth).read().split("\n")
    assert all(l.startswith(("v ", "f ")) for l in lines if l)


def test_state_targets_select_what_the_pinned_consumer_selects(tmp_path):
    """The host half of ComaObjective.from_state on the reference's own exported state, with the pinned oracle of the consumer
    vectors (G17) standing in for the device selection."""
    from coma_amd.app import state_targets
    from oracle import coma_oracle as orc
    state = os.path.join(ROOT, "tests", "golden", "ref_coma_small.pickle")
    with open(state, "rb") as fh:
        info = pickle.load(fh)
    H, O = info["contact_dist_expectation_grid_nom"].shape
    rng = np.random.default_rng(5)
    asset = dict(downsampled_pcd_points_raw=rng.normal(size=(O, 3)), downsampled_pcd_normal_raw=rng.normal(size=(O, 3)))
    asset_pth = str(tmp_path / "asset.pickle")
    with open(asset_pth, "wb") as fh:
        pickle.dump(asset, fh)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = (info["contact_dist_expectation_grid_nom"] / info["contact_dist_expectation_grid_denom"]).max(1)
    seen = set()
    for o_ref in (0, O - 1):
        for thr in (0.0, float(np.median(ratio)), 10.0):
            gt, normal, selected, points = state_targets(state, asset_pth, o_ref, thr, select=orc.orientation_and_contact_targets)
            _, want_gt, want_sel, want_obj = orc.orientation_and_contact_targets(info, o_ref, thr)
            assert np.array_equal(gt, want_gt) and gt.shape == (H, 3)
            assert np.array_equal(selected, want_sel[0]) and np.array_equal(points, asset["downsampled_pcd_points_raw"][want_obj])
            assert np.array_equal(normal, asset["downsampled_pcd_normal_raw"][o_ref])
            seen.add(len(selected))
    assert 0 in seen and max(seen) > 0


def test_objective_checks_indices_on_the_host():
    from coma_amd.app import ComaObjective
    verts, faces = app_ref.grid_mesh(4, seed=1)
    gt = np.zeros((len(verts), 3), np.float32)
    bad = faces.copy()
    bad[3, 1] = len(verts)
    with pytest.raises(IndexError, match="faces"):
        ComaObjective(bad, gt, [0, 0, 1], [1, 2], np.zeros((2, 3)))
    with pytest.raises(IndexError, match="selected_human_indices"):
        ComaObjective(faces, gt, [0, 0, 1], [1, len(verts)], np.zeros((2, 3)))
    with pytest.raises(IndexError, match="selected_human_indices"):
        ComaObjective(faces, gt, [0, 0, 1], [-1, 2], np.zeros((2, 3)))
    with pytest.raises(ValueError, match="distinct"):
        ComaObjective(faces, gt, [0, 0, 1], [2, 2], np.zeros((2, 3)))
    with pytest.raises(ValueError, match="target_points"):
        ComaObjective(faces, gt, [0, 0, 1], [1, 2], np.zeros((3, 3)))
    with pytest.raises(_lib.ComaHipError, match="no CPU path"):
        ComaObjective(faces, gt, [0, 0, 1], [1, 2], np.zeros((2, 3)), device="cpu")
