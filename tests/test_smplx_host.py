"""CPU: the f64 restatement of the SMPL-X body model (tests/smplx_ref.py) against the third-party package's own lbs and SMPLX class
executed in f64 (R64 of tests/golden/smplx_golden.npz), its analytic backward against central differences, and the host half of
coma_amd.body_model.DeviceSMPLX (key handling, refusals), the two CLIs' --body_model flag and the C ABI's new names."""
import os
import re

import numpy as np
import pytest
import torch

from tests import smplx_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return S.load_golden()


def _restated(name):
    _, fm = S.case_model(name)
    inp = S.case_inputs(name)
    fwd = S.forward(fm, inp["coefficients"], inp["theta"], inp["transl"])
    g_pose, g_transl = S.backward(fm, fwd, inp["g"])
    return dict(vertices=fwd["vertices"], joints=fwd["joints"], grad_pose=g_pose, grad_transl=g_transl)


@pytest.mark.parametrize("name", S.CASE_NAMES)
def test_restatement_agrees_with_the_package_in_f64(golden, name):
    inp = S.case_inputs(name)
    for key, v in inp.items():
        assert np.array_equal(golden[f"{name}__{key}"], v), key            # the seeded inputs are the stored ones
    got = _restated(name)
    for q in S.QUANTITIES:
        dev = S.rel_dev(got[q], golden[f"{name}__r64_{q}"])
        print(f"{name} {q}: {dev:.3e}")
        assert dev <= 1e-12, (q, dev)
        assert np.all(np.isfinite(got[q]))


def test_restatement_agrees_with_the_package_s_class_in_f64(golden):
    """Assembly (PCA, mean pose, concatenation order, transl), the extra joints' order and the landmarks, through SMPLX.forward."""
    from coma_amd import body_model as B
    model, kw, g = S.class_case()
    fm = S.flat_model(model, n_pca=45)
    coef = np.concatenate([kw["betas"].reshape(-1), kw["expression"].reshape(-1)])
    fwd = S.forward(fm, coef, S.class_theta(kw), kw["transl"])
    subset = S.class_subset()
    gs = np.zeros_like(g)
    gs[subset] = g[subset]
    g_pose, g_transl = S.backward(fm, fwd, gs)
    # 21 vertex picks sit between the posed joints and the landmarks; their ids are the package's and are not shipped, so they are
    # compared through the joints the fixture stores: every pick is some vertex of the model
    joints = golden["class__r64_joints"]
    assert joints.shape == (55 + 21 + 51, 3)
    got = dict(vertices=fwd["vertices"][subset], full_pose=fwd["full_pose"], grad_pose=g_pose, grad_transl=g_transl,
               joints=np.concatenate([fwd["joints"], S.extra_joints(fwd, *S.extra_joint_table(fm))]))
    want = dict(vertices=golden["class__r64_vertices"], full_pose=golden["class__r64_full_pose"], grad_pose=golden["class__r64_grad_pose"],
                grad_transl=golden["class__r64_grad_transl"], joints=np.concatenate([joints[:55], joints[76:]]))
    for q in want:
        dev = S.rel_dev(got[q], want[q])
        print(f"class {q}: {dev:.3e}")
        assert dev <= 1e-12, (q, dev)
    picks = joints[55:76]
    d = np.linalg.norm(fwd["vertices"][None] - picks[:, None], axis=-1).min(1)
    assert d.max() <= 1e-12 * np.abs(joints).max()
    assert len(B._FACE_FEET) + 2 * len(B._TIPS) == 21


@pytest.mark.parametrize("name", ["zero", "moderate", "no_pca"])
def test_analytic_backward_against_central_differences(name):
    _, fm = S.case_model(name)
    inp = S.case_inputs(name)
    theta, transl, g = inp["theta"].astype(np.float64), inp["transl"].astype(np.float64), inp["g"].astype(np.float64)
    fwd = S.forward(fm, inp["coefficients"], theta, transl)
    g_pose, g_transl = S.backward(fm, fwd, g)
    loss = lambda th, tr: float(np.sum(S.forward(fm, inp["coefficients"], th, tr)["vertices"] * g))
    h = 1e-6
    num = np.zeros_like(theta)
    for k in range(theta.size):
        e = np.zeros_like(theta)
        e[k] = h
        num[k] = (loss(theta + e, transl) - loss(theta - e, transl)) / (2 * h)
    num_t = np.array([(loss(theta, transl + h * np.eye(3)[k]) - loss(theta, transl - h * np.eye(3)[k])) / (2 * h) for k in range(3)])
    print(f"{name}: grad_pose {S.rel_dev(g_pose, num):.3e}, grad_transl {S.rel_dev(g_transl, num_t):.3e}")
    assert np.all(np.isfinite(g_pose))
    assert S.rel_dev(g_pose, num) <= 1e-6 and S.rel_dev(g_transl, num_t) <= 1e-6


def _write(tmp_path, model, nested=True):
    d = tmp_path / "models"
    (d / "smplx").mkdir(parents=True)
    pth = d / "smplx" / "SMPLX_NEUTRAL.npz"
    np.savez(pth, **model)
    return str(d if nested else pth)


def test_from_file_key_handling(tmp_path):
    from coma_amd.body_model import DeviceSMPLX
    model = S.synthetic_model(97, 55, 20, 45, "random", seed=5)
    for pth in (_write(tmp_path / "a", model), _write(tmp_path / "b", model, nested=False)):          # a directory (create's rule) or the file
        body = DeviceSMPLX.from_file(pth, num_pca_comps=12, extra_joint_vertex_ids=[3, 96])
        fm = S.flat_model(model, n_pca=12)
        assert (body.V, body.J, body.P, body.hand_dim, body.num_pca_comps) == (97, 55, 486, 45, 12)
        assert (body.num_betas, body.num_expression_coeffs, body.num_body, body.num_theta) == (10, 10, 63, 75 + 24)
        for key, ref in (("v_template", "v_template"), ("shapedirs", "shapedirs"), ("posedirs", "posedirs"), ("J_regressor", "J_regressor"),
                         ("weights", "weights"), ("hand_components", "comps"), ("pose_mean", "mean")):
            assert body.host[key].dtype == np.float32 and np.array_equal(body.host[key].astype(np.float64), fm[ref]), key
        assert np.array_equal(body.host["parents"], fm["parents"]) and np.array_equal(body.faces, fm["faces"])
        idx, w = S.extra_joint_table(fm, [3, 96])
        assert np.array_equal(body.host["extra_index"], idx) and np.array_equal(body.host["extra_weight"].astype(np.float64), w)
        assert body.extra_joint_source == "caller" and body.num_extra == 2 + 5
    flat = DeviceSMPLX.from_file(pth, flat_hand_mean=True)
    assert not flat.host["pose_mean"].any() and flat.extra_joint_source in ("landmarks only", "smplx.vertex_ids")
    raw = DeviceSMPLX.from_file(pth, use_pca=False)
    assert raw.host["hand_components"] is None and raw.num_theta == 165 and raw.hand_size == 45
    with pytest.raises(FileNotFoundError):
        DeviceSMPLX.from_file(str(tmp_path / "nowhere"))
    with pytest.raises(KeyError, match="weights"):
        DeviceSMPLX({k: v for k, v in model.items() if k != "weights"})


def test_shape_and_expression_slicing():
    from coma_amd.body_model import DeviceSMPLX
    model = S.synthetic_model(40, 55, 20, 6, seed=6)
    rng = np.random.RandomState(7)
    full = dict(model, shapedirs=(rng.normal(size=(40, 3, 400)) * 0.02).astype(np.float32))
    body = DeviceSMPLX(full, n_pca=6, num_betas=16, num_expression_coeffs=7)
    assert (body.num_betas, body.num_expression_coeffs) == (16, 7)
    assert np.array_equal(body.host["shapedirs"], np.concatenate([full["shapedirs"][:, :, :16], full["shapedirs"][:, :, 300:307]], -1))
    short = DeviceSMPLX(model, n_pca=6, num_betas=16, num_expression_coeffs=50)              # 20 directions: the short-file fallback
    assert (short.num_betas, short.num_expression_coeffs) == (10, 10)
    assert np.array_equal(short.host["shapedirs"], model["shapedirs"])
    sd, ed = S.split_shapedirs(full["shapedirs"], 16, 7)
    assert sd.shape[-1] == 16 and np.array_equal(ed, full["shapedirs"][:, :, 300:307])


def test_refusals():
    from coma_amd._lib import ComaHipError
    from coma_amd.body_model import DeviceSMPLX
    model = S.synthetic_model(40, 55, 20, 6, seed=8)
    with pytest.raises(ComaHipError, match="no CPU path"):
        DeviceSMPLX(model, n_pca=6, device="cpu")
    bad = dict(model, kintree_table=model["kintree_table"].copy())
    bad["kintree_table"][0, 7] = 9
    with pytest.raises(ValueError, match="parent"):
        DeviceSMPLX(bad, n_pca=6)
    body = DeviceSMPLX(model, n_pca=6)
    with pytest.raises(ValueError, match="batch size 1"):
        body(betas=torch.zeros(2, 10), body_pose=torch.zeros(2, 63))
    with pytest.raises(ValueError, match="batch size 1"):
        body(betas=torch.zeros(1, 10), body_pose=torch.zeros(2, 63))
    with pytest.raises(ComaHipError, match="betas requires grad"):
        body(betas=torch.zeros(1, 10, requires_grad=True))
    with pytest.raises(ComaHipError, match="expression requires grad"):
        body(betas=torch.zeros(1, 10), expression=torch.zeros(1, 10, requires_grad=True))


def test_clis_accept_the_device_body_model_and_default_to_the_package():
    from src.application import optimize as app
    from src.generation import optimize_depth as depth
    assert app.body_model_choice(app.build_parser().parse_args([])) == "smplx"
    assert app.body_model_choice(app.build_parser().parse_args(["--body_model", "device"])) == "device"
    assert depth.build_parser().parse_args([]).body_model == "smplx"
    assert depth.build_parser().parse_args(["--body_model", "device"]).body_model == "device"
    for parser in (app.build_parser(), depth.build_parser()):
        with pytest.raises(SystemExit):
            parser.parse_args(["--body_model", "eager"])
    try:
        import smplx  # noqa: F401
    except ImportError:
        with pytest.raises(RuntimeError, match="optimize: the `smplx` package is needed for the body model"):
            app.default_body_model("cpu")
        with pytest.raises(RuntimeError, match="optimize_depth: the `smplx` package is needed for the body model"):
            depth.default_body_model(dict(), "nowhere")
    with pytest.raises(FileNotFoundError):                      # --body_model device reads the model files itself
        depth.device_body_model(dict(), "nowhere")


def test_depth_stage_refuses_joints_without_the_vertex_picks(tmp_path):
    """The depth stage reads joints 55..65 (the package's vertex picks); without the id table the device model would put landmarks
    there, so --body_model device is refused unless the ids are supplied."""
    import json
    from src.generation import optimize_depth as depth
    pth = _write(tmp_path, S.synthetic_model(97, 55, 20, 45, "random", seed=5))
    try:
        import smplx  # noqa: F401
    except ImportError:
        with pytest.raises(RuntimeError, match="extra_joint_vertex_ids"):
            depth.device_body_model(dict(), pth)
        assert not depth._DEVICE_MODELS
    ids = tmp_path / "ids.json"
    ids.write_text(json.dumps(list(range(21))))
    assert depth.load_vertex_ids(str(ids)) == list(range(21))
    ids.write_text(json.dumps(list(range(20))))
    with pytest.raises(ValueError, match="21 vertex ids"):
        depth.load_vertex_ids(str(ids))
    assert depth.build_parser().parse_args(["--extra_joint_vertex_ids", "x.json"]).extra_joint_vertex_ids == "x.json"
    assert depth.build_parser().parse_args([]).extra_joint_vertex_ids is None


def test_new_names_are_in_the_header_and_the_ctypes_table():
    from coma_amd import _lib
    header = open(os.path.join(ROOT, "include", "coma_hip.h")).read()
    names = ("coma_smplx_workspace_bytes", "coma_smplx_shape_state_bytes", "coma_smplx_saved_bytes", "coma_smplx_shape_f32",
             "coma_smplx_forward_f32", "coma_smplx_backward_f32", "coma_smplx_extra_joints_f32")
    for name in names:
        assert re.search(rf"\b{name}\(", header), name
        assert name in _lib.SIGNATURES, name
    assert "COMA_ABI_VERSION 11" in header.replace("  ", " ") or _lib.ABI_VERSION == 11


def test_argument_validation_happens_before_any_launch(hip_lib):
    import ctypes as C
    need = hip_lib.coma_smplx_workspace_bytes
    assert need(0, 55) == 0 and need(100, 0) == 0 and need(100, 65) == 0 and need(10475, 55) > 8 * 3 * 10475 * 8
    one = C.c_void_p(16)                                        # never dereferenced: every call below is refused on the host
    parents = (C.c_int32 * 55)(*([-1] + [0] * 54))

    def forward(V=100, J=55, hd=45, n_pca=45, par=parents, theta=one, saved_bytes=1 << 30, ws_bytes=1 << 30):
        return hip_lib.coma_smplx_forward_f32(theta, None, one, one, par, one, None, V, J, hd, n_pca, one, one, one, None, one, saved_bytes, one,
                                              ws_bytes, None)
    assert forward(theta=None) == -1 and b"null pointer" in hip_lib.coma_last_error()
    for kw in (dict(V=0), dict(J=0), dict(J=65)):
        assert forward(**kw) == -1 and b"must lie in" in hip_lib.coma_last_error(), kw
    assert forward(n_pca=65) == -1 and b"n_pca" in hip_lib.coma_last_error()
    for hd in (-3, 44, 84):
        assert forward(hd=hd) == -1 and b"hand_dim" in hip_lib.coma_last_error(), hd
    bad = (C.c_int32 * 55)(*([-1] + [0] * 54))
    bad[7] = 7
    assert forward(par=bad) == -1 and b"parent 7 of joint 7" in hip_lib.coma_last_error()
    assert forward(saved_bytes=8) == -1 and b"saved state" in hip_lib.coma_last_error()
    assert forward(ws_bytes=8) == -1 and b"workspace" in hip_lib.coma_last_error()
    assert hip_lib.coma_smplx_shape_f32(one, one, one, one, 100, 55, 0, one, 1 << 30, None) == -1 and b"NB" in hip_lib.coma_last_error()
    assert hip_lib.coma_smplx_backward_f32(one, one, one, bad, one, 100, 55, 45, 45, one, one, 1 << 30, one, one, one, 1 << 30, None) == -1
    assert b"parent" in hip_lib.coma_last_error()
    assert hip_lib.coma_smplx_extra_joints_f32(None, None, None, None, 100, 3, None, None) == -1 and b"null pointer" in hip_lib.coma_last_error()
