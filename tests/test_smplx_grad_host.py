"""CPU: the f64 restatement of the SMPL-X body model's full backward (tests/smplx_grad_ref.py: gradients through vertices, joints and
full_pose to the pose, transl and the coefficients) against the third-party package's own lbs and SMPLX class under autograd in f64
(R64 of tests/golden/smplx_grad_golden.npz) and against central differences; the C ABI's new names; and the host half of
DeviceSMPLX's `differentiable` keyword."""
import os
import re

import numpy as np
import pytest
import torch

from tests import smplx_grad_ref as GR
from tests import smplx_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return GR.load_golden()


@pytest.mark.parametrize("name", S.CASE_NAMES)
def test_restatement_agrees_with_the_package_in_f64(golden, name):
    _, fm = S.case_model(name)
    inp = S.case_inputs(name)
    gJ, gP = GR.case_upstream(name)
    fwd = S.forward(fm, inp["coefficients"], inp["theta"], inp["transl"])
    for loss in GR.LOSSES:
        got = dict(zip(GR.QUANTITIES, GR.backward_full(fm, fwd, *GR.upstream(loss, inp["g"], gJ, gP))))
        for q in GR.QUANTITIES:
            want = golden[f"{name}__r64_{loss}_{q}"]
            dev = S.rel_dev(got[q], want)
            print(f"{name} {loss} {q}: {dev:.3e}")
            assert got[q].shape == want.shape and np.all(np.isfinite(got[q]))
            assert dev <= 1e-12, (loss, q, dev)


def test_restatement_agrees_with_the_package_s_class_in_f64(golden):
    """Every argument a leaf, betas and expression included; the 21 vertex picks and the 51 landmarks carry gradient too."""
    model, kw, g = S.class_case()
    gJ, gP = GR.class_upstream()
    fm = S.flat_model(model, n_pca=45)
    coef = np.concatenate([kw["betas"].reshape(-1), kw["expression"].reshape(-1)])
    fwd = S.forward(fm, coef, S.class_theta(kw), kw["transl"])
    idx, w = S.extra_joint_table(fm, GR.class_vertex_ids(S.load_golden(), fm, fwd))
    assert idx.shape == (21 + 51, 3)
    for loss in GR.LOSSES:
        got = dict(zip(GR.QUANTITIES, GR.backward_full(fm, fwd, *GR.upstream(loss, g, gJ, gP), idx=idx, w=w)))
        for q in GR.QUANTITIES:
            dev = S.rel_dev(got[q], golden[f"class__r64_{loss}_{q}"])
            print(f"class {loss} {q}: {dev:.3e}")
            assert dev <= 1e-12, (loss, q, dev)


def test_without_the_new_inputs_it_is_the_old_backward():
    _, fm = S.case_model("moderate")
    inp = S.case_inputs("moderate")
    fwd = S.forward(fm, inp["coefficients"], inp["theta"], inp["transl"])
    old = S.backward(fm, fwd, inp["g"])
    new = GR.backward_full(fm, fwd, inp["g"])
    assert np.array_equal(old[0], new[0]) and np.array_equal(old[1], new[1])


@pytest.mark.parametrize("name", ["zero", "moderate", "no_pca"])
def test_coefficient_and_joint_paths_against_central_differences(name):
    """The step and the bound of test_smplx_host.py::test_analytic_backward_against_central_differences.  The joints carry a vertex
    picked twice and landmarks whose faces contain it, so the scatter's repeated indices are differentiated too."""
    _, fm = S.case_model(name)
    inp = S.case_inputs(name)
    coef, theta, transl = (inp[k].astype(np.float64) for k in ("coefficients", "theta", "transl"))
    idx, w = S.extra_joint_table(fm, [7, 7])
    idx[2], idx[3, 1] = [7, 3, 7], 7
    rng = np.random.RandomState(11)
    gJ, gP = rng.normal(size=(fm["J"] + len(idx), 3)), rng.normal(size=3 * fm["J"])
    fwd = S.forward(fm, coef, theta, transl)
    h = 1e-6

    def numeric(up, which, x):
        args = dict(coefficients=coef, theta=theta, transl=transl)
        out = np.zeros_like(x)
        for k in range(x.size):
            e = np.zeros_like(x)
            e[k] = h
            hi, lo = dict(args, **{which: x + e}), dict(args, **{which: x - e})
            out[k] = (GR.loss_value(fm, g=up[0], gJ=up[1], gP=up[2], idx=idx, w=w, **hi) - GR.loss_value(fm, g=up[0], gJ=up[1], gP=up[2], idx=idx, w=w, **lo)) / (2 * h)
        return out

    for loss in ("all", "joints"):
        up = GR.upstream(loss, inp["g"].astype(np.float64), gJ, gP)
        g_pose, g_transl, g_coef = GR.backward_full(fm, fwd, *up, idx=idx, w=w)
        devs = dict(grad_coef=S.rel_dev(g_coef, numeric(up, "coefficients", coef)), grad_transl=S.rel_dev(g_transl, numeric(up, "transl", transl)),
                    grad_pose=S.rel_dev(g_pose, numeric(up, "theta", theta)))
        print(f"{name} {loss}: " + ", ".join(f"{k} {v:.3e}" for k, v in devs.items()))
        assert np.all(np.isfinite(g_coef)) and np.abs(g_coef).max() > 0
        for k, v in devs.items():
            assert v <= 1e-6, (loss, k, v)
    up = GR.upstream("full_pose", None, None, gP)
    g_pose, g_transl, g_coef = GR.backward_full(fm, fwd, *up)
    assert S.rel_dev(g_pose, numeric(up, "theta", theta)) <= 1e-6 and not g_transl.any() and not g_coef.any()


def test_new_names_are_in_the_header_and_the_ctypes_table(hip_lib):
    from coma_amd import _lib
    from tests.test_fit_layouts_host import PINNED
    header = open(os.path.join(ROOT, "include", "coma_hip.h")).read()
    for name in ("coma_smplx_grad_workspace_bytes", "coma_smplx_backward_full_f32"):
        assert re.search(rf"\b{name}\(", header), name
        assert name in _lib.SIGNATURES, name
    assert _lib.ABI_VERSION == 11 and hip_lib.coma_abi_version() == 11
    for name in ("coma_smplx_workspace_bytes", "coma_smplx_shape_state_bytes", "coma_smplx_saved_bytes"):
        for args, want in PINNED[name].items():
            assert int(getattr(hip_lib, name)(*args)) == want, (name, args)
    need = hip_lib.coma_smplx_grad_workspace_bytes
    # gvp, dA_part, dfeat as the backward has them, then g_eff [3V], dJ [3J] and the coefficient partials [ceil(3V / 256), NB], all f64
    assert need(10475, 55, 20) == 251408 + 82 * 663 * 8 + 486 * 8 + 251408 + 1328 + 123 * 20 * 8 and need(1, 1, 0) == 32 + 128 + 16 + 32 + 32 + 16
    assert need(10475, 55, 0) == need(10475, 55, 1) < need(10475, 55, 2)
    for bad in ((0, 55, 20), (100, 65, 20), (100, 55, -1), (100, 55, 1025)):
        assert need(*bad) == 0, bad


def test_full_backward_validates_before_any_launch(hip_lib):
    import ctypes as C
    one = C.c_void_p(16)                                        # never dereferenced: every call below is refused on the host
    parents = (C.c_int32 * 55)(*([-1] + [0] * 54))

    def call(gv=one, gj=None, gp=None, eidx=None, ew=None, E=0, sd=None, jr=None, NB=0, gc=None, V=100, J=55, hd=45, n_pca=45, par=parents,
             ws=one, ws_bytes=1 << 30, saved_bytes=1 << 30, gt=one):
        return hip_lib.coma_smplx_backward_full_f32(gv, gj, gp, one, one, par, one, eidx, ew, E, sd, jr, NB, V, J, hd, n_pca, one, one, saved_bytes,
                                                    gt, one, gc, ws, ws_bytes, None)
    err = hip_lib.coma_last_error
    assert call(gt=None) == -1 and b"null pointer" in err()
    for kw in (dict(V=0), dict(J=65)):
        assert call(**kw) == -1 and b"must lie in" in err(), kw
    assert call(n_pca=65) == -1 and b"n_pca" in err()
    assert call(hd=44) == -1 and b"hand_dim" in err()
    for E in (-1, 4097):
        assert call(E=E) == -1 and b"E=" in err(), E
    assert call(gj=one, E=3) == -1 and b"extra-joint tables" in err()
    assert call(gc=one, sd=one, jr=one, NB=0) == -1 and b"NB=0" in err()
    assert call(gc=one, sd=one, jr=one, NB=1025) == -1 and b"NB=1025" in err()
    assert call(gc=one, sd=None, jr=one, NB=20) == -1 and b"shapedirs" in err()
    assert call(gc=one, sd=one, jr=None, NB=20) == -1 and b"J_regressor" in err()
    assert call(ws_bytes=8) == -1 and b"workspace" in err()
    assert call(ws=C.c_void_p(8)) == -1 and b"aligned" in err()
    assert call(saved_bytes=8) == -1 and b"saved state" in err()
    bad = (C.c_int32 * 55)(*([-1] + [0] * 54))
    bad[7] = 7
    assert call(par=bad) == -1 and b"parent 7 of joint 7" in err()


def test_differentiable_keyword_is_validated_and_the_default_is_unchanged():
    from coma_amd._lib import ComaHipError
    from coma_amd.body_model import DeviceSMPLX
    model = S.synthetic_model(40, 55, 20, 6, seed=8)
    with pytest.raises(ValueError, match="nonsense"):
        DeviceSMPLX(model, n_pca=6, differentiable=("nonsense",))
    with pytest.raises(ValueError, match="differentiable"):
        DeviceSMPLX(model, n_pca=6, differentiable="joints")      # a bare string is a mistake, not a set of letters
    body = DeviceSMPLX(model, n_pca=6)
    assert body.differentiable == frozenset()
    with pytest.raises(ComaHipError, match="betas requires grad"):
        body(betas=torch.zeros(1, 10, requires_grad=True))
    only_joints = DeviceSMPLX(model, n_pca=6, differentiable=["joints", "full_pose"])
    assert only_joints.differentiable == {"joints", "full_pose"}
    with pytest.raises(ComaHipError, match="betas requires grad"):          # "shape" was not asked for
        only_joints(betas=torch.zeros(1, 10, requires_grad=True))
    with pytest.raises(ComaHipError, match="expression requires grad"):
        only_joints(betas=torch.zeros(1, 10), expression=torch.zeros(1, 10, requires_grad=True))
    assert DeviceSMPLX(model, n_pca=6, differentiable={"shape"}).differentiable == {"shape"}
