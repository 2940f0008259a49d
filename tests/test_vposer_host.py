"""CPU: the f64 restatement tests/vposer_ref.py against the reference's own VPoser, rotation_matrix_to_angle_axis and SMPLifyAnglePrior
executed in f64 (R64 of tests/golden/vposer_golden.npz), its backward against central differences, and the host side of
coma_amd.pose_prior and of the app's --pose_prior flag.  No kernel is launched here; only refusals that return before any launch.

Bounds.  F64_TOL: two f64 evaluations of one formula in different summation orders: eps64 = 1.1e-16 times the 512 terms of a row times
three layers is 2e-13, times the tail's conditioning near an angle of pi (the derivative of atan2 over a sine, some tens) -- 1e-11.
FD_TOL: a central difference with step 1e-6 in f64 carries eps64 / step = 1e-10 of rounding and step^2 = 1e-12 of truncation, both
times the same conditioning -- 1e-6 relative to the directional derivative."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import vposer_ref as V

F64_TOL, FD_TOL = 1e-11, 1e-6


@pytest.fixture(scope="module")
def golden():
    return V.load_golden()


@pytest.fixture(scope="module")
def restated():
    return {name: V.restate(name) for name in V.CASE_NAMES}


@pytest.mark.parametrize("name", V.CASE_NAMES)
def test_restatement_matches_the_reference_in_f64(golden, restated, name):
    r = restated[name]
    for q in V.QUANTITIES + ("matrot",):
        dev = V.rel_dev(r[q], golden[f"{name}__r64_{q}"])
        print(f"{name} {q}: {dev:.3e}")
        assert r[q].shape == golden[f"{name}__r64_{q}"].shape and dev <= F64_TOL, (q, dev)


@pytest.mark.parametrize("name", V.CASE_NAMES)
def test_branch_ids_are_the_reference_s(golden, restated, name):
    assert np.array_equal(restated[name]["branch"], golden[f"{name}__r64_branch"])


def test_cases_cover_what_they_are_named_for(golden, restated):
    for name in ("branches", "odd"):
        assert sorted(set(golden[f"{name}__r64_branch"].reshape(-1).tolist())) == [0, 1, 2, 3], name
    assert (restated["cos_negative"]["q"][..., 0] < 0).any()
    angle = lambda name: np.linalg.norm(golden[f"{name}__r64_aa"].reshape(-1, 3), axis=1)
    assert angle("small_angle").max() < 1e-2 and angle("small_angle").min() > 0
    assert angle("near_rest").max() < 0.5 and angle("random_init").max() > 1.0
    assert golden["batch3__r64_aa"].shape == (3, 63) and golden["odd__r64_aa"].shape == (1, 15)
    for q in V.QUANTITIES:                                      # no case is ill-conditioned for the reference's f32: one pool
        assert float(golden[f"e_reg_{q}"]) <= float(golden[f"e_ref_{q}"]) < 2e-6
        if not V.ILL_CONDITIONED:
            assert float(golden[f"e_reg_{q}"]) == float(golden[f"e_ref_{q}"])


@pytest.mark.parametrize("name", V.CASE_NAMES)
def test_backward_against_central_differences(name):
    w, inp = V.case_weights(name), V.case_inputs(name)
    z, g = inp["z"].astype(np.float64), inp["g"].astype(np.float64)
    fwd = V.decode(w, z)
    gz = V.decode_backward(w, fwd, g)
    loss = lambda zz: float(np.sum(V.decode(w, zz, branch=fwd["branch"])["aa"] * g))
    rng = np.random.RandomState(7)
    step = 1e-6
    for _ in range(3):
        v = rng.normal(size=z.shape)
        want = (loss(z + step * v) - loss(z - step * v)) / (2 * step)
        got = float(np.sum(gz * v))
        print(f"{name}: analytic {got:.9e}  central difference {want:.9e}")
        assert abs(got - want) <= FD_TOL * max(abs(want), np.abs(gz).max())
    pose, pg = inp["prior_pose"].astype(np.float64), inp["prior_g"].astype(np.float64)
    gp = V.angle_prior_backward(pose, pg)
    v = rng.normal(size=pose.shape)
    want = (np.sum(V.angle_prior(pose + step * v) * pg) - np.sum(V.angle_prior(pose - step * v) * pg)) / (2 * step)
    assert abs(np.sum(gp * v) - want) <= FD_TOL * max(abs(want), np.abs(gp).max())
    assert np.count_nonzero(gp) == 4 * len(pose)


def test_identity_has_the_finite_gradient_of_the_k_2_branch():
    """DEVIATION from the reference (NaN there): at the exact identity k is the constant 2 and aa = 2 (q1, q2, q3)."""
    o = np.array([[1.0, 0.0, 0.0, 1.0, 0.0, 0.0]])
    f = V.tail_forward(o)
    assert f["branch"][0] == 3 and np.array_equal(f["aa"], np.zeros((1, 3))) and f["s2"][0] == 0.0
    go = V.tail_backward(f, np.array([[0.3, -0.7, 0.2]]))
    assert np.all(np.isfinite(go)) and np.abs(go).max() > 0
    step = 1e-6                                                 # the k = 2 map, aa = 2 q_vec, differentiated numerically
    for e in range(6):
        d = np.zeros((1, 6))
        d[0, e] = step
        q = lambda oo: 2.0 * V.tail_forward(oo)["q"][:, 1:]
        want = float(np.sum((q(o + d) - q(o - d)) / (2 * step) * [0.3, -0.7, 0.2]))
        assert abs(go[0, e] - want) <= 1e-8


# ---- coma_amd.pose_prior on the host ----
def _ini(path, **over):
    settings = dict(num_neurons=80, latentD=7, data_shape="[1, 5, 3]", use_cont_repr=True, base_lr=0.005, expr_code="synthetic")
    settings.update(over)
    with open(path, "w") as fh:
        fh.write("[All]\n" + "".join(f"{k} : {v}\n" for k, v in settings.items()))


def _snapshot(path, seed, mtime):
    w = V.synthetic_weights(80, 7, 5, seed=seed)
    state = {k: torch.from_numpy(v) for k, v in w.items()}
    state["bodyprior_enc_bn1.num_batches_tracked"] = torch.tensor(3)
    torch.save(state, path)
    os.utime(path, (mtime, mtime))
    return w


def test_from_dir_reads_the_settings_and_the_newest_snapshot(tmp_path):
    from coma_amd._lib import ComaHipError
    from coma_amd.pose_prior import DeviceVPoser
    (tmp_path / "snapshots").mkdir()
    _ini(tmp_path / "TR00_synthetic.ini")
    with pytest.raises(FileNotFoundError, match="no snapshot"):
        DeviceVPoser.from_dir(str(tmp_path))
    _snapshot(tmp_path / "snapshots" / "TR00_E100.pt", seed=1, mtime=1_000_000)             # older, though its name sorts last
    newest = _snapshot(tmp_path / "snapshots" / "TR00_E020.pt", seed=2, mtime=2_000_000)
    vp = DeviceVPoser.from_dir(str(tmp_path))                                               # device="cuda": not touched before the first call
    assert (vp.num_neurons, vp.latentD, vp.num_joints) == (80, 7, 5)
    assert np.array_equal(vp.host["bodyprior_dec_out.weight"], newest["bodyprior_dec_out.weight"])
    assert np.array_equal(vp.host["enc_ml.weight"], np.concatenate([newest["bodyprior_enc_mu.weight"], newest["bodyprior_enc_logvar.weight"]]))
    assert vp.host["bodyprior_enc_bn2"].shape == (4, 80) and np.array_equal(vp.host["bodyprior_enc_bn2"][3], newest["bodyprior_enc_bn2.running_var"])
    _ini(tmp_path / "TR00_synthetic.ini", use_cont_repr=False)
    with pytest.raises(NotImplementedError, match="use_cont_repr"):
        DeviceVPoser.from_dir(str(tmp_path))
    _ini(tmp_path / "TR00_synthetic.ini", num_neurons=64)
    with pytest.raises(ValueError, match="bodyprior_enc_fc1.weight"):
        DeviceVPoser.from_dir(str(tmp_path))
    with pytest.raises(FileNotFoundError, match="does not exist"):
        DeviceVPoser.from_dir(str(tmp_path / "absent"))
    with pytest.raises(ComaHipError, match="no CPU path"):
        DeviceVPoser(newest, 80, 7, [1, 5, 3], device="cpu")


def test_host_side_refusals_of_the_wrappers():
    from coma_amd._lib import ComaHipError
    from coma_amd.pose_prior import DeviceAnglePrior, DeviceVPoser
    w = V.synthetic_weights(80, 7, 5, seed=1)
    vp = DeviceVPoser(w, 80, 7, [1, 5, 3])
    with pytest.raises(ComaHipError, match="no CPU path"):
        vp.decode(torch.zeros(1, 7))
    with pytest.raises(ComaHipError, match="requires grad"):
        vp.encode(torch.zeros(1, 15, requires_grad=True))
    with pytest.raises(ValueError, match="output_type"):
        vp.decode(torch.zeros(1, 7), output_type="quaternion")
    with pytest.raises(ValueError, match="data_shape"):
        DeviceVPoser(w, 80, 7, [5, 3])
    with pytest.raises(KeyError, match="bodyprior_dec_out.bias"):
        DeviceVPoser({k: v for k, v in w.items() if k != "bodyprior_dec_out.bias"}, 80, 7, [1, 5, 3])
    with pytest.raises(ComaHipError, match="no CPU path"):
        DeviceAnglePrior(device="cpu")
    with pytest.raises(ComaHipError, match="no CPU path"):
        DeviceAnglePrior()(torch.zeros(1, 63))
    index, sign = DeviceAnglePrior().vectors()
    assert list(index) == [52, 55, 9, 12] and list(sign) == [1.0, -1.0, -1.0, -1.0]
    assert list(DeviceAnglePrior().vectors(with_global_pose=True)[0]) == [55, 58, 12, 15]


def test_the_c_entry_points_refuse_before_any_launch(hip_lib):
    L, one = hip_lib, C.c_void_p(16)                             # never dereferenced: validation fails first
    assert L.coma_vposer_saved_bytes(1, 512, 21) == 2 * 512 * 8 + 126 * 8 + 32 and L.coma_vposer_workspace_bytes(1, 512, 21) == 3 * 512 * 8
    assert L.coma_vposer_workspace_bytes(2, 8, 64) == 3 * 2 * 384 * 8
    for bad in ((0, 512, 21), (65, 512, 21), (1, 0, 21), (1, 2049, 21), (1, 512, 0), (1, 512, 65)):
        assert L.coma_vposer_saved_bytes(*bad) == 0 and L.coma_vposer_workspace_bytes(*bad) == 0
    dec = lambda N=1, D=32, H=512, NJ=21, z=one, saved=one, nbytes=1 << 20: L.coma_vposer_decode_f32(
        z, one, one, one, one, one, one, N, D, H, NJ, one, None, None, saved, nbytes, None)
    text = lambda: L.coma_last_error().decode()
    assert dec(z=None) == -1 and "null pointer" in text()
    for kw in (dict(N=0), dict(N=65), dict(D=0), dict(D=257), dict(H=0), dict(H=2049), dict(NJ=0), dict(NJ=65)):
        assert dec(**kw) == -1 and "must lie in" in text(), kw
    assert dec(nbytes=100) == -1 and "saved state of 100 bytes" in text()
    assert dec(saved=C.c_void_p(24)) == -1 and "16-byte aligned" in text()
    assert dec(z=C.c_void_p(18)) == -1 and "4-byte aligned" in text()
    bwd = lambda ws_bytes=1 << 20, N=1: L.coma_vposer_decode_backward_f32(one, one, one, one, N, 32, 512, 21, one, 1 << 20, one, one, ws_bytes, None)
    assert bwd(ws_bytes=8) == -1 and "workspace of 8 bytes" in text()
    assert bwd(N=-1) == -1 and "must lie in" in text()
    assert L.coma_vposer_encode_f32(one, one, one, one, one, one, one, one, None, 1, 32, 512, 21, one, one, one, 1 << 20, None) == -1 and "null pointer" in text()
    assert L.coma_vposer_encode_f32(*[one] * 9, 1, 32, 512, 21, one, one, one, 8, None) == -1 and "workspace" in text()
    index, sign = (C.c_int32 * 4)(52, 55, 9, 12), (C.c_float * 4)(1, -1, -1, -1)
    assert L.coma_angle_prior_f32(one, 1, 55, index, sign, 4, one, None) == -1 and "index[1]=55 outside [0, 55)" in text()
    assert L.coma_angle_prior_f32(one, 1, 63, index, sign, 17, one, None) == -1 and "K=17" in text()
    assert L.coma_angle_prior_f32(None, 1, 63, index, sign, 4, one, None) == -1 and "null pointer" in text()
    assert L.coma_angle_prior_backward_f32(one, one, 65, 63, index, sign, 4, one, None) == -1 and "N=65" in text()
    assert L.coma_angle_prior_backward_f32(one, one, 1, 63, (C.c_int32 * 4)(52, -1, 9, 12), sign, 4, one, None) == -1 and "index[1]=-1" in text()


# ---- the app's flag ----
def test_parser_accepts_pose_prior_and_keeps_its_defaults(monkeypatch):
    from src.application import optimize as app
    plain = app.build_parser().parse_args([])
    assert "pose_prior" not in vars(plain) and "body_model" not in vars(plain)
    assert app.pose_prior_choice(plain) == "vposer" and app.body_model_choice(plain) == "smplx"
    assert (plain.lr, plain.num_iters, plain.bending_prior_weight, plain.pprior_weight, plain.save_dir) == (1e-2, 2000, 31700, 1e-6, "output/")
    chosen = app.build_parser().parse_args(["--pose_prior", "device", "--body_model", "device"])
    assert app.pose_prior_choice(chosen) == "device" and app.body_model_choice(chosen) == "device"
    assert {k: v for k, v in vars(chosen).items() if k not in ("pose_prior", "body_model")} == vars(plain)
    with pytest.raises(SystemExit):
        app.build_parser().parse_args(["--pose_prior", "gmm"])
    # main() fills both hooks from the factory, and only with the flag
    seen = []
    monkeypatch.setattr(app, "device_pose_prior", lambda device="cuda": ("decoder", "prior"))
    monkeypatch.setattr(app, "optimize_smpl", lambda **kw: seen.append((kw["pose_decoder"], kw["angle_prior"], kw["body_model"])))
    app.main(app.build_parser().parse_args(["--pose_prior", "device"]))
    app.main(app.build_parser().parse_args([]))
    app.main(app.build_parser().parse_args(["--pose_prior", "device"]), pose_decoder="mine")
    assert seen == [("decoder", "prior", None), (None, None, None), ("mine", "prior", None)]
