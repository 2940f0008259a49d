"""GPU: the device VPoser and angle prior (coma_amd.pose_prior, coma_amd/csrc/vposer.hip) against the reference's own VPoser class,
rotation_matrix_to_angle_axis and SMPLifyAnglePrior executed in f64 (R64 of tests/golden/vposer_golden.npz) and against the f64
restatement tests/vposer_ref.py.

Bounds.  e_ref_* (stored by the generator) is max|R32 - R64| / max|R64| pooled over the cases, the reference's own f32 against its f64;
the device must meet 4 * e_ref on every case (two f32 evaluations of one formula in different summation orders), and 4 * e_reg, the
same pool without tests/vposer_ref.ILL_CONDITIONED, on every other case (that set is empty: the two pools are one).  Branch ids are
exact.  The matrices are a rounding of f64 values of size <= 1: 2^-23.  Figures are printed before they are asserted.
"""
import pickle
import sys

import numpy as np
import pytest
import torch

from tests import app_ref
from tests import smplx_ref as S
from tests import vposer_ref as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def golden():
    return V.load_golden()


def _bounds(golden, q, name=None):
    out = [4 * float(golden[f"e_ref_{q}"])]
    if name not in V.ILL_CONDITIONED:
        out.append(4 * float(golden[f"e_reg_{q}"]))
    return out


def _model(name):
    from coma_amd.pose_prior import DeviceVPoser
    c = V.case_shape(name)
    return DeviceVPoser(V.case_weights(name), c["H"], c["D"], [1, c["NJ"], 3], device=DEV)


def _t(a, grad=False):
    return torch.as_tensor(np.asarray(a, dtype=np.float32)).to(DEV).requires_grad_(grad)


def _run(vp, inp):
    """Every quantity of a case from the device, as arrays, and the tensors the calls returned."""
    from coma_amd.pose_prior import DeviceAnglePrior
    z, pose = _t(inp["z"], True), _t(inp["prior_pose"], True)
    aa = vp.decode(z, output_type="aa")
    (aa.reshape(len(inp["z"]), -1) * _t(inp["g"])).sum().backward()
    enc = vp.encode(_t(inp["pose"]))
    out = DeviceAnglePrior(DEV)(pose)
    (out * _t(inp["prior_g"])).sum().backward()
    got = dict(aa=aa.detach().reshape(len(inp["z"]), -1), grad_z=z.grad, mean=enc.mean, scale=enc.scale, prior=out.detach(), grad_prior=pose.grad)
    return {k: v.cpu().numpy() for k, v in got.items()}, (aa, enc.mean, enc.scale, out)


@pytest.mark.parametrize("name", V.CASE_NAMES)
def test_golden_case_within_the_reference_s_own_error(golden, name):
    vp, inp, c = _model(name), V.case_inputs(name), V.case_shape(name)
    got, (aa, _, _, out) = _run(vp, inp)
    assert aa.shape == (c["N"], 1, c["NJ"], 3) and out.shape == (c["N"], 4)
    dev = {q: V.rel_dev(got[q], golden[f"{name}__r64_{q}"]) for q in V.QUANTITIES}
    for q in V.QUANTITIES:
        print(f"{name} {q}: device vs R64 {dev[q]:.3e}   bounds {['%.3e' % b for b in _bounds(golden, q, name)]}")
    branch = vp.branches(_t(inp["z"])).cpu().numpy()
    matrot = vp.decode(_t(inp["z"]), output_type="matrot")
    dev_m = float(np.abs(matrot.cpu().numpy().reshape(c["N"], c["NJ"], 9) - golden[f"{name}__r64_matrot"]).max())
    print(f"{name} matrot: {dev_m:.3e}; branches {np.bincount(branch.reshape(-1), minlength=4).tolist()}")
    for q in V.QUANTITIES:
        assert got[q].shape == golden[f"{name}__r64_{q}"].shape and np.all(np.isfinite(got[q])), q
        for b in _bounds(golden, q, name):
            assert dev[q] <= b, (q, dev[q], b)
    assert np.array_equal(branch, golden[f"{name}__r64_branch"])
    assert matrot.shape == (c["N"], 1, c["NJ"], 9) and dev_m <= 2.0 ** -23
    assert np.count_nonzero(got["grad_prior"]) == 4 * c["N"]


@pytest.mark.parametrize("H,D,NJ,N", [(2048, 256, 64, 64), (1, 1, 1, 1), (65, 64, 11, 2), (200, 63, 3, 5)])
def test_domain_edges_against_the_restatement(golden, H, D, NJ, N):
    """The largest and the smallest accepted sizes, and sizes one past / one short of the 64 lanes of a row, the 4 rows of a forward
    workgroup and the 16 row splits of a transposed one."""
    from coma_amd.pose_prior import DeviceVPoser
    w = V.synthetic_weights(H, D, NJ, seed=H + D + NJ, kind="branches")
    vp = DeviceVPoser(w, H, D, [1, NJ, 3], device=DEV)
    rng = np.random.RandomState(N)
    z, g, pose = rng.normal(size=(N, D)).astype(np.float32), rng.normal(size=(N, 3 * NJ)).astype(np.float32), (rng.normal(size=(N, 3 * NJ)) * 0.3).astype(np.float32)
    fwd = V.decode(w, z)
    want = dict(aa=fwd["aa"], grad_z=V.decode_backward(w, fwd, g))
    want["mean"], want["scale"] = V.encode(w, pose)
    zt = _t(z, True)
    aa = vp.decode(zt)
    (aa.reshape(N, -1) * _t(g)).sum().backward()
    enc = vp.encode(_t(pose))
    got = dict(aa=aa.detach().reshape(N, -1), grad_z=zt.grad, mean=enc.mean, scale=enc.scale)
    dev = {q: V.rel_dev(got[q].cpu().numpy(), want[q]) for q in want}
    print({q: f"{v:.3e}" for q, v in dev.items()})
    for q in want:
        assert dev[q] <= min(_bounds(golden, q)), (q, dev[q])
    assert np.array_equal(vp.branches(_t(z)).cpu().numpy(), fwd["branch"])


def test_two_calls_are_bit_identical_and_returned_tensors_are_not_aliased():
    name = "batch3"
    vp, inp = _model(name), V.case_inputs(name)
    got1, kept = _run(vp, inp)
    copies = [t.detach().clone() for t in kept]
    other = dict(inp, z=inp["z"] * 0.5 + 0.1, pose=inp["pose"] + 0.2, prior_pose=inp["prior_pose"] * -1.0)     # other inputs in between
    got_other, _ = _run(vp, other)
    assert not np.array_equal(got_other["aa"], got1["aa"]) and not np.array_equal(got_other["mean"], got1["mean"])
    for a, b in zip(kept, copies):                                  # the first call's tensors are untouched
        assert torch.equal(a.detach(), b)
    got2, _ = _run(vp, inp)
    for q in got1:
        assert np.array_equal(got1[q], got2[q]), q


def test_a_backward_uses_its_own_forward_s_saved_state():
    """Two forwards in flight: each backward reads the state its own forward wrote."""
    name = "random_init"
    vp, inp = _model(name), V.case_inputs(name)
    w = V.case_weights(name)
    z1, z2 = _t(inp["z"], True), _t(inp["z"] * -0.7, True)
    a1, a2 = vp.decode(z1), vp.decode(z2)
    (a1.reshape(1, -1) * _t(inp["g"])).sum().backward()
    (a2.reshape(1, -1) * _t(inp["g"])).sum().backward()
    for z in (z1, z2):
        fwd = V.decode(w, z.detach().cpu().numpy())
        assert V.rel_dev(z.grad.cpu().numpy(), V.decode_backward(w, fwd, inp["g"])) <= 2.0 ** -22


def test_refusals():
    from coma_amd._lib import ComaHipError
    from coma_amd.pose_prior import DeviceAnglePrior, DeviceVPoser
    vp = _model("odd")                                              # H 80, D 7, NJ 5
    prior = DeviceAnglePrior(DEV)
    with pytest.raises(ValueError, match=r"expected \[N, 7\]"):
        vp.decode(torch.zeros(1, 8, device=DEV))
    with pytest.raises(ValueError, match=r"expected \[N, 15\]"):
        vp.encode(torch.zeros(1, 63, device=DEV))
    with pytest.raises(ValueError, match="batch size 65"):
        vp.decode(torch.zeros(65, 7, device=DEV))
    with pytest.raises(ValueError, match="P >= 56"):
        prior(torch.zeros(1, 15, device=DEV))
    with pytest.raises(ValueError, match="P >= 59"):
        prior(torch.zeros(1, 58, device=DEV), with_global_pose=True)
    with pytest.raises(ComaHipError, match="requires grad"):
        vp.encode(torch.zeros(1, 15, device=DEV, requires_grad=True))
    with pytest.raises(ComaHipError, match="matrot"):
        vp.decode(torch.zeros(1, 7, device=DEV, requires_grad=True), output_type="matrot")
    with pytest.raises(ComaHipError, match="no CPU path"):
        vp.decode(torch.zeros(1, 7))
    with pytest.raises(ComaHipError, match="no CPU path"):
        prior(torch.zeros(1, 63))
    with pytest.raises(ComaHipError, match="no CPU path"):
        DeviceVPoser(V.case_weights("odd"), 80, 7, [1, 5, 3], device="cpu")
    assert vp.decode(torch.zeros(2, 7, device=DEV)).shape == (2, 1, 5, 3)          # and the object still works
    assert prior(torch.zeros(1, 72, device=DEV), with_global_pose=True).shape == (1, 4)


class _Recording:
    """The device decoder with a handle on the embedding the fit optimises."""

    def __init__(self, decoder):
        self.decoder = decoder

    def encode(self, pose):
        return self.decoder.encode(pose)

    def decode(self, embedding, output_type="aa"):
        self.embedding = embedding
        return self.decoder.decode(embedding, output_type=output_type)


def test_one_fit_step_with_every_stage_on_the_device(golden):
    """src/application/optimize.py::fit for one iteration with DeviceSMPLX, DeviceVPoser, DeviceAnglePrior and a ComaObjective: the
    embedding's gradient of the total loss against the f64 restatements chained on the host (vposer_ref.decode_backward of
    smplx_ref.backward of app_ref's vertex gradients, plus the two priors), within 4 x the largest of the modules' e_ref for gradients."""
    from coma_amd.app import ComaObjective
    from coma_amd.body_model import DeviceSMPLX
    from coma_amd.pose_prior import DeviceAnglePrior
    from src.application import optimize as app
    model, fm = S.case_model("moderate")
    body = DeviceSMPLX(model, n_pca=45, device=DEV, extra_joint_vertex_ids=[])
    w = V.case_weights("near_rest")
    decoder = _Recording(_model("near_rest"))
    scale, w_o, w_c, w_body, w_bend, w_prior = 0.84, 10.0, 5.0, 2.0, 0.5, 0.3
    # the host chain up to the vertices: the embedding is the encoder's mean of the T-pose, as fit() takes it
    z0 = V.encode(w, np.zeros((1, 63)))[0].astype(np.float32).astype(np.float64)
    fwd_v = V.decode(w, z0)
    betas = np.concatenate([np.float32(app.DEFAULT_BETAS).reshape(-1), np.zeros(10, np.float32)])
    theta0 = np.zeros(S.n_theta(fm))
    theta0[3:66] = fwd_v["aa"].reshape(-1)
    transl0 = np.float32([3.0, 1.0, 0.0])
    fwd = S.forward(fm, betas, theta0, transl0)
    verts = (fwd["vertices"].astype(np.float32) * np.float32(scale)).astype(np.float32)
    c = app_ref.make_case((verts, fm["faces"]), 40, seed=91)
    c.update(obj_normal=c["obj_normals"][c["ref_index"]], targets=c["obj_verts"][c["objects"]])
    objective = ComaObjective(c["faces"], c["gt"], c["obj_normal"], c["sel"], c["targets"], c["p"], c["sub_p"], c["eps"], device=DEV)
    out = app.fit(lambda v: objective.loss(v, w_o, w_c), body, decoder, DeviceAnglePrior(DEV), lr=1e-2, body_pose_weight=w_body,
                  bending_prior_weight=w_bend, pprior_weight=w_prior, scale_factor=scale, num_iters=1, device=DEV, record=True)
    got = decoder.embedding.grad.cpu().numpy().astype(np.float64)
    z_dev = decoder.embedding.detach().cpu().numpy().astype(np.float64)
    # Adam has stepped the embedding by lr in each component; the gradient was taken at the encoder's mean
    start = z_dev + 1e-2 * np.sign(got)
    dev_z = V.rel_dev(start, z0)
    ev = app_ref.evaluate(verts, c["faces"], c["gt"], c["obj_normal"], c["p"], c["sub_p"], c["eps"], c["sel"], c["targets"])
    g_verts = scale * (w_o * ev["grad_orientation"] + w_c * ev["grad_contact"])
    g_theta, _ = S.backward(fm, fwd, g_verts)
    g_pose = g_theta[3:66][None] + w_bend * V.angle_prior_backward(fwd_v["aa"], np.ones((1, 4)))
    want = V.decode_backward(w, fwd_v, g_pose) + 2.0 * z0 * w_body ** 2 * w_prior
    ga, _ = app_ref.load_golden()
    gs = S.load_golden()
    pools = ((golden, ("grad_z", "grad_prior")), (gs, ("grad_pose", "grad_transl")), (ga, ("grad_orientation", "grad_contact")))
    bound = 4 * max(float(g[f"e_ref_{q}"]) for g, qs in pools for q in qs)
    # the objective's e_ref pool is inflated four orders of magnitude by its own ill-conditioned case, which is not this one: the
    # same maximum over the pools without the modules' ill-conditioned cases is the bound that says something
    regular = 4 * max(float(g[f"e_reg_{q}"]) for g, qs in pools for q in qs)
    dev = V.rel_dev(got, want)
    print(f"fit step: grad_z {dev:.3e}, bound {bound:.3e}, without the ill-conditioned cases {regular:.3e}; start embedding {dev_z:.3e}; "
          f"loss {out['losses'][0]:.6f}")
    assert np.all(np.isfinite(got)) and np.abs(want).max() > 0 and got.shape == (1, 32)
    assert dev_z <= 1e-5                                          # lr * (Adam's eps / |gradient|) and the encoder's rounding: well below lr
    assert dev <= bound and dev <= regular
    assert out["vertices"].shape == (fm["V"], 3) and np.all(np.isfinite(out["vertices"]))


def _experiment_dir(path, name):
    """A VPoser experiment directory with the case's seeded weights: settings file and one snapshot."""
    c = V.case_shape(name)
    (path / "snapshots").mkdir(parents=True)
    (path / "synthetic.ini").write_text(f"[All]\nnum_neurons : {c['H']}\nlatentD : {c['D']}\ndata_shape : [1, {c['NJ']}, 3]\nuse_cont_repr : True\n")
    torch.save({k: torch.from_numpy(v) for k, v in V.case_weights(name).items()}, path / "snapshots" / "synthetic_E001.pt")


def test_device_pose_prior_factory_on_the_default_device(golden, tmp_path, monkeypatch):
    """`--pose_prior device` as the CLI builds it: device="cuda" (no index) with the caller's tensors on cuda:0, from an experiment
    directory on disk."""
    from src.application import optimize as app
    name = "near_rest"
    _experiment_dir(tmp_path / "vposer", name)
    monkeypatch.setattr(app, "VPOSER_PATH", str(tmp_path / "vposer"))
    decoder, prior = app.device_pose_prior()
    assert (decoder.latentD, decoder.num_joints, decoder.num_neurons) == (32, 21, 512)
    got, _ = _run(decoder, {k: v for k, v in V.case_inputs(name).items()})
    for q in V.QUANTITIES:
        dev = V.rel_dev(got[q], golden[f"{name}__r64_{q}"])
        print(f"factory {q}: {dev:.3e}")
        assert dev <= min(_bounds(golden, q, name)), q
    body_pose = decoder.decode(torch.zeros(1, 32, device="cuda")).view(1, -1)
    assert prior(body_pose).shape == (1, 4)


def test_cli_runs_a_short_fit_without_third_party_packages(tmp_path, monkeypatch):
    """src/application/optimize.py --body_model device --pose_prior device on synthetic model files: three iterations, the mesh written,
    with smplx, configer and torchgeometry made impossible to import."""
    from src.application import optimize as app
    model, fm = S.case_model("moderate")
    (tmp_path / "smplx").mkdir()
    np.savez(tmp_path / "smplx" / "SMPLX_NEUTRAL.npz", **model)
    _experiment_dir(tmp_path / "vposer", "near_rest")
    monkeypatch.setattr(app, "BODY_MOCAP_PATH", str(tmp_path))
    monkeypatch.setattr(app, "VPOSER_PATH", str(tmp_path / "vposer"))
    Vn, O, k = fm["V"], 20, 30
    rng = np.random.default_rng(5)
    unit = lambda n: (lambda a: (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32))(rng.normal(size=(n, 3)))
    prob = np.zeros((Vn, O, Vn), np.float32)
    prob[np.arange(Vn), 0, np.arange(Vn)] = 1.0                    # vertex h's most likely bin for object vertex 0 is bin h
    nom = np.full((Vn, O), 0.1, np.float32)
    nom[rng.choice(Vn, size=k, replace=False), rng.integers(0, O, size=k)] = 1.0
    state = dict(prob_grid_canon_human_wrt_obj=prob, canon_normal_grid=unit(Vn), contact_dist_expectation_grid_nom=nom,
                 contact_dist_expectation_grid_denom=np.ones((Vn, O), np.float32))
    asset = dict(downsampled_pcd_points_raw=(rng.uniform(-1, 1, size=(O, 3)) + [3.0, 1.0, 0.0]).astype(np.float32), downsampled_pcd_normal_raw=unit(O))
    for pth, obj in ((tmp_path / "coma.pickle", state), (tmp_path / "asset.pickle", asset)):
        with open(pth, "wb") as fh:
            pickle.dump(obj, fh)
    args = app.build_parser().parse_args(["--supercategory", "super", "--category", "cat", "--coma_path", str(tmp_path / "coma.pickle"),
                                          "--asset_downsample_pth", str(tmp_path / "asset.pickle"), "--save_dir", str(tmp_path / "out"),
                                          "--num_iters", "3", "--body_model", "device", "--pose_prior", "device"])
    for package in ("smplx", "configer", "torchgeometry"):         # an import of any of them raises from here on
        monkeypatch.setitem(sys.modules, package, None)
    out = app.main(args)
    assert out["vertices"].shape == (Vn, 3) and np.all(np.isfinite(out["vertices"]))
    from coma_amd.downsample import load_obj
    v, f = load_obj(out["path"])
    assert out["path"] == str(tmp_path / "out" / "super" / "cat" / "optimized.obj") and v.shape == (Vn, 3) and np.array_equal(f, fm["faces"])
