"""GPU: the device SMPL-X body model (coma_amd.body_model.DeviceSMPLX, coma_amd/csrc/smplx.hip) against the third-party package's own
lbs and SMPLX class executed in f64 (R64 of tests/golden/smplx_golden.npz) and against the f64 restatement tests/smplx_ref.py.

Bounds.  e_ref_* (stored by the generator) is max|R32 - R64| / max|R64| pooled over the cases, the package's own f32 against its f64;
the device must meet 4 * e_ref on every case (two f32 evaluations of one formula in different summation orders).  One case
(`small_angle`, a joint at |r| of about 1e-4) is ill-conditioned for the package's f32 and inflates the pooled grad_pose figure by
more than 10x (4.8e-6 against 4.2e-7), so every OTHER case is also held to 4 * e_reg, the same pool without `small_angle`.  Figures
are printed before they are asserted.
"""
import numpy as np
import pytest
import torch

from tests import app_ref
from tests import smplx_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POSE_KEYS = ("global_orient", "body_pose", "jaw_pose", "leye_pose", "reye_pose", "left_hand_pose", "right_hand_pose")


@pytest.fixture(scope="module")
def golden():
    return S.load_golden()


@pytest.fixture(scope="module")
def real_size():
    """The V = 10 475 model (the one the generator ran through the package's class), its device object and the restatement's results
    for the FULL upstream gradient, computed once."""
    from coma_amd.body_model import DeviceSMPLX
    model, kw, g = S.class_case()
    fm = S.flat_model(model, n_pca=45)
    coef = np.concatenate([kw["betas"].reshape(-1), kw["expression"].reshape(-1)])
    fwd = S.forward(fm, coef, S.class_theta(kw), kw["transl"])
    g_pose, g_transl = S.backward(fm, fwd, g)
    picks = [9, 10474, 5000, 123]
    body = DeviceSMPLX(model, n_pca=45, device=DEV, extra_joint_vertex_ids=picks)
    want = dict(vertices=fwd["vertices"], joints=S.all_joints(fm, fwd, picks), grad_pose=g_pose, grad_transl=g_transl)
    return dict(model=model, kw=kw, g=g, fm=fm, body=body, want=want)


def _bounds(golden, q, name=None):
    out = [4 * float(golden[f"e_ref_{q}"])]
    if name not in S.ILL_CONDITIONED:
        out.append(4 * float(golden[f"e_reg_{q}"]))
    return out


def _split(body, theta, coefficients, transl):
    """The packed parameters as DeviceSMPLX's keyword arguments ([1, n] device tensors; the pose arguments and transl are leaves)."""
    sizes = (3, body.num_body, 3, 3, 3, body.hand_size, body.hand_size)
    kw, at = {}, 0
    for key, n in zip(POSE_KEYS, sizes):
        kw[key] = torch.as_tensor(np.asarray(theta[at:at + n], dtype=np.float32)).reshape(1, n).to(DEV).requires_grad_(True)
        at += n
    assert at == len(theta) == body.num_theta
    kw["transl"] = torch.as_tensor(np.asarray(transl, dtype=np.float32)).reshape(1, 3).to(DEV).requires_grad_(True)
    c = torch.as_tensor(np.asarray(coefficients, dtype=np.float32)).reshape(1, -1).to(DEV)
    kw["betas"] = c[:, :body.num_betas]
    kw["expression"] = c[:, body.num_betas:] if body.num_expression_coeffs else None
    return kw


def _run(body, kw, g):
    for v in kw.values():
        if v is not None and v.requires_grad:
            v.grad = None
    out = body(**kw, return_verts=True, return_full_pose=True)
    (out.vertices[0] * torch.as_tensor(g).to(DEV)).sum().backward()
    return out, dict(vertices=out.vertices[0].detach().cpu().numpy(), joints=out.joints[0].detach().cpu().numpy(),
                     full_pose=out.full_pose[0].cpu().numpy(),
                     grad_pose=np.concatenate([kw[k].grad.cpu().numpy().reshape(-1) for k in POSE_KEYS]), grad_transl=kw["transl"].grad.cpu().numpy().reshape(-1))


@pytest.mark.parametrize("name", S.CASE_NAMES)
def test_golden_case_within_the_package_s_own_error(golden, name):
    from coma_amd.body_model import DeviceSMPLX
    model, fm = S.case_model(name)
    body = DeviceSMPLX(model, n_pca=max(fm["n_pca"], 1), use_pca=bool(fm["n_pca"]), device=DEV, extra_joint_vertex_ids=[])
    kw = _split(body, golden[f"{name}__theta"], golden[f"{name}__coefficients"], golden[f"{name}__transl"])
    _, got = _run(body, kw, golden[f"{name}__g"])
    got["joints"] = got["joints"][:fm["J"]]
    dev = {q: S.rel_dev(got[q], golden[f"{name}__r64_{q}"]) for q in S.QUANTITIES}
    for q in S.QUANTITIES:
        print(f"{name} {q}: device vs R64 {dev[q]:.3e}   bounds {['%.3e' % b for b in _bounds(golden, q, name)]}")
    for q in S.QUANTITIES:
        assert np.all(np.isfinite(got[q])), q
        for b in _bounds(golden, q, name):
            assert dev[q] <= b, (q, dev[q], b)


def test_real_size_against_the_restatement_and_the_package_s_class(golden, real_size):
    r = real_size
    kw = _split(r["body"], S.class_theta(r["kw"]), np.concatenate([r["kw"]["betas"].reshape(-1), r["kw"]["expression"].reshape(-1)]), r["kw"]["transl"])
    _, got = _run(r["body"], kw, r["g"])
    dev = {q: S.rel_dev(got[q], r["want"][q]) for q in S.QUANTITIES}
    print({q: f"{v:.3e}" for q, v in dev.items()}, "extra joints:", r["body"].num_extra)
    subset = S.class_subset()
    cls = dict(vertices=S.rel_dev(got["vertices"][subset], golden["class__r64_vertices"]), joints=S.rel_dev(got["joints"][:55], golden["class__r64_joints"][:55]),
               landmarks=S.rel_dev(got["joints"][59:], golden["class__r64_joints"][76:]), full_pose=S.rel_dev(got["full_pose"], golden["class__r64_full_pose"]))
    print("against the class:", {q: f"{v:.3e}" for q, v in cls.items()})
    for q in S.QUANTITIES:
        for b in _bounds(golden, q):
            assert dev[q] <= b, (q, dev[q], b)
    assert cls["vertices"] <= min(_bounds(golden, "vertices"))
    assert max(cls["joints"], cls["landmarks"]) <= min(_bounds(golden, "joints"))
    assert cls["full_pose"] <= 2.0 ** -23                      # a handful of f32 products: the f32 rounding of the f64 value


def test_extra_joints_against_the_restatement(golden, real_size):
    r = real_size
    assert r["body"].extra_joint_source == "caller" and r["body"].num_extra == 4 + 51
    with torch.no_grad():
        kw = _split(r["body"], S.class_theta(r["kw"]), np.concatenate([r["kw"]["betas"].reshape(-1), r["kw"]["expression"].reshape(-1)]), r["kw"]["transl"])
        out = r["body"](**kw)
    joints = out.joints[0].cpu().numpy()
    assert joints.shape == (55 + 4 + 51, 3)
    dev = S.rel_dev(joints[55:], r["want"]["joints"][55:])
    print(f"extra joints: {dev:.3e}")
    assert dev <= min(_bounds(golden, "joints"))
    assert not out.joints.requires_grad and out.full_pose is None


def test_two_calls_are_bit_identical_and_returned_tensors_are_not_aliased(golden, real_size):
    r = real_size
    theta = S.class_theta(r["kw"])
    coef = np.concatenate([r["kw"]["betas"].reshape(-1), r["kw"]["expression"].reshape(-1)])
    kw = _split(r["body"], theta, coef, r["kw"]["transl"])
    out1, got1 = _run(r["body"], kw, r["g"])
    keep = [out1.vertices.detach().clone(), out1.joints.detach().clone(), out1.full_pose.clone()]
    other = _split(r["body"], theta * 0.5 + 0.01, coef, r["kw"]["transl"] * -1.0)          # a changed pose in between
    out_other, _ = _run(r["body"], other, r["g"])
    assert not torch.equal(out_other.vertices, keep[0])
    for a, b in zip((out1.vertices, out1.joints, out1.full_pose), keep):                   # the first call's tensors are untouched
        assert torch.equal(a.detach(), b)
    _, got2 = _run(r["body"], kw, r["g"])
    for q in got1:
        assert np.array_equal(got1[q], got2[q]), q


def test_shape_stage_runs_only_when_the_coefficients_change(golden):
    from coma_amd.body_model import DeviceSMPLX
    name = "moderate"
    model, fm = S.case_model(name)
    body = DeviceSMPLX(model, n_pca=45, device=DEV, extra_joint_vertex_ids=[])
    theta, coef, transl = golden[f"{name}__theta"], golden[f"{name}__coefficients"], golden[f"{name}__transl"]
    with torch.no_grad():
        first = body(**_split(body, theta, coef, transl)).vertices.clone()
        assert body.shape_stage_runs == 1
        body(**_split(body, theta * 0.5, coef, transl))
        assert body.shape_stage_runs == 1
        coef2 = coef.copy()
        coef2[3] += 0.5
        moved = body(**_split(body, theta, coef2, transl)).vertices
        assert body.shape_stage_runs == 2 and not torch.equal(moved, first)
        want = S.forward(fm, coef2, theta, transl)["vertices"]
        assert S.rel_dev(moved[0].cpu().numpy(), want) <= min(_bounds(golden, "vertices"))
        again = body(**_split(body, theta, coef, transl)).vertices
        assert body.shape_stage_runs == 3 and torch.equal(again, first)


def test_same_betas_tensor_is_not_read_again_until_it_changes(golden):
    """The app's path: the SAME betas / expression tensors every call.  The shape stage runs once; an in-place change through torch
    moves the version counter and re-runs it; requires_grad set later is still refused."""
    from coma_amd._lib import ComaHipError
    from coma_amd.body_model import DeviceSMPLX
    name = "moderate"
    model, fm = S.case_model(name)
    body = DeviceSMPLX(model, n_pca=45, device=DEV, extra_joint_vertex_ids=[])
    theta, coef, transl = golden[f"{name}__theta"], golden[f"{name}__coefficients"], golden[f"{name}__transl"]
    kw = _split(body, theta, coef, transl)
    betas, expression = kw["betas"].clone(), kw["expression"].clone()
    kw.update(betas=betas, expression=expression)
    with torch.no_grad():
        first = body(**kw).vertices.clone()
        for _ in range(3):
            assert torch.equal(body(**kw).vertices, first)
        assert body.shape_stage_runs == 1
        betas[0, 3] += 0.5
        moved = body(**kw).vertices
        assert body.shape_stage_runs == 2 and not torch.equal(moved, first)
        coef2 = coef.copy()
        coef2[3] += 0.5
        assert S.rel_dev(moved[0].cpu().numpy(), S.forward(fm, coef2, theta, transl)["vertices"]) <= min(_bounds(golden, "vertices"))
    betas.requires_grad_(True)
    with pytest.raises(ComaHipError, match="betas requires grad"):
        body(**kw)


def test_cli_factories_on_the_default_device(golden, tmp_path, monkeypatch):
    """`--body_model device` as the two CLIs build it: device="cuda" (no index) with the callers' tensors on cuda:0, from a model
    file on disk, through one call each (the app's with a backward)."""
    from src.application import optimize as app
    from src.generation import optimize_depth as depth
    name = "moderate"
    model, fm = S.case_model(name)
    (tmp_path / "smplx").mkdir()
    np.savez(tmp_path / "smplx" / "SMPLX_NEUTRAL.npz", **model)
    theta, coef, transl, g = (golden[f"{name}__{k}"] for k in ("theta", "coefficients", "transl", "g"))
    monkeypatch.setattr(app, "BODY_MOCAP_PATH", str(tmp_path))
    body = app.device_body_model()
    kw = {k: v.detach().to("cuda").requires_grad_(v.requires_grad) if v is not None else None for k, v in _split(body, theta, coef, transl).items()}
    _, got = _run(body, kw, g)
    for q in ("vertices", "grad_pose", "grad_transl"):
        dev = S.rel_dev(got[q], golden[f"{name}__r64_{q}"])
        print(f"app factory {q}: {dev:.3e}")
        assert dev <= min(_bounds(golden, q)), q
    ids = list(range(0, 210, 10))
    data = {k: v.detach().cpu().numpy() for k, v in kw.items() if v is not None}
    verts, joints = depth.device_body_model(data, str(tmp_path), extra_joint_vertex_ids=ids)          # drops transl, as the default hook does
    again = depth.device_body_model(data, str(tmp_path), extra_joint_vertex_ids=ids)
    assert len(depth._DEVICE_MODELS) == 1 and np.array_equal(again[0], verts)                         # the model is built once
    fwd = S.forward(fm, coef, theta, None)
    assert joints.shape == (55 + 21 + 5, 3)
    assert S.rel_dev(verts, fwd["vertices"]) <= min(_bounds(golden, "vertices"))
    assert S.rel_dev(joints, S.all_joints(fm, fwd, ids)) <= min(_bounds(golden, "joints"))
    depth._DEVICE_MODELS.clear()


class _IdentityDecoder:
    """Pose-decoder stand-in: the embedding IS the body pose; keeps a handle on the embedding the fit optimises."""

    def encode(self, pose):
        from types import SimpleNamespace
        return SimpleNamespace(mean=pose)

    def decode(self, embedding, output_type="aa"):
        self.embedding = embedding
        return embedding.view(1, -1, 3)


def test_one_fit_step_of_the_app_runs_on_the_device(golden):
    """src/application/optimize.py::fit for one iteration with DeviceSMPLX as the body model and a ComaObjective as the loss: the
    parameter gradients of the total loss against the f64 restatements chained on the host (smplx_ref.backward of app_ref's vertex
    gradients), within 4 x the larger of the two modules' e_ref for gradients."""
    from coma_amd.app import ComaObjective
    from coma_amd.body_model import DeviceSMPLX
    from src.application import optimize as app
    model, fm = S.case_model("moderate")
    body = DeviceSMPLX(model, n_pca=45, device=DEV, extra_joint_vertex_ids=[])
    scale, w_o, w_c = 0.84, 10.0, 5.0
    betas = np.concatenate([np.float32(app.DEFAULT_BETAS).reshape(-1), np.zeros(10, np.float32)])
    theta0 = np.zeros(S.n_theta(fm))
    transl0 = np.float32([3.0, 1.0, 0.0])
    fwd = S.forward(fm, betas, theta0, transl0)
    verts = (fwd["vertices"].astype(np.float32) * np.float32(scale)).astype(np.float32)
    c = app_ref.make_case((verts, fm["faces"]), 40, seed=91)
    c.update(obj_normal=c["obj_normals"][c["ref_index"]], targets=c["obj_verts"][c["objects"]])
    objective = ComaObjective(c["faces"], c["gt"], c["obj_normal"], c["sel"], c["targets"], c["p"], c["sub_p"], c["eps"], device=DEV)
    seen = {}

    def recording_body(**kw):
        seen.update({k: kw[k] for k in ("global_orient", "transl", "left_hand_pose", "right_hand_pose")})
        return body(**kw)
    recording_body.faces = body.faces
    decoder = _IdentityDecoder()
    out = app.fit(lambda v: objective.loss(v, w_o, w_c), recording_body, decoder, app_ref.null_angle_prior, lr=1e-2, body_pose_weight=1.0,
                  bending_prior_weight=1.0, pprior_weight=1.0, scale_factor=scale, num_iters=1, device=DEV, record=True)
    got = np.concatenate([seen["global_orient"].grad.cpu().numpy().ravel(), decoder.embedding.grad.cpu().numpy().ravel(), np.zeros(9),
                          seen["left_hand_pose"].grad.cpu().numpy().ravel(), seen["right_hand_pose"].grad.cpu().numpy().ravel()])
    got_t = seen["transl"].grad.cpu().numpy().ravel()
    ev = app_ref.evaluate(verts, c["faces"], c["gt"], c["obj_normal"], c["p"], c["sub_p"], c["eps"], c["sel"], c["targets"])
    g_verts = scale * (w_o * ev["grad_orientation"] + w_c * ev["grad_contact"])
    want, want_t = S.backward(fm, fwd, g_verts)
    want[66:75] = 0                                           # jaw and eyes are not optimised: fit holds them fixed
    ga, _ = app_ref.load_golden()
    bound = 4 * max(float(golden["e_ref_grad_pose"]), float(golden["e_ref_grad_transl"]), float(ga["e_ref_grad_orientation"]), float(ga["e_ref_grad_contact"]))
    dev, dev_t = S.rel_dev(got, want), S.rel_dev(got_t, want_t)
    print(f"fit step: grad_pose {dev:.3e}, grad_transl {dev_t:.3e}, bound {bound:.3e}; loss {out['losses'][0]:.6f}")
    assert np.all(np.isfinite(got)) and np.abs(want).max() > 0
    assert dev <= bound and dev_t <= bound
    assert out["vertices"].shape == (fm["V"], 3)
