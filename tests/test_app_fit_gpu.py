"""GPU: the fitting app's Adam loop as one device call (coma_amd.app.DeviceFit, coma_app_fit_f32 of coma_amd/csrc/app_fit.hip) against
the reference's own parts run in f64 (R64 of tests/golden/app_fit_golden.npz), against the Python loop it replaces
(src/application/optimize.py::fit with the three device hooks) and against itself (determinism, resume, guard bytes, refusals).

Bounds.  e_ref (stored by the generator, per case) is max|R32 - R64| over the trajectory of all pinned parameters, the reference's own
f32 against its f64; the device -- f32 models around f64 arithmetic, as R32 is f32 throughout -- must stay within 4 e_ref on every row of
the trajectory and, relative to max|R64|, on the last forward's vertices; each loss column within 4 x its own R32 - R64 deviation.
The generator keeps 4 e_ref below lr / 10 and every gradient above 1e-3, so a wiring mistake (a step of order lr) cannot hide.
Against the Python loop the shared kernels see the same f32 seed, so what comes out of them is equal bit for bit.
Figures are printed before they are asserted."""
import ctypes as C
import pickle
import sys

import numpy as np
import pytest
import torch

from tests import fit_ref as R
from tests import smplx_ref as S
from tests import vposer_ref as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BETAS = [R.DEFAULT_BETAS]
RUN = dict(R.WEIGHTS, betas=BETAS, record=True)


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


def _decoder():
    from coma_amd.pose_prior import DeviceVPoser
    c = V.case_shape(R.DECODER)
    return DeviceVPoser(V.case_weights(R.DECODER), c["H"], c["D"], [1, c["NJ"], 3], device=DEV)


def _objective(obj):
    from coma_amd.app import ComaObjective
    return ComaObjective(obj["faces"], obj["gt"], obj["obj_normal"], obj["sel"], obj["targets"], obj["p"], obj["sub_p"], obj["eps"], device=DEV)


def _fit(golden, name):
    from coma_amd.app import DeviceFit
    from coma_amd.body_model import DeviceSMPLX
    from coma_amd.pose_prior import DeviceAnglePrior
    model, _, _, n_pca, _, _ = R.case_models(name)
    body = DeviceSMPLX(model, n_pca=n_pca, device=DEV, extra_joint_vertex_ids=[])
    return DeviceFit(body, _decoder(), DeviceAnglePrior(DEV), _objective(R.golden_objective(*golden, name)))


@pytest.fixture(scope="module")
def runs(golden):
    """Every golden case run once for its 20 iterations; shared and left unchanged."""
    out = {}
    for name in R.CASE_NAMES:
        fit = _fit(golden, name)
        out[name] = (fit, fit.run(num_iters=R.ITERS, **RUN))
    return out


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_golden_case_within_the_reference_s_own_error(golden, runs, name):
    g, meta = golden
    _, got = runs[name]
    r64, e_ref = g[f"{name}__r64_parameters"], float(g[f"{name}__e_ref"])
    cols = R.pinned_columns(name, r64.shape[1])
    dev = float(np.max(np.abs(got["parameters"] - r64)[:, cols]))
    v64 = R.untranslated(name, g[f"{name}__r64_vertices"], r64)
    dev_v = float(np.max(np.abs(R.untranslated(name, got["vertices"], got["parameters"]) - v64)) / np.max(np.abs(v64)))
    dev_l, bound_l = np.max(np.abs(got["loss_terms"] - g[f"{name}__r64_loss_terms"]), axis=0), 4 * g[f"{name}__loss_dev"]
    dev_g = float(np.max(np.abs(got["first_gradient"] - g[f"{name}__r64_first_gradient"])[cols]) / np.max(np.abs(g[f"{name}__r64_first_gradient"])))
    print(f"{name}: device vs R64: parameters {dev:.3e} (bound 4 e_ref = {4 * e_ref:.3e}); vertices {dev_v:.3e} (R32's own {float(g[f'{name}__e_ref_vertices']):.3e}); "
          f"first gradient {dev_g:.3e}; loss columns {['%.2e' % x for x in dev_l]} (bounds {['%.2e' % x for x in bound_l]}); "
          f"loss {got['losses'][0]:.6f} -> {got['losses'][-1]:.6f}")
    assert got["parameters"].shape == r64.shape and got["loss_terms"].shape == (R.ITERS, 5) and got["vertices"].shape == v64.shape
    assert got["trajectory"].shape == (R.ITERS + 1, 6) and np.array_equal(got["trajectory"], got["parameters"][:, :6])
    assert np.array_equal(np.asarray(got["losses"]), got["loss_terms"][:, 0])
    assert all(np.all(np.isfinite(got[key])) for key in ("parameters", "loss_terms", "vertices", "first_gradient"))
    assert dev <= 4 * e_ref
    assert dev_v <= 4 * e_ref
    assert np.all(dev_l <= bound_l), (dev_l, bound_l)
    assert got["losses"][-1] < got["losses"][0]


class _RecordingBody:
    """The device body model with a handle on the parameters fit() builds."""

    def __init__(self, body):
        self.body, self.faces = body, body.faces

    def __call__(self, **kw):
        self.kw = kw
        return self.body(**kw)


class _RecordingDecoder:
    def __init__(self, decoder):
        self.decoder = decoder

    def encode(self, pose):
        return self.decoder.encode(pose)

    def decode(self, embedding, output_type="aa"):
        self.embedding = embedding
        return self.decoder.decode(embedding, output_type=output_type)


def test_first_gradient_is_the_python_loop_s(golden, runs):
    """One iteration of fit() with the three device hooks and one of DeviceFit from the same start: what the shared kernels return
    (global_orient, transl, both hands) is equal bit for bit -- the f32 seed is built in the order of torch's eager ops -- and the
    embedding's gradient, which the device loop assembles in f64, within the bound of test_one_fit_step_with_every_stage_on_the_device."""
    from coma_amd.pose_prior import DeviceAnglePrior
    from src.application import optimize as app
    from tests import app_ref
    fit, got = runs["app"]
    body, decoder = _RecordingBody(fit.body), _RecordingDecoder(fit.decoder)
    w = R.WEIGHTS
    app.fit(lambda v: fit.objective.loss(v, w["orientation_weight"], w["contact_weight"]), body, decoder, DeviceAnglePrior(DEV), lr=w["lr"],
            body_pose_weight=w["body_pose_weight"], bending_prior_weight=w["bending_prior_weight"], pprior_weight=w["pprior_weight"],
            scale_factor=w["scale_factor"], num_iters=1, device=DEV)
    grad = lambda t: t.grad.detach().reshape(-1).cpu().numpy()
    python = {name: grad(body.kw[name]) for name in ("global_orient", "transl", "left_hand_pose", "right_hand_pose")}
    g0 = got["first_gradient"]
    for name, want in python.items():
        mine = g0[fit.layout["p"][name]].astype(np.float32)
        ulp = np.max(np.abs(mine.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)))
        print(f"{name}: {len(want)} entries, largest difference {ulp} ulp, max|g| {np.abs(want).max():.3e}")
        assert want.dtype == np.float32 and np.all(np.isfinite(want)) and np.abs(want).max() > 0
        assert np.array_equal(mine.view(np.int32), want.view(np.int32)), name
    ga, _ = app_ref.load_golden()
    pools = ((V.load_golden(), ("grad_z", "grad_prior")), (S.load_golden(), ("grad_pose", "grad_transl")), (ga, ("grad_orientation", "grad_contact")))
    regular = 4 * max(float(g[f"e_reg_{q}"]) for g, qs in pools for q in qs)
    dev = V.rel_dev(g0[fit.layout["p"]["embedding"]], grad(decoder.embedding).astype(np.float64))
    print(f"embedding: DeviceFit against the Python loop {dev:.3e}, bound {regular:.3e}")
    assert dev <= regular


@pytest.mark.parametrize("name", ("app", "pca6"))
def test_vertices_are_the_last_forward(golden, runs, name):
    fit, got = runs[name]
    p = torch.as_tensor(got["parameters"][R.ITERS - 1]).to(torch.float32).to(DEV)
    at = fit.layout["p"]
    row = lambda key: p[at[key]][None]
    body_pose = fit.decoder.decode(row("embedding"), output_type="aa").view(1, -1)
    out = fit.body(betas=torch.tensor(BETAS, dtype=torch.float32, device=DEV), global_orient=row("global_orient"), body_pose=body_pose,
                   left_hand_pose=row("left_hand_pose"), right_hand_pose=row("right_hand_pose"), transl=row("transl"))
    want = (out.vertices * R.WEIGHTS["scale_factor"])[0].cpu().numpy()
    print(f"{name}: last forward, largest difference {np.max(np.abs(want - got['vertices'])):.3e}")
    assert want.dtype == np.float32 and np.array_equal(want.view(np.int32), got["vertices"].view(np.int32))


RECORDS = ("parameters", "loss_terms", "first_gradient", "vertices", "trajectory")


def test_two_runs_give_the_same_bits_and_a_resumed_run_continues(golden, runs):
    fit, first = runs["app"]
    again = _fit(golden, "app").run(num_iters=R.ITERS, **RUN)
    for key in RECORDS:
        assert np.array_equal(first[key].view(np.uint8), again[key].view(np.uint8)), key
    parts = _fit(golden, "app")
    a = parts.run(num_iters=8, **RUN)
    b = parts.run(num_iters=12, resume=True, **RUN)
    assert np.array_equal(a["parameters"], first["parameters"][:9]) and np.array_equal(b["parameters"], first["parameters"][8:])
    assert np.array_equal(a["loss_terms"], first["loss_terms"][:8]) and np.array_equal(b["loss_terms"], first["loss_terms"][8:])
    assert np.array_equal(a["first_gradient"], first["first_gradient"]) and np.array_equal(b["vertices"].view(np.int32), first["vertices"].view(np.int32))
    assert np.array_equal(parts.parameters().cpu().numpy(), first["parameters"][-1])
    from coma_amd._lib import ComaHipError
    with pytest.raises(ComaHipError, match="has not run yet"):
        _fit(golden, "app").run(num_iters=1, resume=True, **RUN)


GUARD, PATTERN = 4096, 0xA5


def _guarded(nbytes):
    """A device buffer of nbytes between two guard blocks: (whole buffer, address of the inner part)."""
    whole = torch.full([GUARD + nbytes + GUARD], PATTERN, dtype=torch.uint8, device=DEV)
    return whole, whole.data_ptr() + GUARD


def _guards_intact(whole):
    return bool((whole[:GUARD] == PATTERN).all()) and bool((whole[-GUARD:] == PATTERN).all())


@pytest.mark.parametrize("Vn, k", [(257, 40), (256, 0), (513, 513)])
def test_workspace_and_state_stay_inside_their_bytes(Vn, k):
    """A direct ctypes call with the workspace, the state and every record between guard blocks.  Sizes: the golden model's, one
    vertex less (a full last workgroup) and one more than two workgroups, J and F from smplx_ref.synthetic_model; k = 0 and k = V."""
    from coma_amd import _lib
    from coma_amd.app import ComaObjective, DeviceFit
    from coma_amd.body_model import DeviceSMPLX
    from coma_amd.pose_prior import DeviceAnglePrior
    model = S.synthetic_model(Vn, 55, 20, 45, "random", seed=7000 + Vn)
    rng = np.random.default_rng(Vn)
    unit = lambda n: (lambda a: (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32))(rng.normal(size=(n, 3)))
    objective = ComaObjective(model["f"], unit(Vn), unit(1)[0], rng.permutation(Vn)[:k], (rng.uniform(-1, 1, size=(k, 3)) + [3, 1, 0]).astype(np.float32),
                              device=DEV)
    fit = DeviceFit(DeviceSMPLX(model, n_pca=45, device=DEV, extra_joint_vertex_ids=[]), _decoder(), DeviceAnglePrior(DEV), objective)
    fit.body._shape_stage(torch.as_tensor(np.float32(BETAS)), None)
    p0 = fit.start()
    fit._buffers()
    E, P, L = 3, fit.P, _lib.lib()
    assert fit._ws_bytes == L.coma_app_fit_workspace_bytes(Vn, 2 * Vn, 55, k, 512, 21, 165) and fit._state_bytes == L.coma_app_fit_state_bytes(P)
    ws, ws_at = _guarded(fit._ws_bytes)
    state, state_at = _guarded(fit._state_bytes)
    traj, traj_at = _guarded(8 * (E + 1) * P)
    losses, losses_at = _guarded(8 * E * 5)
    grad0, grad0_at = _guarded(8 * P)
    verts, verts_at = _guarded(4 * 3 * Vn)
    vertices = verts[GUARD:GUARD + 12 * Vn].view(torch.float32).view(Vn, 3)
    weights = {key: v for key, v in R.WEIGHTS.items()}
    d, keep = fit.descriptor(E, weights, C.c_void_p(traj_at), C.c_void_p(losses_at), C.c_void_p(grad0_at), vertices)
    with _lib.on_device(torch.device(DEV)) as stream:
        rc = L.coma_app_fit_init_f64(_lib.ptr(p0, torch.float64), P, C.c_void_p(state_at), fit._state_bytes, stream)
        assert rc == 0, L.coma_last_error()
        rc = L.coma_app_fit_f32(C.byref(d), C.c_void_p(state_at), fit._state_bytes, C.c_void_p(ws_at), fit._ws_bytes, stream)
        assert rc == 0, L.coma_last_error()
        iteration = C.c_int(-1)
        assert L.coma_app_fit_status(C.c_void_p(state_at), stream, C.byref(iteration)) == 0, L.coma_last_error()
    for name, whole in (("workspace", ws), ("state", state), ("traj", traj), ("losses", losses), ("grad0", grad0), ("vertices", verts)):
        assert _guards_intact(whole), name
    rows = traj[GUARD:-GUARD].view(torch.float64).view(E + 1, P).cpu().numpy()
    terms = losses[GUARD:-GUARD].view(torch.float64).view(E, 5).cpu().numpy()
    print(f"V={Vn} k={k}: workspace {fit._ws_bytes} bytes, state {fit._state_bytes}; loss {terms[0, 0]:.6f} -> {terms[-1, 0]:.6f}")
    assert np.array_equal(rows[0], p0.cpu().numpy()) and np.all(np.isfinite(rows)) and np.all(np.isfinite(terms)) and np.all(np.isfinite(vertices.cpu().numpy()))
    assert np.all(np.abs(np.diff(rows, axis=0)[:, :3]) > 0)                                   # every iteration stepped
    assert np.array_equal(state[GUARD + 64:GUARD + 64 + 8 * P].view(torch.float64).cpu().numpy(), rows[-1])
    if k == 0:
        assert np.all(terms[:, 4] == 0)


def test_non_finite_gradient_freezes_the_parameters_and_is_reported(golden):
    """orientation_weight = 3e38 on a mesh scaled to 1e-3: the orientation gradients are of order 1 / scale, so the f32 seed
    fl32(w_o) g_o overflows in the first iteration (at the golden scale of 0.84 the largest |g_o| is 0.04 and nothing would).  Expected:
    no step is ever applied, every row of the trajectory is row 0, status names iteration 0, run raises.
    The backward kernels of smplx.hip and vposer.hip were read for this test: a gradient value is only ever an operand of floating-point
    arithmetic there, never an index or a loop bound (neither file converts a floating-point value to an integer)."""
    from coma_amd._lib import ComaHipError
    fit = _fit(golden, "app")
    run = dict(RUN, orientation_weight=3e38, scale_factor=1e-3)
    with pytest.raises(ComaHipError, match="iteration 0") as e:
        fit.run(num_iters=5, **run)
    print(f"non-finite: {e.value}")
    assert "not finite" in str(e.value)
    got = fit.last
    assert got["parameters"].shape == (6, fit.P) and np.all(got["parameters"] == got["parameters"][0]) and np.all(np.isfinite(got["parameters"]))
    assert not np.all(np.isfinite(got["first_gradient"]))
    assert np.array_equal(fit.parameters().cpu().numpy(), got["parameters"][0])
    # the state stays refused until it is initialised again, and a fresh run on the same object is clean
    with pytest.raises(ComaHipError, match="iteration 0"):
        fit.run(num_iters=1, resume=True, **run)
    clean = fit.run(num_iters=2, **RUN)
    assert np.all(np.isfinite(clean["parameters"])) and np.all(clean["parameters"][1] != clean["parameters"][0])


def test_refusals_write_nothing(golden):
    """Every host refusal of coma_app_fit_f32 with real device buffers: COMA_E_INVALID, a coma_last_error text, and the state, the
    workspace and the records as they were."""
    from coma_amd import _lib
    fit = _fit(golden, "app")
    fit.body._shape_stage(torch.as_tensor(np.float32(BETAS)), None)
    p0 = fit.start()
    fit._buffers()
    E, P, L = 4, fit.P, _lib.lib()
    filled = lambda n: torch.full([n], PATTERN, dtype=torch.uint8, device=DEV)
    ws, state, traj, losses, grad0 = filled(fit._ws_bytes), filled(fit._state_bytes), filled(8 * (E + 1) * P), filled(8 * E * 5), filled(8 * P)
    vertices = filled(12 * fit.body.V).view(torch.float32).view(-1, 3)
    buffers = (ws, state, traj, losses, grad0, vertices.view(-1).view(torch.uint8))
    address = lambda t: C.c_void_p(t.data_ptr())

    def call(state_bytes=None, ws_bytes=None, state_at=None, ws_at=None, **over):
        d, keep = fit.descriptor(E, dict(R.WEIGHTS), address(traj), address(losses), address(grad0), vertices)
        for key, value in over.items():
            setattr(d, key, value)
        with _lib.on_device(torch.device(DEV)) as stream:
            rc = L.coma_app_fit_f32(C.byref(d), address(state) if state_at is None else state_at, fit._state_bytes if state_bytes is None else state_bytes,
                                    address(ws) if ws_at is None else ws_at, fit._ws_bytes if ws_bytes is None else ws_bytes, stream)
        return rc, L.coma_last_error().decode()

    cases = [(dict(E=0), "E=0"), (dict(E=4097), "E=4097"), (dict(P=P - 1), "6 + 2 hs + D"), (dict(V=0), "outside what"), (dict(k=fit.body.V + 1), "outside what"),
             (dict(H=0), "outside what"), (dict(D=0), "D=0"), (dict(NJ=22), "do not fill"), (dict(n_pca=65), "n_pca=65"), (dict(prior_K=17), "prior_K=17"),
             (dict(eps=-1.0), "eps"), (dict(lr=float("inf")), "finite"), (dict(contact_weight=float("nan")), "finite"), (dict(scale_factor=float("nan")), "finite"),
             (dict(weights=None), "null pointer"), (dict(W1=None), "null pointer"), (dict(orientation_gt=None), "null pointer"), (dict(losses=None), "null pointer"),
             (dict(vertices=None), "null pointer"), (dict(parents=None), "null pointer"), (dict(targets=None), "selected / targets"),
             (dict(state_bytes=fit._state_bytes - 16), "state of"), (dict(ws_bytes=fit._ws_bytes - 16), "workspace of"),
             (dict(state_at=C.c_void_p(state.data_ptr() + 8)), "state must be 16-byte aligned"), (dict(ws_at=C.c_void_p(ws.data_ptr() + 4)), "workspace must be 16-byte aligned"),
             (dict(state_at=None, ws_at=C.c_void_p(0)), "null pointer"),
             # refusals of a stage alone (the decoder's alignment, the objective's bound on F): from its plan, before the first launch
             (dict(W1=fit.decoder._w["bodyprior_dec_fc1.weight"].data_ptr() + 2), "4-byte aligned"),
             (dict(b3=fit.decoder._w["bodyprior_dec_out.bias"].data_ptr() + 2), "4-byte aligned"),
             (dict(F=715827883), "F=715827883")]
    for kw, text in cases:
        rc, said = call(**kw)
        assert rc == -1 and text in said and said.startswith("coma_app_fit_f32: "), (kw, said)
    torch.cuda.synchronize()
    for t in buffers:
        assert bool((t == PATTERN).all())
    # a state that no init has written: the call is accepted (the host cannot see device memory), its kernels write nothing to the
    # records, and status says so
    rc, said = call()
    assert rc == 0, said
    with _lib.on_device(torch.device(DEV)) as stream:
        assert L.coma_app_fit_status(address(state), stream, None) == -1 and "not written by coma_app_fit_init_f64" in L.coma_last_error().decode()
    for t in (state, traj, losses, grad0):
        assert bool((t == PATTERN).all())
    # ... and one initialised for another P
    with _lib.on_device(torch.device(DEV)) as stream:
        assert L.coma_app_fit_init_f64(_lib.ptr(p0, torch.float64), P - 2, address(state), fit._state_bytes, stream) == 0
    assert call()[0] == 0
    with _lib.on_device(torch.device(DEV)) as stream:
        assert L.coma_app_fit_status(address(state), stream, None) == -1 and f"initialised for P={P - 2}" in L.coma_last_error().decode()
    for t in (traj, losses, grad0):
        assert bool((t == PATTERN).all())


def test_device_fit_refuses_what_does_not_fit_together(golden):
    from coma_amd._lib import ComaHipError
    from coma_amd.app import DeviceFit
    from coma_amd.body_model import DeviceSMPLX
    from coma_amd.pose_prior import DeviceAnglePrior, DeviceVPoser
    fit = _fit(golden, "app")
    body, decoder, prior, objective = fit.body, fit.decoder, fit.prior, fit.objective
    for args, name in (((object(), decoder, prior, objective), "body"), ((body, object(), prior, objective), "decoder"),
                       ((body, decoder, lambda pose: pose, objective), "prior"), ((body, decoder, prior, object()), "objective")):
        with pytest.raises(TypeError, match=f"{name} must be a"):
            DeviceFit(*args)
    odd = DeviceVPoser(V.case_weights("odd"), 80, 7, [1, 5, 3], device=DEV)
    with pytest.raises(ValueError, match="15 body-pose entries, the body model takes 63"):
        DeviceFit(body, odd, prior, objective)
    small = DeviceSMPLX(S.synthetic_model(63, 55, 20, 45, "random", seed=1), n_pca=45, device=DEV, extra_joint_vertex_ids=[])
    with pytest.raises(ValueError, match="built for 257 vertices, the body model has 63"):
        DeviceFit(small, decoder, prior, objective)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ComaHipError, match="different devices"):
            DeviceFit(body, decoder, DeviceAnglePrior("cuda:1"), objective)
    assert DeviceFit(body, decoder, DeviceAnglePrior("cuda"), objective).P == 128          # "cuda" is the current device: the same one


def _experiment_dir(path, name):
    c = V.case_shape(name)
    (path / "snapshots").mkdir(parents=True)
    (path / "synthetic.ini").write_text(f"[All]\nnum_neurons : {c['H']}\nlatentD : {c['D']}\ndata_shape : [1, {c['NJ']}, 3]\nuse_cont_repr : True\n")
    torch.save({k: torch.from_numpy(v) for k, v in V.case_weights(name).items()}, path / "snapshots" / "synthetic_E001.pt")


def test_cli_runs_a_short_fit_in_the_device_loop(tmp_path, monkeypatch):
    """src/application/optimize.py --body_model device --pose_prior device --loop device on the synthetic model files of
    test_cli_runs_a_short_fit_without_third_party_packages: three iterations, the mesh written with the vertices the fit returned;
    --loop device alone stops with the pinned text."""
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
    prob[np.arange(Vn), 0, np.arange(Vn)] = 1.0
    nom = np.full((Vn, O), 0.1, np.float32)
    nom[rng.choice(Vn, size=k, replace=False), rng.integers(0, O, size=k)] = 1.0
    state = dict(prob_grid_canon_human_wrt_obj=prob, canon_normal_grid=unit(Vn), contact_dist_expectation_grid_nom=nom,
                 contact_dist_expectation_grid_denom=np.ones((Vn, O), np.float32))
    asset = dict(downsampled_pcd_points_raw=(rng.uniform(-1, 1, size=(O, 3)) + [3.0, 1.0, 0.0]).astype(np.float32), downsampled_pcd_normal_raw=unit(O))
    for pth, obj in ((tmp_path / "coma.pickle", state), (tmp_path / "asset.pickle", asset)):
        with open(pth, "wb") as fh:
            pickle.dump(obj, fh)
    flags = ["--supercategory", "super", "--category", "cat", "--coma_path", str(tmp_path / "coma.pickle"), "--asset_downsample_pth",
             str(tmp_path / "asset.pickle"), "--num_iters", "3", "--body_model", "device", "--pose_prior", "device"]
    for package in ("smplx", "configer", "torchgeometry"):
        monkeypatch.setitem(sys.modules, package, None)
    out = app.main(app.build_parser().parse_args(flags + ["--save_dir", str(tmp_path / "out"), "--loop", "device"]))
    assert out["vertices"].shape == (Vn, 3) and np.all(np.isfinite(out["vertices"])) and len(out["losses"]) == 3
    from coma_amd.downsample import load_obj
    v, f = load_obj(out["path"])
    assert out["path"] == str(tmp_path / "out" / "super" / "cat" / "optimized.obj") and v.shape == (Vn, 3) and np.array_equal(f, fm["faces"])
    assert np.array_equal(v.astype(np.float32), out["vertices"])                            # nine significant digits: f32 round-trips
    with pytest.raises(SystemExit) as e:
        app.main(app.build_parser().parse_args(["--loop", "device"]))
    assert str(e.value) == app.LOOP_NEEDS_BODY_MODEL
