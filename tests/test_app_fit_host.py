"""No GPU: the fitting app's device loop seen from the host -- the restatement tests/fit_ref.py against the reference's own parts run in
f64 (R64 of tests/golden/app_fit_golden.npz), the fixture's own conditions, the CLI's --loop flag and its refusals, the index
bookkeeping and chunking of coma_amd.app.DeviceFit, and the refusals coma_app_fit_f32 gives before it launches anything.

Bound of the restatement: 1e-3 e_ref per case, e_ref = max|R32 - R64| over the trajectory, the reference's own f32 error.  Only
below that can the restatement stand in for R64 where no golden case exists.  Figures are printed before they are asserted."""
import ctypes as C

import numpy as np
import pytest

from tests import app_ref
from tests import fit_ref as R


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_restatement_within_a_thousandth_of_the_reference_s_own_error(golden, name):
    g, meta = golden
    _, fm, w, _, k, _ = R.case_models(name)
    m = meta[name]
    assert {key: m[key] for key in R.WEIGHTS} == R.WEIGHTS and m["iters"] == R.ITERS and m["k"] == k
    obj = R.golden_objective(g, meta, name)
    mine = R.run(fm, w, R.coefficients(), obj, R.WEIGHTS, R.ITERS)
    r64, e_ref = g[f"{name}__r64_parameters"], float(g[f"{name}__e_ref"])
    cols = R.pinned_columns(name, r64.shape[1])
    dev = float(np.max(np.abs(mine["parameters"] - r64)[:, cols]))
    dev_l = np.max(np.abs(mine["loss_terms"] - g[f"{name}__r64_loss_terms"]), axis=0)
    dev_g = float(np.max(np.abs(mine["gradients"][0] - g[f"{name}__r64_first_gradient"])[cols]))
    v64 = R.untranslated(name, g[f"{name}__r64_vertices"], r64)
    dev_v = float(np.max(np.abs(R.untranslated(name, mine["vertices"], mine["parameters"]) - v64)) / np.max(np.abs(v64)))
    print(f"{name}: restatement vs R64: parameters {dev:.3e} = {dev / e_ref:.2e} e_ref (e_ref {e_ref:.3e}); first gradient {dev_g:.3e}; "
          f"loss columns {['%.2e' % x for x in dev_l]}; vertices {dev_v:.3e}")
    assert mine["parameters"].shape == r64.shape == (R.ITERS + 1, m["P"])
    assert dev <= 1e-3 * e_ref
    assert dev_v <= 1e-3 * float(g[f"{name}__e_ref_vertices"])
    assert np.all(dev_l[1:] <= 1e-3 * np.maximum(g[f"{name}__loss_dev"][1:], 1e-12))          # a zero deviation (no contact term): exact up to f64
    assert dev_l[0] <= 1e-3 * g[f"{name}__loss_dev"][0]


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_fixture_meets_its_own_conditions(golden, name):
    """(a) |g| >= 1e-3 in every pinned component at every iteration -- read off the restatement, which the test above ties to R64 --
    and (b) 4 e_ref <= lr / 10; the loss goes down."""
    g, meta = golden
    _, fm, w, _, _, _ = R.case_models(name)
    mine = R.run(fm, w, R.coefficients(), R.golden_objective(g, meta, name), R.WEIGHTS, R.ITERS)
    cols = R.pinned_columns(name, mine["parameters"].shape[1])
    g_min, e_ref = float(np.min(np.abs(mine["gradients"][:, cols]))), float(g[f"{name}__e_ref"])
    print(f"{name}: min|g| {g_min:.3e}; 4 e_ref {4 * e_ref:.3e} against lr / 10 = {R.WEIGHTS['lr'] / 10:.1e}")
    assert g_min >= 1e-3 and 4 * e_ref <= R.WEIGHTS["lr"] / 10
    losses = g[f"{name}__r64_loss_terms"][:, 0]
    assert losses[-1] < losses[0]
    free = [i for i in range(mine["parameters"].shape[1]) if i not in cols]
    if free:                                                   # the loss does not depend on them: their gradient is rounding noise
        assert np.max(np.abs(mine["gradients"][:, free])) <= 1e-9 * np.max(np.abs(mine["gradients"]))


# ---- host logic of DeviceFit ----
def test_chunks_of_at_most_4096():
    from coma_amd.app import MAX_FIT_ITERATIONS, fit_chunks
    assert MAX_FIT_ITERATIONS == 4096
    assert fit_chunks(0) == [] and fit_chunks(1) == [1] and fit_chunks(2000) == [2000] and fit_chunks(4096) == [4096]
    assert fit_chunks(4097) == [4096, 1] and fit_chunks(10000) == [4096, 4096, 1808] and fit_chunks(7, limit=3) == [3, 3, 1]
    with pytest.raises(ValueError):
        fit_chunks(-1)


@pytest.mark.parametrize("hand_size, latent, num_body", [(45, 32, 63), (6, 32, 63), (0, 7, 15), (12, 1, 3)])
def test_parameter_layout_follows_the_body_model_s_order(hand_size, latent, num_body):
    """p's groups and theta's slots against the order DeviceSMPLX.__call__ concatenates its arguments in (its `sizes` tuple, transl
    last and apart) and the order fit() hands its parameters to Adam."""
    from coma_amd.app import fit_parameter_layout
    L = fit_parameter_layout(hand_size, latent, num_body)
    sizes = (("global_orient", 3), ("body_pose", num_body), ("jaw_pose", 3), ("leye_pose", 3), ("reye_pose", 3), ("left_hand_pose", hand_size),
             ("right_hand_pose", hand_size))
    at = 0
    for name, n in sizes:
        assert L["theta"][name] == slice(at, at + n), name
        at += n
    assert L["n_theta"] == at == num_body + 12 + 2 * hand_size
    at = 0
    for name, n in (("global_orient", 3), ("transl", 3), ("left_hand_pose", hand_size), ("right_hand_pose", hand_size), ("embedding", latent)):
        assert L["p"][name] == slice(at, at + n), name
        at += n
    assert L["P"] == at == 6 + 2 * hand_size + latent
    # the restatement's packing is the same one
    fm = dict(n_pca=hand_size, hd=0, J=(num_body + 12) // 3)
    p = np.arange(L["P"], dtype=np.float64) + 1
    theta = R.theta_of(fm, p, -np.arange(num_body, dtype=np.float64))
    for name in ("global_orient", "left_hand_pose", "right_hand_pose"):
        assert np.array_equal(theta[L["theta"][name]], p[L["p"][name]]), name
    assert np.array_equal(theta[L["theta"]["body_pose"]], -np.arange(num_body)) and not theta[L["theta"]["jaw_pose"].start:L["theta"]["reye_pose"].stop].any()
    assert R.layout(fm, latent) == (hand_size, num_body, L["P"])


def test_device_fit_refuses_other_types():
    from coma_amd.app import DeviceFit
    with pytest.raises(TypeError, match="body must be a DeviceSMPLX"):
        DeviceFit(object(), None, None, None)


def test_descriptor_is_bound_from_the_header():
    from coma_amd import _abi
    from coma_amd.app import FitDesc
    fields = dict(_abi.STRUCTS["coma_app_fit_desc"])
    assert FitDesc._fields_ == _abi.STRUCTS["coma_app_fit_desc"]
    assert fields["posedirs"] is C.c_void_p and fields["V"] is C.c_int and fields["eps"] is C.c_double and fields["scale_factor"] is C.c_double
    assert [n for n, _ in FitDesc._fields_][-4:] == ["traj", "losses", "grad0", "vertices"]
    assert _abi.DEFINES["COMA_ABI_VERSION"] == 11


# ---- the entry points' refusals that need no device ----
def _desc(**over):
    """A descriptor of the app's sizes whose pointers are never followed: every refusal below comes before any launch."""
    from coma_amd.app import FitDesc
    d, one = FitDesc(), 16
    for name, ctype in FitDesc._fields_:
        if ctype is C.c_void_p:
            setattr(d, name, one)
    keep = [(C.c_int32 * 55)(*([0] + list(range(54)))), (C.c_float * 3)(0, 0, 1), (C.c_float * 3)(0, 0, 1), (C.c_float * 3)(0, 1, 0),
            (C.c_int32 * 4)(52, 55, 9, 12), (C.c_float * 4)(1, -1, -1, -1)]
    for name, array in zip(("parents", "obj_normal", "principle_vec", "sub_principle_vec", "prior_index", "prior_sign"), keep):
        setattr(d, name, C.cast(array, C.c_void_p))
    d.V, d.J, d.hand_dim, d.n_pca, d.D, d.H, d.NJ, d.prior_K, d.F, d.k, d.eps, d.P, d.E = 257, 55, 45, 45, 32, 512, 21, 4, 514, 40, 1e-6, 128, 20
    d.lr, d.body_pose_weight, d.bending_prior_weight, d.pprior_weight, d.orientation_weight, d.contact_weight, d.scale_factor = 1e-2, 2, 0.5, 0.3, 10, 5, 0.84
    for name, value in over.items():
        setattr(d, name, value)
    d._keep = keep
    return d


def _refused(hip_lib, d, state=16, state_bytes=None, ws=16, ws_bytes=None):
    sb = hip_lib.coma_app_fit_state_bytes(128) if state_bytes is None else state_bytes
    wb = hip_lib.coma_app_fit_workspace_bytes(257, 514, 55, 40, 512, 21, 165) if ws_bytes is None else ws_bytes
    rc = hip_lib.coma_app_fit_f32(C.byref(d) if d is not None else None, state, sb, ws, wb, None)
    return rc, hip_lib.coma_last_error().decode()


REFUSALS = [(dict(E=0), "E=0 outside [1, 4096]"), (dict(E=4097), "E=4097 outside [1, 4096]"), (dict(P=127), "P=127, but 6 + 2 hs + D = 128"),
            (dict(D=0), "D=0 outside"), (dict(D=257), "D=257 outside"), (dict(V=0), "outside what the body model"), (dict(F=0), "outside what the body model"),
            (dict(k=258), "outside what the body model"), (dict(H=2049), "outside what the body model"), (dict(J=65, NJ=31), "outside what the body model"),
            (dict(NJ=20), "do not fill"), (dict(hand_dim=44), "hand_dim=44"), (dict(n_pca=65), "n_pca=65"), (dict(prior_K=0), "prior_K=0"),
            (dict(prior_K=17), "prior_K=17"), (dict(eps=-1.0), "eps must be finite"), (dict(lr=float("nan")), "must be finite"),
            (dict(orientation_weight=float("inf")), "must be finite"), (dict(scale_factor=float("-inf")), "must be finite"),
            (dict(posedirs=None), "null pointer"), (dict(shape_state=None), "null pointer"), (dict(lead_fixed=None), "null pointer"),
            (dict(W3=None), "null pointer"), (dict(prior_sign=None), "null pointer"), (dict(vf_faces=None), "null pointer"),
            (dict(losses=None), "null pointer"), (dict(vertices=None), "null pointer"), (dict(hand_components=None), "hand_components"),
            (dict(selected=None), "selected / targets"), (dict(shape_state=24), "shape state must be 16-byte aligned"), (dict(traj=20), "8-byte"),
            # refusals of a stage alone, which the fit never restated: they come from the stage's plan, before the first launch
            (dict(W1=18), "4-byte aligned"), (dict(b3=18), "4-byte aligned"), (dict(F=715827883), "F=715827883")]


@pytest.mark.parametrize("over, text", REFUSALS, ids=[",".join(f"{k}={v}" for k, v in o.items()) for o, _ in REFUSALS])
def test_refused_before_any_launch(hip_lib, over, text):
    rc, said = _refused(hip_lib, _desc(**over))
    assert rc == -1 and text in said and said.startswith("coma_app_fit_f32: "), said


def test_refusals_of_buffers_and_host_tables(hip_lib):
    assert _refused(hip_lib, None)[0] == -1 and "null pointer" in hip_lib.coma_last_error().decode()
    for kw, text in ((dict(state=None), "null pointer"), (dict(ws=None), "null pointer"), (dict(state_bytes=3135), "state of 3135 bytes, 3136 needed"),
                     (dict(state=24), "state must be 16-byte aligned"), (dict(ws_bytes=1000), "workspace of 1000 bytes"),
                     (dict(ws=8), "workspace must be 16-byte aligned")):
        rc, said = _refused(hip_lib, _desc(), **kw)
        assert rc == -1 and text in said, (kw, said)
    d = _desc()
    d._keep[0][7] = 7                                           # joint 7 its own parent
    assert _refused(hip_lib, d) == (-1, "coma_app_fit_f32: parent 7 of joint 7 outside [0, 7)")
    d = _desc()
    d._keep[4][1] = 63
    assert _refused(hip_lib, d) == (-1, "coma_app_fit_f32: prior_index[1]=63 outside [0, 63)")
    d = _desc()
    d._keep[3][2] = 0.5                                         # sub_principle_vec no longer orthogonal to principle_vec
    assert _refused(hip_lib, d) == (-1, "coma_app_fit_f32: principle_vec and sub_principle_vec are not orthogonal")
    # the accepted descriptor passes every host check: proof that each refusal above is its own (nothing is launched: the last
    # check, the alignment of an output, is made to fail)
    rc, said = _refused(hip_lib, _desc(grad0=12))
    assert rc == -1 and "8-byte" in said
    # sizes
    L = hip_lib
    assert L.coma_app_fit_state_bytes(128) == 8 * (8 + 3 * 128) and L.coma_app_fit_state_bytes(50) == 8 * (8 + 150)
    assert L.coma_app_fit_state_bytes(6) == 0 and L.coma_app_fit_state_bytes(513) == 0 and L.coma_app_fit_state_bytes(512) > 0
    need = L.coma_app_fit_workspace_bytes
    assert need(257, 514, 55, 40, 512, 21, 165) > need(257, 514, 55, 0, 512, 21, 165) > 0
    for bad in ((0, 514, 55, 40, 512, 21, 165), (257, 0, 55, 40, 512, 21, 165), (257, 514, 65, 40, 512, 21, 165), (257, 514, 55, 258, 512, 21, 165),
                (257, 514, 55, 40, 2049, 21, 165), (257, 514, 55, 40, 512, 65, 165), (257, 514, 55, 40, 512, 21, 74), (257, 514, 55, 40, 512, 21, 268)):
        assert need(*bad) == 0, bad
    one = C.c_void_p(16)
    assert L.coma_app_fit_init_f64(None, 128, one, 3136, None) == -1 and b"null pointer" in L.coma_last_error()
    assert L.coma_app_fit_init_f64(one, 6, one, 3136, None) == -1 and b"P=6 outside [7, 512]" in L.coma_last_error()
    assert L.coma_app_fit_init_f64(one, 128, one, 3120, None) == -1 and b"state of 3120 bytes" in L.coma_last_error()
    assert L.coma_app_fit_init_f64(C.c_void_p(12), 128, one, 3136, None) == -1 and b"p0 must be 8-byte aligned" in L.coma_last_error()
    assert L.coma_app_fit_status(None, None, None) == -1 and b"null pointer" in L.coma_last_error()


# ---- the CLI ----
def test_loop_flag_is_absent_unless_given():
    from src.application import optimize as app
    plain = app.build_parser().parse_args([])
    assert "loop" not in vars(plain) and app.loop_choice(plain) == "torch"
    chosen = app.build_parser().parse_args(["--loop", "device"])
    assert app.loop_choice(chosen) == "device" and {k: v for k, v in vars(chosen).items() if k != "loop"} == vars(plain)
    assert app.loop_choice(app.build_parser().parse_args(["--loop", "torch"])) == "torch"
    with pytest.raises(SystemExit):
        app.build_parser().parse_args(["--loop", "graph"])


def test_loop_device_says_which_flag_is_missing(monkeypatch):
    from src.application import optimize as app
    parse = lambda *flags: app.build_parser().parse_args(["--loop", "device", *flags])
    with pytest.raises(SystemExit) as e:
        app.main(parse())
    assert str(e.value) == app.LOOP_NEEDS_BODY_MODEL == ("--loop device needs --body_model device: the device loop drives "
                                                         "coma_amd.body_model.DeviceSMPLX, not a body-model hook")
    with pytest.raises(SystemExit) as e:
        app.main(parse("--pose_prior", "device"))
    assert str(e.value) == app.LOOP_NEEDS_BODY_MODEL
    with pytest.raises(SystemExit) as e:
        app.main(parse("--body_model", "device"))
    assert str(e.value) == app.LOOP_NEEDS_POSE_PRIOR == ("--loop device needs --pose_prior device: the device loop drives coma_amd.pose_prior's "
                                                         "decoder and angle prior, not hooks")
    for hook in ("body_model", "pose_decoder", "angle_prior"):
        with pytest.raises(SystemExit) as e:
            app.main(parse("--body_model", "device", "--pose_prior", "device"), **{hook: object()})
        assert str(e.value) == app.LOOP_TAKES_NO_HOOKS and "hooks passed to main() cannot be used" in str(e.value)
    with pytest.raises(SystemExit, match="COAP"):             # --use_collision keeps its refusal, and it comes first
        app.main(parse("--use_collision"))
    # with both flags main() builds the device models and hands the choice on; without --loop the keyword is not passed at all
    seen = []
    monkeypatch.setattr(app, "device_body_model", lambda device="cuda": "body")
    monkeypatch.setattr(app, "device_pose_prior", lambda device="cuda": ("decoder", "prior"))
    monkeypatch.setattr(app, "optimize_smpl", lambda **kw: seen.append((kw["body_model"], kw["pose_decoder"], kw["angle_prior"], kw.get("loop"))))
    app.main(parse("--body_model", "device", "--pose_prior", "device"))
    app.main(app.build_parser().parse_args(["--body_model", "device", "--pose_prior", "device"]))
    app.main(app.build_parser().parse_args(["--body_model", "device", "--pose_prior", "device", "--loop", "torch"]))
    assert seen == [("body", "decoder", "prior", "device"), ("body", "decoder", "prior", None), ("body", "decoder", "prior", None)]


def test_optimize_smpl_loop_torch_calls_fit_as_before(monkeypatch, tmp_path):
    """loop="torch" and no keyword at all reach fit() with the same arguments -- shown on the CPU with app_ref's stand-in hooks as far
    as that goes without a device: the objective's constructor and fit() itself are recorded, not run."""
    import coma_amd.app as device_app
    from src.application import optimize as app
    verts, faces = app_ref.grid_mesh(5, seed=3)
    body = app_ref.RigidBody(None, faces)
    decoder, prior = app_ref.NullPoseDecoder(), app_ref.null_angle_prior
    calls = []

    class Objective:
        @classmethod
        def from_state(cls, *a):
            return cls()

        def loss(self, vertices, w_o, w_c):
            return ("loss", w_o, w_c)

    def fit(objective_loss, *a, **kw):
        calls.append((objective_loss("v"), a, kw))
        return dict(vertices=verts, losses=[], trajectory=[])

    monkeypatch.setattr(device_app, "ComaObjective", Objective)
    monkeypatch.setattr(app, "fit", fit)
    kw = dict(supercategory="s", category="c", coma_path={}, asset_downsample_pth={}, eps=1e-6, principle_vec=[0, 0, 1], sub_principle_vec=[0, 1, 0],
              reference_object_vertex_index=0, lr=1e-2, body_pose_weight=2.0, bending_prior_weight=0.5, pprior_weight=0.3, orientation_weight=10.0,
              contact_weight=5.0, contact_threshold=0.3, scale_factor=0.84, use_collision=False, save_dir=str(tmp_path), num_iters=3, body_model=body,
              pose_decoder=decoder, angle_prior=prior, device="cpu")
    a, b = app.optimize_smpl(**kw), app.optimize_smpl(loop="torch", **kw)
    assert len(calls) == 2 and calls[0] == calls[1]
    assert calls[0][0] == ("loss", 10.0, 5.0) and calls[0][1] == (body, decoder, prior, 1e-2, 2.0, 0.5, 0.3, 0.84, 3, "cpu") and calls[0][2] == dict(record=False)
    assert a["path"] == b["path"] == str(tmp_path / "s" / "c" / "optimized.obj")
    with pytest.raises(ValueError, match="loop must be 'torch' or 'device'"):
        app.optimize_smpl(loop="graph", **kw)
    with pytest.raises(NotImplementedError, match="COAP"):
        app.optimize_smpl(loop="device", **dict(kw, use_collision=True))
    assert len(calls) == 2
