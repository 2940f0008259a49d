"""GPU: the device SMPL-X body model's full backward (DeviceSMPLX(differentiable=...), coma_smplx_backward_full_f32) against the
third-party package's own lbs and SMPLX class under autograd in f64 (R64 of tests/golden/smplx_grad_golden.npz) and against the f64
restatement tests/smplx_grad_ref.py.

Bounds, with the margin and the reasoning of tests/test_smplx_gpu.py.  e_ref_* (stored by the generator) is max|R32 - R64| / max|R64|
pooled over the cases and the four losses, the package's own f32 against its f64; the device must meet 4 * e_ref on every case (two
f32 evaluations of one formula in different summation orders).  `small_angle` inflates the pooled grad_pose figure (1.3e-5 against
5.9e-7), so every OTHER case is also held to 4 * e_reg, the same pool without it.  Against the restatement (the same rule set in
f64, of which the device returns the f32 rounding) the tighter of the two bounds is used.  Figures are printed before they are asserted.

Measured on MI355X, device against R64, the largest over the four losses (bounds: grad_pose 5.2e-5 / 2.3e-6, grad_transl 1.1e-6,
grad_coef 4.3e-6): see DESIGN.md section 2x.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import smplx_grad_ref as GR
from tests import smplx_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POSE_KEYS = ("global_orient", "body_pose", "jaw_pose", "leye_pose", "reye_pose", "left_hand_pose", "right_hand_pose")
ALL = ("joints", "full_pose", "shape")


@pytest.fixture(scope="module")
def golden():
    return GR.load_golden()


def _bounds(golden, q, name=None):
    out = [4 * float(golden[f"e_ref_{q}"])]
    if name not in S.ILL_CONDITIONED:
        out.append(4 * float(golden[f"e_reg_{q}"]))
    return out


def _leaves(body, theta, coefficients, transl):
    """DeviceSMPLX's keyword arguments as [1, n] device LEAVES: the pose arguments, transl, betas and expression."""
    leaf = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).reshape(1, -1).to(DEV).requires_grad_(True)
    sizes = (3, body.num_body, 3, 3, 3, body.hand_size, body.hand_size)
    kw, at = {}, 0
    for key, n in zip(POSE_KEYS, sizes):
        kw[key] = leaf(theta[at:at + n])
        at += n
    assert at == len(theta) == body.num_theta
    kw["transl"] = leaf(transl)
    coefficients = np.asarray(coefficients).reshape(-1)
    assert len(coefficients) == body.num_betas + body.num_expression_coeffs
    kw["betas"] = leaf(coefficients[:body.num_betas])
    kw["expression"] = leaf(coefficients[body.num_betas:]) if body.num_expression_coeffs else None
    return kw


def _loss(out, loss, g, gJ, gP):
    """The loss over the outputs named by `loss`; the others are not read, so their gradients reach the backward absent.  gJ may
    cover only the leading joints (the lbs cases have no extra joints: the device's landmarks then get no gradient)."""
    ug, ugJ, ugP = GR.upstream(loss, g, gJ, gP)
    d = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32)).to(DEV)
    total = 0.0
    if ug is not None:
        total = total + (out.vertices[0] * d(ug)).sum()
    if ugJ is not None:
        total = total + (out.joints[0][:len(ugJ)] * d(ugJ)).sum()
    if ugP is not None:
        total = total + (out.full_pose[0] * d(ugP)).sum()
    return total


def _grads(kw):
    n = lambda k: kw[k].grad.cpu().numpy().reshape(-1)
    return dict(grad_pose=np.concatenate([n(k) for k in POSE_KEYS]), grad_transl=n("transl"),
                grad_coef=np.concatenate([n("betas")] + ([n("expression")] if kw["expression"] is not None else [])))


def _run(body, kw, loss, g, gJ, gP):
    for v in kw.values():
        if v is not None:
            v.grad = None
    out = body(**kw, return_verts=True, return_full_pose=True)
    assert out.vertices.requires_grad and out.joints.requires_grad and out.full_pose.requires_grad
    _loss(out, loss, g, gJ, gP).backward()
    return _grads(kw)


def _check(golden, tag, got, want, name=None, tight=False):
    dev = {q: S.rel_dev(got[q], want[q]) for q in GR.QUANTITIES}
    for q in GR.QUANTITIES:
        print(f"{tag} {q}: device vs reference {dev[q]:.3e}   bounds {['%.3e' % b for b in _bounds(golden, q, name)]}")
    for q in GR.QUANTITIES:
        assert got[q].shape == np.asarray(want[q]).shape and np.all(np.isfinite(got[q])), q
        bounds = _bounds(golden, q, name)
        for b in ([min(bounds)] if tight else bounds):
            assert dev[q] <= b, (tag, q, dev[q], b)


@pytest.mark.parametrize("name", S.CASE_NAMES)
def test_golden_case_within_the_package_s_own_error(golden, name):
    from coma_amd.body_model import DeviceSMPLX
    model, fm = S.case_model(name)
    inp = S.case_inputs(name)
    gJ, gP = GR.case_upstream(name)
    body = DeviceSMPLX(model, n_pca=max(fm["n_pca"], 1), use_pca=bool(fm["n_pca"]), device=DEV, extra_joint_vertex_ids=[], differentiable=ALL)
    kw = _leaves(body, inp["theta"], inp["coefficients"], inp["transl"])
    for loss in GR.LOSSES:
        got = _run(body, kw, loss, inp["g"], gJ, gP)
        _check(golden, f"{name} {loss}", got, {q: golden[f"{name}__r64_{loss}_{q}"] for q in GR.QUANTITIES}, name)
    assert body.shape_stage_runs == 1                          # the same leaves at the same versions: one shape state for the four


@pytest.fixture(scope="module")
def real_size():
    """The V = 10 475 model the generator ran through the package's class, with the class's 21 vertex picks recovered from the
    forward fixture, its device object and the restatement's forward, computed once."""
    from coma_amd.body_model import DeviceSMPLX
    model, kw, g = S.class_case()
    fm = S.flat_model(model, n_pca=45)
    coef = np.concatenate([kw["betas"].reshape(-1), kw["expression"].reshape(-1)])
    fwd = S.forward(fm, coef, S.class_theta(kw), kw["transl"])
    ids = GR.class_vertex_ids(S.load_golden(), fm, fwd)
    body = DeviceSMPLX(model, n_pca=45, device=DEV, extra_joint_vertex_ids=ids, differentiable=ALL)
    return dict(model=model, kw=kw, g=g, fm=fm, fwd=fwd, coef=coef, ids=ids, body=body)


def test_class_case_every_argument_a_leaf(golden, real_size):
    r = real_size
    assert r["body"].num_extra == 21 + 51
    gJ, gP = GR.class_upstream()
    kw = _leaves(r["body"], S.class_theta(r["kw"]), r["coef"], r["kw"]["transl"])
    for loss in GR.LOSSES:
        got = _run(r["body"], kw, loss, r["g"], gJ, gP)
        _check(golden, f"class {loss}", got, {q: golden[f"class__r64_{loss}_{q}"] for q in GR.QUANTITIES})


def _collision_model():
    """`moderate` with vertex 7 picked twice and two landmark faces that contain it (one of them twice)."""
    model, _ = S.case_model("moderate")
    model = dict(model, f=model["f"].copy())
    a, b = model["lmk_faces_idx"][:2]
    assert a != b
    model["f"][a] = [7, 3, 7]
    model["f"][b][1] = 7
    return model, S.flat_model(model, n_pca=45)


def test_scatter_collisions_against_the_restatement_and_bit_identical(golden):
    from coma_amd.body_model import DeviceSMPLX
    model, fm = _collision_model()
    inp = S.case_inputs("moderate")
    body = DeviceSMPLX(model, n_pca=45, device=DEV, extra_joint_vertex_ids=[7, 7], differentiable=ALL)
    idx, w = S.extra_joint_table(fm, [7, 7])
    assert np.array_equal(body.host["extra_index"], idx) and (idx == 7).sum() == 6 + 2 + 1
    rng = np.random.RandomState(21)
    gJ, gP = rng.normal(size=(fm["J"] + len(idx), 3)).astype(np.float32), rng.normal(size=3 * fm["J"]).astype(np.float32)
    fwd = S.forward(fm, inp["coefficients"], inp["theta"], inp["transl"])
    kw = _leaves(body, inp["theta"], inp["coefficients"], inp["transl"])
    for loss in ("joints", "all"):
        want = dict(zip(GR.QUANTITIES, GR.backward_full(fm, fwd, *GR.upstream(loss, inp["g"], gJ, gP), idx=idx, w=w)))
        got = _run(body, kw, loss, inp["g"], gJ, gP)
        _check(golden, f"collisions {loss}", got, want, tight=True)
        again = _run(body, kw, loss, inp["g"], gJ, gP)
        for q in GR.QUANTITIES:
            assert np.array_equal(got[q], again[q]), (loss, q)


@pytest.mark.parametrize("NB", [1, 300])
def test_reduction_shape_of_the_coefficient_gradient(golden, NB):
    """V = 63 (189 rows: one workgroup, not full) with one coefficient and with 300 (more coefficients than threads in a workgroup)."""
    from coma_amd.body_model import DeviceSMPLX
    model = S.synthetic_model(63, 5, 1 if NB == 1 else 400, 6, "random", seed=77)
    split = dict(num_betas=10, num_expression_coeffs=10) if NB == 1 else dict(num_betas=290, num_expression_coeffs=10)
    fm = S.flat_model(model, n_pca=6, **split)
    body = DeviceSMPLX(model, n_pca=6, device=DEV, extra_joint_vertex_ids=[], differentiable=ALL, **split)
    assert body.num_betas + body.num_expression_coeffs == NB == fm["shapedirs"].shape[-1]
    rng = np.random.RandomState(78)
    coef, theta, transl = rng.normal(size=NB).astype(np.float32), (rng.normal(size=S.n_theta(fm)) * 0.3).astype(np.float32), rng.normal(size=3).astype(np.float32)
    idx, w = S.extra_joint_table(fm)
    g, gJ, gP = (rng.normal(size=s).astype(np.float32) for s in ((63, 3), (5 + len(idx), 3), 15))
    fwd = S.forward(fm, coef, theta, transl)
    want = dict(zip(GR.QUANTITIES, GR.backward_full(fm, fwd, g, gJ, gP, idx=idx, w=w)))
    got = _run(body, _leaves(body, theta, coef, transl), "all", g, gJ, gP)
    _check(golden, f"NB={NB}", got, want, tight=True)


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).to(DEV)


def test_smallest_accepted_size_through_the_c_abi(golden, hip_lib):
    """V = 1, J = 1, NB = 1, E = 0, hand_dim = 0, n_pca = 0: no pose features (P = 0) and a chain that is its root.  The regressor's
    one entry is not 1, so the joint is not the vertex and the rotation's gradient is not identically zero."""
    from coma_amd import _lib
    rng = np.random.RandomState(31)
    f32 = lambda *s: rng.normal(size=s).astype(np.float32)
    fm = dict(V=1, J=1, hd=0, n_pca=0, v_template=f32(1, 3).astype(np.float64), shapedirs=f32(1, 3, 1).astype(np.float64), posedirs=np.zeros((0, 3)),
              J_regressor=np.full((1, 1), 0.625), parents=np.array([-1]), weights=np.ones((1, 1)), comps=None, mean=np.zeros(3))
    coef, theta, transl, g, gJ, gP = f32(1), f32(3), f32(3), f32(1, 3), f32(1, 3), f32(3)
    fwd = S.forward(fm, coef, theta, transl)
    want = dict(zip(GR.QUANTITIES, GR.backward_full(fm, fwd, g, gJ, gP)))
    L = hip_lib
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    buf = lambda n: torch.zeros([int(n)], dtype=torch.uint8, device=DEV)
    shape_b, saved_b, ws_b, gws_b = L.coma_smplx_shape_state_bytes(1, 1), L.coma_smplx_saved_bytes(1, 1), L.coma_smplx_workspace_bytes(1, 1), L.coma_smplx_grad_workspace_bytes(1, 1, 1)
    shape, saved, ws, gws = buf(shape_b), buf(saved_b), buf(ws_b), buf(gws_b)
    d = {k: _dev(v) for k, v in dict(vt=fm["v_template"], sd=fm["shapedirs"], jr=fm["J_regressor"], w=fm["weights"], coef=coef, theta=theta,
                                     transl=transl, g=g, gJ=gJ, gP=gP, pd=np.zeros(4)).items()}
    parents = (C.c_int32 * 1)(-1)
    verts, joints, g_theta, g_transl, g_coef = (torch.zeros(n, device=DEV) for n in (3, 3, 3, 3, 1))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(L.coma_smplx_shape_f32(p(d["vt"]), p(d["sd"]), p(d["coef"]), p(d["jr"]), 1, 1, 1, p(shape), shape_b, stream), "shape")
    _lib.check(L.coma_smplx_forward_f32(p(d["theta"]), p(d["transl"]), p(d["pd"]), p(d["w"]), parents, None, None, 1, 1, 0, 0, p(shape), p(verts),
                                        p(joints), None, p(saved), saved_b, p(ws), ws_b, stream), "forward")
    _lib.check(L.coma_smplx_backward_full_f32(p(d["g"]), p(d["gJ"]), p(d["gP"]), p(d["pd"]), p(d["w"]), parents, None, None, None, 0, p(d["sd"]),
                                              p(d["jr"]), 1, 1, 1, 0, 0, p(shape), p(saved), saved_b, p(g_theta), p(g_transl), p(g_coef), p(gws), gws_b,
                                              stream), "backward_full")
    assert S.rel_dev(verts.cpu().numpy(), fwd["vertices"].reshape(-1)) <= 2.0 ** -22
    got = dict(grad_pose=g_theta.cpu().numpy(), grad_transl=g_transl.cpu().numpy(), grad_coef=g_coef.cpu().numpy())
    _check(golden, "V=J=NB=1", got, want, tight=True)


def _forward_and_saved(body, name_or_inputs):
    theta, coef, transl = name_or_inputs
    kw = _leaves(body, theta, coef, transl)
    with torch.no_grad():
        body._shape_stage(kw["betas"], kw["expression"])
        th = torch.cat([kw[k].reshape(-1) for k in POSE_KEYS]).contiguous()
        _, _, _, saved = body._forward(th, kw["transl"].reshape(-1).contiguous())
    return saved


@pytest.mark.parametrize("which", ["moderate", "class"])
def test_without_the_new_inputs_the_bits_are_the_old_backward_s(real_size, which):
    from coma_amd.body_model import DeviceSMPLX
    if which == "class":
        body, r = real_size["body"], real_size
        inputs, g = (S.class_theta(r["kw"]), r["coef"], r["kw"]["transl"]), r["g"]
    else:
        model, _ = S.case_model(which)
        inp = S.case_inputs(which)
        body = DeviceSMPLX(model, n_pca=45, device=DEV, extra_joint_vertex_ids=[], differentiable=ALL)
        inputs, g = (inp["theta"], inp["coefficients"], inp["transl"]), inp["g"]
    saved = _forward_and_saved(body, inputs)
    gd = _dev(g)
    old = body._backward(gd, saved)
    new = body._backward_full(gd, None, None, saved, body._shape_state, False)
    assert new[2] is None and old[0].abs().max() > 0
    assert torch.equal(old[0], new[0]) and torch.equal(old[1], new[1])


def test_refusals_leave_the_outputs_untouched(hip_lib):
    from coma_amd.body_model import DeviceSMPLX
    model, _ = S.case_model("moderate")
    inp = S.case_inputs("moderate")
    body = DeviceSMPLX(model, n_pca=45, device=DEV, extra_joint_vertex_ids=[], differentiable=ALL)
    saved = _forward_and_saved(body, (inp["theta"], inp["coefficients"], inp["transl"]))
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    g, gJ = _dev(inp["g"]), torch.ones([body.J + body.num_extra, 3], device=DEV)
    outs = [torch.full([n], 7.5, device=DEV) for n in (body.num_theta, 3, 20)]
    big_ws = torch.zeros([body._grad_ws_bytes + 16], dtype=torch.uint8, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(E=body.num_extra, NB=20, sd=body._shapedirs, ws=p(big_ws), ws_bytes=body._grad_ws_bytes):
        return hip_lib.coma_smplx_backward_full_f32(p(g), p(gJ), None, p(body._posedirs), p(body._weights), body._parents, p(body._comps),
                                                    p(body._extra_index), p(body._extra_weight), E, p(sd), p(body._J_regressor), NB, body.V, body.J,
                                                    body.hand_dim, body.num_pca_comps, p(body._shape_state), p(saved), body._saved_bytes, p(outs[0]),
                                                    p(outs[1]), p(outs[2]), ws, ws_bytes, stream)
    for kw, text in ((dict(E=4097), b"E=4097"), (dict(E=-1), b"E=-1"), (dict(NB=0), b"NB=0"), (dict(ws_bytes=body._grad_ws_bytes - 16), b"workspace"),
                     (dict(ws=C.c_void_p(big_ws.data_ptr() + 8)), b"aligned"), (dict(sd=None), b"shapedirs")):
        assert call(**kw) == -1 and text in hip_lib.coma_last_error(), kw
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == 7.5).all())
    assert call() == 0                                          # the same call with nothing wrong goes through
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t != 7.5).all()) and bool(torch.isfinite(t).all())


def test_every_forward_differentiates_its_own_shape_state(golden):
    """forward(betas A), forward(betas B), then both backwards: each gradient is the one at its own coefficients."""
    from coma_amd.body_model import DeviceSMPLX
    model, fm = S.case_model("moderate")
    inp = S.case_inputs("moderate")
    gJ, gP = GR.case_upstream("moderate")
    body = DeviceSMPLX(model, n_pca=45, device=DEV, extra_joint_vertex_ids=[], differentiable=ALL)
    coefs = (inp["coefficients"], (inp["coefficients"] * -0.7 + 0.3).astype(np.float32))
    kws = [_leaves(body, inp["theta"], c, inp["transl"]) for c in coefs]
    losses = [_loss(body(**kw, return_verts=True, return_full_pose=True), "all", inp["g"], gJ, gP) for kw in kws]
    assert body.shape_stage_runs == 2
    losses[0].backward()
    losses[1].backward()
    wants = []
    for c, kw in zip(coefs, kws):
        fwd = S.forward(fm, c, inp["theta"], inp["transl"])
        wants.append(dict(zip(GR.QUANTITIES, GR.backward_full(fm, fwd, inp["g"], gJ, gP))))
        _check(golden, "own shape state", _grads(kw), wants[-1], tight=True)
    assert S.rel_dev(wants[0]["grad_pose"], wants[1]["grad_pose"]) > 1e-3          # a stale state would have been seen


def test_joints_only_model_keeps_the_shape_state_of_its_forward(golden):
    """differentiable without "shape": the coefficients take the host path, and a backward after they changed is still its forward's."""
    from coma_amd._lib import ComaHipError
    from coma_amd.body_model import DeviceSMPLX
    model, fm = S.case_model("moderate")
    inp = S.case_inputs("moderate")
    gJ, _ = GR.case_upstream("moderate")
    body = DeviceSMPLX(model, n_pca=45, device=DEV, extra_joint_vertex_ids=[], differentiable=("joints",))
    kw = _leaves(body, inp["theta"], inp["coefficients"], inp["transl"])
    kw["betas"], kw["expression"] = kw["betas"].detach(), kw["expression"].detach()
    out = body(**kw, return_verts=True, return_full_pose=True)
    assert out.joints.requires_grad and not out.full_pose.requires_grad
    other = dict(kw, betas=kw["betas"] * -0.7 + 0.3)
    with torch.no_grad():
        body(**other)
    assert body.shape_stage_runs == 2
    _loss(out, "joints", None, gJ, None).backward()
    fwd = S.forward(fm, inp["coefficients"], inp["theta"], inp["transl"])
    want = GR.backward_full(fm, fwd, None, gJ, None)
    got_pose = np.concatenate([kw[k].grad.cpu().numpy().reshape(-1) for k in POSE_KEYS])
    dev = S.rel_dev(got_pose, want[0])
    print(f"joints-only grad_pose: {dev:.3e}")
    assert dev <= min(_bounds(golden, "grad_pose"))
    with pytest.raises(ComaHipError, match="betas requires grad"):
        body(**dict(kw, betas=kw["betas"].clone().requires_grad_(True)))


def test_device_resident_coefficients_are_not_read_back(golden, monkeypatch):
    """Three iterations of an in-place update of betas (a device leaf): the shape stage runs three times, nothing is copied to the
    host, and the third gradient is the one at the third betas.  As test_same_betas_tensor_is_not_read_again_until_it_changes counts
    shape_stage_runs; on top of it every tensor-to-host route raises while the iterations run."""
    from coma_amd.body_model import DeviceSMPLX
    model, fm = S.case_model("moderate")
    inp = S.case_inputs("moderate")
    gJ, gP = GR.case_upstream("moderate")
    body = DeviceSMPLX(model, n_pca=45, device=DEV, extra_joint_vertex_ids=[], differentiable=ALL)
    kw = _leaves(body, inp["theta"], inp["coefficients"], inp["transl"])
    d = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32)).to(DEV)
    g_d, gJ_d, gP_d = d(inp["g"]), d(gJ), d(gP)
    with torch.no_grad():
        body(**kw)                                             # uploads the model
    assert body.shape_stage_runs == 1
    with torch.no_grad():
        for _ in range(2):
            body(**kw)
    assert body.shape_stage_runs == 1                          # the same-tensor, same-version shortcut stays

    def refuse(*a, **k):
        raise AssertionError("a tensor was copied to the host")
    step = 1e-3
    with monkeypatch.context() as m:
        for route in ("cpu", "numpy", "tolist", "item", "__array__"):
            m.setattr(torch.Tensor, route, refuse)
        for it in range(3):
            with torch.no_grad():                              # in place: the same leaf, a new version
                if kw["betas"].grad is None:
                    kw["betas"] += 0.01
                else:
                    kw["betas"] -= step * kw["betas"].grad
            for v in kw.values():
                v.grad = None
            out = body(**kw, return_verts=True, return_full_pose=True)
            ((out.vertices[0] * g_d).sum() + (out.joints[0][:fm["J"]] * gJ_d).sum() + (out.full_pose[0] * gP_d).sum()).backward()
            assert body.shape_stage_runs == 2 + it             # one more per update
    assert body.shape_stage_runs == 4
    coef = np.concatenate([kw["betas"].detach().cpu().numpy().reshape(-1), kw["expression"].detach().cpu().numpy().reshape(-1)])
    assert not np.array_equal(coef, inp["coefficients"])
    fwd = S.forward(fm, coef, inp["theta"], inp["transl"])
    want = dict(zip(GR.QUANTITIES, GR.backward_full(fm, fwd, inp["g"], gJ, gP)))
    _check(golden, "third iteration", _grads(kw), want, tight=True)
