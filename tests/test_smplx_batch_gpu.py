"""GPU: the batched SMPL-X body model (coma_smplx_*_batch_f32, DeviceSMPLX(batch_size=N)).

1. Golden: the device at batch_size = 3 against the third-party package at batch_size = 3 in f64 (R64 of
   tests/golden/smplx_batch_golden.npz), within 4 x the stored e_ref of each quantity -- the package's own f32 error, the bound of
   tests/test_smplx_gpu.py.  full_pose has no e_ref: it is the f32 rounding of a handful of f64 products, 2^-23 relative.
2. Bit-identity: body n of a batched C call equals the single-body C call on the same inputs in every output and gradient, for both
   backward forms, at the sizes where a batch can go wrong: V = 300 (tiles 128, 128, 44; 3V no multiple of 256) and 129, J = 5 and 55,
   n_pca = 0 and 6, N = 1, 2, C, C + 1, 2C + 3 (C = 8 bodies per sweep; the skinning kernels walk 2), one shape state and one per
   body, transl given and NULL; once at V = 10 475.
3. Two calls give the same bits, and the guards around every output, `saved` and the workspaces stay intact (all batched calls here
   write into guarded buffers).
4. Every refusal leaves the outputs untouched.
5. The Python object: broadcasting, the gradient of a broadcast argument, bit-identity with three single-body objects, a second
   forward before the first backward."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import domain_kit as K
from tests import smplx_batch_ref as B
from tests import smplx_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CH = B.C_CHUNK
F32, U8 = torch.float32, torch.uint8


def _p(t, offset=0):
    return None if t is None else C.c_void_p(t.data_ptr() + offset)


class Guarded:
    """A device buffer between two guards (tests/domain_kit.guarded); `ptr` is the address of the body."""

    def __init__(self, n, dtype):
        self.n, self.dtype = n, dtype
        self.flat = K.guarded(torch.zeros(n, dtype=dtype)).to(DEV)
        self.ptr = C.c_void_p(self.flat.data_ptr() + K.GUARD * self.flat.element_size())

    def body(self):
        return self.flat[K.GUARD:K.GUARD + self.n]

    def intact(self):
        return K.guards_intact(self.flat.cpu())


class Rig:
    """A seeded model on the device (uploaded by a DeviceSMPLX object) and the raw C calls on it, single-body and batched."""

    def __init__(self, model, n_pca, extra_ids=(0, 7)):
        from coma_amd import _lib
        from coma_amd.body_model import DeviceSMPLX
        self.body = b = DeviceSMPLX(model, n_pca=max(n_pca, 1), use_pca=bool(n_pca), device=DEV, extra_joint_vertex_ids=list(extra_ids))
        b._upload()
        self.L = L = _lib.lib()
        self.V, self.J, self.NT, self.E, self.NB = b.V, b.J, b.num_theta, b.num_extra, b.num_betas + b.num_expression_coeffs
        self.stride = (b._shape_bytes + 15) // 16 * 16
        self.model = (_p(b._posedirs), _p(b._weights), b._parents, _p(b._comps))
        self.gws_bytes = L.coma_smplx_grad_workspace_bytes(self.V, self.J, 0)
        self.ws, self.gws = torch.empty(b._ws_bytes, dtype=U8, device=DEV), torch.empty(self.gws_bytes, dtype=U8, device=DEV)

    def inputs(self, N, seed, per_body_shape, with_transl):
        """Seeded inputs on the device; body 0 at zero pose.  The shape states are written here by coma_smplx_shape_f32."""
        rng = np.random.RandomState(seed)
        t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32)).to(DEV)
        theta = rng.normal(size=(N, self.NT)) * 0.3
        theta[0] = 0
        coef = t(rng.normal(size=(N if per_body_shape else 1, self.NB)))
        b = self.body
        states = torch.empty(coef.shape[0] * self.stride, dtype=U8, device=DEV)
        for n in range(coef.shape[0]):
            rc = self.L.coma_smplx_shape_f32(_p(b._v_template), _p(b._shapedirs), _p(coef, 4 * n * self.NB), _p(b._J_regressor), self.V, self.J, self.NB,
                                             _p(states, n * self.stride), b._shape_bytes, None)
            assert rc == 0, self.L.coma_last_error()
        return dict(N=N, theta=t(theta), transl=t(rng.uniform(-1, 1, (N, 3))) if with_transl else None, states=states,
                    stride=self.stride if per_body_shape else 0, g=t(rng.normal(size=(N, self.V, 3))), gJ=t(rng.normal(size=(N, self.J + self.E, 3))),
                    gP=t(rng.normal(size=(N, 3 * self.J))))

    def single(self, i, n):
        """Body n through the single-body calls: forward, extra joints, the vertices-only backward, the full backward."""
        b, L, V, J, E = self.body, self.L, self.V, self.J, self.E
        posedirs, weights, parents, comps = self.model
        z = lambda *shape: torch.empty(shape, dtype=F32, device=DEV)
        o = dict(vertices=z(V, 3), joints=z(J, 3), full_pose=z(3 * J), extra=z(E, 3), gt_v=z(self.NT), gtr_v=z(3), gt_f=z(self.NT), gtr_f=z(3))
        saved = torch.zeros(b._saved_bytes, dtype=U8, device=DEV)          # zeros, as the guarded buffers: the layout has alignment gaps
        theta, transl, state = _p(i["theta"], 4 * n * self.NT), _p(i["transl"], 12 * n), _p(i["states"], n * i["stride"])
        rcs = [L.coma_smplx_forward_f32(theta, transl, posedirs, weights, parents, comps, _p(b._mean), V, J, b.hand_dim, b.num_pca_comps, state,
                                        _p(o["vertices"]), _p(o["joints"]), _p(o["full_pose"]), _p(saved), b._saved_bytes, _p(self.ws), b._ws_bytes, None),
               L.coma_smplx_extra_joints_f32(_p(o["vertices"]), transl, _p(b._extra_index), _p(b._extra_weight), V, E, _p(o["extra"]), None),
               L.coma_smplx_backward_f32(_p(i["g"], 12 * n * V), posedirs, weights, parents, comps, V, J, b.hand_dim, b.num_pca_comps, state, _p(saved),
                                         b._saved_bytes, _p(o["gt_v"]), _p(o["gtr_v"]), _p(self.ws), b._ws_bytes, None),
               L.coma_smplx_backward_full_f32(_p(i["g"], 12 * n * V), _p(i["gJ"], 12 * n * (J + E)), _p(i["gP"], 12 * n * J), posedirs, weights, parents,
                                              comps, _p(b._extra_index), _p(b._extra_weight), E, None, None, 0, V, J, b.hand_dim, b.num_pca_comps, state,
                                              _p(saved), b._saved_bytes, _p(o["gt_f"]), _p(o["gtr_f"]), None, _p(self.gws), self.gws_bytes, None)]
        assert rcs == [0, 0, 0, 0], (rcs, L.coma_last_error())
        o["saved"] = saved
        return o

    def batch_outputs(self, N):
        L, V, J = self.L, self.V, self.J
        f = lambda *shape: Guarded(int(np.prod(shape)), F32)
        return dict(vertices=f(N, V, 3), joints=f(N, J, 3), full_pose=f(N, 3 * J), extra=f(N, self.E, 3), gt_v=f(N, self.NT), gtr_v=f(N, 3),
                    gt_f=f(N, self.NT), gtr_f=f(N, 3), saved=Guarded(L.coma_smplx_batch_saved_bytes(V, J, N), U8),
                    ws=Guarded(L.coma_smplx_batch_workspace_bytes(V, J, N), U8), gws=Guarded(L.coma_smplx_batch_grad_workspace_bytes(V, J, N), U8))

    def batch(self, i, o, full=True):
        """All N bodies through the batched calls, into the guarded buffers `o`."""
        b, L, V, J, E, N = self.body, self.L, self.V, self.J, self.E, i["N"]
        posedirs, weights, parents, comps = self.model
        sv, ws, gws = o["saved"], o["ws"], o["gws"]
        rcs = [L.coma_smplx_forward_batch_f32(_p(i["theta"]), _p(i["transl"]), posedirs, weights, parents, comps, _p(b._mean), V, J, b.hand_dim,
                                              b.num_pca_comps, N, _p(i["states"]), i["stride"], o["vertices"].ptr, o["joints"].ptr, o["full_pose"].ptr,
                                              sv.ptr, sv.n, ws.ptr, ws.n, None),
               L.coma_smplx_extra_joints_batch_f32(o["vertices"].ptr, _p(i["transl"]), _p(b._extra_index), _p(b._extra_weight), V, E, N, o["extra"].ptr, None),
               L.coma_smplx_backward_batch_f32(_p(i["g"]), None, None, posedirs, weights, parents, comps, _p(b._extra_index), _p(b._extra_weight), E, V, J,
                                               b.hand_dim, b.num_pca_comps, N, _p(i["states"]), i["stride"], sv.ptr, sv.n, o["gt_v"].ptr, o["gtr_v"].ptr,
                                               gws.ptr, gws.n, None)]
        if full:
            rcs.append(L.coma_smplx_backward_batch_f32(_p(i["g"]), _p(i["gJ"]), _p(i["gP"]), posedirs, weights, parents, comps, _p(b._extra_index),
                                                       _p(b._extra_weight), E, V, J, b.hand_dim, b.num_pca_comps, N, _p(i["states"]), i["stride"], sv.ptr,
                                                       sv.n, o["gt_f"].ptr, o["gtr_f"].ptr, gws.ptr, gws.n, None))
        assert not any(rcs), (rcs, L.coma_last_error())


QUANTS = ("vertices", "joints", "full_pose", "extra", "gt_v", "gtr_v", "gt_f", "gtr_f", "saved")
_rigs = {}


def _rig(V, J, n_pca):
    key = (V, J, n_pca)
    if key not in _rigs:
        model = B.model_of("class")[0] if V == S.CLASS_V else S.synthetic_model(V, J, 20, max(n_pca, 1), "random", seed=5000 + V + J + n_pca)
        _rigs[key] = Rig(model, n_pca)
    return _rigs[key]


def _compare(rig, i, o, quants):
    """Body n of the batched buffers against the single-body calls, bit for bit; every guard intact."""
    singles = []
    with K.device_guard("single-body calls"):
        for n in range(i["N"]):
            singles.append(rig.single(i, n))
    for q in quants:
        got = o[q].body().reshape(i["N"], -1).cpu()
        for n, s in enumerate(singles):
            assert torch.equal(K.bits(got[n]), K.bits(s[q].reshape(-1).cpu())), (q, n)
    for name, buf in o.items():
        assert buf.intact(), f"guard of `{name}` written"


#                                   V    J   n_pca N            per-body shape  transl
@pytest.mark.parametrize("case", [(300, 55, 6, 2 * CH + 3, True, True),
                                  (300, 55, 0, CH + 1, False, False),
                                  (129, 5, 6, CH, True, False),
                                  (129, 5, 0, 2, False, True),
                                  (129, 55, 6, 1, True, True),
                                  (300, 5, 0, CH + 1, True, True),
                                  (300, 55, 6, CH, False, True),
                                  (129, 55, 0, 2 * CH + 3, True, False)], ids=lambda c: "V{}-J{}-pca{}-N{}-{}-{}".format(*c[:4], "strided" if c[4] else "shared", "transl" if c[5] else "notransl"))
def test_body_n_of_a_batched_call_has_the_bits_of_the_single_body_call(case):
    V, J, n_pca, N, per_body, with_transl = case
    rig = _rig(V, J, n_pca)
    assert rig.E == 2 + 5 and rig.body.hand_dim == (0 if J == 5 else 45)
    i = rig.inputs(N, K.seed(str(case)) % 2 ** 31, per_body, with_transl)
    o = rig.batch_outputs(N)
    with K.device_guard("batched calls"):
        rig.batch(i, o)
    _compare(rig, i, o, QUANTS)
    assert bool(torch.isfinite(o["gt_f"].body()).all()) and bool(o["gt_v"].body().reshape(N, -1)[min(1, N - 1)].any())


def test_real_size_batch_has_the_bits_of_the_single_body_calls():
    """V = 10 475, J = 55, n_pca = 45, N = C + 1: the vertices-only form."""
    rig = _rig(S.CLASS_V, 55, 45)
    N = CH + 1
    i = rig.inputs(N, 77, True, True)
    o = rig.batch_outputs(N)
    with K.device_guard("batched calls at the real size"):
        rig.batch(i, o, full=False)
    _compare(rig, i, o, ("vertices", "joints", "full_pose", "extra", "gt_v", "gtr_v", "saved"))


def test_two_batched_calls_give_the_same_bits_and_stay_inside_their_buffers():
    rig = _rig(300, 55, 6)
    N = CH + 1
    i = rig.inputs(N, 78, True, True)
    first, second = K.launch_twice(lambda: rig.batch_outputs(N), lambda o: rig.batch(i, o), "two batched calls")
    for q in QUANTS:
        assert torch.equal(K.bits(first[q].body().cpu()), K.bits(second[q].body().cpu())), q
        assert bool(first[q].body().cpu().ne(0).any()), q                                 # ... and were written at all
    for o in (first, second):
        for name, buf in o.items():
            assert buf.intact(), f"guard of `{name}` written"
    last = first["vertices"].body().reshape(N, -1)[N - 1]
    assert bool(torch.isfinite(last).all()) and bool(last.ne(0).any())


def test_refusals_leave_the_outputs_untouched():
    from coma_amd import _lib
    L = _lib.lib()
    _, fm = B.model_of("lbs")
    parents = (C.c_int32 * 55)(*[max(int(p), 0) for p in fm["parents"]])
    bad = (C.c_int32 * 55)(*parents)
    bad[7] = 9
    resolve, outs, small = K.device_resolver(B.OUTPUT_ARGS, device=DEV)
    table = B.refusal_table(L, parents, bad)
    with K.device_guard("refusals"):
        n = K.check_refusals(L, table, resolve, expect_control=False)
    assert n >= 60
    K.refusal_outputs_untouched(outs, small)


# ---- 1. golden ----
@pytest.fixture(scope="module")
def golden():
    return B.load_golden()


def _kwargs(fm, inp, leaves=True):
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)
    kw = {k: t(v).requires_grad_(leaves) for k, v in B.split_theta(fm, inp["theta"]).items()}
    kw["transl"] = t(inp["transl"]).requires_grad_(leaves)
    kw["betas"], kw["expression"] = t(inp["coefficients"][:, :10]), t(inp["coefficients"][:, 10:])
    return kw


@pytest.mark.parametrize("case", B.CASES)
def test_golden_batch_within_the_package_s_own_error(golden, case):
    from coma_amd.body_model import DeviceSMPLX
    kind = case.split("_", 1)[0]
    model, fm = B.model_of(kind)
    body = DeviceSMPLX(model, n_pca=fm["n_pca"], device=DEV, extra_joint_vertex_ids=[], batch_size=B.N)
    inp = B.case_inputs(case)
    kw = _kwargs(fm, inp)
    out = body(**kw, return_full_pose=True)
    assert out.vertices.shape == (B.N, fm["V"], 3) and out.joints.shape == (B.N, fm["J"] + body.num_extra, 3) and out.full_pose.shape == (B.N, 3 * fm["J"])
    (out.vertices * torch.as_tensor(inp["g"]).to(DEV)).sum().backward()
    verts, joints = out.vertices.detach().cpu().numpy(), out.joints.cpu().numpy()
    got = dict(vertices=verts[:, B.class_subset()] if kind == "class" else verts, joints=joints if kind == "class" else joints[:, :fm["J"]],
               grad_pose=np.concatenate([kw[k].grad.cpu().numpy() for k in B.POSE_KEYS], 1), grad_transl=kw["transl"].grad.cpu().numpy())
    want = {q: golden[f"{case}__r64_{q}"] for q in B.QUANTITIES}
    want["joints"] = B.golden_joints(golden, case)
    dev = {q: S.rel_dev(got[q], want[q]) for q in B.QUANTITIES}
    pose_dev = S.rel_dev(out.full_pose.cpu().numpy(), golden[f"{case}__r64_full_pose"])
    for q in B.QUANTITIES:
        print(f"{case} {q}: device vs R64 {dev[q]:.3e}   bound {4 * float(golden[f'e_ref_{q}']):.3e}")
    print(f"{case} full_pose: {pose_dev:.3e}")
    for q in B.QUANTITIES:
        assert got[q].shape == want[q].shape and np.all(np.isfinite(got[q])), q
        assert dev[q] <= 4 * float(golden[f"e_ref_{q}"]), (q, dev[q])
    assert pose_dev <= 2.0 ** -23
    assert body.shape_stage_runs == (B.N if case.endswith("per_body") else 1)


# ---- 5. the Python object ----
def _grads(kw):
    return {k: v.grad.clone() for k, v in kw.items() if v is not None and v.requires_grad}


def test_batch_object_broadcasts_and_sums_the_gradient_of_a_broadcast_argument():
    from coma_amd.body_model import DeviceSMPLX
    model, fm = B.model_of("lbs")
    inp = B.case_inputs("lbs_shared")
    g = torch.as_tensor(inp["g"]).to(DEV)
    body = DeviceSMPLX(model, n_pca=6, device=DEV, extra_joint_vertex_ids=[3, 200], batch_size=3)
    full = _kwargs(fm, inp)
    full["transl"] = full["transl"].detach()[1:2].expand(3, 3).contiguous().requires_grad_(True)
    full["global_orient"] = full["global_orient"].detach()[2:3].expand(3, 3).contiguous().requires_grad_(True)
    one = {k: v.detach().clone().requires_grad_(v.requires_grad) for k, v in full.items()}
    one["transl"] = full["transl"].detach()[:1].clone().requires_grad_(True)                    # [1, 3] and [1, 3]: broadcast
    one["global_orient"] = full["global_orient"].detach()[:1].clone().requires_grad_(True)
    one["jaw_pose"] = None                                                                      # None is zeros for every body
    full["jaw_pose"] = torch.zeros(3, 3, device=DEV, requires_grad=True)
    outs = []
    for kw in (full, one):
        out = body(**kw)
        (out.vertices * g).sum().backward()
        outs.append(out)
    assert outs[1].vertices.shape == (3, fm["V"], 3) and outs[1].full_pose is None and not outs[1].joints.requires_grad
    assert torch.equal(outs[0].vertices, outs[1].vertices) and torch.equal(outs[0].joints, outs[1].joints)
    gf, go = _grads(full), _grads(one)
    assert go["transl"].shape == (1, 3) and go["global_orient"].shape == (1, 3) and go["body_pose"].shape == (3, 63)
    assert torch.equal(go["transl"], gf["transl"].sum(0, keepdim=True)) and torch.equal(go["global_orient"], gf["global_orient"].sum(0, keepdim=True))
    assert torch.equal(go["body_pose"], gf["body_pose"]) and bool(gf["transl"].ne(0).all())
    assert body.shape_stage_runs == 1                                                           # the same coefficients, other tensors


def test_batch_object_has_the_bits_of_three_single_body_objects_and_forwards_do_not_disturb_each_other():
    from coma_amd.body_model import DeviceSMPLX
    model, fm = B.model_of("lbs")
    inp = B.case_inputs("lbs_per_body")
    ids = [3, 200, 299]
    batch = DeviceSMPLX(model, n_pca=6, device=DEV, extra_joint_vertex_ids=ids, batch_size=3, differentiable=("joints",))
    g = torch.as_tensor(inp["g"]).to(DEV)
    gj = torch.as_tensor(np.random.RandomState(9).normal(size=(3, 55 + batch.num_extra, 3)).astype(np.float32)).to(DEV)
    kw = _kwargs(fm, inp)
    out = batch(**kw, return_full_pose=True)
    keep = [out.vertices.detach().clone(), out.joints.detach().clone(), out.full_pose.clone()]
    other = _kwargs(fm, dict(inp, theta=inp["theta"] * 0.5 + 0.01, transl=-inp["transl"]), leaves=False)
    out_other = batch(**other)                                                                   # a second forward before the first backward
    assert out.joints.requires_grad and not out.full_pose.requires_grad and not torch.equal(out_other.vertices, keep[0])
    ((out.vertices * g).sum() + (out.joints * gj).sum()).backward()
    for a, b in zip((out.vertices, out.joints, out.full_pose), keep):
        assert torch.equal(a.detach(), b)
    got = _grads(kw)
    assert batch.shape_stage_runs == 3
    for n in range(3):
        single = DeviceSMPLX(model, n_pca=6, device=DEV, extra_joint_vertex_ids=ids, differentiable=("joints",))
        kn = {k: v.detach()[n:n + 1].clone().requires_grad_(v.requires_grad) for k, v in kw.items()}
        o = single(**kn, return_full_pose=True)
        ((o.vertices * g[n:n + 1]).sum() + (o.joints * gj[n:n + 1]).sum()).backward()
        for q in ("vertices", "joints", "full_pose"):
            assert torch.equal(getattr(o, q).detach(), getattr(out, q).detach()[n:n + 1]), (q, n)
        for k, v in _grads(kn).items():
            assert torch.equal(K.bits(v), K.bits(got[k][n:n + 1])), (k, n)
    # one row of the coefficients changes: only that body's shape stage runs again (an object without `differentiable`)
    plain = DeviceSMPLX(model, n_pca=6, device=DEV, extra_joint_vertex_ids=ids, batch_size=3)
    with torch.no_grad():
        first = plain(**other).vertices
        betas = other["betas"].clone()
        betas[1, 3] += 0.5
        moved = plain(**dict(other, betas=betas)).vertices
    assert plain.shape_stage_runs == 4 and torch.equal(moved[0], first[0]) and torch.equal(moved[2], first[2]) and not torch.equal(moved[1], first[1])
    assert torch.equal(first, out_other.vertices)
