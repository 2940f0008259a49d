"""GPU: the ComA objective for N bodies in one call (coma_app_objective_batch_f32, coma_amd.app.ComaObjective on [N,V,3]).

The contract is bit-identity: body n of a batched call has the bits of the single-body call on body n's vertices (terms, both
gradients, NaN for NaN), whatever column split the batch chooses.  Bodies: one case's vertices under N distinct rigid motions plus
seeded noise (tests/app_batch_ref.batch_vertices), so every body gives other numbers.  Cases: golden `small_k20` (V = 145, one
workgroup per stage) at N = 3, and a fresh k = 333 on a 40 x 40 grid (V = 1601: 7 vertex workgroups, 6 row tiles with a ragged last one
of 13, two workgroups of the contact stages) at N = 9, more than a chunk of 8 -- and at N = 40, where the column split differs from
the single call's: the library aims at 1024 workgroups per launch of the double minimum, so one body's 6 column tiles are 6 splits of
one tile (1024 / 6 > 6), 9 bodies' still are (1024 / 54 = 18 > 6), and 40 bodies' are 3 splits of two tiles (1024 / 240 = 4).  The
merge takes (min, first argmin) in ascending split order on exact comparisons, so the bits must not depend on that.
Against f64: every body of the k = 333 batch within 4 e_reg of tests/app_ref.evaluate, the bound of the single-body fresh-case test.
Figures are printed before they are asserted."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import app_batch_ref as AB
from tests import app_ref
from tests import domain_kit as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, I32, U8 = torch.float32, torch.int32, torch.uint8
NAMES = ("terms", "grad_orientation", "grad_contact")


@pytest.fixture(scope="module")
def fixture():
    return app_ref.load_golden()


def _objective(c, sel=None, targets=None):
    from coma_amd.app import ComaObjective
    sel = c["sel"] if sel is None else sel
    targets = c["targets"] if targets is None else targets
    return ComaObjective(c["faces"], c["gt"], c["obj_normal"], sel, targets, c["p"], c["sub_p"], c["eps"], device=DEV)


class Batch:
    """A case, its objective, N bodies on the device, ONE batched evaluation and the N single ones; shared and left unchanged."""

    def __init__(self, c, N, seed, sel=None, targets=None):
        self.c, self.N = c, N
        self.objective = _objective(c, sel, targets)
        self.host = AB.batch_vertices(c, N, seed)
        self.verts = torch.as_tensor(self.host).to(DEV)
        with K.device_guard("batched and single evaluations"):
            self.batched = self.objective.evaluate(self.verts)
            self.single = [self.objective.evaluate(self.verts[n]) for n in range(N)]


def _fresh_case():
    c = app_ref.make_case(app_ref.grid_mesh(40, seed=77), 333, seed=78)
    c.update(obj_normal=c["obj_normals"][c["ref_index"]], targets=c["obj_verts"][c["objects"]])
    return c


@pytest.fixture(scope="module")
def small(fixture):
    return Batch(app_ref.golden_case(*fixture, "small_k20"), 3, seed=501)


@pytest.fixture(scope="module")
def fresh():
    return Batch(_fresh_case(), 9, seed=502)


@pytest.fixture(scope="module")
def wide():
    return Batch(_fresh_case(), 40, seed=503)


def _same_bits(a, b, equal_nan=False):
    a, b = a.cpu(), b.cpu()
    if equal_nan:                                   # NaN for NaN, every other element bit for bit
        return a.shape == b.shape and bool(((K.bits(a) == K.bits(b)) | (a.isnan() & b.isnan())).all())
    return a.shape == b.shape and torch.equal(K.bits(a), K.bits(b))


@pytest.mark.parametrize("which", ("small", "fresh", "wide"))
def test_body_n_has_the_single_call_s_bits(request, which):
    b = request.getfixturevalue(which)
    V = len(b.c["verts"])
    terms, g_o, g_c = b.batched
    assert tuple(terms.shape) == (b.N, 2) and tuple(g_o.shape) == tuple(g_c.shape) == (b.N, V, 3)
    assert all(t.dtype == F32 and t.is_contiguous() for t in b.batched)
    for n in range(b.N):
        for name, got, want in zip(NAMES, b.batched, b.single[n]):
            assert tuple(want.shape) == ((2,) if name == "terms" else (V, 3))
            assert torch.equal(got[n], want), (which, name, n)
            assert _same_bits(got[n], want), (which, name, n)
    # the bodies are different bodies, and finite: equal bits mean something
    t = terms.cpu().numpy()
    assert np.all(np.isfinite(t)) and len(np.unique(t[:, 0])) == b.N and len(np.unique(t[:, 1])) == b.N
    assert bool(torch.isfinite(g_o).all()) and bool(torch.isfinite(g_c).all()) and bool(g_c.ne(0).any(-1).any(-1).all())


def test_every_body_against_the_f64_restatement(fixture, fresh):
    g, _ = fixture
    c = fresh.c
    got = [t.cpu().numpy() for t in fresh.batched]
    worst = {q: 0.0 for q in app_ref.QUANTITIES}
    for n in range(fresh.N):
        want = app_ref.evaluate(fresh.host[n], c["faces"], c["gt"], c["obj_normal"], c["p"], c["sub_p"], c["eps"], c["sel"], c["targets"])
        dev = app_ref.deviations(dict(terms=got[0][n], grad_orientation=got[1][n], grad_contact=got[2][n]), {f"r64_{key}": v for key, v in want.items()})
        print(f"body {n}: " + "  ".join(f"{q} {dev[q]:.3e}" for q in app_ref.QUANTITIES))
        worst = {q: max(worst[q], dev[q]) for q in worst}
    for q in app_ref.QUANTITIES:
        print(f"{q}: worst body {worst[q]:.3e}, bound 4 e_reg = {4 * float(g[f'e_reg_{q}']):.3e}")
    for q in app_ref.QUANTITIES:
        assert worst[q] <= 4 * float(g[f"e_reg_{q}"]), (q, worst[q])


def test_no_selected_vertices(small):
    c = small.c
    with K.device_guard("k = 0"):
        empty = _objective(c, sel=np.zeros(0, np.int64), targets=np.zeros((0, 3), np.float32))
        terms, g_o, g_c = empty.evaluate(small.verts)
        single = [empty.evaluate(small.verts[n]) for n in range(small.N)]
    assert tuple(terms.shape) == (3, 2) and bool((terms[:, 1] == 0).all()) and not bool(g_c.any())
    assert _same_bits(terms[:, 1], torch.zeros(3))                                # +0, not -0
    for n in range(small.N):
        assert _same_bits(terms[n], single[n][0]) and _same_bits(g_o[n], single[n][1]) and _same_bits(g_c[n], single[n][2])
        # the orientation output does not know about the selection
        assert _same_bits(terms[n, 0], small.batched[0][n, 0]) and _same_bits(g_o[n], small.batched[1][n])


def test_a_nan_stays_in_its_body(small):
    """One selected vertex of body 1 is NaN: ordinary data for these kernels (comparisons with NaN are false, a row outside its range
    is never followed), not a fault.  Bodies 0 and 2 keep their bits; body 1 is the single call's on the same vertices, NaN for NaN."""
    poisoned = small.verts.clone()
    poisoned[1, int(small.c["sel"][3])] = float("nan")
    with K.device_guard("poisoned batch"):
        got = small.objective.evaluate(poisoned)
        alone = small.objective.evaluate(poisoned[1])
    for name, g, clean, a in zip(NAMES, got, small.batched, alone):
        assert _same_bits(g[0], clean[0]) and _same_bits(g[2], clean[2]), name
        assert _same_bits(g[1], a, equal_nan=True), name
        assert torch.equal(g[1].isnan(), a.isnan())
    assert bool(got[0][1].isnan().any()) and bool(torch.isfinite(got[0][[0, 2]]).all())


def test_two_batched_evaluations_are_bit_identical(fixture, fresh):
    with K.device_guard("second evaluation"):
        filler = _objective(app_ref.golden_case(*fixture, "small_k60")).evaluate(torch.as_tensor(fixture[0]["mesh_small__verts"]).to(DEV))
        again = fresh.objective.evaluate(fresh.verts)
    assert tuple(filler[0].shape) == (2,)
    for name, a, b in zip(NAMES, fresh.batched, again):
        assert _same_bits(a, b), name
    assert len(fresh.objective._batch_ws) == 1 and 9 in fresh.objective._batch_ws          # the workspace of N = 9: made once, kept


def test_loss_of_n_bodies_and_its_backward(small):
    """loss -> [N]; weighted by a fixed vector and summed, the gradient at the vertices is weight[n] (w_o g_o[n] + w_c g_c[n]) in f32,
    the very products the backward forms, so bit for bit.  One body ([V,3], [1,V,3]) still gives a 0-dim scalar."""
    w_o, w_c = 10.0, 5.0
    weight = torch.tensor([0.5, -2.0, 3.25], device=DEV)
    v = small.verts.clone().requires_grad_(True)
    with K.device_guard("loss of three bodies"):
        loss = small.objective.loss(v, w_o, w_c)
        (loss * weight).sum().backward()
    terms, g_o, g_c = small.batched
    assert tuple(loss.shape) == (3,) and loss.dtype == F32
    assert _same_bits(loss.detach(), w_o * terms[:, 0] + w_c * terms[:, 1])
    want = torch.stack([weight[n] * (w_o * g_o[n] + w_c * g_c[n]) for n in range(3)])
    assert tuple(v.grad.shape) == (3, len(small.c["verts"]), 3) and _same_bits(v.grad, want)
    assert bool(v.grad[1].ne(0).any())
    for shape in ((-1, 3), (1, -1, 3)):
        one = small.verts[2].reshape(shape).clone().requires_grad_(True)
        with K.device_guard("loss of one body"):
            scalar = small.objective.loss(one, w_o, w_c)
            scalar.backward()
        assert scalar.dim() == 0 and _same_bits(scalar.detach(), loss[2].detach())
        assert one.grad.shape == one.shape and _same_bits(one.grad.reshape(-1, 3), w_o * g_o[2] + w_c * g_c[2])
    with pytest.raises(ValueError, match=r"expected \[145,3\], \[1,145,3\] or \[N,145,3\]"):
        small.objective.evaluate(small.verts[:, :100])


# ---- the C entry point ----
def _p(t, offset=0):
    return None if t is None else C.c_void_p(t.data_ptr() + offset)


class Guarded:
    """A device buffer between two guards (tests/domain_kit.guarded), its body the kit's sentinel; `ptr` is the address of the body."""

    def __init__(self, n, dtype):
        self.n = n
        self.flat = K.guarded(K.sentinel(n, dtype)).to(DEV)
        self.ptr = C.c_void_p(self.flat.data_ptr() + K.GUARD * self.flat.element_size())

    def body(self):
        return self.flat[K.GUARD:K.GUARD + self.n]

    def intact(self):
        return K.guards_intact(self.flat.cpu())


def test_refusals_leave_the_outputs_untouched():
    from coma_amd import _lib
    L = _lib.lib()
    resolve, outs, small_buffer = K.device_resolver(AB.OUTPUT_ARGS, AB.HOST_ARGS, device=DEV)
    table = AB.refusal_table(L)
    assert K.check_refusals(L, table, resolve, expect_control=False) == len(table["coma_app_objective_batch_f32"][1]) >= 30
    K.refusal_outputs_untouched(outs, small_buffer)


def test_size_function():
    from coma_amd import _lib
    L = _lib.lib()
    size, one = L.coma_app_objective_batch_workspace_bytes, L.coma_app_objective_workspace_bytes
    for V, F, k, N in ((0, 242, 0, 3), (145, 0, 20, 3), (145, 242, -1, 3), (145, 242, 146, 3), (145, 242, 20, 0), (145, 242, 20, -1), (145, 242, 20, 1025)):
        assert size(V, F, k, N) == 0, (V, F, k, N)
    for V, F, k in ((145, 242, 20), (145, 242, 0), (1601, 3042, 333), (10475, 20908, 1000)):
        assert 0 < size(V, F, k, 1) <= (one(V, F, k) + 15) // 16 * 16
        assert size(V, F, k, 1) < size(V, F, k, 2) < size(V, F, k, 1024) and size(V, F, k, 9) % 16 == 0


def test_an_accepted_call_writes_exactly_its_outputs(small):
    """V = 145, k = 20, N = 3 through ctypes into guarded buffers, twice: [N][2], [N][V,3], [N][V,3] are written completely (no sentinel
    left), every guard -- the workspace's too -- is intact, the two calls agree, and the bits are those of ComaObjective.evaluate."""
    from coma_amd import _lib
    L, o, N = _lib.lib(), small.objective, 3
    V, ws_bytes = o.V, L.coma_app_objective_batch_workspace_bytes(o.V, o.F, o.k, N)
    assert (V, o.F, o.k) == (145, 242, 20)

    def outputs():
        return dict(terms=Guarded(N * 2, F32), grad_orientation=Guarded(N * V * 3, F32), grad_contact=Guarded(N * V * 3, F32), workspace=Guarded(ws_bytes, U8))

    def launch(b):
        rc = L.coma_app_objective_batch_f32(_p(small.verts), _p(o.faces), _p(o.vf_offsets), _p(o.vf_faces), V, o.F, _p(o.orientation_gt), o._b, o._p, o._s,
                                            o.eps, _p(o.selected), _p(o.targets), o.k, N, b["terms"].ptr, b["grad_orientation"].ptr, b["grad_contact"].ptr,
                                            b["workspace"].ptr, ws_bytes, None)
        assert rc == 0, L.coma_last_error()

    first, second = K.launch_twice(outputs, launch, "coma_app_objective_batch_f32 into guarded buffers")
    for b in (first, second):
        for name, buf in b.items():
            assert buf.intact(), f"guard of `{name}` written"
    for name, want in zip(NAMES, small.batched):
        got = first[name].body().cpu()
        assert not bool((K.bits(got) == K.sentinel_bits(F32)).any()), f"`{name}` keeps a sentinel: not written completely"
        assert _same_bits(got, second[name].body()) and _same_bits(got, want.reshape(-1)), name
