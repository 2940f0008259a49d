"""GPU: the optimisation app's ComA objective (coma_amd.app.ComaObjective, coma_amd/csrc/app_objective.hip) against the reference's own
functions executed in f64 (R64 of tests/golden/app_objective_golden.npz) and against the f64 restatement tests/app_ref.py.

Bounds.  e_ref_* (stored by the generator) is max|R32 - R64| / max|R64| pooled over the cases, the reference's own f32 against its f64;
the device must meet 4 * e_ref on every case (two f32 evaluations of one formula in different summation orders).  One case (`near`,
1 + b.p just above eps) is ill-conditioned for the reference's f32 and inflates the pooled orientation figures by four orders of
magnitude, so every OTHER case is also held to 4 * e_reg, the same pool without `near`.  Figures are printed before they are asserted.
"""
import os
import pickle

import numpy as np
import pytest
import torch

from tests import app_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def fixture():
    return app_ref.load_golden()


def _objective(c, sel=None, targets=None):
    from coma_amd.app import ComaObjective
    sel = c["sel"] if sel is None else sel
    targets = c["targets"] if targets is None else targets
    return ComaObjective(c["faces"], c["gt"], c["obj_normal"], sel, targets, c["p"], c["sub_p"], c["eps"], device=DEV)


def _evaluate(objective, verts):
    terms, g_o, g_c = objective.evaluate(torch.as_tensor(verts).to(DEV))
    return dict(terms=terms.cpu().numpy(), grad_orientation=g_o.cpu().numpy(), grad_contact=g_c.cpu().numpy())


@pytest.mark.parametrize("name", app_ref.CASES)
def test_golden_case_within_the_reference_s_own_error(fixture, name):
    g, meta = fixture
    c = app_ref.golden_case(g, meta, name)
    got = _evaluate(_objective(c), c["verts"])
    dev = app_ref.deviations(got, c)
    for q in app_ref.QUANTITIES:
        print(f"{name} {q}: device vs R64 {dev[q]:.3e}   4 e_ref {4 * float(g[f'e_ref_{q}']):.3e}   4 e_reg {4 * float(g[f'e_reg_{q}']):.3e}")
    for q in app_ref.QUANTITIES:
        assert dev[q] <= 4 * float(g[f"e_ref_{q}"]), (q, dev[q])
        if name != "near":
            assert dev[q] <= 4 * float(g[f"e_reg_{q}"]), (q, dev[q])
    # the isolated vertex (the last one): exactly zero rows
    assert not got["grad_orientation"][-1].any()
    if len(c["verts"]) - 1 not in c["sel"]:
        assert not got["grad_contact"][-1].any()
    rows = np.ones(len(c["verts"]), bool)
    rows[c["sel"]] = False
    assert not got["grad_contact"][rows].any()


def test_fresh_case_with_k_off_the_tile_width_against_the_restatement(fixture):
    g, _ = fixture
    k = 333                                  # the double minimum stages 64 points at a time: 5 tiles and 13 left over, several splits
    c = app_ref.make_case(app_ref.grid_mesh(40, seed=77), k, seed=78)
    c.update(obj_normal=c["obj_normals"][c["ref_index"]], targets=c["obj_verts"][c["objects"]])
    want = app_ref.evaluate(c["verts"], c["faces"], c["gt"], c["obj_normal"], c["p"], c["sub_p"], c["eps"], c["sel"], c["targets"])
    got = _evaluate(_objective(c), c["verts"])
    want = {f"r64_{key}": v for key, v in want.items()}
    dev = app_ref.deviations(got, want)
    print({q: f"{v:.3e}" for q, v in dev.items()})
    for q in app_ref.QUANTITIES:
        assert dev[q] <= 4 * float(g[f"e_reg_{q}"]), (q, dev[q])


def test_two_evaluations_are_bit_identical(fixture):
    g, meta = fixture
    c = app_ref.golden_case(g, meta, "large_k1000")
    objective = _objective(c)
    v = torch.as_tensor(c["verts"]).to(DEV)
    first = [t.clone() for t in objective.evaluate(v)]
    filler = _evaluate(_objective(app_ref.golden_case(g, meta, "small_k60")), g["mesh_small__verts"])      # other work in between
    second = objective.evaluate(v)
    assert filler["terms"].shape == (2,)
    for a, b in zip(first, second):
        assert torch.equal(a, b)


def test_no_selected_vertices(fixture):
    g, meta = fixture
    c = app_ref.golden_case(g, meta, "small_k20")
    got = _evaluate(_objective(c, sel=np.zeros(0, np.int64), targets=np.zeros((0, 3), np.float32)), c["verts"])
    assert got["terms"][1] == 0.0 and not got["grad_contact"].any()
    assert app_ref.rel_dev(got["terms"][0], c["r64_terms"][0]) <= 4 * float(g["e_reg_term_orientation"])
    assert app_ref.rel_dev(got["grad_orientation"], c["r64_grad_orientation"]) <= 4 * float(g["e_reg_grad_orientation"])


def _chain_gradients(c, dtype, device, loss_of):
    body = app_ref.RigidBody(torch.as_tensor(c["verts"]).to(device=device, dtype=dtype), c["faces"])
    orient = torch.tensor([[0.3, -0.2, 0.5]], dtype=dtype, device=device, requires_grad=True)
    transl = torch.tensor([[0.1, 0.05, -0.2]], dtype=dtype, device=device, requires_grad=True)
    loss = loss_of(body(global_orient=orient, transl=transl).vertices)
    loss.backward()
    return float(loss.detach()), np.concatenate([orient.grad.cpu().numpy().ravel(), transl.grad.cpu().numpy().ravel()]).astype(np.float64)


def test_loss_backward_through_a_stand_in_body_model(fixture):
    """d loss / d (global_orient, transl) through the Rodrigues stand-in, against the same chain over the restatement in f64.
    Bound: the device's vertex gradients are within 4 e_reg of f64 (above); the chain behind them is torch f32, whose sums over the
    V = 145 vertices are within V 2^-24 of the exact ones: (4 e_reg + V 2^-24) relative to the largest component."""
    g, meta = fixture
    c = app_ref.golden_case(g, meta, "small_k20")
    w_o, w_c = 10.0, 5.0
    objective = _objective(c)
    for shape in ((1, -1, 3), (-1, 3)):
        loss, grad = _chain_gradients(c, torch.float32, DEV, lambda v: objective.loss(v.reshape(shape), w_o, w_c))

        def restated(v):
            t_o, t_c = app_ref.objective(v.reshape(-1, 3), c["faces"], c["gt"], c["obj_normal"], c["p"], c["sub_p"], c["eps"], c["sel"], c["targets"])
            return w_o * t_o + w_c * t_c
        want_loss, want = _chain_gradients(c, torch.float64, "cpu", restated)
        bound = 4 * max(float(g["e_reg_grad_orientation"]), float(g["e_reg_grad_contact"])) + len(c["verts"]) * 2.0 ** -24
        print(f"loss {loss:.8f} vs {want_loss:.8f}; gradients {grad} vs {want}; deviation {app_ref.rel_dev(grad, want):.3e}, bound {bound:.3e}")
        assert app_ref.rel_dev(grad, want) <= bound
        assert abs(loss - want_loss) <= bound * abs(want_loss)


def test_twenty_adam_iterations_of_optimize_smpl(fixture, tmp_path):
    """src/application/optimize.py's optimize_smpl with the stand-in hooks, on a state and an asset pickle built so that the target
    selection gives the fixture's constants: the trajectory of (global_orient, transl) stays within 4x the deviation between the
    restatement's f32 and f64 trajectories (measured on the CPU by the generator), and the loss decreases."""
    from src.application.optimize import optimize_smpl
    g, meta = fixture
    m = meta["traj"]
    c = app_ref.golden_case(g, meta, "traj")
    V, O = len(c["verts"]), len(c["obj_verts"])
    prob = np.zeros((V, O, V), np.float32)
    prob[np.arange(V), m["ref_index"], np.arange(V)] = 1.0                  # vertex h's most likely bin is bin h, whose direction is gt[h]
    nom = np.full((V, O), 0.1, np.float32)
    nom[c["sel"], c["objects"]] = 1.0
    state = dict(prob_grid_canon_human_wrt_obj=prob, canon_normal_grid=c["gt"], contact_dist_expectation_grid_nom=nom,
                 contact_dist_expectation_grid_denom=np.ones((V, O), np.float32))
    asset_pth = str(tmp_path / "asset.pickle")
    with open(asset_pth, "wb") as fh:
        pickle.dump(dict(downsampled_pcd_points_raw=c["obj_verts"], downsampled_pcd_normal_raw=c["obj_normals"]), fh)
    body = app_ref.RigidBody(torch.as_tensor(c["verts"]).to(DEV), c["faces"])
    out = optimize_smpl("super", "cat", state, asset_pth, eps=m["eps"], principle_vec=c["p"], sub_principle_vec=c["sub_p"],
                        reference_object_vertex_index=m["ref_index"], lr=m["lr"], body_pose_weight=m["body_pose_weight"],
                        bending_prior_weight=m["bending_prior_weight"], pprior_weight=m["pprior_weight"], orientation_weight=m["orientation_weight"],
                        contact_weight=m["contact_weight"], contact_threshold=0.3, scale_factor=m["scale_factor"], use_collision=False,
                        save_dir=str(tmp_path), num_iters=m["iters"], body_model=body, pose_decoder=app_ref.NullPoseDecoder(device=DEV),
                        angle_prior=app_ref.null_angle_prior, device=DEV, record=True)
    traj, want = np.asarray(out["trajectory"]), c["r64_trajectory"]
    dev, bound = float(np.max(np.abs(traj - want))), 4 * float(g["traj__e_ref"])
    print(f"trajectory deviation {dev:.3e}, bound {bound:.3e}; loss {out['losses'][0]:.6f} -> {out['losses'][-1]:.6f} (f64: {c['r64_losses'][0]:.6f} -> {c['r64_losses'][-1]:.6f})")
    assert traj.shape == want.shape == (m["iters"] + 1, 6)
    assert dev <= bound
    assert out["losses"][-1] < out["losses"][0]
    from coma_amd.downsample import load_obj
    v, f = load_obj(os.path.join(str(tmp_path), "super", "cat", "optimized.obj"))
    assert np.array_equal(f, c["faces"]) and np.array_equal(v.astype(np.float32), out["vertices"].astype(np.float32))
