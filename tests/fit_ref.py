"""The project's own restatement of the fitting app's Adam loop (rule set: include/coma_hip.h, "The fitting app's whole Adam loop"):
NumPy in f64, chaining the restatements of its stages -- vposer_ref.decode / decode_backward, smplx_ref.forward / backward,
app_ref.objective (under CPU autograd, f64), vposer_ref.angle_prior(_backward) -- and Adam as torch states it.  Pinned against the
reference's own parts run in f64 (tests/golden/app_fit_golden.npz, R64) by tests/test_app_fit_host.py.

Nothing is rounded to f32 here (the device rounds the parameters before its f32 models and the vertices after the scale): this is the
formula, the device's f32 evaluation of it is held to the reference's own f32 error.

Also here: the golden cases (model, decoder weights, weights of the loss; the objective's inputs come from the fixture)."""
import json
import os

import numpy as np
import torch

from tests import app_ref
from tests import smplx_ref as S
from tests import vposer_ref as V

DEFAULT_BETAS = [-0.00982137, 0.03693837, 0.0949352, -0.01299302, 0.00492086, -0.04505398, -0.0008909, -0.00054313, 0.03646483, -0.00803524]
BETA1, BETA2, ADAM_EPS = 0.9, 0.999, 1e-8
LOSS_COLUMNS = ("total", "pprior", "angle_prior", "orientation", "contact")


def coefficients():
    """The app's shape: its default betas (as f32, the models' precision) followed by a zero expression."""
    return np.concatenate([np.float32(DEFAULT_BETAS), np.zeros(10, np.float32)]).astype(np.float64)


def layout(fm, D):
    """(hs, nb, P): entries per hand, body-pose entries, length of p = [global_orient 3 | transl 3 | left hs | right hs | embedding D]."""
    hs = fm["n_pca"] if fm["n_pca"] else fm["hd"]
    nb = 3 * fm["J"] - 2 * fm["hd"] - 12
    return hs, nb, 6 + 2 * hs + D


def start(fm, w):
    """fit()'s initial values: global_orient 0, transl (3, 1, 0), hands 0, the embedding the encoder's mean of the T-pose."""
    D = np.asarray(w["bodyprior_dec_fc1.weight"]).shape[1]
    hs, nb, P = layout(fm, D)
    p = np.zeros(P)
    p[3:6] = [3.0, 1.0, 0.0]
    p[6 + 2 * hs:] = V.encode(w, np.zeros((1, nb)))[0][0]
    return p


def theta_of(fm, p, aa):
    """The body model's packed pose [global_orient | body_pose | jaw, eyes (zero) | left hand | right hand]."""
    hs = fm["n_pca"] if fm["n_pca"] else fm["hd"]
    return np.concatenate([p[:3], np.asarray(aa, dtype=np.float64).reshape(-1), np.zeros(9), p[6:6 + 2 * hs]])


def objective_f64(vs, obj):
    """(terms [2], grad_orientation, grad_contact) of the scaled vertices in f64: app_ref.objective under autograd, no f32 rounding."""
    v = torch.as_tensor(np.asarray(vs, dtype=np.float64)).requires_grad_(True)
    t_o, t_c = app_ref.objective(v, obj["faces"], obj["gt"], obj["obj_normal"], obj["p"], obj["sub_p"], obj["eps"], obj["sel"], obj["targets"])
    g_o, = torch.autograd.grad(t_o, v, retain_graph=True)
    g_c, = torch.autograd.grad(t_c, v, allow_unused=True)
    g_c = torch.zeros_like(v) if g_c is None else g_c
    return np.array([float(t_o.detach()), float(t_c.detach())]), g_o.numpy(), g_c.numpy()


def evaluate(fm, w, coef, obj, wt, p):
    """One forward and backward at p: dict(loss_terms [5], gradient [P], vertices [V,3] (scaled), aa)."""
    D = np.asarray(w["bodyprior_dec_fc1.weight"]).shape[1]
    hs, nb, P = layout(fm, D)
    z = p[6 + 2 * hs:]
    fwd_v = V.decode(w, z[None])
    aa = fwd_v["aa"].reshape(-1)
    fwd = S.forward(fm, coef, theta_of(fm, p, aa), p[3:6])
    vs = fwd["vertices"] * wt["scale_factor"]
    terms, g_o, g_c = objective_f64(vs, obj)
    prior = V.angle_prior(aa[None])
    g_theta, g_transl = S.backward(fm, fwd, wt["scale_factor"] * (wt["orientation_weight"] * g_o + wt["contact_weight"] * g_c))
    g_pose = g_theta[3:3 + nb][None] + wt["bending_prior_weight"] * V.angle_prior_backward(aa[None], np.ones((1, 4)))
    w_pp = wt["body_pose_weight"] ** 2 * wt["pprior_weight"]
    g_z = V.decode_backward(w, fwd_v, g_pose)[0] + 2.0 * z * w_pp
    pprior = (np.sum(z * z) * wt["body_pose_weight"] ** 2) * wt["pprior_weight"]
    bend = wt["bending_prior_weight"] * float(np.sum(prior))
    total = ((pprior + bend) + wt["orientation_weight"] * terms[0]) + wt["contact_weight"] * terms[1]
    return dict(loss_terms=np.array([total, pprior, bend, terms[0], terms[1]]), gradient=np.concatenate([g_theta[:3], g_transl, g_theta[12 + nb:], g_z]),
                vertices=vs, aa=aa)


def adam_step(p, g, m, v, p1, p2, lr):
    """torch.optim.Adam's single-tensor form: returns the new (p, m, v, p1, p2)."""
    m = BETA1 * m + (1.0 - BETA1) * g
    v = BETA2 * v + ((1.0 - BETA2) * g) * g
    p1, p2 = p1 * BETA1, p2 * BETA2
    return p - ((lr / (1.0 - p1)) * m) / (np.sqrt(v) / np.sqrt(1.0 - p2) + ADAM_EPS), m, v, p1, p2


def run(fm, w, coef, obj, wt, num_iters, p0=None):
    """The loop: dict(parameters [E+1,P], loss_terms [E,5], gradients [E,P], vertices [V,3] of the last iteration's forward)."""
    p = start(fm, w) if p0 is None else np.asarray(p0, dtype=np.float64).copy()
    m, v, p1, p2 = np.zeros_like(p), np.zeros_like(p), 1.0, 1.0
    rows, losses, grads, vertices = [p.copy()], [], [], None
    for _ in range(num_iters):
        ev = evaluate(fm, w, coef, obj, wt, p)
        p, m, v, p1, p2 = adam_step(p, ev["gradient"], m, v, p1, p2, wt["lr"])
        rows.append(p.copy()), losses.append(ev["loss_terms"]), grads.append(ev["gradient"])
        vertices = ev["vertices"]
    return dict(parameters=np.array(rows), loss_terms=np.array(losses).reshape(-1, 5), gradients=np.array(grads).reshape(-1, len(p)), vertices=vertices)


# ---- the golden cases ----
ITERS = 20
# test_one_fit_step_with_every_stage_on_the_device's weights with the two objective weights x 1e4 (the app's own are 1e12 and 2.6e11):
# at 10 and 5 the hands' and the embedding's gradients come down to 1e-5 within 20 iterations, which the generator's condition (a) refuses
WEIGHTS = dict(lr=1e-2, scale_factor=0.84, orientation_weight=1e5, contact_weight=5e4, body_pose_weight=2.0, bending_prior_weight=0.5,
               pprior_weight=0.3)
# Columns of p on which a case's loss does not depend.  Without selected vertices nothing depends on transl (normals, and so the
# orientation term, do not move with a translation): its gradient is a sum of rounding errors, exactly zero in no precision, and Adam
# turns any such sum above its eps into steps of order lr -- in the reference's own f32 as on the device.  Such a column is a random
# walk, not a trajectory to compare: it is left out of e_ref, of condition (a) and of the parameter comparison, and the vertices of
# such a case are compared with their own translation taken off.
FREE_COLUMNS = {"k0": (3, 4, 5)}


def pinned_columns(name, P):
    return np.array([i for i in range(P) if i not in FREE_COLUMNS.get(name, ())])


def untranslated(name, vertices, parameters):
    """The last forward's vertices (scaled), with scale_factor x its own transl taken off where the case's transl is a free column."""
    if 3 not in FREE_COLUMNS.get(name, ()):
        return np.asarray(vertices, dtype=np.float64)
    return np.asarray(vertices, dtype=np.float64) - WEIGHTS["scale_factor"] * np.asarray(parameters, dtype=np.float64)[-2, 3:6]
#        name    n_pca  k   seed of the objective's inputs
CASES = (("app",  45,   40, 91),
         ("pca6", 6,    40, 91),
         ("k0",   45,   0,  91))
CASE_NAMES = tuple(c[0] for c in CASES)
BODY, DECODER = "moderate", "near_rest"


def case_models(name):
    """(file-style model, flat model, decoder weights, n_pca, k, seed) of a golden case."""
    _, n_pca, k, seed = CASES[CASE_NAMES.index(name)]
    model, _ = S.case_model(BODY)
    return model, S.flat_model(model, n_pca=n_pca), V.case_weights(DECODER), n_pca, k, seed


def make_objective_inputs(name):
    """The objective's seeded inputs of a case, drawn around the f32 vertices of the start pose (the generator stores them: tests
    read the fixture and do not redraw)."""
    _, fm, w, _, k, seed = case_models(name)
    p0 = start(fm, w)
    aa = V.decode(w, p0[None, -np.asarray(w["bodyprior_dec_fc1.weight"]).shape[1]:])["aa"]
    verts = (S.forward(fm, coefficients(), theta_of(fm, p0, aa), p0[3:6])["vertices"] * WEIGHTS["scale_factor"]).astype(np.float32)
    c = app_ref.make_case((verts, fm["faces"]), max(k, 1) if k else 40, seed=seed)
    if k == 0:
        c["sel"], c["objects"] = c["sel"][:0], c["objects"][:0]
    return {key: c[key] for key in ("gt", "obj_verts", "obj_normals", "sel", "objects", "p", "sub_p")}, dict(eps=c["eps"], ref_index=c["ref_index"])


def load_golden():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "app_fit_golden.npz"), allow_pickle=False)
    return g, json.loads(str(g["meta_json"]))


def golden_objective(g, meta, name):
    """The objective's inputs of a case as the arguments of app_ref.objective / ComaObjective."""
    _, fm, _, _, _, _ = case_models(name)
    c = {key: g[f"{name}__{key}"] for key in ("gt", "obj_verts", "obj_normals", "sel", "objects", "p", "sub_p")}
    c.update(faces=fm["faces"], eps=float(meta[name]["eps"]), obj_normal=c["obj_normals"][meta[name]["ref_index"]],
             targets=c["obj_verts"][c["objects"]].reshape(-1, 3), sel=c["sel"].astype(np.int64))
    return c
