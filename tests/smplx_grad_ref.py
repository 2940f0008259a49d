"""The project's own restatement of the SMPL-X body model's FULL backward (rule set: include/coma_hip.h, "The SMPL-X body model",
the `full backward` rules): NumPy in f64, from dL/dvertices, dL/djoints and dL/dfull_pose to dL/dtheta, dL/dtransl and
dL/dcoefficients (betas followed by expression); the seeded upstream gradients of the golden cases; and the fixture's loader.  Pinned
against the third-party package's own lbs and SMPLX class under CPU autograd in f64 (tests/golden/smplx_grad_golden.npz, R64) by
tests/test_smplx_grad_host.py.  The forward, the models and the cases are those of tests/smplx_ref.py."""
import os

import numpy as np

from tests import smplx_ref as S

LOSSES = ("all", "vertices", "joints", "full_pose")        # which outputs the loss reads; the others' gradients are absent
QUANTITIES = ("grad_pose", "grad_transl", "grad_coef")


def backward_full(fm, fwd, g=None, gJ=None, gP=None, idx=None, w=None):
    """(dL/dtheta [NT], dL/dtransl [3], dL/dcoefficients [NB]) from g = dL/dvertices [V,3], gJ = dL/djoints [J + E, 3] (posed joints,
    then the extra joints of the table idx [E,3] / w [E,3]) and gP = dL/dfull_pose [3J]; each may be None, which means zeros."""
    V, J, parents, Jr, R, G = fm["V"], fm["J"], fm["parents"], fwd["J_rest"], fwd["R"], fwd["G"]
    d = lambda a: np.asarray(a, dtype=np.float64)
    g_eff = np.zeros((V, 3)) if g is None else d(g).reshape(V, 3).copy()
    d_transl = np.zeros(3)
    gJp = np.zeros((J, 3))
    if gJ is not None:
        gJ = d(gJ).reshape(-1, 3)
        gJp = gJ[:J]
        E = 0 if idx is None else len(idx)
        assert gJ.shape[0] == J + E
        for e in range(E):                                     # ascending (e, i); repeated indices add up
            for i in range(3):
                g_eff[idx[e][i]] += w[e][i] * gJ[J + e]
            d_transl += (1.0 - ((w[e][0] + w[e][1]) + w[e][2])) * gJ[J + e]
    vp1 = np.concatenate([fwd["v_posed"], np.ones((V, 1))], 1)
    dA = np.einsum("vj,vr,vc->jrc", fm["weights"], g_eff, vp1)
    g_vp = np.einsum("vrc,vr->vc", fwd["T"][:, :, :3], g_eff)
    dfeat = fm["posedirs"] @ g_vp.reshape(-1)
    dJ = -np.einsum("jrc,jr->jc", G[:, :, :3], dA[:, :, 3])    # A_i.t = G_i.t - G_i.R J_i
    dG = dA.copy()
    dG[:, :, :3] -= np.einsum("jr,jc->jrc", dA[:, :, 3], Jr)
    dG[:, :, 3] += gJp                                         # joints_i = G_i.t + transl
    dR = np.zeros((J, 3, 3))
    for i in range(J - 1, 0, -1):
        p = parents[i]
        dR[i] = G[p, :, :3].T @ dG[i, :, :3]
        dG[p, :, :3] += dG[i, :, :3] @ R[i].T + np.outer(dG[i, :, 3], Jr[i] - Jr[p])
        dG[p, :, 3] += dG[i, :, 3]
        u = G[p, :, :3].T @ dG[i, :, 3]                        # G_i.t = G_p.R (J_i - J_p) + G_p.t
        dJ[i] += u
        dJ[p] -= u
    dR[0] = dG[0, :, :3]
    dJ[0] += dG[0, :, 3]
    dR[1:] += dfeat.reshape(J - 1, 3, 3)
    dpose = S.rodrigues_backward(fwd["full_pose"].reshape(J, 3), dR).reshape(-1)
    if gP is not None:
        dpose = dpose + d(gP).reshape(-1)                      # full_pose = assembled theta + pose_mean
    if fm["n_pca"]:
        nb, hd = 3 * J - 2 * fm["hd"], fm["hd"]
        dpose = np.concatenate([dpose[:nb], fm["comps"][0] @ dpose[nb:nb + hd], fm["comps"][1] @ dpose[nb + hd:]])
    d_vshaped = g_vp + fm["J_regressor"].T @ dJ
    d_coef = d_vshaped.reshape(-1) @ fm["shapedirs"].reshape(3 * V, -1)
    return dpose, g_eff.sum(0) + gJp.sum(0) + d_transl, d_coef


def upstream(loss, g, gJ, gP):
    """The three upstream gradients of one of LOSSES: the outputs the loss does not read get None."""
    return (g if loss in ("all", "vertices") else None, gJ if loss in ("all", "joints") else None, gP if loss in ("all", "full_pose") else None)


def loss_value(fm, coefficients, theta, transl, g=None, gJ=None, gP=None, idx=None, w=None):
    """sum(vertices g) + sum(joints gJ) + sum(full_pose gP) of the restated forward, f64 (central differences run on this)."""
    fwd = S.forward(fm, coefficients, theta, transl)
    total = 0.0
    if g is not None:
        total += float(np.sum(fwd["vertices"] * g))
    if gJ is not None:
        joints = fwd["joints"] if idx is None or not len(idx) else np.concatenate([fwd["joints"], S.extra_joints(fwd, idx, w)])
        total += float(np.sum(joints * gJ))
    if gP is not None:
        total += float(np.sum(fwd["full_pose"] * gP))
    return total


# ---- seeded upstream gradients and the fixture ----
def case_upstream(name):
    """(gJ f32 [J,3], gP f32 [3J]) of a golden case; g is smplx_ref.case_inputs(name)["g"].  The lbs cases have no extra joints."""
    i = S.CASE_NAMES.index(name)
    J = S.CASES[i][2]
    rng = np.random.RandomState(4000 + i)
    return rng.normal(size=(J, 3)).astype(np.float32), rng.normal(size=3 * J).astype(np.float32)


def class_upstream():
    """(gJ f32 [55 + 21 + 51, 3], gP f32 [165]) of the class case; g is the full smplx_ref.class_case()[2]."""
    rng = np.random.RandomState(4100)
    return rng.normal(size=(127, 3)).astype(np.float32), rng.normal(size=165).astype(np.float32)


def class_vertex_ids(golden_forward, fm, fwd):
    """The 21 vertex picks of the class case.  The package's id table is not shipped; the picks are recovered from the joints the
    FORWARD fixture stores (rows 55..75 of class__r64_joints): each is the one vertex of the seeded model it coincides with."""
    picks = golden_forward["class__r64_joints"][55:76]
    dist = np.linalg.norm(fwd["vertices"][None] - picks[:, None], axis=-1)
    ids = dist.argmin(1)
    assert dist[np.arange(21), ids].max() <= 1e-12 * np.abs(picks).max()
    return [int(i) for i in ids]


def load_golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "smplx_grad_golden.npz"), allow_pickle=False)
