"""The project's own restatement of the SMPL-X body model (rule set: include/coma_hip.h, "The SMPL-X body model"): NumPy in f64,
forward (vertices, posed joints, extra joints) and the analytic backward from dL/dvertices to dL/dtheta and dL/dtransl; a torch form
of the forward (autograd gives its backward) that scripts/time_body_model.py uses as the eager baseline; and the seeded synthetic
model.  Pinned against the third-party package's own lbs and SMPLX class executed in f64 (tests/golden/smplx_golden.npz, R64) by
tests/test_smplx_host.py.

A synthetic model is a dict with the keys of an SMPL-X model file; `flat_model` turns such a dict into the arrays the arithmetic
works on.  Joint layout for any J >= 5: H = min(15, (J - 5) // 2) joints per hand at the end, before them global orientation, the
body joints, jaw and both eyes; theta = [3 (J - 2H) axis-angle entries | n_pca left | n_pca right] (use_pca) or all 3J entries."""
import json
import os

import numpy as np

SHAPE_SPACE_DIM, EXPRESSION_SPACE_DIM = 300, 100


def hand_joints(J):
    return max(0, min(15, (J - 5) // 2))


# ---- the seeded model ----
def make_tree(J, kind, rng):
    if kind == "chain":
        parents = np.arange(-1, J - 1)
    elif kind == "star":
        parents = np.zeros(J, np.int64)
    elif kind == "random":
        parents = np.array([0] + [int(rng.randint(0, i)) for i in range(1, J)])
    else:
        raise ValueError(kind)
    parents = parents.astype(np.int64)
    parents[0] = -1
    return parents


def synthetic_model(V, J, NB, n_pca, tree="random", seed=0, n_faces=None, n_landmarks=5):
    """A deterministic model file's content (f32 / integer arrays): row-normalised J_regressor, skinning weights rand**8
    row-normalised (a few joints dominate), small shapedirs [V,3,NB] / posedirs [V,3,P], square hand component matrices and hand
    means, faces and landmark faces with barycentric weights.  n_pca only bounds the hand matrices from below."""
    rng = np.random.RandomState(seed)
    P, hd = 9 * (J - 1), 3 * hand_joints(J)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    Jr = rng.rand(J, V) ** 4
    W = rng.rand(V, J) ** 8
    parents = make_tree(J, tree, rng)
    F = n_faces or 2 * V
    rows = max(hd, n_pca)
    bary = rng.rand(n_landmarks, 3) + 0.1
    m = dict(v_template=f32(rng.uniform(-1, 1, (V, 3)) * [0.3, 0.9, 0.2]), shapedirs=f32(rng.normal(size=(V, 3, NB)) * 0.02),
             posedirs=f32(rng.normal(size=(V, 3, P)) * 0.01), J_regressor=f32(Jr / Jr.sum(1, keepdims=True)),
             kintree_table=np.stack([np.where(parents < 0, 2 ** 32 - 1, parents), np.arange(J)]).astype(np.int64),
             weights=f32(W / W.sum(1, keepdims=True)), f=rng.randint(0, V, size=(F, 3)).astype(np.int64),
             hands_componentsl=f32(rng.normal(size=(rows, hd)) * 0.3), hands_componentsr=f32(rng.normal(size=(rows, hd)) * 0.3),
             hands_meanl=f32(rng.normal(size=hd) * 0.2), hands_meanr=f32(rng.normal(size=hd) * 0.2),
             lmk_faces_idx=rng.randint(0, F, size=n_landmarks).astype(np.int64), lmk_bary_coords=f32(bary / bary.sum(1, keepdims=True)))
    return m


def split_shapedirs(shapedirs, num_betas=10, num_expression_coeffs=10):
    """(shape directions, expression directions) as the package slices them: [:, :, :num_betas], and the expression block from 300
    on -- or, for a file with fewer than 400 directions, from 10 to 20 with at most 10 coefficients."""
    sd = np.asarray(shapedirs)
    if sd.ndim < 3:
        sd = sd[:, :, None]
    num_betas = min(num_betas, 10) if sd.shape[-1] < SHAPE_SPACE_DIM else min(num_betas, SHAPE_SPACE_DIM)
    if sd.shape[-1] < SHAPE_SPACE_DIM + EXPRESSION_SPACE_DIM:
        start, end = 10, 20
    else:
        start, end = SHAPE_SPACE_DIM, SHAPE_SPACE_DIM + num_expression_coeffs
    return sd[:, :, :num_betas], sd[:, :, start:end]


def flat_model(model, n_pca=45, use_pca=True, flat_hand_mean=False, num_betas=10, num_expression_coeffs=10):
    """The arrays of the rule set, f64: v_template [V,3], shapedirs [V,3,NB] (shape then expression), posedirs [P,3V], J_regressor
    [J,V], parents [J], weights [V,J], comps [2,n_pca,hd] (None without PCA), mean [3J], plus sizes."""
    d = lambda a: np.asarray(a, dtype=np.float64)
    sd, ed = split_shapedirs(model["shapedirs"], num_betas, num_expression_coeffs)
    V, J = d(model["v_template"]).shape[0], d(model["J_regressor"]).shape[0]
    pd = d(model["posedirs"])
    parents = np.asarray(model["kintree_table"])[0].astype(np.int64).copy()
    parents[0] = -1
    hd = int(np.asarray(model["hands_meanl"]).size)
    mean = np.zeros(3 * J)
    if not flat_hand_mean and hd:
        mean[3 * J - 2 * hd:3 * J - hd], mean[3 * J - hd:] = d(model["hands_meanl"]), d(model["hands_meanr"])
    comps = np.stack([d(model["hands_componentsl"])[:n_pca], d(model["hands_componentsr"])[:n_pca]]) if use_pca else None
    return dict(V=V, J=J, hd=hd, n_pca=n_pca if use_pca else 0, num_betas=sd.shape[-1], num_expr=ed.shape[-1], v_template=d(model["v_template"]),
                shapedirs=np.concatenate([d(sd), d(ed)], -1), posedirs=np.ascontiguousarray(pd.reshape(-1, pd.shape[-1]).T), J_regressor=d(model["J_regressor"]),
                parents=parents, weights=d(model["weights"]), comps=comps, mean=mean, faces=np.asarray(model["f"]).astype(np.int64),
                lmk_faces_idx=np.asarray(model["lmk_faces_idx"]).astype(np.int64), lmk_bary_coords=d(model["lmk_bary_coords"]))


def n_theta(fm):
    return 3 * fm["J"] - 2 * fm["hd"] + 2 * fm["n_pca"] if fm["n_pca"] else 3 * fm["J"]


# ---- forward ----
def assemble(fm, theta):
    theta = np.asarray(theta, dtype=np.float64).reshape(-1)
    if fm["n_pca"]:
        nb = 3 * fm["J"] - 2 * fm["hd"]
        k = fm["n_pca"]
        theta = np.concatenate([theta[:nb], theta[nb:nb + k] @ fm["comps"][0], theta[nb + k:nb + 2 * k] @ fm["comps"][1]])
    return theta + fm["mean"]


def _skew(d):
    K = np.zeros(d.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0], K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -d[..., 2], d[..., 1], d[..., 2], -d[..., 0], -d[..., 1], d[..., 0]
    return K


def rodrigues(r):
    """[J,3] -> [J,3,3]; the angle is the norm of r + 1e-8 (added to each component), the direction r / angle."""
    a = np.sqrt(np.sum((r + 1e-8) ** 2, axis=1))
    K = _skew(r / a[:, None])
    return np.eye(3) + np.sin(a)[:, None, None] * K + (1 - np.cos(a))[:, None, None] * (K @ K)


def rodrigues_backward(r, dR):
    a = np.sqrt(np.sum((r + 1e-8) ** 2, axis=1))
    K = _skew(r / a[:, None])
    s, c = np.sin(a)[:, None, None], np.cos(a)[:, None, None]
    da = np.sum(dR * (c * K + s * (K @ K)), axis=(1, 2))
    Kt = np.swapaxes(K, 1, 2)
    dK = s * dR + (1 - c) * (dR @ Kt + Kt @ dR)
    dd = np.stack([dK[:, 2, 1] - dK[:, 1, 2], dK[:, 0, 2] - dK[:, 2, 0], dK[:, 1, 0] - dK[:, 0, 1]], 1)
    dat = da - np.sum(dd * r, axis=1) / a ** 2
    return dd / a[:, None] + dat[:, None] * (r + 1e-8) / a[:, None]


def _chain(R, Jr, parents):
    G = np.zeros((len(R), 3, 4))
    G[0, :, :3], G[0, :, 3] = R[0], Jr[0]
    for i in range(1, len(R)):
        p = parents[i]
        G[i, :, :3] = G[p, :, :3] @ R[i]
        G[i, :, 3] = G[p, :, :3] @ (Jr[i] - Jr[p]) + G[p, :, 3]
    return G


def forward(fm, coefficients, theta, transl=None):
    """dict(vertices [V,3], joints [J,3], full_pose [3J]) plus what the backward needs."""
    V, J = fm["V"], fm["J"]
    t = np.zeros(3) if transl is None else np.asarray(transl, dtype=np.float64).reshape(3)
    v_shaped = fm["v_template"] + fm["shapedirs"] @ np.asarray(coefficients, dtype=np.float64).reshape(-1)
    Jr = fm["J_regressor"] @ v_shaped
    pose = assemble(fm, theta)
    R = rodrigues(pose.reshape(J, 3))
    feat = (R[1:] - np.eye(3)).reshape(-1)
    v_posed = v_shaped + (feat @ fm["posedirs"]).reshape(V, 3)
    G = _chain(R, Jr, fm["parents"])
    A = G.copy()
    A[:, :, 3] -= np.einsum("jrc,jc->jr", G[:, :, :3], Jr)
    T = np.einsum("vj,jrc->vrc", fm["weights"], A)
    verts = np.einsum("vrc,vc->vr", T[:, :, :3], v_posed) + T[:, :, 3]
    return dict(vertices=verts + t, joints=G[:, :, 3] + t, full_pose=pose, R=R, G=G, A=A, T=T, v_posed=v_posed, J_rest=Jr, transl=t)


def backward(fm, fwd, grad_vertices):
    """(dL/dtheta [NT], dL/dtransl [3]) from dL/dvertices [V,3]; nothing flows to the coefficients or through the joints."""
    J, parents, Jr, R, G = fm["J"], fm["parents"], fwd["J_rest"], fwd["R"], fwd["G"]
    g = np.asarray(grad_vertices, dtype=np.float64).reshape(-1, 3)
    vp1 = np.concatenate([fwd["v_posed"], np.ones((fm["V"], 1))], 1)
    dA = np.einsum("vj,vr,vc->jrc", fm["weights"], g, vp1)
    g_vp = np.einsum("vrc,vr->vc", fwd["T"][:, :, :3], g)
    dfeat = fm["posedirs"] @ g_vp.reshape(-1)
    dG = dA.copy()
    dG[:, :, :3] -= np.einsum("jr,jc->jrc", dA[:, :, 3], Jr)
    dR = np.zeros((J, 3, 3))
    for i in range(J - 1, 0, -1):
        p = parents[i]
        dR[i] = G[p, :, :3].T @ dG[i, :, :3]
        dG[p, :, :3] += dG[i, :, :3] @ R[i].T + np.outer(dG[i, :, 3], Jr[i] - Jr[p])
        dG[p, :, 3] += dG[i, :, 3]
    dR[0] = dG[0, :, :3]
    dR[1:] += dfeat.reshape(J - 1, 3, 3)
    dpose = rodrigues_backward(fwd["full_pose"].reshape(J, 3), dR).reshape(-1)
    if fm["n_pca"]:
        nb, hd = 3 * J - 2 * fm["hd"], fm["hd"]
        dpose = np.concatenate([dpose[:nb], fm["comps"][0] @ dpose[nb:nb + hd], fm["comps"][1] @ dpose[nb + hd:]])
    return dpose, g.sum(0)


def extra_joint_table(fm, vertex_ids=()):
    """(index i64 [E,3], weight f64 [E,3]): the vertex picks as (i, i, i) / (1, 0, 0), then the static landmarks."""
    ids = np.asarray(list(vertex_ids), dtype=np.int64).reshape(-1)
    idx = np.concatenate([np.repeat(ids[:, None], 3, 1), fm["faces"][fm["lmk_faces_idx"]]])
    w = np.concatenate([np.tile([1.0, 0.0, 0.0], (len(ids), 1)), fm["lmk_bary_coords"].reshape(-1, 3)])
    return idx, w


def extra_joints(fwd, idx, w):
    v = fwd["vertices"] - fwd["transl"]
    return np.einsum("ei,eic->ec", w, v[idx]) + fwd["transl"]


def all_joints(fm, fwd, vertex_ids=()):
    return np.concatenate([fwd["joints"], extra_joints(fwd, *extra_joint_table(fm, vertex_ids))])


# ---- the torch form (eager baseline of scripts/time_body_model.py; autograd gives the backward) ----
def torch_model(fm, device, dtype):
    import torch
    keys = ("v_template", "shapedirs", "posedirs", "J_regressor", "weights", "mean")
    tm = {k: torch.as_tensor(fm[k]).to(device=device, dtype=dtype) for k in keys}
    tm["comps"] = None if fm["comps"] is None else torch.as_tensor(fm["comps"]).to(device=device, dtype=dtype)
    tm.update(J=fm["J"], hd=fm["hd"], n_pca=fm["n_pca"], parents=[int(p) for p in fm["parents"]])
    return tm


def torch_forward(tm, coefficients, theta, transl):
    """vertices [V,3] of coefficients [NB], theta [NT], transl [3]: the same arithmetic, one torch op per step."""
    import torch
    J = tm["J"]
    if tm["n_pca"]:
        nb, k = 3 * J - 2 * tm["hd"], tm["n_pca"]
        theta = torch.cat([theta[:nb], theta[nb:nb + k] @ tm["comps"][0], theta[nb + k:] @ tm["comps"][1]])
    r = (theta + tm["mean"]).reshape(J, 3)
    v_shaped = tm["v_template"] + tm["shapedirs"] @ coefficients
    Jr = tm["J_regressor"] @ v_shaped
    angle = torch.norm(r + 1e-8, dim=1, keepdim=True)
    x, y, z = (r / angle).unbind(1)
    zero = torch.zeros_like(x)
    K = torch.stack([zero, -z, y, z, zero, -x, -y, x, zero], 1).reshape(J, 3, 3)
    eye = torch.eye(3, dtype=r.dtype, device=r.device)
    R = eye + torch.sin(angle)[:, :, None] * K + (1 - torch.cos(angle))[:, :, None] * (K @ K)
    v_posed = v_shaped + ((R[1:] - eye).reshape(-1) @ tm["posedirs"]).reshape(-1, 3)
    GR, Gt = [R[0]], [Jr[0]]
    for i in range(1, J):
        p = tm["parents"][i]
        GR.append(GR[p] @ R[i])
        Gt.append(GR[p] @ (Jr[i] - Jr[p]) + Gt[p])
    GR, Gt = torch.stack(GR), torch.stack(Gt)
    A = torch.cat([GR, (Gt - torch.einsum("jrc,jc->jr", GR, Jr))[:, :, None]], 2)
    T = (tm["weights"] @ A.reshape(J, 12)).reshape(-1, 3, 4)
    return torch.einsum("vrc,vc->vr", T[:, :, :3], v_posed) + T[:, :, 3] + transl


# ---- cases and the fixture ----
def rel_dev(x, ref):
    """max|x - ref| / max|ref| (0 / 0 = 0)."""
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    top, scale = float(np.max(np.abs(x - ref), initial=0.0)), float(np.max(np.abs(ref), initial=0.0))
    return 0.0 if top == 0.0 else top / scale


#        name             V     J   NB  n_pca tree      pose             use_pca
CASES = (("moderate",     257,  55, 20, 45,   "random", "moderate",      True),
         ("zero",         257,  55, 20, 45,   "random", "zero",          True),
         ("zero_hands",   257,  55, 20, 45,   "random", "zero_hands",    True),
         ("chain",        257,  55, 20, 45,   "chain",  "moderate",      True),
         ("star",         257,  55, 20, 45,   "star",   "moderate",      True),
         ("pca6",         257,  55, 20, 6,    "random", "moderate",      True),
         ("no_pca",       257,  55, 20, 45,   "random", "moderate",      False),
         ("tiny_model",   63,   5,  1,  6,    "random", "moderate",      True),
         ("smpl_like",    1000, 24, 10, 6,    "random", "moderate",      True),
         ("small_angle",  257,  55, 20, 45,   "random", "small_angle",   True),
         ("near_pi",      257,  55, 20, 45,   "random", "near_pi",       True))
CASE_NAMES = tuple(c[0] for c in CASES)
QUANTITIES = ("vertices", "joints", "grad_pose", "grad_transl")
ILL_CONDITIONED = ("small_angle",)          # inflates the package's own pooled f32 error of grad_pose by more than 10x: a pool of its own
CLASS_V, CLASS_SUBSET = 10475, 512          # the case run through the package's SMPLX class, and how many of its vertices are stored


def case_model(name):
    """(file-style model, flat model) of a golden case, regenerated from its seed."""
    i = CASE_NAMES.index(name)
    _, V, J, NB, n_pca, tree, _, use_pca = CASES[i]
    model = synthetic_model(V, J, NB, n_pca, tree, seed=1000 + i)
    return model, flat_model(model, n_pca=n_pca, use_pca=use_pca)


def case_inputs(name):
    """The seeded inputs of a golden case (f32): coefficients [NB'], theta [NT], transl [3], the upstream gradient g [V,3]."""
    i = CASE_NAMES.index(name)
    _, V, J, NB, n_pca, tree, kind, use_pca = CASES[i]
    _, fm = case_model(name)
    rng = np.random.RandomState(2000 + i)
    nb = 3 * J - 2 * fm["hd"]
    theta = rng.normal(size=n_theta(fm)) * 0.3
    if kind == "zero":
        theta[:] = 0
    elif kind == "zero_hands":
        theta[nb:] = 0
        theta[:3] = 0
    elif kind == "small_angle":
        theta[9:12] = np.array([0.6, -0.5, 0.62]) * 1e-4
    elif kind == "near_pi":
        theta[9:12] = np.array([0.6, -0.5, 0.62449979983984]) * np.pi
    return dict(coefficients=(rng.normal(size=fm["shapedirs"].shape[-1])).astype(np.float32), theta=theta.astype(np.float32),
                transl=rng.uniform(-1, 1, 3).astype(np.float32), g=rng.normal(size=(V, 3)).astype(np.float32))


def load_golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "smplx_golden.npz"), allow_pickle=False)


def class_case():
    """The model and call arguments of the case run through the package's SMPLX class (V = 10 475: the class indexes the vertices of
    its own extra-joint table): (file-style model, kwargs of f32 [1, n] arrays, upstream gradient g [V,3])."""
    model = synthetic_model(CLASS_V, 55, 20, 45, "random", seed=3000, n_faces=2000, n_landmarks=51)
    rng = np.random.RandomState(3001)
    f = lambda n, s: (rng.normal(size=(1, n)) * s).astype(np.float32)
    kw = dict(betas=f(10, 1.0), global_orient=f(3, 0.3), body_pose=f(63, 0.3), left_hand_pose=f(45, 0.3), right_hand_pose=f(45, 0.3),
              transl=f(3, 0.5), expression=f(10, 1.0), jaw_pose=f(3, 0.2), leye_pose=f(3, 0.2), reye_pose=f(3, 0.2))
    return model, kw, rng.normal(size=(CLASS_V, 3)).astype(np.float32)


def class_theta(kw):
    order = ("global_orient", "body_pose", "jaw_pose", "leye_pose", "reye_pose", "left_hand_pose", "right_hand_pose")
    return np.concatenate([np.asarray(kw[k], dtype=np.float64).reshape(-1) for k in order])


def class_subset():
    return np.random.RandomState(3002).choice(CLASS_V, CLASS_SUBSET, replace=False)
