"""The project's own restatement of VPoser's decoder (forward and backward), its encoder (forward) and the SMPLify angle prior (rule
set: include/coma_hip.h, "VPoser's pose decoder"): NumPy in f64; and the seeded synthetic weight sets and cases.  Pinned against the
reference's own VPoser class, rotation_matrix_to_angle_axis and SMPLifyAnglePrior executed in f64 (tests/golden/vposer_golden.npz,
R64) by tests/test_vposer_host.py.

A weight set is a dict with the keys of a VPoser snapshot (a torch state_dict), f32 arrays, regenerated from its seed: the fixture
holds results only."""
import os

import numpy as np

SLOPE, NORM_EPS, DIAG_EPS, BN_EPS = 0.2, 1e-12, 1e-6, 1e-5
PRIOR_INDEX, PRIOR_SIGN = (55, 58, 12, 15), (1.0, -1.0, -1.0, -1.0)      # the reference's vectors, before its "- 3"
LAYERS = ("bodyprior_enc_fc1", "bodyprior_enc_fc2", "bodyprior_enc_mu", "bodyprior_enc_logvar", "bodyprior_dec_fc1", "bodyprior_dec_fc2",
          "bodyprior_dec_out")
NORMS = ("bodyprior_enc_bn1", "bodyprior_enc_bn2")


# ---- the seeded weights ----
def _rot(axis, angle):
    c, s = np.cos(angle), np.sin(angle)
    return {0: np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), 1: np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            2: np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[axis]


def six_d(R):
    """The decoder output whose Gram-Schmidt frame is R: its first two columns, interleaved as the [3,2] view reads them."""
    return np.stack([R[:, 0], R[:, 1]], 1).reshape(-1)


def synthetic_weights(H, D, NJ, seed, kind="random"):
    """kind: random (torch's Linear range, uniform +-1/sqrt(in), everywhere), near_rest / small_angle (output bias = the identity's
    6-D form plus noise; small_angle also scales the output layer by 1e-2), branches / cos_negative (output bias = rotations by +2.5 /
    -2.5 rad about x, y, z and a small one, joint j taking design j % 4: the four selector branches, and q0 < 0 for the negative angles)."""
    rng = np.random.RandomState(seed)
    F = 3 * NJ
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    shapes = dict(bodyprior_enc_fc1=(H, F), bodyprior_enc_fc2=(H, H), bodyprior_enc_mu=(D, H), bodyprior_enc_logvar=(D, H),
                  bodyprior_dec_fc1=(H, D), bodyprior_dec_fc2=(H, H), bodyprior_dec_out=(6 * NJ, H))
    w = {}
    for name in LAYERS:
        out, inn = shapes[name]
        w[name + ".weight"] = f32(rng.uniform(-1, 1, (out, inn)) / np.sqrt(inn))
        w[name + ".bias"] = f32(rng.uniform(-1, 1, out) / np.sqrt(inn))
    for name, C in zip(NORMS, (F, H)):
        w[name + ".weight"], w[name + ".bias"] = f32(rng.uniform(0.5, 1.5, C)), f32(rng.normal(size=C) * 0.1)
        w[name + ".running_mean"], w[name + ".running_var"] = f32(rng.normal(size=C) * 0.1), f32(rng.uniform(0.5, 1.5, C))
    if kind != "random":
        sign = -1.0 if kind == "cos_negative" else 1.0
        designs = [np.eye(3)] * 4 if kind in ("near_rest", "small_angle") else [_rot(0, 2.5 * sign), _rot(1, 2.5 * sign), _rot(2, 2.5 * sign),
                                                                              _rot(0, 0.3 * sign)]
        noise = 1e-3 if kind == "small_angle" else 0.05
        bias = np.concatenate([six_d(designs[j % 4]) for j in range(NJ)]) + rng.normal(size=6 * NJ) * noise
        w["bodyprior_dec_out.bias"] = f32(bias)
        if kind == "small_angle":
            w["bodyprior_dec_out.weight"] = f32(w["bodyprior_dec_out.weight"] * 1e-2)
    return w


# ---- the decoder ----
def _lrelu(x):
    return np.where(x > 0, x, SLOPE * x)


def _linear(w, name, x):
    return x @ np.asarray(w[name + ".weight"], dtype=np.float64).T + np.asarray(w[name + ".bias"], dtype=np.float64)


def _norm(v):
    return np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


# per branch: the signs of (T00, T11, T22) in t, the slot of t among the candidates, and the other three slots as (slot, a, b, sign):
# cand[slot] = T[a] + sign T[b], with a, b index pairs into T
_BRANCH = ((+1, -1, -1, 1, ((0, (1, 2), (2, 1), -1), (2, (0, 1), (1, 0), +1), (3, (2, 0), (0, 2), +1))),
           (-1, +1, -1, 2, ((0, (2, 0), (0, 2), -1), (1, (0, 1), (1, 0), +1), (3, (1, 2), (2, 1), +1))),
           (-1, -1, +1, 3, ((0, (0, 1), (1, 0), -1), (1, (2, 0), (0, 2), +1), (2, (1, 2), (2, 1), +1))),
           (+1, +1, +1, 0, ((1, (1, 2), (2, 1), -1), (2, (2, 0), (0, 2), -1), (3, (0, 1), (1, 0), -1))))


def select_branch(T):
    """T [M,3,3], the TRANSPOSED rotation (rows b1, b2, b3) -> branch id [M]."""
    low = T[:, 2, 2] < DIAG_EPS
    return np.where(low, np.where(T[:, 0, 0] > T[:, 1, 1], 0, 1), np.where(T[:, 0, 0] < -T[:, 1, 1], 2, 3)).astype(np.int8)


def tail_forward(o, branch=None):
    """o [M,6] -> dict(aa [M,3], T [M,3,3], branch [M], and what the backward reads)."""
    c0, c1 = o[:, 0::2], o[:, 1::2]
    l0 = _norm(c0)
    n0 = np.maximum(l0, NORM_EPS)
    b1 = c0 / n0[:, None]
    d = _dot(b1, c1)
    u = c1 - d[:, None] * b1
    l1 = _norm(u)
    n1 = np.maximum(l1, NORM_EPS)
    b2 = u / n1[:, None]
    b3 = np.cross(b1, b2)
    T = np.stack([b1, b2, b3], 1)
    branch = select_branch(T) if branch is None else np.asarray(branch)
    t, cand = np.zeros(len(o)), np.zeros((len(o), 4))
    for k, (s0, s1, s2, slot, rest) in enumerate(_BRANCH):
        m = branch == k
        tk = ((1.0 + s0 * T[m, 0, 0]) + s1 * T[m, 1, 1]) + s2 * T[m, 2, 2]
        t[m] = tk
        cand[m, slot] = tk
        for sl, a, b, sg in rest:
            cand[m, sl] = T[m, a[0], a[1]] + sg * T[m, b[0], b[1]]
    q = cand / np.sqrt(t)[:, None] * 0.5
    s2 = (q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3]
    s = np.sqrt(s2)
    neg = q[:, 0] < 0
    tt = 2.0 * np.where(neg, np.arctan2(-s, -q[:, 0]), np.arctan2(s, q[:, 0]))
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where(s2 > 0, tt / s, 2.0)
    return dict(aa=q[:, 1:] * k[:, None], T=T, branch=branch, q=q, t=t, s2=s2, s=s, tt=tt, k=k, n0=n0, n1=n1, free0=l0 >= NORM_EPS,
                free1=l1 >= NORM_EPS, dot=d, c1=c1)


def tail_backward(f, ga):
    """dL/do [M,6] from dL/daa [M,3]; at s2 == 0 the finite gradient of the k = 2 branch."""
    q, k, s2, s, tt, T = f["q"], f["k"], f["s2"], f["s"], f["tt"], f["T"]
    M = len(q)
    gq = np.zeros((M, 4))
    gq[:, 1:] = ga * k[:, None]
    gk = (ga[:, 0] * q[:, 1] + ga[:, 1] * q[:, 2]) + ga[:, 2] * q[:, 3]
    m = s2 > 0
    gtt = gk[m] / s[m]
    r2 = s2[m] + q[m, 0] ** 2
    gs = -gk[m] * tt[m] / s2[m] + 2.0 * gtt * q[m, 0] / r2
    gq[m, 0] = -2.0 * gtt * s[m] / r2
    gq[m, 1:] += 2.0 * q[m, 1:] * (gs / (2.0 * s[m]))[:, None]
    gc = 0.5 * gq / np.sqrt(f["t"])[:, None]
    gt = -0.5 * np.sum(gq * q, 1) / f["t"]
    g = np.zeros((M, 3, 3))
    for b, (s0, s1, s2_, slot, rest) in enumerate(_BRANCH):
        m = f["branch"] == b
        gtb = gt[m] + gc[m, slot]
        g[m, 0, 0], g[m, 1, 1], g[m, 2, 2] = s0 * gtb, s1 * gtb, s2_ * gtb
        for sl, a, bb, sg in rest:
            g[m, a[0], a[1]] += gc[m, sl]
            g[m, bb[0], bb[1]] += sg * gc[m, sl]
    b1, b2 = T[:, 0], T[:, 1]
    gb1 = g[:, 0] + np.cross(b2, g[:, 2])
    gb2 = g[:, 1] + np.cross(g[:, 2], b1)
    gu = (gb2 - b2 * np.where(f["free1"], _dot(b2, gb2), 0.0)[:, None]) / f["n1"][:, None]
    pu = _dot(gu, b1)
    gc1 = gu - pu[:, None] * b1
    gb1 = gb1 - (f["dot"][:, None] * gu + pu[:, None] * f["c1"])
    gc0 = (gb1 - b1 * np.where(f["free0"], _dot(b1, gb1), 0.0)[:, None]) / f["n0"][:, None]
    go = np.zeros((M, 6))
    go[:, 0::2], go[:, 1::2] = gc0, gc1
    return go


def decode(w, z, branch=None):
    """z [N,D] -> dict(aa [N,3NJ], matrot [N,NJ,9] (R row-major), branch i8 [N,NJ], ...)."""
    z = np.asarray(z, dtype=np.float64)
    N = len(z)
    h1 = _lrelu(_linear(w, "bodyprior_dec_fc1", z))
    h2 = _lrelu(_linear(w, "bodyprior_dec_fc2", h1))
    o = _linear(w, "bodyprior_dec_out", h2)
    f = tail_forward(o.reshape(-1, 6), None if branch is None else np.asarray(branch).reshape(-1))
    NJ = o.shape[1] // 6
    return dict(aa=f["aa"].reshape(N, 3 * NJ), matrot=np.swapaxes(f["T"], 1, 2).reshape(N, NJ, 9), branch=f["branch"].reshape(N, NJ),
                q=f["q"].reshape(N, NJ, 4), h1=h1, h2=h2, o=o, tail=f)


def decode_backward(w, fwd, grad_aa):
    """dL/dz [N,D] from dL/daa [N,3NJ]."""
    d = lambda k: np.asarray(w[k], dtype=np.float64)
    go = tail_backward(fwd["tail"], np.asarray(grad_aa, dtype=np.float64).reshape(-1, 3)).reshape(fwd["o"].shape)
    gh2 = (go @ d("bodyprior_dec_out.weight")) * np.where(fwd["h2"] > 0, 1.0, SLOPE)
    gh1 = (gh2 @ d("bodyprior_dec_fc2.weight")) * np.where(fwd["h1"] > 0, 1.0, SLOPE)
    return gh1 @ d("bodyprior_dec_fc1.weight")


# ---- the encoder ----
def _bn(w, name, x):
    d = lambda k: np.asarray(w[name + k], dtype=np.float64)
    return (x - d(".running_mean")) / np.sqrt(d(".running_var") + BN_EPS) * d(".weight") + d(".bias")


def encode(w, pose):
    """pose [N,3NJ] -> (mean [N,D], scale [N,D])."""
    x = _bn(w, "bodyprior_enc_bn1", np.asarray(pose, dtype=np.float64).reshape(len(pose), -1))
    x = _bn(w, "bodyprior_enc_bn2", _lrelu(_linear(w, "bodyprior_enc_fc1", x)))
    x = _lrelu(_linear(w, "bodyprior_enc_fc2", x))
    lv = _linear(w, "bodyprior_enc_logvar", x)
    with np.errstate(over="ignore"):
        scale = np.where(lv > 20, lv, np.log1p(np.exp(lv)))
    return _linear(w, "bodyprior_enc_mu", x), scale


# ---- the angle prior ----
def prior_vectors(with_global_pose=False):
    return np.asarray(PRIOR_INDEX, dtype=np.int64) - (0 if with_global_pose else 3), np.asarray(PRIOR_SIGN, dtype=np.float64)


def angle_prior(pose, index=None, sign=None):
    if index is None:
        index, sign = prior_vectors()
    return np.exp(np.asarray(pose, dtype=np.float64)[:, index] * sign) ** 2


def angle_prior_backward(pose, grad_out, index=None, sign=None):
    if index is None:
        index, sign = prior_vectors()
    pose = np.asarray(pose, dtype=np.float64)
    g = np.zeros_like(pose)
    for i, (p, s) in enumerate(zip(index, sign)):
        g[:, p] += np.asarray(grad_out, dtype=np.float64)[:, i] * 2.0 * s * np.exp(s * pose[:, p]) ** 2
    return g


# ---- cases and the fixture ----
def rel_dev(x, ref):
    """max|x - ref| / max|ref| (0 / 0 = 0)."""
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    top, scale = float(np.max(np.abs(x - ref), initial=0.0)), float(np.max(np.abs(ref), initial=0.0))
    return 0.0 if top == 0.0 else top / scale


#        name            H    D   NJ  N  weights
CASES = (("random_init", 512, 32, 21, 1, "random"),
         ("near_rest",   512, 32, 21, 1, "near_rest"),
         ("branches",    512, 32, 21, 1, "branches"),
         ("cos_negative", 512, 32, 21, 1, "cos_negative"),
         ("batch3",      512, 32, 21, 3, "random"),
         ("odd",         80,  7,  5,  1, "branches"),
         ("small_angle", 512, 32, 21, 1, "small_angle"))
CASE_NAMES = tuple(c[0] for c in CASES)
QUANTITIES = ("aa", "grad_z", "mean", "scale", "prior", "grad_prior")
# Cases on which the reference's own f32 loses digits get a pool of their own (as tests/smplx_ref.py does).  None here: `small_angle`
# (every joint at about 1e-3 rad) was the candidate, but the Gram-Schmidt frame is built from the small numbers themselves, which f32
# holds to full relative precision; the generator measured 2.2e-7 for its aa against 4.5e-7 for `random_init`.  The generator checks
# that no case stands out by more than 10x.
ILL_CONDITIONED = ()


def case_shape(name):
    _, H, D, NJ, N, kind = CASES[CASE_NAMES.index(name)]
    return dict(H=H, D=D, NJ=NJ, N=N, kind=kind)


def case_weights(name):
    c = case_shape(name)
    return synthetic_weights(c["H"], c["D"], c["NJ"], seed=5000 + CASE_NAMES.index(name), kind=c["kind"])


def case_inputs(name):
    """The seeded inputs of a golden case (f32): z [N,D], g [N,3NJ] (upstream gradient of aa), pose [N,3NJ] (encoder input),
    prior_pose [N,63], prior_g [N,4]."""
    c = case_shape(name)
    rng = np.random.RandomState(6000 + CASE_NAMES.index(name))
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return dict(z=f32(rng.normal(size=(c["N"], c["D"]))), g=f32(rng.normal(size=(c["N"], 3 * c["NJ"]))),
                pose=f32(rng.normal(size=(c["N"], 3 * c["NJ"])) * 0.3), prior_pose=f32(rng.normal(size=(c["N"], 63)) * 0.5),
                prior_g=f32(rng.normal(size=(c["N"], 4))))


def restate(name):
    """Every quantity of a case from the restatement, plus branch and matrot."""
    w, inp = case_weights(name), case_inputs(name)
    fwd = decode(w, inp["z"])
    mean, scale = encode(w, inp["pose"])
    return dict(aa=fwd["aa"], grad_z=decode_backward(w, fwd, inp["g"]), mean=mean, scale=scale, prior=angle_prior(inp["prior_pose"]),
                grad_prior=angle_prior_backward(inp["prior_pose"], inp["prior_g"]), branch=fwd["branch"], matrot=fwd["matrot"], q=fwd["q"])


def load_golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vposer_golden.npz"), allow_pickle=False)
