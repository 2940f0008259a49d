"""The seeded cases of the BATCHED SMPL-X body model (DeviceSMPLX(batch_size=N), coma_smplx_*_batch_f32) and their fixture
tests/golden/smplx_batch_golden.npz (written by tests/golden/make_golden_smplx_batch.py from the third-party package's own lbs and
SMPLX class at batch_size = 3).  The arithmetic is tests/smplx_ref.py called once per body: the batch adds no rule.

Two models, each with shared and with per-body coefficients:
  lbs    V = 300 (skinning tiles 128, 128, 44; 3V = 900 is no multiple of 256), J = 55, n_pca = 6, through the package's lbs.lbs;
  class  V = 10 475 (the package's class picks the vertices of its own extra-joint table), n_pca = 45, through SMPLX(batch_size=3).
The three bodies have distinct poses: body 0 at zero pose, body 1 moderate, body 2 moderate with one joint near |r| = pi."""
import os

import numpy as np

from tests import smplx_ref as S

N = 3
LBS_V, LBS_J, LBS_NB, LBS_PCA = 300, 55, 20, 6
CLASS_SUBSET = 256
MODELS = ("lbs", "class")
SHARING = ("shared", "per_body")
CASES = tuple(f"{m}_{s}" for m in MODELS for s in SHARING)
QUANTITIES = S.QUANTITIES
POSE_KEYS = ("global_orient", "body_pose", "jaw_pose", "leye_pose", "reye_pose", "left_hand_pose", "right_hand_pose")
_models = {}


def model_of(kind):
    """(file-style model, flat model) of "lbs" or "class", regenerated from its seed and kept."""
    if kind not in _models:
        if kind == "lbs":
            model = S.synthetic_model(LBS_V, LBS_J, LBS_NB, LBS_PCA, "random", seed=4000)
            _models[kind] = (model, S.flat_model(model, n_pca=LBS_PCA))
        else:
            model = S.class_case()[0]
            _models[kind] = (model, S.flat_model(model, n_pca=45))
    return _models[kind]


def case_inputs(case):
    """The seeded inputs of a case (f32): coefficients [1 or N, 20], theta [N, NT], transl [N, 3], the upstream gradient g [N, V, 3]
    (class: zero outside class_subset())."""
    kind, sharing = case.split("_", 1)
    _, fm = model_of(kind)
    rng = np.random.RandomState(4100 + CASES.index(case))
    theta = rng.normal(size=(N, S.n_theta(fm))) * 0.3
    theta[0] = 0
    theta[2, 9:12] = np.array([0.6, -0.5, 0.62449979983984]) * np.pi
    coef = rng.normal(size=(N if sharing == "per_body" else 1, fm["shapedirs"].shape[-1]))
    g = rng.normal(size=(N, fm["V"], 3))
    if kind == "class":
        keep = np.zeros(fm["V"], bool)
        keep[class_subset()] = True
        g[:, ~keep] = 0
    return dict(coefficients=coef.astype(np.float32), theta=theta.astype(np.float32), transl=rng.uniform(-1, 1, (N, 3)).astype(np.float32),
                g=g.astype(np.float32))


def class_subset():
    return np.sort(np.random.RandomState(4002).choice(S.CLASS_V, CLASS_SUBSET, replace=False))


def split_theta(fm, theta):
    """theta [N, NT] -> the seven pose arguments [N, n] in the package's order (n_pca > 0)."""
    sizes = (3, 3 * fm["J"] - 2 * fm["hd"] - 12, 3, 3, 3, fm["n_pca"], fm["n_pca"])
    out, at = {}, 0
    for key, n in zip(POSE_KEYS, sizes):
        out[key] = theta[:, at:at + n]
        at += n
    assert at == theta.shape[1]
    return out


def restated(case):
    """tests/smplx_ref.py once per body -> the stored quantities: vertices [N, V or subset, 3], joints [N, J (+ landmarks), 3],
    full_pose [N, 3J], grad_pose [N, NT], grad_transl [N, 3]."""
    kind = case.split("_", 1)[0]
    _, fm = model_of(kind)
    inp = case_inputs(case)
    out = {q: [] for q in QUANTITIES + ("full_pose",)}
    for n in range(N):
        coef = inp["coefficients"][n if len(inp["coefficients"]) > 1 else 0]
        fwd = S.forward(fm, coef, inp["theta"][n], inp["transl"][n])
        g_pose, g_transl = S.backward(fm, fwd, inp["g"][n])
        joints = fwd["joints"]
        if kind == "class":                                     # the landmarks; the package's 21 vertex picks are not shipped
            joints = np.concatenate([joints, S.extra_joints(fwd, *S.extra_joint_table(fm))])
        for q, v in (("vertices", fwd["vertices"][class_subset()] if kind == "class" else fwd["vertices"]), ("joints", joints),
                     ("full_pose", fwd["full_pose"]), ("grad_pose", g_pose), ("grad_transl", g_transl)):
            out[q].append(v)
    return {q: np.stack(v) for q, v in out.items()}


def golden_joints(golden, case, which="r64"):
    """The stored joints without the package's 21 vertex picks (class: [55 posed | 51 landmarks])."""
    j = golden[f"{case}__{which}_joints"]
    return np.concatenate([j[:, :55], j[:, 76:]], 1) if case.startswith("class") else j


def load_golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "smplx_batch_golden.npz"), allow_pickle=False)


# ---- the refusals of the batched entry points (tests/domain_kit.check_refusals runs them: on the CPU and, outputs watched, on the GPU) ----
C_CHUNK = 8                     # C: the bodies one sweep over posedirs serves (kChunk of coma_amd/csrc/smplx.hip)
OUTPUT_ARGS = ("vertices", "joints", "full_pose", "saved", "workspace", "grad_theta", "grad_transl", "out")


def refusal_table(lib, parents, bad_parents):
    """entry point -> (accepted base, [(text of the refusal, change), ...]) for V = 300, J = 55, hand_dim = 45, n_pca = 6, N = 3.
    parents / bad_parents: HOST i32 arrays (ctypes), a valid tree and one whose joint 7 has parent 9."""
    from tests.domain_kit import PTR, Off
    V, J, N = 300, 55, 3
    shape_bytes = lib.coma_smplx_shape_state_bytes(V, J)
    saved, ws, gws = (f(V, J, N) for f in (lib.coma_smplx_batch_saved_bytes, lib.coma_smplx_batch_workspace_bytes, lib.coma_smplx_batch_grad_workspace_bytes))
    assert saved == N * lib.coma_smplx_saved_bytes(V, J) and ws > 0 and gws > 0
    model = dict(posedirs=PTR, weights=PTR, parents=parents, hand_components=PTR, V=V, J=J, hand_dim=45, n_pca=6, N=N, shape_state=PTR, shape_stride=0)
    common = [("N=0 outside [1, 1024]", dict(N=0)), ("N=1025 outside [1, 1024]", dict(N=1025)), ("N=-3 outside", dict(N=-3)),
              ("shape_stride=16 must be 0", dict(shape_stride=16)), (f"shape_stride={shape_bytes + 8} must be 0", dict(shape_stride=shape_bytes + 8)),
              ("shape state must be 16-byte aligned", dict(shape_state=Off(8))),
              ("null pointer", dict(posedirs=None)), ("null pointer", dict(weights=None)), ("null pointer", dict(parents=None)),
              ("null pointer", dict(shape_state=None)), ("null pointer", dict(saved=None)), ("null pointer", dict(workspace=None)),
              ("null pointer (hand_components", dict(hand_components=None)),
              ("V=0 must lie", dict(V=0)), ("V=16777217 must lie", dict(V=(1 << 24) + 1)), ("J=0 in", dict(J=0)), ("J=65 in", dict(J=65)),
              ("n_pca=-1 outside", dict(n_pca=-1)), ("n_pca=65 outside", dict(n_pca=65)), ("hand_dim=44 must be", dict(hand_dim=44)),
              ("hand_dim=84 must be", dict(hand_dim=84)), ("parent 9 of joint 7", dict(parents=bad_parents)),
              ("saved state of 16 bytes", dict(saved_bytes=16)), (f"saved state of {saved - 16} bytes", dict(saved_bytes=saved - 16)),
              ("saved state must be 16-byte aligned", dict(saved=Off(8))), ("workspace of 16 bytes", dict(workspace_bytes=16)),
              ("workspace must be 16-byte aligned", dict(workspace=Off(4)))]
    forward = dict(model, theta=PTR, transl=PTR, pose_mean=PTR, vertices=PTR, joints=PTR, full_pose=PTR, saved=PTR, saved_bytes=saved, workspace=PTR,
                   workspace_bytes=ws)
    backward = dict(model, grad_vertices=PTR, grad_joints=PTR, grad_full_pose=PTR, extra_index=PTR, extra_weight=PTR, E=5, saved=PTR, saved_bytes=saved,
                    grad_theta=PTR, grad_transl=PTR, workspace=PTR, workspace_bytes=gws)
    extra = dict(vertices=PTR, transl=PTR, vertex_index=PTR, vertex_weight=PTR, V=V, E=5, N=N, out=PTR)
    return {
        "coma_smplx_forward_batch_f32": (forward, common + [
            ("null pointer", dict(theta=None)), ("null pointer", dict(vertices=None)), ("null pointer", dict(joints=None)),
            (f"workspace of {ws - 16} bytes", dict(workspace_bytes=ws - 16))]),
        "coma_smplx_backward_batch_f32": (backward, common + [
            ("null pointer", dict(grad_theta=None)), ("null pointer", dict(grad_transl=None)), ("E=-1 outside [0, 4096]", dict(E=-1)),
            ("E=4097 outside [0, 4096]", dict(E=4097)), ("null pointer (the extra-joint tables", dict(extra_index=None)),
            ("null pointer (the extra-joint tables", dict(extra_weight=None)), (f"workspace of {gws - 16} bytes", dict(workspace_bytes=gws - 16))]),
        "coma_smplx_extra_joints_batch_f32": (extra, [
            ("N=0 outside [1, 1024]", dict(N=0)), ("N=1025 outside [1, 1024]", dict(N=1025)), ("null pointer", dict(vertices=None)),
            ("null pointer", dict(vertex_index=None)), ("null pointer", dict(vertex_weight=None)), ("null pointer", dict(out=None)),
            ("bad sizes V=0", dict(V=0)), ("bad sizes V=300 E=-1", dict(E=-1))]),
    }
