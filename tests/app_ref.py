"""The project's own restatement of the optimisation app's ComA objective (rule set: include/coma_hip.h, "The optimisation app's
ComA objective"), in torch on the CPU with autograd for the gradients.  f64 is the yardstick; the dtype follows the vertices so that
the golden generator can also run it in f32.  Pinned against the reference's own functions executed in f64
(tests/golden/app_objective_golden.npz, R64) by tests/test_app_objective_host.py.

Also here: the stand-ins the tests use for the app's third-party hooks (a rigid body model, a pose decoder and an angle prior that
contribute nothing) and the seeded grid mesh."""
from types import SimpleNamespace

import numpy as np
import torch


# ---- the objective ----
def _unit(v, eps):
    return v / (torch.sqrt(torch.sum(v * v, dim=-1, keepdim=True)) + eps)


def canonicalisation_matrix(b, p, sub_p, eps, dtype=torch.float64):
    """f = M a for the one column b; the b_cross of the reference as written ([0][0] = b0 set, [2][1] = b0 not)."""
    b, p, s = (_unit(torch.as_tensor(np.asarray(x, dtype=np.float32)).to(dtype).reshape(1, 3), eps)[0] for x in (b, p, sub_p))
    bp = torch.dot(b, p)
    eye = torch.eye(3, dtype=dtype)
    if float(1 + bp) < eps:
        return 2 * torch.outer(s, s) - eye
    B = torch.zeros(3, 3, dtype=dtype)
    B[0, 0], B[0, 1], B[0, 2], B[1, 0], B[1, 2], B[2, 0] = b[0], -b[2], b[1], b[2], -b[0], -b[1]
    c = B @ p
    return torch.outer(c, c) / (1 + bp) + bp * eye + torch.outer(p, b) - torch.outer(b, p)


def vertex_normal_sums(verts, faces):
    v0, v1, v2 = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    n = torch.cross(v1 - v0, v2 - v0, dim=1)
    N = torch.zeros_like(verts)
    for s in range(3):
        N = N.index_add(0, faces[:, s], n)
    return N


def orientation_term(verts, faces, gt, M, eps):
    N = vertex_normal_sums(verts, faces)
    n0 = torch.sqrt(torch.sum(N * N, dim=1, keepdim=True))
    live = n0[:, 0] > 0
    ez = torch.zeros_like(N)
    ez[:, 2] = 1
    N = torch.where(live[:, None], N, ez)                      # a zero normal sum: no share in the term, no gradient
    n1 = N / torch.sqrt(torch.sum(N * N, dim=1, keepdim=True)).clamp_min(1e-6)
    a = _unit(_unit(n1, eps), eps)
    f = a @ M.T
    fh = f / torch.sqrt(torch.sum(f * f, dim=1, keepdim=True))
    t = 1 - (torch.sum(gt * fh, dim=1) + 1) / 2
    t = torch.where(live & ~torch.isnan(t), t, torch.zeros_like(t))
    return t.sum() / verts.shape[0]


def contact_term(verts, sel, targets):
    k = int(len(sel))
    if k == 0:
        return verts.sum() * 0
    A = verts[sel]
    with torch.no_grad():
        d = A[:, None, :] - targets[None, :, :]
        D = torch.sqrt((d[..., 0] ** 2 + d[..., 1] ** 2) + d[..., 2] ** 2).numpy()
        j_of_i, i_of_j = np.argmin(D, axis=1), np.argmin(D, axis=0)            # NumPy: the first minimum

    def lengths(x):
        sq = (x[:, 0] ** 2 + x[:, 1] ** 2) + x[:, 2] ** 2
        pos = sq > 0
        return torch.where(pos, torch.sqrt(torch.where(pos, sq, torch.ones_like(sq))), torch.zeros_like(sq))   # zero distance: zero gradient
    return lengths(A - targets[j_of_i]).sum() / k + lengths(A[i_of_j] - targets).sum() / k


def objective(verts, faces, gt, obj_normal, p, sub_p, eps, sel, targets):
    """(orientation term, contact term) as tensors of verts' graph and dtype; the constants are cast to that dtype."""
    dt = verts.dtype
    c = lambda x: torch.as_tensor(np.asarray(x, dtype=np.float32)).to(dt)
    faces = torch.as_tensor(np.asarray(faces, dtype=np.int64))
    sel = torch.as_tensor(np.asarray(sel, dtype=np.int64))
    M = canonicalisation_matrix(obj_normal, p, sub_p, eps, dt)
    return orientation_term(verts, faces, c(gt), M, eps), contact_term(verts, sel, c(targets).reshape(-1, 3))


def evaluate(verts, faces, gt, obj_normal, p, sub_p, eps, sel, targets, dtype=torch.float64):
    """NumPy in, NumPy out: dict(terms [2], grad_orientation [V,3], grad_contact [V,3])."""
    v = torch.as_tensor(np.asarray(verts, dtype=np.float32)).to(dtype).requires_grad_(True)
    t_o, t_c = objective(v, faces, gt, obj_normal, p, sub_p, eps, sel, targets)
    g_o, = torch.autograd.grad(t_o, v, retain_graph=True)
    g_c, = torch.autograd.grad(t_c, v, allow_unused=True)
    g_c = torch.zeros_like(v) if g_c is None else g_c
    return dict(terms=np.array([float(t_o.detach()), float(t_c.detach())]), grad_orientation=g_o.numpy(), grad_contact=g_c.numpy())


def rel_dev(x, ref):
    """max|x - ref| / max|ref| (0 / 0 = 0)."""
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    top, scale = float(np.max(np.abs(x - ref), initial=0.0)), float(np.max(np.abs(ref), initial=0.0))
    return 0.0 if top == 0.0 else top / scale


# ---- seeded inputs ----
def grid_mesh(n, seed, extent=2.0):
    """An n x n perturbed, bumpy grid plus ONE isolated vertex (the last): verts f32 [n*n + 1, 3], faces i64 [2 (n-1)^2, 3]."""
    rng = np.random.default_rng(seed)
    step = extent / (n - 1)
    ij = np.stack(np.meshgrid(np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 2).astype(np.float64)
    xy = ij * step + rng.uniform(-0.2, 0.2, size=ij.shape) * step
    z = 0.15 * np.sin(3.0 * xy[:, 0]) * np.cos(2.0 * xy[:, 1]) + rng.uniform(-0.1, 0.1, size=len(xy)) * step
    verts = np.concatenate([np.column_stack([xy - extent / 2, z]), [[0.3, -0.2, 0.9]]]).astype(np.float32)
    idx = np.arange(n * n).reshape(n, n)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    faces = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)]).astype(np.int64)
    return verts, faces


def unit_rows(rng, n):
    x = rng.normal(size=(n, 3))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


GAP = 1e-4


def gaps_ok(case):
    """Every row's smallest and second-smallest distance (to DISTINCT points) differ by more than GAP, in both directions."""
    A = case["verts"][case["sel"]].astype(np.float64)
    B = np.unique(case["obj_verts"][case["objects"]].astype(np.float64), axis=0)
    D = np.linalg.norm(A[:, None] - B[None], axis=-1)
    for M in (D, D.T):
        if M.shape[1] >= 2:
            two = np.partition(M, 1, axis=1)[:, :2]
            if np.min(two[:, 1] - two[:, 0]) <= GAP:
                return False
    return True


def make_case(mesh, k, seed, O=50, b=None, p=(0, 0, 1), sub_p=(0, 1, 0), eps=1e-6):
    verts, faces = mesh
    V = len(verts)
    for attempt in range(1000):
        rng = np.random.default_rng([seed, attempt])
        obj_verts = (rng.uniform(-1.0, 1.0, size=(O, 3)) * [1.0, 1.0, 0.3] + [0.0, 0.0, 0.4]).astype(np.float32)
        obj_normals = unit_rows(rng, O)
        ref_index = int(rng.integers(0, O))
        if b is not None:
            obj_normals[ref_index] = np.asarray(b, dtype=np.float32)
        case = dict(verts=verts, faces=faces, gt=unit_rows(rng, V), obj_verts=obj_verts, obj_normals=obj_normals, ref_index=ref_index,
                    p=np.asarray(p, dtype=np.float32), sub_p=np.asarray(sub_p, dtype=np.float32), eps=float(eps),
                    sel=np.sort(rng.choice(V, size=k, replace=False)).astype(np.int64), objects=rng.integers(0, O, size=k).astype(np.int64))
        if gaps_ok(case):
            return case
    raise RuntimeError(f"no seed gives distance gaps above {GAP} for k = {k}")


# ---- stand-ins for the app's third-party hooks ----
def rodrigues(r):
    """Rotation matrix of the axis-angle vector r [3]; differentiable at r = 0 (the angle is taken of r + 1e-8)."""
    angle = torch.sqrt(torch.sum((r + 1e-8) ** 2))
    x, y, z = (r / angle).unbind()
    zero = torch.zeros_like(x)
    K = torch.stack([torch.stack([zero, -z, y]), torch.stack([z, zero, -x]), torch.stack([-y, x, zero])])
    return torch.eye(3, dtype=r.dtype, device=r.device) + torch.sin(angle) * K + (1 - torch.cos(angle)) * (K @ K)


class RigidBody:
    """Body-model stand-in: the template rotated by `global_orient` (Rodrigues) plus `transl`; every other parameter is ignored."""

    def __init__(self, template, faces):
        self.template, self.faces = template, np.asarray(faces, dtype=np.int64)

    def __call__(self, global_orient=None, transl=None, **_):
        return SimpleNamespace(vertices=(self.template @ rodrigues(global_orient[0]).T + transl)[None])


class NullPoseDecoder:
    """Pose-decoder stand-in: a 32-number embedding that decodes to a zero body pose (but stays in the graph)."""

    def __init__(self, dtype=torch.float32, device="cpu"):
        self.w = torch.zeros(32, 63, dtype=dtype, device=device)

    def encode(self, pose):
        return SimpleNamespace(mean=pose[:, :32] * 0)

    def decode(self, embedding, output_type="aa"):
        return (embedding @ self.w).view(1, 21, 3)


def null_angle_prior(body_pose):
    return body_pose[:, :4] * 0


# ---- the fixture ----
def load_golden():
    """(npz, meta) of tests/golden/app_objective_golden.npz; meta: per case dict(mesh, k, eps, ref_index, ...)."""
    import json
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "app_objective_golden.npz"), allow_pickle=False)
    return g, json.loads(str(g["meta_json"]))


def golden_case(g, meta, name):
    """The inputs of one case as the arguments of `evaluate` / ComaObjective, plus its recorded results (r64_*, r32_*)."""
    m = meta[name]
    c = {key.split("__", 1)[1]: g[key] for key in g.files if key.startswith(name + "__")}
    c.update(verts=g[f"mesh_{m['mesh']}__verts"], faces=g[f"mesh_{m['mesh']}__faces"].astype(np.int64), eps=float(m["eps"]),
             obj_normal=c["obj_normals"][m["ref_index"]], targets=c["obj_verts"][c["objects"]])
    return c


CASES = ("small_k1", "small_k7", "small_k20", "small_k25", "small_k60", "large_k300", "large_k1000", "opposite", "opposite_replacer", "near",
         "tilted")
QUANTITIES = ("term_orientation", "term_contact", "grad_orientation", "grad_contact")


def deviations(result, case, which="r64"):
    """rel_dev of a result dict(terms, grad_orientation, grad_contact) against the recorded one, per quantity."""
    return dict(term_orientation=rel_dev(result["terms"][0], case[f"{which}_terms"][0]), term_contact=rel_dev(result["terms"][1], case[f"{which}_terms"][1]),
                grad_orientation=rel_dev(result["grad_orientation"], case[f"{which}_grad_orientation"]),
                grad_contact=rel_dev(result["grad_contact"], case[f"{which}_grad_contact"]))
