"""What the tests of the batched ComA objective (coma_app_objective_batch_f32, coma_amd.app.ComaObjective on [N,V,3]) share: the
bodies of a batch and the refusal table of the entry point.  CPU-importable; not product code."""
import numpy as np
import torch

from tests import app_ref

OUTPUT_ARGS = ("terms", "grad_orientation", "grad_contact", "workspace")
HOST_ARGS = ("obj_normal", "principle_vec", "sub_principle_vec")
MAX_BATCH = 1024


def batch_vertices(case, N, seed):
    """f32 [N,V,3]: the case's vertices under N distinct rigid motions (body 0 unmoved; the others a rotation of up to 0.3 rad about a
    seeded axis through the mesh's centre and a shift of up to 0.1) plus seeded noise of 1e-3 of the mesh's extent, so that every body
    gives other numbers.  Each body is redrawn until it keeps the argmin gaps of app_ref.gaps_ok, as app_ref.make_case does."""
    verts = np.asarray(case["verts"], dtype=np.float64)
    centre, extent = verts.mean(0), float(np.ptp(verts, axis=0).max())

    def body(n):
        for attempt in range(1000):
            rng = np.random.default_rng([seed, n, attempt])
            axis = rng.normal(size=3)
            r = torch.as_tensor(axis / np.linalg.norm(axis) * rng.uniform(0.05, 0.3) * (n > 0))
            moved = (verts - centre) @ app_ref.rodrigues(r).numpy().T + centre + rng.uniform(-0.1, 0.1, size=3) * (n > 0)
            b = (moved + 1e-3 * extent * rng.uniform(-1, 1, size=verts.shape)).astype(np.float32)
            if app_ref.gaps_ok(dict(case, verts=b)):
                return b
        raise RuntimeError(f"no seed keeps the distance gaps for body {n}")
    return np.stack([body(n) for n in range(N)])


def refusal_table(lib, V=145, F=242, k=20, N=3):
    """entry point -> (accepted base, [(text of the refusal, change), ...]) for tests/domain_kit.check_refusals.  The three host
    vectors of the base are the kit's (0, 0, 1): every row here is refused before they are looked at."""
    from tests.domain_kit import PTR, Off
    ws = lib.coma_app_objective_batch_workspace_bytes(V, F, k, N)
    assert ws > 0 and ws % 16 == 0
    base = dict(verts=PTR, faces=PTR, vf_offsets=PTR, vf_faces=PTR, V=V, F=F, orientation_gt=PTR, obj_normal=PTR, principle_vec=PTR,
                sub_principle_vec=PTR, eps=1e-6, selected=PTR, targets=PTR, k=k, N=N, terms=PTR, grad_orientation=PTR, grad_contact=PTR,
                workspace=PTR, workspace_bytes=ws)
    nulls = ("verts", "faces", "vf_offsets", "vf_faces", "orientation_gt", "obj_normal", "principle_vec", "sub_principle_vec", "terms",
             "grad_orientation", "grad_contact", "workspace")
    rows = [("null pointer", {name: None}) for name in nulls]
    rows += [("null pointer (selected / targets with k > 0)", dict(selected=None)), ("null pointer (selected / targets with k > 0)", dict(targets=None)),
             ("bad sizes V=0", dict(V=0)), ("bad sizes V=145 F=0", dict(F=0)), (f"k={V + 1} outside [0, V={V}]", dict(k=V + 1)),
             ("k=-1 outside", dict(k=-1)), ("eps must be finite", dict(eps=-1.0)), ("eps must be finite", dict(eps=float("nan"))),
             (f"N=0 outside [1, {MAX_BATCH}]", dict(N=0)), (f"N={MAX_BATCH + 1} outside [1, {MAX_BATCH}]", dict(N=MAX_BATCH + 1)),
             ("N=-2 outside", dict(N=-2)), (f"workspace of {ws - 1} bytes, {ws} needed", dict(workspace_bytes=ws - 1)),
             ("workspace of 0 bytes", dict(workspace_bytes=0)), ("workspace must be 16-byte aligned", dict(workspace=Off(4))),
             # the order: a null pointer before the sizes, the sizes before eps, eps before N, N before the workspace
             ("null pointer", dict(verts=None, V=0, N=0)), ("bad sizes V=0", dict(V=0, eps=-1.0, N=0)), ("eps must be finite", dict(eps=-1.0, N=0)),
             ("N=0 outside", dict(N=0, workspace_bytes=0))]
    return {"coma_app_objective_batch_f32": (base, rows)}
