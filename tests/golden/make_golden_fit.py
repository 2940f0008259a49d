#!/usr/bin/env python
"""Generate tests/golden/app_fit_golden.npz: 20 iterations of the fitting app's Adam loop, from the reference's own parts on the CPU.

Run where a checkout of the reference is available (COMA_REFERENCE, default: a directory `reference` beside this repository):
    python tests/golden/make_golden_fit.py

The reference's loop (src/application/optimize.py:236-307) cannot run as a whole: it needs COAP, pytorch3d, open3d and a GPU.  It is
built here from the parts it is made of, each the reference's OWN code, loaded as the other generators load them:
  * the vendored `smplx` package's SMPLX class (make_golden_smplx.py), created from a synthetic SMPLX_NEUTRAL.npz of the seeded
    257-vertex model.  The class's table of extra-joint vertex ids belongs to the 10 475-vertex template, so its
    vertex_joint_selector gets an empty index buffer -- the package's own idiom for models without such a table; only .joints
    changes, which the loop does not read;
  * the vendored VPoser class and SMPLifyAnglePrior (make_golden_vposer.py), with the seeded `near_rest` weights;
  * the objective's own lines, :274-289 and :295-296 (make_golden_app.py), with their weights;
  * torch.optim.Adam over the parameter set of :236-250 with its initial values, and the loss composition of :292-298.
Everything runs once with every tensor in f32 (R32) and once in f64 (R64).  Nothing of the reference is copied: the fixture holds
the objective's seeded inputs and recorded results -- per case the R64 trajectory of all P parameters, its five loss columns and
their R32 - R64 deviation, the first gradient, the last forward's vertices, and e_ref = max|R32 - R64| over the trajectory.

Cases (tests/fit_ref.CASES), 20 iterations at lr 1e-2 each: `app` (n_pca 45, k = 40, P = 128), `pca6` (n_pca 6, P = 50), `k0` (no
selected vertices: no contact term; the reference's chamfer line raises on an empty selection and is left out there).
Conditions, asserted for every case:
  (a) in R64 every component of the gradient at every iteration has |g| >= 1e-3, 1e5 x Adam's eps, so rounding noise in a gradient
      cannot turn into a step of order lr;
  (b) 4 e_ref <= lr / 10: a missing term or a wrong sign moves a parameter by up to 2 lr in one step, so the tests' bound stays 20 x
      tighter than the smallest wiring mistake.
Also printed: the deviation of the restatement tests/fit_ref.py from R64 (tests/test_app_fit_host.py holds it to 1e-3 e_ref)."""
import importlib.util
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("COMA_REFERENCE") or os.path.join(os.path.dirname(ROOT), "reference")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(REF, "imports", "hand4whole", "common", "utils_hand4whole", "smplx"))

import smplx  # noqa: E402  (the vendored package)

from tests import fit_ref as R  # noqa: E402
from tests import vposer_ref as V  # noqa: E402


def _generator(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


vposer_generator = _generator("make_golden_vposer")          # loads the reference's vposer_smpl.py and prior.py
app_generator = _generator("make_golden_app")                # reads the objective's lines
OUT = os.path.join(HERE, "app_fit_golden.npz")


def run_reference(name, directory, obj, meta, space, loss_src, dtype):
    _, fm, w, n_pca, k, _ = R.case_models(name)
    wt = R.WEIGHTS
    c = lambda x: torch.as_tensor(np.asarray(x, dtype=np.float32)).to(dtype)
    body = smplx.create(model_path=directory, model_type="smplx", num_pca_comps=n_pca, dtype=dtype)
    body.vertex_joint_selector.extra_joints_idxs = torch.zeros(0, dtype=torch.long)
    shape = V.case_shape(R.DECODER)
    vposer = vposer_generator.vposer_smpl.VPoser(num_neurons=shape["H"], latentD=shape["D"], data_shape=[1, shape["NJ"], 3])
    state = {key: torch.as_tensor(v) for key, v in w.items()}
    for bn in V.NORMS:
        state[bn + ".num_batches_tracked"] = torch.tensor(0)
    vposer.load_state_dict(state)
    vposer = vposer.to(dtype).eval()
    angle_prior = vposer_generator.prior_module.SMPLifyAnglePrior(dtype=dtype)

    # the parameter set of optimize.py:236-250
    t_pose_embedding = vposer.encode(torch.zeros(1, 63, dtype=dtype)).mean
    pose_embedding = t_pose_embedding.clone().detach().requires_grad_(True)
    betas, expression = c([R.DEFAULT_BETAS]), torch.zeros(1, 10, dtype=dtype)
    leye_pose, reye_pose = torch.zeros(1, 3, dtype=dtype), torch.zeros(1, 3, dtype=dtype)
    global_orient = torch.nn.Parameter(torch.tensor([[0.0, 0.0, 0.0]], dtype=dtype), requires_grad=True)
    transl = torch.nn.Parameter(torch.tensor([[3.0, 1.0, 0.0]], dtype=dtype), requires_grad=True)
    left_hand_pose = torch.nn.Parameter(torch.zeros((1, n_pca), dtype=dtype), requires_grad=True)
    right_hand_pose = torch.nn.Parameter(torch.zeros((1, n_pca), dtype=dtype), requires_grad=True)
    jaw_pose = torch.nn.Parameter(torch.zeros((1, 3), dtype=dtype))
    params = [global_orient, transl, left_hand_pose, right_hand_pose, pose_embedding]
    optimizer = torch.optim.Adam(params, lr=wt["lr"])
    flat = lambda ts: np.concatenate([t.detach().numpy().reshape(-1) for t in ts]).astype(np.float64)

    lines = loss_src.split("\n")
    assert lines[-1].startswith("contact_loss = chamfer_distance("), lines[-1]
    source = loss_src if k else "\n".join(lines[:-1])
    rows, losses, grads, vertices = [flat(params)], [], [], None
    for _ in range(R.ITERS):
        optimizer.zero_grad()
        body_pose = vposer.decode(pose_embedding, output_type="aa").view(1, -1)
        output = body(betas=betas, global_orient=global_orient, body_pose=body_pose, left_hand_pose=left_hand_pose,
                      right_hand_pose=right_hand_pose, transl=transl, expression=expression, jaw_pose=jaw_pose, leye_pose=leye_pose,
                      reye_pose=reye_pose, return_verts=True, return_full_pose=True)
        vertices = output.vertices * wt["scale_factor"]
        ns = dict(space)
        ns.update(Meshes=app_generator.Meshes, vertices=vertices, faces=torch.as_tensor(fm["faces"]), eps=float(meta["eps"]),
                  obj_normals=c(obj["obj_normals"]), principle_vec=c(obj["p"]), sub_principle_vec=c(obj["sub_p"]),
                  reference_object_vertex_index=int(meta["ref_index"]), relative_orientation_GT=c(obj["gt"]),
                  orientation_weight=wt["orientation_weight"], contact_weight=wt["contact_weight"], selected_human_indices=(obj["sel"],),
                  corresponding_object_indices=obj["objects"], obj_verts=c(obj["obj_verts"]))
        exec(source, ns)
        orientation_loss = ns["orientation_loss"]
        contact_loss = ns["contact_loss"] if k else torch.zeros((), dtype=dtype)
        pprior_loss = (pose_embedding.pow(2).sum() * wt["body_pose_weight"] ** 2) * wt["pprior_weight"]
        angle_prior_loss = torch.sum(angle_prior(body_pose)) * wt["bending_prior_weight"]
        loss = pprior_loss + angle_prior_loss + contact_loss + orientation_loss
        loss.backward()
        grads.append(flat([t.grad for t in params]))
        optimizer.step()
        number = lambda t: float(t.detach())
        losses.append([number(loss), number(pprior_loss), number(angle_prior_loss), number(orientation_loss) / wt["orientation_weight"],
                       number(contact_loss) / wt["contact_weight"]])
        rows.append(flat(params))
    return dict(parameters=np.array(rows), loss_terms=np.array(losses, dtype=np.float64), gradients=np.array(grads),
                vertices=vertices.detach().numpy().reshape(-1, 3).astype(np.float64))


def main():
    space, loss_src = app_generator.reference_pieces()
    store, meta = {}, {}
    for name in R.CASE_NAMES:
        model, fm, w, n_pca, k, _ = R.case_models(name)
        obj, info = R.make_objective_inputs(name)
        with tempfile.TemporaryDirectory() as tmp:
            os.makedirs(os.path.join(tmp, "smplx"))
            np.savez(os.path.join(tmp, "smplx", "SMPLX_NEUTRAL.npz"), **model)
            r32 = run_reference(name, tmp, obj, info, space, loss_src, torch.float32)
            r64 = run_reference(name, tmp, obj, info, space, loss_src, torch.float64)
        cols = R.pinned_columns(name, r64["parameters"].shape[1])
        e_ref = float(np.max(np.abs(r32["parameters"] - r64["parameters"])[:, cols]))
        g_min = float(np.min(np.abs(r64["gradients"][:, cols])))
        free = [i for i in range(r64["parameters"].shape[1]) if i not in cols]
        if free:
            print(f"{name}: free columns {free}: max|g| in R64 {np.max(np.abs(r64['gradients'][:, free])):.3e}, in R32 {np.max(np.abs(r32['gradients'][:, free])):.3e}; "
                  f"they move by {np.max(np.abs(r64['parameters'][-1, free] - r64['parameters'][0, free])):.3e} in R64 and "
                  f"{np.max(np.abs(r32['parameters'][-1, free] - r32['parameters'][0, free])):.3e} in R32")
        loss_dev = np.max(np.abs(r32["loss_terms"] - r64["loss_terms"]), axis=0)
        for key, v in obj.items():
            store[f"{name}__{key}"] = v
        meta[name] = dict(n_pca=n_pca, k=k, P=int(r64["parameters"].shape[1]), iters=R.ITERS, **info, **R.WEIGHTS)
        store[f"{name}__r64_parameters"], store[f"{name}__r64_loss_terms"] = r64["parameters"], r64["loss_terms"]
        store[f"{name}__r64_first_gradient"], store[f"{name}__r64_vertices"] = r64["gradients"][0], r64["vertices"]
        store[f"{name}__loss_dev"], store[f"{name}__e_ref"] = loss_dev, np.float64(e_ref)
        v32, v64 = (R.untranslated(name, r["vertices"], r["parameters"]) for r in (r32, r64))
        store[f"{name}__e_ref_vertices"] = np.float64(np.max(np.abs(v32 - v64)) / np.max(np.abs(v64)))
        objective = dict(obj, faces=fm["faces"], eps=info["eps"], obj_normal=obj["obj_normals"][info["ref_index"]],
                         targets=obj["obj_verts"][obj["objects"]].reshape(-1, 3))
        mine = R.run(fm, w, R.coefficients(), objective, R.WEIGHTS, R.ITERS)
        pin = float(np.max(np.abs(mine["parameters"] - r64["parameters"])[:, cols]))
        print(f"{name:5s} P={meta[name]['P']} k={k}: e_ref {e_ref:.3e} (4 e_ref = {4 * e_ref:.3e}, lr / 10 = {R.WEIGHTS['lr'] / 10:.1e})  min|g| {g_min:.3e}  "
              f"loss {r64['loss_terms'][0, 0]:.6f} -> {r64['loss_terms'][-1, 0]:.6f}  loss dev {['%.2e' % x for x in loss_dev]}  "
              f"vertices R32 vs R64 {float(store[f'{name}__e_ref_vertices']):.3e}  restatement vs R64 {pin:.3e} = {pin / e_ref:.2e} e_ref")
        assert g_min >= 1e-3, f"{name}: condition (a) fails, min|g| = {g_min:.3e}"
        assert 4 * e_ref <= R.WEIGHTS["lr"] / 10, f"{name}: condition (b) fails, 4 e_ref = {4 * e_ref:.3e}"
        assert r64["loss_terms"][-1, 0] < r64["loss_terms"][0, 0], name
    store["meta_json"] = np.array(json.dumps(meta))
    np.savez_compressed(OUT, **store)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
