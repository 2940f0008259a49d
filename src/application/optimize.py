"""Optimisation app: fit an SMPL-X pose to an object under a learned ComA state -- the one program of the reference that uses a
learned state -- with ComA's own objective on the device (coma_amd.app.ComaObjective) and the third-party models as hooks.

CLI surface, parameter set, initial values and loss composition of the reference's ``src/application/optimize.py``:
  * flags and defaults of :321-339 (unknown flags are rejected); principle / sub-principle vectors (0,0,1) / (0,1,0) and reference
    object vertex 0 as its __main__ passes them (:348-350);
  * parameters and initial values of :236-250: Adam over global_orient (0), transl (3, 1, 0), both hand poses (0) and the pose
    embedding (the decoder's encoding of the T-pose); betas, expression, eye and jaw poses fixed;
  * loss = pose-prior + angle-prior + contact + orientation (:292-298), the last two from ONE device evaluation per iteration, its
    gradient with respect to the vertices handed to torch's autograd, which continues into the body model;
  * output {save_dir}/{supercategory}/{category}/optimized.obj (:317), written by a plain v / f writer (the reference writes through
    open3d, absent here; its file also carries vertex normals).
The hooks own their torch arithmetic; the optimiser stays torch.optim.Adam beside them:
  * body_model(betas=, global_orient=, body_pose=, left_hand_pose=, right_hand_pose=, transl=, expression=, jaw_pose=, leye_pose=,
    reye_pose=, return_verts=True, return_full_pose=True) -> object with .vertices [1,V,3]; it also has .faces [F,3].  Default:
    smplx.create(BODY_MOCAP_PATH, model_type="smplx", num_pca_comps=45), imported when first needed;
  * pose_decoder with .encode(pose [1,63]).mean and .decode(embedding, output_type="aa").  Default: the reference's VPoser loader
    (utils.vposer), which this repository does not carry -- a clear error says so;
  * angle_prior(body_pose [1,63]) -> tensor, summed.  Default: likewise.
--use_collision is REFUSED: COAP (a learned occupancy network with a downloaded checkpoint) is unpinned and not reproduced, as in the
depth stage.  Five flags are added: --num_iters (the reference's loop count, 2000, is a literal there), --body_model {smplx,device}
(default smplx, the hook described above; device = coma_amd.body_model.DeviceSMPLX, the same model files read with NumPy and the
skinning and its backward run by the library's own kernels) and --pose_prior {vposer,device} (default vposer, the two hooks described
above; device = coma_amd.pose_prior.DeviceVPoser on the same experiment directory, imports/vposer, read with configparser and
torch.load, and coma_amd.pose_prior.DeviceAnglePrior: decoder, its backward and the prior run by the library's own kernels).  With
--body_model device --pose_prior device the loop needs no third-party package; the torch arithmetic left in it is Adam and the
embedding's pow(2).sum().  --loop {torch,device} (default torch: fit() below, the Python loop with torch.optim.Adam) chooses who runs the
iterations; device = coma_amd.app.DeviceFit, which needs both device flags and hands the whole loop -- Adam included -- to the library:
one C call enqueues every launch of up to 4096 iterations and nothing waits for the device until the fit is over.
--num_starts N (default 1, at most 64) is this project's own, not the reference's: the fit is non-convex and the reference starts it from
one hard-wired pose, so N > 1 runs the N starts of default_starts() at once -- every parameter [N, n], one batched call per hook and
per iteration (DeviceSMPLX(batch_size=N), DeviceVPoser and DeviceAnglePrior on N rows, ComaObjective on [N,V,3]) -- and writes the start
with the smallest final loss as optimized.obj, every start as optimized_start{n:02d}.obj, and starts.json.  Each start evolves as it
would alone (the loss is a sum over starts, Adam is element-wise).  --loop device runs one start: DeviceFit is not batched.
"""
import argparse
import json
import os
import pickle
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BODY_MOCAP_PATH = "imports/hand4whole/common/utils_hand4whole/human_model_files/"
VPOSER_PATH = "imports/vposer"
DEFAULT_BETAS = [[-0.00982137, 0.03693837, 0.0949352, -0.01299302, 0.00492086, -0.04505398, -0.0008909, -0.00054313, 0.03646483, -0.00803524]]
LOOP_NEEDS_BODY_MODEL = "--loop device needs --body_model device: the device loop drives coma_amd.body_model.DeviceSMPLX, not a body-model hook"
LOOP_NEEDS_POSE_PRIOR = "--loop device needs --pose_prior device: the device loop drives coma_amd.pose_prior's decoder and angle prior, not hooks"
LOOP_TAKES_NO_HOOKS = ("--loop device builds its own body model, pose decoder and angle prior from --body_model device --pose_prior device; "
                       "hooks passed to main() cannot be used with it")
LOOP_RUNS_ONE_START = ("--loop device runs one start: coma_amd.app.DeviceFit is not batched; use --loop torch (the default) with "
                       "--num_starts above 1")
MAX_STARTS = 64                                    # coma_amd.pose_prior.MAX_BATCH: the rows DeviceVPoser and DeviceAnglePrior take
NUM_STARTS_RANGE = f"--num_starts must lie in [1, {MAX_STARTS}] (the rows coma_amd.pose_prior's decoder takes in one call)"
COLLISION_REFUSAL = ("--use_collision is not supported: the reference's collision term is COAP's (a learned occupancy network whose "
                     "checkpoint is not available to this project); run without it")


def default_body_model(device, batch_size=1):
    try:
        import smplx
    except ImportError as exc:
        raise RuntimeError("optimize: the `smplx` package is needed for the body model (pass body_model=... to run without it)") from exc
    batch = {"batch_size": batch_size} if batch_size != 1 else {}
    return smplx.create(model_path=BODY_MOCAP_PATH, model_type="smplx", num_pca_comps=45, **batch).to(device)


def default_pose_decoder(device):
    try:
        from utils.vposer.model_loader import load_vposer
    except ImportError as exc:
        raise RuntimeError("optimize: VPoser (utils.vposer of the reference, third party) is needed for the pose embedding "
                           "(pass pose_decoder=... to run without it)") from exc
    vposer = load_vposer(VPOSER_PATH, vp_model="snapshot").to(device=device)
    vposer.eval()
    return vposer


def default_angle_prior(device):
    try:
        from utils.vposer.prior import create_prior
    except ImportError as exc:
        raise RuntimeError("optimize: the angle prior (utils.vposer.prior of the reference, third party) is needed "
                           "(pass angle_prior=... to run without it)") from exc
    return create_prior(prior_type="angle").to(device)


def write_obj(pth, vertices, faces):
    """Plain Wavefront OBJ: `v x y z` lines, then 1-based `f a b c` lines; coordinates with 9 significant digits (f32 round-trips)."""
    vertices, faces = np.asarray(vertices, dtype=np.float64).reshape(-1, 3), np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    with open(pth, "w") as fh:
        for v in vertices:
            fh.write(f"v {v[0]:.9g} {v[1]:.9g} {v[2]:.9g}\n")
        for f in faces:
            fh.write(f"f {f[0] + 1} {f[1] + 1} {f[2] + 1}\n")


def default_starts(num_starts):
    """The start rows of a multi-start fit, f64 [num_starts, 6] = [global_orient | transl]: start n faces 2 pi n / num_starts about
    the vertical axis, global_orient = (0, 2 pi n / num_starts, 0), at the reference's transl (3, 1, 0).  Row 0 is the reference's one
    start; the others are a policy of THIS project -- the reference runs one start and has no such notion."""
    num_starts = int(num_starts)
    if num_starts < 1:
        raise ValueError(f"default_starts: num_starts = {num_starts} must be positive")
    rows = np.zeros((num_starts, 6), dtype=np.float64)
    rows[:, 1] = 2.0 * np.pi * np.arange(num_starts) / num_starts
    rows[:, 3:] = [3.0, 1.0, 0.0]
    return rows


def best_start(start_losses):
    """The first index of the smallest finite loss; no finite loss raises and names the starts."""
    losses = np.asarray(start_losses, dtype=np.float64).reshape(-1)
    finite = np.isfinite(losses)
    if not finite.any():
        raise FloatingPointError(f"fit: none of the {len(losses)} starts ended with a finite loss: " +
                                 ", ".join(f"start {n}: {x}" for n, x in enumerate(losses)))
    return int(np.argmin(np.where(finite, losses, np.inf)))                      # np.argmin: the first minimum


def fit(objective_loss, body_model, pose_decoder, angle_prior, lr, body_pose_weight, bending_prior_weight, pprior_weight, scale_factor,
        num_iters=2000, device="cuda", dtype=None, record=False, starts=None):
    """The loop of :236-307 around any `objective_loss(vertices [1,V,3]) -> scalar` (the weighted orientation + contact terms).
    Returns dict(vertices [V,3] of the last iteration's forward, as the reference saves them; losses; trajectory = global_orient and
    transl after every step, [num_iters + 1, 6], when record).

    starts [N,6] (rows [global_orient | transl], e.g. default_starts(N)): N starts at once, not in the reference.  Every parameter is
    [N, n], the embedding the T-pose's N times; the hooks take N rows (body_model.batch_size must be N) and `objective_loss(vertices
    [N,V,3]) -> [N]`.  What goes backward is the sum over the starts and Adam is element-wise, so each start evolves as it would alone.
    Returns in addition vertices_all [N,V,3], start_losses [N] (each start's total at the last iteration's forward, read once after the
    loop), best (the first index of the smallest finite one; none finite raises) and vertices = vertices_all[best]; with record, losses
    is a list of [N] arrays and trajectory [num_iters + 1, N, 6]."""
    import torch
    dtype = dtype or torch.float32
    mk = lambda x: torch.as_tensor(np.asarray(x, dtype=np.float64)).to(device=device, dtype=dtype)
    rows = None if starts is None else np.asarray(starts, dtype=np.float64)
    if rows is not None and (rows.ndim != 2 or rows.shape[1] != 6 or rows.shape[0] < 1):
        raise ValueError(f"fit: starts must be [N,6] = [global_orient | transl] with N >= 1, got shape {rows.shape}")
    N = 1 if rows is None else rows.shape[0]
    if rows is not None and getattr(body_model, "batch_size", N) != N:
        raise ValueError(f"fit: {N} starts, but the body model was built with batch_size={body_model.batch_size}")
    t_pose_embedding = pose_decoder.encode(mk(np.zeros((1, 63)))).mean
    pose_embedding = (t_pose_embedding.clone() if rows is None else t_pose_embedding.repeat(N, 1)).detach().requires_grad_(True)
    betas, expression = mk(DEFAULT_BETAS), mk(np.zeros((1, 10)))
    leye_pose, reye_pose = mk(np.zeros((1, 3))), mk(np.zeros((1, 3)))
    global_orient = torch.nn.Parameter(mk([[0.0, 0.0, 0.0]] if rows is None else rows[:, :3]), requires_grad=True)
    transl = torch.nn.Parameter(mk([[3.0, 1.0, 0.0]] if rows is None else rows[:, 3:]), requires_grad=True)
    left_hand_pose = torch.nn.Parameter(mk(np.zeros((N, 45))), requires_grad=True)
    right_hand_pose = torch.nn.Parameter(mk(np.zeros((N, 45))), requires_grad=True)
    jaw_pose = torch.nn.Parameter(mk(np.zeros((N, 3))))
    optimizer = torch.optim.Adam([global_orient, transl, left_hand_pose, right_hand_pose, pose_embedding], lr=lr)
    if rows is None:
        state = lambda: torch.cat([global_orient.detach().reshape(-1), transl.detach().reshape(-1)]).cpu().numpy().astype(np.float64)
    else:
        state = lambda: torch.cat([global_orient.detach(), transl.detach()], 1).cpu().numpy().astype(np.float64)

    def start_totals():
        # each start's total by the single-start loop's own operations on that start's rows, so that it has that loop's bits
        with torch.no_grad():
            per_start = objective_terms.reshape(-1)
            totals = [(squares[n:n + 1].sum() * body_pose_weight ** 2) * pprior_weight
                      + torch.sum(prior_rows[n:n + 1]) * bending_prior_weight + per_start[n] for n in range(N)]
            return torch.stack(totals).cpu().numpy()

    losses, trajectory = [], [state()] if record else []
    vertices = None
    for _ in range(num_iters):
        optimizer.zero_grad()
        body_pose = pose_decoder.decode(pose_embedding, output_type="aa").view(N, -1)
        output = body_model(betas=betas, global_orient=global_orient, body_pose=body_pose, left_hand_pose=left_hand_pose,
                            right_hand_pose=right_hand_pose, transl=transl, expression=expression, jaw_pose=jaw_pose, leye_pose=leye_pose,
                            reye_pose=reye_pose, return_verts=True, return_full_pose=True)
        vertices = output.vertices * scale_factor
        squares = pose_embedding.pow(2)                                      # kept: the step below changes the embedding
        pprior_loss = (squares.sum() * body_pose_weight ** 2) * pprior_weight
        prior_rows = angle_prior(body_pose)
        angle_prior_loss = torch.sum(prior_rows) * bending_prior_weight
        objective_terms = objective_loss(vertices)                           # a scalar; [N] for N >= 2 starts
        loss = pprior_loss + angle_prior_loss + (objective_terms if objective_terms.dim() == 0 else objective_terms.sum())
        loss.backward()
        optimizer.step()
        if record:
            losses.append(float(loss.detach()) if rows is None else start_totals())
            trajectory.append(state())
    if rows is None:
        return dict(vertices=None if vertices is None else vertices.detach().reshape(-1, 3).cpu().numpy(), losses=losses, trajectory=trajectory)
    out = dict(vertices=None, vertices_all=None, start_losses=None, best=None, losses=losses,
               trajectory=np.asarray(trajectory).reshape(-1, N, 6) if record else trajectory)
    if vertices is not None:
        out["start_losses"] = start_totals()
        out["best"] = best_start(out["start_losses"])
        out["vertices_all"] = vertices.detach().reshape(N, -1, 3).cpu().numpy()
        out["vertices"] = out["vertices_all"][out["best"]]
    return out


def optimize_smpl(supercategory, category, coma_path, asset_downsample_pth, eps, principle_vec, sub_principle_vec, reference_object_vertex_index,
                  lr, body_pose_weight, bending_prior_weight, pprior_weight, orientation_weight, contact_weight, contact_threshold, scale_factor,
                  use_collision, save_dir="", num_iters=2000, body_model=None, pose_decoder=None, angle_prior=None, device="cuda", record=False,
                  loop="torch", num_starts=1):
    """The reference's optimize_smpl with the three third-party models as hooks (None = the reference's own, imported lazily).
    coma_path / asset_downsample_pth: the pickles, or the dicts they hold.  Writes {save_dir}/{supercategory}/{category}/optimized.obj
    and returns fit()'s dict plus the faces and the path.  loop="device": the iterations run in coma_amd.app.DeviceFit, which takes
    the library's own DeviceSMPLX, DeviceVPoser and DeviceAnglePrior as the three models and nothing else.
    num_starts > 1 (this project's own; the reference runs one start): the starts of default_starts(num_starts) at once through fit()'s
    `starts` -- the hooks take num_starts rows, a body model passed in was built with batch_size=num_starts -- and, besides
    optimized.obj (the best start), optimized_start{n:02d}.obj for every start and starts.json (start_losses, best, the start rows);
    the dict is fit()'s for N starts.  loop="device" runs one start and refuses more."""
    if use_collision:
        raise NotImplementedError(COLLISION_REFUSAL)
    if loop not in ("torch", "device"):
        raise ValueError(f"optimize_smpl: loop must be 'torch' or 'device', got {loop!r}")
    num_starts = int(num_starts)
    if num_starts < 1:
        raise ValueError(f"optimize_smpl: num_starts = {num_starts} must be positive")
    if loop == "device" and num_starts > 1:
        raise ValueError(LOOP_RUNS_ONE_START)
    from coma_amd.app import ComaObjective
    body_model = body_model if body_model is not None else default_body_model(device, num_starts)
    pose_decoder = pose_decoder if pose_decoder is not None else default_pose_decoder(device)
    angle_prior = angle_prior if angle_prior is not None else default_angle_prior(device)
    faces = np.asarray(body_model.faces).astype(np.int64)
    objective = ComaObjective.from_state(coma_path, asset_downsample_pth, faces, reference_object_vertex_index, contact_threshold,
                                         principle_vec, sub_principle_vec, eps, device)
    if loop == "device":
        from coma_amd.app import DeviceFit
        out = DeviceFit(body_model, pose_decoder, angle_prior, objective).run(lr, body_pose_weight, bending_prior_weight, pprior_weight,
                                                                               orientation_weight, contact_weight, scale_factor, num_iters,
                                                                               betas=DEFAULT_BETAS, record=record)
    else:
        out = fit(lambda vertices: objective.loss(vertices, orientation_weight, contact_weight), body_model, pose_decoder, angle_prior, lr,
                  body_pose_weight, bending_prior_weight, pprior_weight, scale_factor, num_iters, device, record=record,
                  **({"starts": default_starts(num_starts)} if num_starts > 1 else {}))
    out["faces"] = faces
    out["path"] = None
    if out["vertices"] is not None:
        directory = os.path.join(save_dir, supercategory, category)
        os.makedirs(directory, exist_ok=True)
        out["path"] = os.path.join(directory, "optimized.obj")
        write_obj(out["path"], out["vertices"], faces)
        if num_starts > 1:
            for n in range(num_starts):
                write_obj(os.path.join(directory, f"optimized_start{n:02d}.obj"), out["vertices_all"][n], faces)
            with open(os.path.join(directory, "starts.json"), "w") as fh:
                json.dump(dict(start_losses=[float(x) for x in out["start_losses"]], best=out["best"],
                               starts=default_starts(num_starts).tolist()), fh, indent=1)
    return out


def build_parser():
    p = argparse.ArgumentParser(allow_abbrev=False)
    p.add_argument("--supercategory", type=str)
    p.add_argument("--category", type=str)
    p.add_argument("--coma_path", type=str)
    p.add_argument("--save_dir", type=str, default="output/")
    p.add_argument("--asset_downsample_pth", type=str)
    p.add_argument("--eps", type=float, default=1e-6)
    p.add_argument("--lr", type=float, default=1e-2)
    p.add_argument("--body_pose_weight", type=float, default=10000)
    p.add_argument("--bending_prior_weight", type=float, default=31700)
    p.add_argument("--pprior_weight", type=float, default=1e-6)
    p.add_argument("--orientation_weight", type=float, default=1e12)
    p.add_argument("--contact_weight", type=float, default=2.6e11)
    p.add_argument("--contact_threshold", type=float, default=0.3)
    p.add_argument("--scale_factor", type=float, default=0.84)
    p.add_argument("--use_collision", action="store_true", help="refused: COAP is not reproduced")
    p.add_argument("--num_iters", type=int, default=2000, help="Adam iterations (a literal 2000 in the reference)")
    # absent from the namespace unless given (the parsed defaults stay the reference's parameter set); read through body_model_choice()
    p.add_argument("--body_model", choices=("smplx", "device"), default=argparse.SUPPRESS,
                   help="smplx (default): the third-party package (the reference's); device: coma_amd.body_model.DeviceSMPLX on the same model files")
    p.add_argument("--pose_prior", choices=("vposer", "device"), default=argparse.SUPPRESS,
                   help="vposer (default): the reference's VPoser loader and angle prior (third party); device: coma_amd.pose_prior on the same "
                        "experiment directory")
    p.add_argument("--loop", choices=("torch", "device"), default=argparse.SUPPRESS,
                   help="torch (default): the Python loop with torch.optim.Adam; device: coma_amd.app.DeviceFit, the whole loop in one library call "
                        "(needs --body_model device --pose_prior device)")
    p.add_argument("--num_starts", type=int, default=argparse.SUPPRESS,
                   help=f"1 (default): the reference's one start; N in [2, {MAX_STARTS}]: N starts at once (default_starts, this project's own "
                        "policy), the best one written as optimized.obj (needs --loop torch)")
    return p


def num_starts_choice(args):
    return getattr(args, "num_starts", 1)


def loop_choice(args):
    return getattr(args, "loop", "torch")


def body_model_choice(args):
    return getattr(args, "body_model", "smplx")


def pose_prior_choice(args):
    return getattr(args, "pose_prior", "vposer")


def device_body_model(device="cuda", batch_size=1):
    from coma_amd.body_model import DeviceSMPLX
    return DeviceSMPLX.from_file(BODY_MOCAP_PATH, num_pca_comps=45, device=device, batch_size=batch_size)


def device_pose_prior(device="cuda"):
    """(pose decoder, angle prior) on the device, the decoder from the experiment directory the reference's loader reads."""
    from coma_amd.pose_prior import DeviceAnglePrior, DeviceVPoser
    return DeviceVPoser.from_dir(VPOSER_PATH, device=device), DeviceAnglePrior(device=device)


def main(args, body_model=None, pose_decoder=None, angle_prior=None):
    if args.use_collision:
        raise SystemExit(COLLISION_REFUSAL)
    num_starts = num_starts_choice(args)
    if not 1 <= num_starts <= MAX_STARTS:
        raise SystemExit(NUM_STARTS_RANGE)
    if loop_choice(args) == "device":
        if num_starts > 1:
            raise SystemExit(LOOP_RUNS_ONE_START)
        if body_model_choice(args) != "device":
            raise SystemExit(LOOP_NEEDS_BODY_MODEL)
        if pose_prior_choice(args) != "device":
            raise SystemExit(LOOP_NEEDS_POSE_PRIOR)
        if body_model is not None or pose_decoder is not None or angle_prior is not None:
            raise SystemExit(LOOP_TAKES_NO_HOOKS)
    if body_model is None and body_model_choice(args) == "device":
        body_model = device_body_model(batch_size=num_starts) if num_starts > 1 else device_body_model()
    if pose_prior_choice(args) == "device" and (pose_decoder is None or angle_prior is None):
        decoder, prior = device_pose_prior()
        pose_decoder = pose_decoder if pose_decoder is not None else decoder
        angle_prior = angle_prior if angle_prior is not None else prior
    return optimize_smpl(supercategory=args.supercategory, category=args.category, coma_path=args.coma_path,
                         asset_downsample_pth=args.asset_downsample_pth, eps=args.eps, principle_vec=[0, 0, 1], sub_principle_vec=[0, 1, 0],
                         reference_object_vertex_index=0, lr=args.lr, body_pose_weight=args.body_pose_weight,
                         bending_prior_weight=args.bending_prior_weight, pprior_weight=args.pprior_weight,
                         orientation_weight=args.orientation_weight, contact_weight=args.contact_weight,
                         contact_threshold=args.contact_threshold, scale_factor=args.scale_factor, use_collision=args.use_collision,
                         save_dir=args.save_dir, num_iters=args.num_iters, body_model=body_model, pose_decoder=pose_decoder,
                         angle_prior=angle_prior, **({"loop": "device"} if loop_choice(args) == "device" else {}),
                         **({"num_starts": num_starts} if num_starts > 1 else {}))


if __name__ == "__main__":
    main(build_parser().parse_args())
