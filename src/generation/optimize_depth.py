"""Depth optimisation: slide the depth-initialised human along the viewing axis until its joints agree with the
other views' predictions and it stops intersecting the asset -- the stage between src/generation/initialize_depth.py and
src/generation/compute_metrics.py -- with the whole Adam loop on the device (coma_amd.depth_opt); COAP's collision loss is opt-in.

CLI surface, work list, slice rule, string sentinels and output pickle of the reference's ``src/generation/optimize_depth.py``:
  * inputs  {inpaint_dir}/{SC}/{C}/{asset}/{view}/{mask}/{prompt}/{id}.png of registered assets, {human_initial_dir}/.../{id:06}.pickle
    (faces, displacement, or a sentinel string; an inpainting without one is skipped), {human_preds_dir}/.../{id:06}.pickle
    (smplx_data, joints_proj, convert_data), {camera_dir}/{SC}/{C}/{asset}/{view}.pickle (:461-480);
  * outputs {save_dir}/.../{prompt}/{id:06}.pickle, the prompt directory prefixed "total:" with --enable_aggregate_total_prompts
    (:483-487): dict(verts f32 [V,3], faces uint32 [F,3], num_inliers) (:775-776), or one of the sentinels "NO HUMANS",
    "MORE THAN 2 HUMANS", "LARGELY PENETRATED HUMAN", "ERRONEOUS SAMPLE DUE TO TOO SMALL HUMAN" copied from the input (:498-521),
    "NOT ALLOWED VIEWPOINT PROMPTS" (:523-535), "TOO LITTLE INLIERS" (:710-713);
  * per-process slice ``sub = len // n + 1`` of the list sorted by save path (:591-597); --no_initialize / --no_collision suffix the
    directories as the reference does (:833-841).
The optimiser holds the displacement alone (:695), so the body model runs ONCE: `body_model(smplx_data, smplx_path)` gives the
vertices and the 137 joints in the pose estimator's camera space, and everything after that is this project's.  The default hook
imports `smplx` when it is first called.
The collision term is chosen by --collision.  `columns` (the default): --w_collision weights the intersection ratio in [0, 1] of
include/coma_hip.h's column rule set (see coma_amd/depth_opt.py), not COAP's loss.  `coap`: --w_collision weights COAP's sum of
relu(occupancy - 0.5) over the asset's vertices, as in the reference (:752-753), through coma_amd.coap.DeviceCOAP with the checkpoint
--coap_ckpt FILE (a {"state_dict": ...} file in the reference's key layout; a missing file is an error).  COAP's ARCHITECTURE is
pinned against the code the reference vendors with seeded weights; the real checkpoint is a download that has never been executed
here.  Deviations with `coap`: the body is encoded ONCE per item from --coap_samples surface samples drawn with pytorch3d's method
from the seed --coap_seed (the reference re-draws them with pytorch3d every epoch), and where more than 10 000 asset vertices survive
the epoch's filter all of them count (the reference keeps a random 10 000).  The body model hook is then called with full_pose=True
and returns (verts, joints, full_pose [165]).  --w_refview is accepted and, as in the reference (:757), not part
of the loss.  --asset_seg_dir is accepted and unused, as in the reference.
Three flags are added: --asset_obj_root (as in initialize_depth.py; OBJ assets only), --volume_resolution (cells along the longer
side of the collision grid) and --perturb_view_num (the reference restricts the inlier search to the reference view's group of
`view_num` cameras for perturbed categories, from a table this repository does not carry; unset = all views).
--body_model {smplx,device} (default smplx: the hook above) and --extra_joint_vertex_ids FILE: `device` runs the body model through
coma_amd.body_model.DeviceSMPLX; the joints this stage reads include the package's 21 vertex picks, whose id table is not shipped, so
without the package the ids come from FILE (a JSON list) or the run is refused.
"""
import argparse
import os
import pickle
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from constants.generation.assets import CATEGORY2DATASET_TYPE  # noqa: E402
from constants.metadata import DEFAULT_SEED  # noqa: E402
from src.generation.initialize_depth import TOO_SMALL, asset_obj_path, asset_world, prepare_inpainting_pths  # noqa: E402

BODY_MOCAP_PATH = "imports/hand4whole/common/utils_hand4whole/human_model_files/"
COPIED_SENTINELS = ("NO HUMANS", "MORE THAN 2 HUMANS", "LARGELY PENETRATED HUMAN", TOO_SMALL)
NOT_ALLOWED, TOO_FEW = "NOT ALLOWED VIEWPOINT PROMPTS", "TOO LITTLE INLIERS"
DEFAULT_INITIAL_DIR, DEFAULT_SAVE_DIR = "results/generation/human_before_opt", "results/generation/human_after_opt"


def default_body_model(smplx_data, smplx_path, full_pose=False):
    """(verts [V,3], joints [137,3]) of the SMPL-X model for one prediction, before its translation (optimize_depth.py:670-684); with
    full_pose also the 165 axis-angle entries COAP reads."""
    try:
        import smplx
    except ImportError as exc:
        raise RuntimeError("optimize_depth: the `smplx` package is needed for the body model (pass body_model=... to run without it)") from exc
    import torch
    human = smplx.create(model_path=smplx_path, model_type="smplx", num_pca_comps=45)
    params = {k: torch.as_tensor(np.asarray(v)).float() for k, v in smplx_data.items() if k != "transl"}
    with torch.no_grad():
        out = human(**params, return_verts=True, return_full_pose=True)
    if full_pose:
        return out.vertices[0].cpu().numpy(), out.joints[0].cpu().numpy(), out.full_pose[0].cpu().numpy()
    return out.vertices[0].cpu().numpy(), out.joints[0].cpu().numpy()


_DEVICE_MODELS = {}        # (smplx_path, device, ids) -> DeviceSMPLX: the model file is read and uploaded once, not per item
NO_VERTEX_IDS = ("optimize_depth: --body_model device needs the 21 extra-joint vertex ids (nose, eyes, ears, toes, heels, finger tips): the "
                 "joints this stage reads (coma_amd.depth_opt.BODY_INDICES) include them, the table lives in the `smplx` package, which "
                 "does not import here, and it is not shipped; pass --extra_joint_vertex_ids FILE (a JSON list of 21 vertex ids)")


def load_vertex_ids(pth):
    """The 21 vertex ids of the package's extra joints, in its order, from a JSON list."""
    import json
    with open(pth) as fh:
        ids = [int(i) for i in json.load(fh)]
    if len(ids) != 21:
        raise ValueError(f"{pth}: expected a JSON list of 21 vertex ids, got {len(ids)}")
    return ids


def device_body_model(smplx_data, smplx_path, device="cuda", extra_joint_vertex_ids=None, full_pose=False):
    """default_body_model's contract through coma_amd.body_model.DeviceSMPLX (--body_model device): no third-party package.  Refused
    when the vertex picks among the joints cannot be had: the stage would read face landmarks in their place."""
    import torch
    from coma_amd.body_model import DeviceSMPLX
    key = (os.path.abspath(smplx_path), str(device), None if extra_joint_vertex_ids is None else tuple(extra_joint_vertex_ids))
    human = _DEVICE_MODELS.get(key)
    if human is None:
        human = DeviceSMPLX.from_file(smplx_path, num_pca_comps=45, device=device, extra_joint_vertex_ids=extra_joint_vertex_ids)
        if human.extra_joint_source == "landmarks only":
            raise RuntimeError(NO_VERTEX_IDS)
        _DEVICE_MODELS[key] = human
    params = {k: torch.as_tensor(np.asarray(v)).float().to(device) for k, v in smplx_data.items() if k != "transl"}
    with torch.no_grad():
        out = human(**params, return_verts=True, return_full_pose=True)
    if full_pose:
        return out.vertices[0].cpu().numpy(), out.joints[0].cpu().numpy(), out.full_pose[0].cpu().numpy()
    return out.vertices[0].cpu().numpy(), out.joints[0].cpu().numpy()


_COAP_MODELS = {}          # (smplx_path, checkpoint, samples, seed, device) -> DeviceCOAP: partition and packing happen once, not per item


def coap_model(smplx_path, coap, device="cuda"):
    """The DeviceCOAP of --collision coap: the partition from the SMPL-X model file at smplx_path (read with NumPy), the weights from
    coap["ckpt"]."""
    from coma_amd.body_model import DeviceSMPLX
    from coma_amd.coap import DeviceCOAP
    key = (os.path.abspath(smplx_path), os.path.abspath(coap["ckpt"]), coap["samples"], coap["seed"], str(device))
    if key not in _COAP_MODELS:
        if not os.path.exists(coap["ckpt"]):
            raise FileNotFoundError(f"optimize_depth: --coap_ckpt {coap['ckpt']} does not exist (COAP's checkpoint is a download; see the reference's "
                                    "imports/coap)")
        body = DeviceSMPLX.from_file(smplx_path, num_pca_comps=45, device=device, extra_joint_vertex_ids=[])
        _COAP_MODELS[key] = DeviceCOAP(body, coap["ckpt"], n_samples=coap["samples"], seed=coap["seed"], device=device)
    return _COAP_MODELS[key]


def solve_displacement_coap(model, full_pose, human_verts, joints, asset_verts, cam_R, inliers, lr, w_multiview, w_collision, num_epoch):
    """solve_displacement with COAP's term: the body encoded once at d = 0, the asset's vertices as the scene points."""
    from coma_amd import depth_opt as D
    model.detach_cache()
    model.encode_body(dict(full_pose=full_pose, joints=joints, vertices=human_verts))
    views, cand_view, cand_xy = D.inlier_views(inliers)
    joints0 = np.asarray(joints, dtype=np.float64)[D.BODY_INDICES]
    return D.optimize_displacement_coap(model, asset_verts, views, joints0, np.asarray(cam_R, dtype=np.float64)[:, 2], cand_view, cand_xy, 0.0, lr,
                                        w_multiview, w_collision, num_epoch)["d"]


def _dump(payload, pth):
    with open(pth, "wb") as fh:
        pickle.dump(payload, fh, protocol=pickle.HIGHEST_PROTOCOL)


def build_work_list(inpaint_pths, human_initial_dir, human_preds_dir, camera_dir, save_dir, enable_aggregate_total_prompts,
                    allowed_viewpoint_prompts, skip_done, verbose=False):
    """The items to optimise, sorted by save path.  An input that is a sentinel string, or whose viewpoint prompt is not allowed, is
    answered at once with the sentinel (:465-535)."""
    items = []
    for pth in inpaint_pths:
        sc_str, c_str, asset_id, view_id, mask_id, prompt, id_ext = pth.split("/")[-7:]
        inpaint_id, ext = id_ext.split(".")
        assert ext == "png", "Inpainting must have '.png' extension"
        name = f"{int(inpaint_id):06}.pickle"
        below = f"{sc_str}/{c_str}/{asset_id}/{view_id}/{mask_id}"
        initial_pth = f"{human_initial_dir}/{below}/{prompt}/{name}"
        if not os.path.exists(initial_pth):
            continue
        save_directory = f"{save_dir}/{below}/{'total:' if enable_aggregate_total_prompts else ''}{prompt}"
        save_path = f"{save_directory}/{name}"
        if skip_done and os.path.exists(save_path):
            if verbose:
                print(f"skipping {save_path}: already done")
            continue
        with open(initial_pth, "rb") as fh:
            initial = pickle.load(fh)
        parts = prompt.split(",")
        view_prompt = "original" if len(parts) == 1 else parts[-1]
        answer = None
        if isinstance(initial, str) and initial in COPIED_SENTINELS:
            answer = initial
        elif view_prompt.strip().lower() not in allowed_viewpoint_prompts:
            answer = NOT_ALLOWED
        if answer is not None:
            os.makedirs(save_directory, exist_ok=True)
            _dump(answer, save_path)
            continue
        items.append(dict(inpaint_pth=pth, human_initial_pth=initial_pth, human_preds_pth=f"{human_preds_dir}/{below}/{prompt}/{name}",
                          camera_pth=f"{camera_dir}/{sc_str}/{c_str}/{asset_id}/{view_id}.pickle", save_directory=save_directory,
                          save_path=save_path, supercategory=sc_str.replace(":", "/"), category=c_str.replace(":", "/"), asset_id=asset_id))
    return sorted(items, key=lambda x: x["save_path"])


def find_inliers(joints_proj, item, human_preds_dir, camera_dir, maximum_candidates, ransac_threshold, triangulation_threshold,
                 enable_aggregate_total_prompts, allowed_viewpoint_prompts, perturb_view_num, device):
    from coma_amd.triangulate import compute_ransac_inclusives_with_triangulation
    return compute_ransac_inclusives_with_triangulation(joints_proj, item["inpaint_pth"], human_preds_dir, camera_dir, maximum_candidates,
                                                        ransac_threshold, triangulation_threshold, enable_aggregate_total_prompts,
                                                        allowed_viewpoint_prompts, perturb_view_num=perturb_view_num, device=device)


def solve_displacement(human_verts, human_faces, asset_verts, asset_faces, cam_R, joints, inliers, lr, w_multiview, w_collision, num_epoch,
                       volume_resolution=512, device="cuda"):
    """The displacement along cam_R[:, 2] after num_epoch epochs of Adam from 0, on the device."""
    from coma_amd import depth_opt as D
    columns = None
    if w_collision != 0.0:
        columns = D.collision_columns(human_verts, human_faces, asset_verts, asset_faces, cam_R, volume_resolution, device)
    views, cand_view, cand_xy = D.inlier_views(inliers)
    joints0 = np.asarray(joints, dtype=np.float64)[D.BODY_INDICES]
    return D.optimize_displacement(columns, views, joints0, np.asarray(cam_R, dtype=np.float64)[:, 2], cand_view, cand_xy, 0.0, lr, w_multiview,
                                   w_collision, num_epoch, device)["d"]


def optimize_item(item, human_preds_dir, camera_dir, smplx_path, maximum_candidates, ransac_threshold, triangulation_threshold, num_epoch,
                  minimum_inliers, lr, w_collision, w_multiview, enable_aggregate_total_prompts, allowed_viewpoint_prompts,
                  disable_lowres_switch_for_behave, asset_obj_root, volume_resolution, perturb_view_num, body_model, device, coap=None):
    """One work item -> what the reference pickles for it (:598-780).  coap: None (the column term), or dict(ckpt, samples, seed)."""
    from coma_amd import depth_opt as D
    from coma_amd.downsample import load_obj
    with open(item["human_initial_pth"], "rb") as fh:
        initial = pickle.load(fh)
    with open(item["human_preds_pth"], "rb") as fh:
        preds = pickle.load(fh)
    with open(item["camera_pth"], "rb") as fh:
        camera_data = pickle.load(fh)
    if "resolution" in camera_data:
        cam_resolution = camera_data["resolution"]
    else:
        from PIL import Image
        cam_resolution = Image.open(item["inpaint_pth"]).size
    inliers = find_inliers(preds["joints_proj"], item, human_preds_dir, camera_dir, maximum_candidates, ransac_threshold, triangulation_threshold,
                           enable_aggregate_total_prompts, allowed_viewpoint_prompts, perturb_view_num, device)
    if len(inliers) < minimum_inliers:
        return TOO_FEW
    smplx_data = preds["smplx_data"]
    use_coap = coap is not None and w_collision != 0.0
    if use_coap:
        verts_cam, joints_cam, full_pose = body_model(smplx_data, smplx_path, full_pose=True)
    else:
        verts_cam, joints_cam = body_model(smplx_data, smplx_path)
    placed = initial.get("displacement")                       # where the depth initialisation put the human (None with --no_initialize)
    placed = np.zeros((1, 3)) if placed is None else np.asarray(placed, dtype=np.float64).reshape((1, 3))
    to_real = [D.convert_cam2real(x, smplx_data["transl"], cam_resolution, camera_data, preds["convert_data"]).astype(np.float64) + placed
               for x in (verts_cam, joints_cam)]
    human_verts, joints = to_real
    human_faces = np.asarray(initial["faces"])
    asset_verts = asset_faces = None
    if w_collision != 0.0:
        obj_verts, asset_faces = load_obj(asset_obj_path(asset_obj_root, item["supercategory"], item["category"], item["asset_id"],
                                                         disable_lowres_switch_for_behave))
        asset_verts = asset_world(obj_verts, camera_data, CATEGORY2DATASET_TYPE[(item["supercategory"], item["category"])])
    if use_coap:
        d = solve_displacement_coap(coap_model(smplx_path, coap, device), full_pose, human_verts, joints, asset_verts, camera_data["R"], inliers, lr,
                                    w_multiview, w_collision, num_epoch)
    else:
        d = solve_displacement(human_verts, human_faces, asset_verts, asset_faces, camera_data["R"], joints, inliers, lr, w_multiview, w_collision,
                               num_epoch, volume_resolution, device)
    front = np.asarray(camera_data["R"], dtype=np.float64)[:, 2].reshape((1, 3))
    return dict(verts=(human_verts + d * front).astype(np.float32), faces=human_faces.astype(np.uint32), num_inliers=len(inliers))


def run_depth_optimization(supercategories, categories, prompts, inpaint_dir, asset_seg_dir, human_initial_dir, human_preds_dir, camera_dir,
                           save_dir, smplx_path, maximum_candidates, ransac_threshold, triangulation_threshold, num_epoch, minimum_inliers, lr,
                           w_collision, w_multiview, w_refview, enable_aggregate_total_prompts, allowed_viewpoint_prompts,
                           disable_lowres_switch_for_behave, skip_done, verbose, parallel_num, parallel_idx, asset_obj_root="data",
                           volume_resolution=512, perturb_view_num=None, body_model=None, device="cuda", coap=None):
    """This process's share of the work list -> optimised humans; returns the paths written by the loop (sentinels answered while the
    list is built are not among them)."""
    body_model = body_model or default_body_model
    items = build_work_list(prepare_inpainting_pths(inpaint_dir, supercategories, categories, prompts), human_initial_dir, human_preds_dir,
                            camera_dir, save_dir, enable_aggregate_total_prompts, allowed_viewpoint_prompts, skip_done, verbose)
    sub = len(items) // parallel_num + 1
    done = []
    for item in items[parallel_idx * sub:(parallel_idx + 1) * sub]:
        if skip_done and os.path.exists(item["save_path"]):
            continue
        os.makedirs(item["save_directory"], exist_ok=True)
        result = optimize_item(item, human_preds_dir, camera_dir, smplx_path, maximum_candidates, ransac_threshold, triangulation_threshold,
                               num_epoch, minimum_inliers, lr, w_collision, w_multiview, enable_aggregate_total_prompts,
                               allowed_viewpoint_prompts, disable_lowres_switch_for_behave, asset_obj_root, volume_resolution, perturb_view_num,
                               body_model, device, coap)
        _dump(result, item["save_path"])
        done.append(item["save_path"])
    return done


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--supercategories", type=str, nargs="+")
    p.add_argument("--categories", type=str, nargs="+")
    p.add_argument("--prompts", type=str, nargs="+")
    p.add_argument("--inpaint_dir", type=str, default="results/generation/inpaintings")
    p.add_argument("--asset_seg_dir", type=str, default="results/generation/asset_segs")
    p.add_argument("--human_initial_dir", type=str, default=DEFAULT_INITIAL_DIR)
    p.add_argument("--human_preds_dir", type=str, default="results/generation/human_preds")
    p.add_argument("--camera_dir", type=str, default="results/generation/cameras")
    p.add_argument("--save_dir", type=str, default=DEFAULT_SAVE_DIR)
    p.add_argument("--smplx_path", type=str, default=BODY_MOCAP_PATH)
    p.add_argument("--maximum_candidates", type=int, default=400)
    p.add_argument("--ransac_threshold", type=int, default=200)
    p.add_argument("--triangulation_threshold", type=int, default=100)
    p.add_argument("--num_epoch", type=int, default=200)
    p.add_argument("--minimum_inliers", type=int, default=1)
    p.add_argument("--lr", type=float, default=0.01)
    p.add_argument("--w_collision", type=float, default=0.4,
                   help="weight of the collision term: the intersection ratio in [0, 1] (--collision columns) or COAP's loss (--collision coap)")
    p.add_argument("--collision", choices=("columns", "coap"), default="columns",
                   help="columns: the geometric intersection ratio; coap: COAP's learned occupancy loss, as in the reference (needs --coap_ckpt)")
    p.add_argument("--coap_ckpt", type=str, default=None, help="with --collision coap: COAP's checkpoint, a {'state_dict': ...} file")
    p.add_argument("--coap_samples", type=int, default=1000, help="surface samples per body part for COAP's encoder")
    p.add_argument("--coap_seed", type=int, default=0, help="seed of the surface sample table")
    p.add_argument("--w_multiview", type=float, default=1e-3)
    p.add_argument("--w_refview", type=float, default=0.0)
    p.add_argument("--disable_lowres_switch_for_behave", action="store_true")
    p.add_argument("--enable_aggregate_total_prompts", action="store_true")
    p.add_argument("--allowed_viewpoint_prompts", nargs="+", default=["original", "full body"])
    p.add_argument("--no_initialize", action="store_true")
    p.add_argument("--no_collision", action="store_true")
    p.add_argument("--skip_done", action="store_true")
    p.add_argument("--verbose", action="store_true")
    p.add_argument("--seed", type=int, default=DEFAULT_SEED)
    p.add_argument("--parallel_num", type=int, default=1)
    p.add_argument("--parallel_idx", type=int, default=0)
    p.add_argument("--asset_obj_root", type=str, default="data", help="directory that holds the dataset folders (3D-FUTURE-model, BEHAVE, ...)")
    p.add_argument("--volume_resolution", type=int, default=512, help="cells along the longer side of the collision grid")
    p.add_argument("--perturb_view_num", type=int, default=None, help="cameras per perturbation group (inlier search stays inside the group)")
    p.add_argument("--body_model", choices=("smplx", "device"), default="smplx",
                   help="smplx: the third-party package (the reference's); device: coma_amd.body_model.DeviceSMPLX on the same model files")
    p.add_argument("--extra_joint_vertex_ids", type=str, default=None,
                   help="with --body_model device and no `smplx` package: a JSON list of the 21 extra-joint vertex ids, in the package's order")
    return p


def main(args, body_model=None):
    if body_model is None and getattr(args, "body_model", "smplx") == "device":
        ids = load_vertex_ids(args.extra_joint_vertex_ids) if getattr(args, "extra_joint_vertex_ids", None) else None
        body_model = lambda smplx_data, smplx_path, **kw: device_body_model(smplx_data, smplx_path, extra_joint_vertex_ids=ids, **kw)
    coap = None
    if getattr(args, "collision", "columns") == "coap" and not args.no_collision and args.w_collision != 0.0:
        if not getattr(args, "coap_ckpt", None):
            raise SystemExit("optimize_depth: --collision coap needs --coap_ckpt FILE (COAP's checkpoint is a download that this repository does not hold)")
        if not os.path.exists(args.coap_ckpt):
            raise SystemExit(f"optimize_depth: --coap_ckpt {args.coap_ckpt} does not exist")
        coap = dict(ckpt=args.coap_ckpt, samples=int(getattr(args, "coap_samples", 1000)), seed=int(getattr(args, "coap_seed", 0)))
    for name in ("supercategories", "categories", "prompts", "allowed_viewpoint_prompts"):
        if getattr(args, name) is not None:
            setattr(args, name, [x.lower() for x in getattr(args, name)])
    if args.no_initialize:
        args.human_initial_dir = f"{args.human_initial_dir}_no_initialize"
        args.save_dir = f"{args.save_dir}_no_initialize"
        assert args.human_initial_dir != DEFAULT_INITIAL_DIR
        assert args.save_dir != DEFAULT_SAVE_DIR
    if args.no_collision:
        args.save_dir = f"{args.save_dir}_no_collision"
        args.w_collision = 0.0
        assert args.save_dir != DEFAULT_SAVE_DIR
    from utils.reproducibility import seed_everything
    seed_everything(args.seed)
    return run_depth_optimization(supercategories=args.supercategories, categories=args.categories, prompts=args.prompts,
                                  inpaint_dir=args.inpaint_dir, asset_seg_dir=args.asset_seg_dir, human_initial_dir=args.human_initial_dir,
                                  human_preds_dir=args.human_preds_dir, camera_dir=args.camera_dir, save_dir=args.save_dir,
                                  smplx_path=args.smplx_path, maximum_candidates=args.maximum_candidates, ransac_threshold=args.ransac_threshold,
                                  triangulation_threshold=args.triangulation_threshold, num_epoch=args.num_epoch,
                                  minimum_inliers=args.minimum_inliers, lr=args.lr, w_collision=args.w_collision, w_multiview=args.w_multiview,
                                  w_refview=args.w_refview, enable_aggregate_total_prompts=args.enable_aggregate_total_prompts,
                                  allowed_viewpoint_prompts=args.allowed_viewpoint_prompts,
                                  disable_lowres_switch_for_behave=args.disable_lowres_switch_for_behave, skip_done=args.skip_done,
                                  verbose=args.verbose, parallel_num=args.parallel_num, parallel_idx=args.parallel_idx,
                                  asset_obj_root=args.asset_obj_root, volume_resolution=args.volume_resolution,
                                  perturb_view_num=args.perturb_view_num, body_model=body_model, coap=coap)


if __name__ == "__main__":
    main(build_parser().parse_args())
