"""Depth initialisation: place the fitted human along the viewing axis where its silhouette, in front of the asset,
matches the person mask of the inpainted picture best -- the stage between src/generation/segment_human.py and the depth
optimisation -- WITHOUT Blender: the silhouette test runs on the device (coma_amd.depth_init).

CLI surface, work list, slice rule, string sentinels and output pickle of the reference's ``src/generation/initialize_depth.py``:
  * inputs  {inpaint_dir}/{SC}/{C}/{asset}/{view}/{mask}/{prompt}/{id}.png of registered assets, {camera_dir}/{SC}/{C}/{asset}/{view}.pickle
    (R, t, scale, resolution, obj_R, obj_t), {human_pred_dir}/.../{id}.pickle (verts, faces, pelvis in pixel space,
    kps_aux.mask_person_list) (:224-277);
  * outputs {save_dir}/.../{id}.pickle: the dict {idx, verts, faces, IoU, human_segmentation, interval_from_center, displacement}, or
    the sentinel found in the prediction ("NO HUMANS", "MORE THAN 2 HUMANS"), or "ERRONEOUS SAMPLE DUE TO TOO SMALL HUMAN" when no
    candidate is visible (:250-265, :361-370);
  * per-process slice ``sub = len // n + 1`` of the list sorted by save path (:280-285).
One flag is added: --asset_obj_root, the directory the dataset folders live in (the reference hard-codes "data").  The asset is read
from its Wavefront OBJ (paths of utils/blenderproc.py:116-141) and transformed as :338-345.
The reference reads the vertices back from Blender after `bpy.ops.import_scene.obj` (`vertex.co`).  The importer keeps the file's
coordinates in the mesh data and puts its axis conversion into the OBJECT matrix, so `vertex.co` equals the OBJ file's vertices:
src/generation/optimize_depth.py:639-659 applies the identical chain (P3D -> Blender matrix, z_min, obj_R, obj_t, floor shift) to the
vertices `load_obj` reads straight from the file, and the two stages must agree on where the asset is; utils/blenderproc.py:151-156
takes the floor height from the y column of `vertex.co` before it applies the same matrix.  So the OBJ vertices enter `asset_world`
unchanged.  [3rd-party, unpinned] Blender's importer may merge or reorder vertices; that is not modelled (the vertex set, and with
it the nearest asset vertex of compute_nearest_point, is the file's).  Assets in any other format are refused.
"""
import argparse
import json
import os
import pickle
import sys
from glob import glob

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from constants.generation.assets import CATEGORY2DATASET_TYPE, DATASET_DIRS, FLOOR_SHIFTED_DATASETS  # noqa: E402
from constants.generation.inpaint_config import CATEGORY2ASSET  # noqa: E402
from constants.metadata import DEFAULT_SEED  # noqa: E402

OPENGL_TO_BLENDER = np.array([[1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, -1.0]])
TRIMESH_P3D_TO_BLENDER = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, -1.0, 0.0]])
SENTINELS = ("NO HUMANS", "MORE THAN 2 HUMANS")
TOO_SMALL = "ERRONEOUS SAMPLE DUE TO TOO SMALL HUMAN"


def prepare_inpainting_pths(inpaint_dir, supercategories, categories, prompts):
    out = []
    for pth in sorted(glob(f"{inpaint_dir}/*/*/*/*/*/*/*.png")):
        sc_str, c_str, asset_id = pth.split("/")[-7:-4]
        if asset_id not in CATEGORY2ASSET.get(sc_str.replace(":", "/"), {}).get(c_str.replace(":", "/"), []):
            continue
        if supercategories is not None and sc_str.lower() not in supercategories:
            continue
        if categories is not None and c_str.lower() not in categories:
            continue
        if prompts is not None and pth.split("/")[-2].lower() not in prompts:
            continue
        out.append(pth)
    return sorted(out)


def asset_obj_path(asset_obj_root, supercategory, category, asset_id, disable_lowres_switch_for_behave=False):
    """Where the asset's mesh lives (utils/blenderproc.py:116-141)."""
    kind = CATEGORY2DATASET_TYPE[(supercategory, category)]
    base = f"{asset_obj_root}/{DATASET_DIRS[kind]}"
    if kind == "3D-FUTURE":
        pth = f"{base}/{asset_id}/raw_model.obj"
    elif kind == "SHAPENET":
        with open(f"{base}/taxonomy.json") as fh:
            synset = [c for c in json.load(fh) if c["name"] == category][0]["synsetId"]
        pth = f"{base}/{synset}/{asset_id}/models/model_normalized.obj"
    elif kind in ("SKETCHFAB", "SAPIEN"):
        pth = f"{base}/{supercategory}/{asset_id}/model.obj"
    elif kind == "BEHAVE":
        pth = f"{base}/objects/{category}/{category}.obj" if disable_lowres_switch_for_behave else \
            f"{base}/objects/{category}/{category}_canon_lowres_in_gen_coord.obj"
    else:
        pth = f"{base}/objects/{category}/mesh.obj"
    if not pth.lower().endswith(".obj"):
        raise ValueError(f"{pth}: only Wavefront OBJ assets can be read without Blender")
    return pth


def asset_world(co, camera_data, dataset_type):
    """World-space asset vertices from the OBJ file's vertices (= Blender's `vertex.co`; initialize_depth.py:338-345, the same chain as
    optimize_depth.py:639-659)."""
    v = np.asarray(co) @ TRIMESH_P3D_TO_BLENDER
    z_min = v[:, 2].min()
    v = v @ camera_data["obj_R"].T + camera_data["obj_t"].T
    if dataset_type in FLOOR_SHIFTED_DATASETS:
        v -= [0.0, 0.0, z_min]
    return v


def human_world(human_verts, pelvis, camera_data, cam_resolution):
    """Pixel space -> the camera's world scale -> world (initialize_depth.py:312-319); column by column, in the arrays' own dtype."""
    v, p = human_verts.copy(), pelvis.copy()
    side, scale = max(cam_resolution), camera_data["scale"]
    to_world = OPENGL_TO_BLENDER @ camera_data["R"].T
    for k in range(3):
        shift = -(cam_resolution[k] / 2) if k < 2 else 0          # the depth column is only rescaled
        v[:, k] = (v[:, k] + shift) / side * scale
        p[k] = (p[k] + shift) / side * scale
    return v @ to_world + camera_data["t"], p @ to_world + camera_data["t"]


def build_work_list(inpaint_pths, camera_dir, human_pred_dir, save_dir, verbose=False):
    """The items that carry a human; a prediction that is a sentinel string is copied to the save path at once (:228-277)."""
    items = []
    for pth in inpaint_pths:
        sc_str, c_str, asset_id, view_id, mask_id, prompt, id_ext = pth.split("/")[-7:]
        inpaint_id, ext = id_ext.split(".")
        assert ext == "png", "Inpainting must have '.png' extension"
        with open(f"{camera_dir}/{sc_str}/{c_str}/{asset_id}/{view_id}.pickle", "rb") as handle:
            camera_data = pickle.load(handle)
        pred_pth = f"{human_pred_dir}/{sc_str}/{c_str}/{asset_id}/{view_id}/{mask_id}/{prompt}/{inpaint_id}.pickle"
        save_directory = f"{save_dir}/{sc_str}/{c_str}/{asset_id}/{view_id}/{mask_id}/{prompt}"
        save_path = f"{save_directory}/{inpaint_id}.pickle"
        os.makedirs(save_directory, exist_ok=True)
        with open(pred_pth, "rb") as handle:
            mesh_pred = pickle.load(handle)
        if isinstance(mesh_pred, str) and mesh_pred in SENTINELS:
            if verbose:
                print(f"{mesh_pred} for: {pred_pth}")
            with open(save_path, "wb") as handle:
                pickle.dump(mesh_pred, handle, protocol=pickle.HIGHEST_PROTOCOL)
            continue
        items.append(dict(inpaint_pth=pth, mesh_pred=mesh_pred, camera_data=camera_data, save_path=save_path,
                          supercategory=sc_str.replace(":", "/"), category=c_str.replace(":", "/"), asset_id=asset_id))
    return sorted(items, key=lambda x: x["save_path"])


def initialize_item(item, asset_obj_root, interval_ratio, retrieval_range, kernel_size, max_collisions, disable_lowres_switch_for_behave,
                    no_initialize, device="cuda"):
    """One work item -> what the reference pickles for it (:305-364)."""
    from coma_amd import depth_init as D
    from coma_amd.downsample import load_obj
    camera_data, mesh_pred = item["camera_data"], item["mesh_pred"]
    cam_front = camera_data["R"][:, 2].reshape((3, 1))
    if "resolution" in camera_data:
        cam_resolution = camera_data["resolution"]
    else:
        from PIL import Image
        cam_resolution = Image.open(item["inpaint_pth"]).size
        camera_data = dict(camera_data, resolution=cam_resolution)
    human_verts, pelvis = human_world(mesh_pred["verts"], mesh_pred["pelvis"], camera_data, cam_resolution)
    human_faces = mesh_pred["faces"]
    if no_initialize:
        return dict(idx=None, verts=human_verts, faces=human_faces, IoU=None, human_segmentation=None, interval_from_center=None, displacement=None)
    obj_verts, asset_faces = load_obj(asset_obj_path(asset_obj_root, item["supercategory"], item["category"], item["asset_id"],
                                                     disable_lowres_switch_for_behave))
    asset_verts = asset_world(obj_verts, camera_data, CATEGORY2DATASET_TYPE[(item["supercategory"], item["category"])])
    interval = D.compute_directional_size(mesh_verts=human_verts, direction=cam_front) * interval_ratio
    _, distance = D.compute_nearest_point(asset_verts=asset_verts, point=pelvis, direction=cam_front)
    candidates = D.extract_candidates(human_verts, human_faces, asset_verts, asset_faces, D.candidate_displacements(distance, interval, retrieval_range),
                                      cam_front, kernel_size, max_collisions)
    selected = D.select_human(candidates, camera_data, mesh_pred["kps_aux"]["mask_person_list"][0], asset_verts, asset_faces, device=device)
    return TOO_SMALL if selected is None else selected


def initialize_depth(supercategories, categories, prompts, inpaint_dir, camera_dir, human_pred_dir, human_prefilter_dir, save_dir, interval_ratio,
                     retrieval_range, kernel_size, max_collisions, parallel_num, parallel_idx, disable_lowres_switch_for_behave, no_initialize,
                     skip_done, verbose, asset_obj_root="data", device="cuda"):
    items = build_work_list(prepare_inpainting_pths(inpaint_dir, supercategories, categories, prompts), camera_dir, human_pred_dir, save_dir, verbose)
    sub = len(items) // parallel_num + 1
    done = []
    for item in items[parallel_idx * sub:(parallel_idx + 1) * sub]:
        if skip_done and os.path.exists(item["save_path"]):
            continue
        result = initialize_item(item, asset_obj_root, interval_ratio, retrieval_range, kernel_size, max_collisions,
                                 disable_lowres_switch_for_behave, no_initialize, device)
        with open(item["save_path"], "wb") as handle:
            pickle.dump(result, handle, protocol=pickle.HIGHEST_PROTOCOL)
        done.append(item["save_path"])
    return done


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--supercategories", type=str, nargs="+")
    p.add_argument("--categories", type=str, nargs="+")
    p.add_argument("--prompts", type=str, nargs="+")
    p.add_argument("--inpaint_dir", type=str, default="results/generation/inpaintings")
    p.add_argument("--camera_dir", type=str, default="results/generation/cameras")
    p.add_argument("--human_pred_dir", type=str, default="results/generation/human_preds")
    p.add_argument("--human_prefilter_dir", type=str, default="results/generation/human_prefilterings")
    p.add_argument("--save_dir", type=str, default="results/generation/human_before_opt")
    p.add_argument("--interval_ratio", type=float, default=0.3)
    p.add_argument("--retrieval_range", type=int, default=3)
    p.add_argument("--kernel_size", type=int, default=9)
    p.add_argument("--max_collisions", type=int, default=1000)
    p.add_argument("--parallel_num", type=int, default=1)
    p.add_argument("--parallel_idx", type=int, default=0)
    p.add_argument("--disable_lowres_switch_for_behave", action="store_true")
    p.add_argument("--no_initialize", action="store_true")
    p.add_argument("--skip_done", action="store_true")
    p.add_argument("--verbose", action="store_true")
    p.add_argument("--seed", type=int, default=DEFAULT_SEED)
    p.add_argument("--asset_obj_root", type=str, default="data", help="directory that holds the dataset folders (3D-FUTURE-model, BEHAVE, ...)")
    return p


def main(args):
    for name in ("supercategories", "categories", "prompts"):
        if getattr(args, name) is not None:
            setattr(args, name, [x.lower() for x in getattr(args, name)])
    if args.no_initialize:
        args.save_dir = f"{args.save_dir}_no_initialize"
    from utils.reproducibility import seed_everything
    seed_everything(args.seed)
    return initialize_depth(supercategories=args.supercategories, categories=args.categories, prompts=args.prompts, inpaint_dir=args.inpaint_dir,
                            camera_dir=args.camera_dir, human_pred_dir=args.human_pred_dir, human_prefilter_dir=args.human_prefilter_dir,
                            save_dir=args.save_dir, interval_ratio=args.interval_ratio, retrieval_range=args.retrieval_range,
                            kernel_size=args.kernel_size, max_collisions=args.max_collisions, parallel_num=args.parallel_num,
                            parallel_idx=args.parallel_idx, disable_lowres_switch_for_behave=args.disable_lowres_switch_for_behave,
                            no_initialize=args.no_initialize, skip_done=args.skip_done, verbose=args.verbose, asset_obj_root=args.asset_obj_root)


if __name__ == "__main__":
    main(build_parser().parse_args())
