"""Sample metrics: for every optimised human, the IoU of its silhouette with the person mask and the ratio of its
volume that lies inside the asset -- the stage between the depth optimisation and src/coma/filter.py -- WITHOUT Blender or trimesh:
both metrics run on the device (coma_amd.metrics, coma_amd.depth_init).

CLI surface, work list, slice rule, string sentinels and output pickle of the reference's ``src/generation/compute_metrics.py``:
  * inputs  {human_after_opt_dir}/{SC}/{C}/{asset}/{view}/{mask}/{prompt}/{id}.pickle (verts, faces in world space, or a sentinel
    string), {camera_dir}/{SC}/{C}/{asset}/{view}.pickle (R, t, scale, resolution, obj_R, obj_t), {human_pred_dir}/.../{id}.pickle
    (kps_aux.mask_person_list; the prompt directory without its "total:" prefix) (:186-213);
  * outputs {save_dir}/.../{id}.pickle: the input dict with `interscetion_ratio`, `IoU` and `z_min` added and `verts` moved to the
    object-canonical frame (:237-247), or the sentinel string unchanged (:222-224);
  * the glob keeps "total*" prompt directories with --enable_aggregate_total_prompts and drops every directory whose name starts with
    one of the letters t, o, a, l otherwise (the character class "[!total]" of :189, the reference's own rule);
  * per-process slice ``sub = len // n + 1`` of the sorted list (:200-203).
Two flags are added: --asset_obj_root, the directory the dataset folders live in (as in initialize_depth.py; OBJ assets only), and
--volume_resolution, the cells along the longer side of the intersection grid.
--disable_lowres_switch_for_behave keeps the reference's declaration (`default=True`, no action): it is on unless an empty string is
passed.
"""
import argparse
import collections
import os
import pickle
import sys
from glob import glob

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from constants.metadata import DEFAULT_SEED  # noqa: E402

# one sample file: .../{SC}/{C}/{asset}/{view}/{mask}/{prompt}/{id}.pickle
Sample = collections.namedtuple("Sample", "supercategory category asset_id view_id mask_id prompt inpaint_id")


def parse_sample_path(pth):
    """The seven trailing path components of a sample file, the last one without its extension."""
    *levels, file_name = pth.split("/")[-7:]
    return Sample(*levels, file_name.split(".")[0])


def list_human_pths(human_dir, supercategories, categories, prompts, enable_aggregate_total_prompts):
    """The sorted work list: every sample pickle six directories below human_dir whose prompt directory matches the mode, kept when
    its lower-cased supercategory / category / prompt is among the requested ones (an empty or missing request keeps all).
    src/coma/filter.py lists its inputs the same way."""
    prompt_dirs = "total*" if enable_aggregate_total_prompts else "[!total]*"
    wanted = ((supercategories, "supercategory"), (categories, "category"), (prompts, "prompt"))
    out = []
    for pth in glob(os.path.join(human_dir, "*", "*", "*", "*", "*", prompt_dirs, "*.pickle")):
        sample = parse_sample_path(pth)
        if all(not names or getattr(sample, field).lower() in names for names, field in wanted):
            out.append(pth)
    return sorted(out)


def load_person_mask(human_pred_pth):
    """The first person mask of a human-prediction pickle, as stored; coma_amd.depth_init.person_mask makes it 0 / 1."""
    with open(human_pred_pth, "rb") as fh:
        return pickle.load(fh)["kps_aux"]["mask_person_list"][0]


def _dump(payload, pth):
    with open(pth, "wb") as fh:
        pickle.dump(payload, fh, protocol=pickle.HIGHEST_PROTOCOL)


def measure_sample(human_mesh, sample, camera_dir, human_pred_dir, disable_lowres_switch_for_behave, asset_obj_root, volume_resolution, device):
    """The dict the sample pickle holds: the optimised human with both metrics and z_min added, its vertices in the asset's frame."""
    from coma_amd import metrics as M
    below_view = os.path.join(sample.supercategory, sample.category, sample.asset_id)
    with open(os.path.join(camera_dir, below_view, f"{sample.view_id}.pickle"), "rb") as fh:
        camera_data = pickle.load(fh)
    # the mask was predicted for the plain prompt: an aggregated directory "total:<prompt>" points back at "<prompt>"
    pred_prompt = sample.prompt.split("total:")[-1]
    mask = load_person_mask(os.path.join(human_pred_dir, below_view, sample.view_id, sample.mask_id, pred_prompt, f"{sample.inpaint_id}.pickle"))
    # directory names carry ":" where category names carry "/" (as in initialize_depth.py's work list)
    asset = M.get_asset_info(sample.supercategory.replace(":", "/"), sample.category.replace(":", "/"), sample.asset_id, sample.view_id,
                             camera_data, disable_lowres_switch_for_behave, asset_obj_root)
    world_verts = human_mesh["verts"]
    result = dict(human_mesh)
    result.update(M.compute_metrics(camera_data, mask, world_verts, human_mesh["faces"], asset["verts"], asset["faces"], volume_resolution, device))
    result["verts"] = M.to_object_frame(world_verts, asset["z_min"], camera_data)
    result["z_min"] = asset["z_min"]
    return result


def save_human(supercategories, categories, prompts, human_after_opt_dir, human_pred_dir, camera_dir, save_dir, enable_aggregate_total_prompts,
               disable_lowres_switch_for_behave, skip_done, parallel_idx, parallel_num, asset_obj_root="data", volume_resolution=512, device="cuda"):
    """This process's share of the work list -> sample pickles; returns the paths written."""
    from coma_amd.metrics import parallel_slice
    work = list_human_pths(human_after_opt_dir, supercategories, categories, prompts, enable_aggregate_total_prompts)
    first, last = parallel_slice(len(work), parallel_num, parallel_idx)
    written = []
    for pth in work[first:last]:
        sample = parse_sample_path(pth)
        out_dir = os.path.join(save_dir, *sample[:6])
        out_pth = os.path.join(out_dir, f"{sample.inpaint_id}.pickle")
        if skip_done and os.path.exists(out_pth):
            continue
        with open(pth, "rb") as fh:
            human_mesh = pickle.load(fh)
        os.makedirs(out_dir, exist_ok=True)
        if isinstance(human_mesh, str):          # "NO HUMANS" and the like travel on unchanged
            _dump(human_mesh, out_pth)
        else:
            _dump(measure_sample(human_mesh, sample, camera_dir, human_pred_dir, disable_lowres_switch_for_behave, asset_obj_root,
                                 volume_resolution, device), out_pth)
        written.append(out_pth)
    return written


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("--supercategories", type=str, nargs="+")
    parser.add_argument("--categories", type=str, nargs="+")
    parser.add_argument("--prompts", type=str, nargs="+")
    parser.add_argument("--camera_dir", type=str, default="results/generation/cameras")
    parser.add_argument("--human_after_opt_dir", type=str, default="results/generation/human_after_opt")
    parser.add_argument("--human_pred_dir", type=str, default="results/generation/human_preds")
    parser.add_argument("--save_dir", type=str, default="results/generation/human_sample")
    parser.add_argument("--enable_aggregate_total_prompts", action="store_true")
    parser.add_argument("--disable_lowres_switch_for_behave", default=True)
    parser.add_argument("--skip_done", action="store_true")
    parser.add_argument("--seed", type=int, default=DEFAULT_SEED)
    parser.add_argument("--parallel_num", type=int, default=1)
    parser.add_argument("--parallel_idx", type=int, default=0)
    parser.add_argument("--asset_obj_root", type=str, default="data", help="directory that holds the dataset folders (3D-FUTURE-model, BEHAVE, ...)")
    parser.add_argument("--volume_resolution", type=int, default=512, help="cells along the longer side of the intersection grid")
    return parser


def main(args):
    for name in ("supercategories", "categories", "prompts"):
        if getattr(args, name) is not None:
            setattr(args, name, [x.lower() for x in getattr(args, name)])
    from utils.reproducibility import seed_everything
    seed_everything(args.seed)
    return save_human(supercategories=args.supercategories, categories=args.categories, prompts=args.prompts,
                      human_after_opt_dir=args.human_after_opt_dir, human_pred_dir=args.human_pred_dir, camera_dir=args.camera_dir,
                      save_dir=args.save_dir, enable_aggregate_total_prompts=args.enable_aggregate_total_prompts,
                      disable_lowres_switch_for_behave=args.disable_lowres_switch_for_behave, skip_done=args.skip_done,
                      parallel_num=args.parallel_num, parallel_idx=args.parallel_idx, asset_obj_root=args.asset_obj_root,
                      volume_resolution=args.volume_resolution)


if __name__ == "__main__":
    main(build_parser().parse_args())
