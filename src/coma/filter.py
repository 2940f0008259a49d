"""Post-filtering: which samples of src/generation/compute_metrics.py enter ComA learning.  Host only.

CLI surface, rules, JSON layout and printed summary of the reference's ``src/coma/filter.py``:
  * inputs  {human_sample_dir}/{SC}/{C}/{asset}/{view}/{mask}/{prompt}/{id}.pickle with IoU, interscetion_ratio and (optionally)
    num_inliers, or a sentinel string (skipped, not counted) (:26-37, :61-74);
  * only prompts that are their base prompt (the part before the first comma) alone or followed by ", full body" are looked at
    (:48-50);
  * a sample is rejected, in this order, for IoU < IoU_threshold_min, interscetion_ratio > intersection_volume_ratio_threshold_max,
    num_inliers < inlier_num_threshold_min (:76-87); each rejection is counted once, under the first rule that fires;
  * outputs {save_dir}/{SC}/{C}/{asset}/{base prompt}.json (or total.json with --enable_aggregate_total_prompts): the list of
    [view_id, asset_mask_id, prompt, inpaint_id] that were kept, `indent=1`; a key whose samples were all rejected still gets its
    (empty) file (:52-59, :99-113) -- what src/coma/extract_coma.py reads.
--skip_done, --parallel_num and --parallel_idx are accepted and unused, as in the reference.
"""
import argparse
import json
import os
import pickle
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from constants.metadata import DEFAULT_SEED  # noqa: E402
from src.generation.compute_metrics import list_human_pths, parse_sample_path  # noqa: E402

ACCEPTED_SUFFIXES = ("", ", full body")
REASONS = ("IoU", "INTERSECTION", "INLIERS")       # in the order the rules are tried


def rejection_reason(sample, IoU_threshold_min, intersection_volume_ratio_threshold_max, inlier_num_threshold_min):
    """The first rule a sample dict fails, or None when it is kept.  A sample without `num_inliers` skips the last rule."""
    if sample["IoU"] < IoU_threshold_min:
        return "IoU"
    if sample["interscetion_ratio"] > intersection_volume_ratio_threshold_max:
        return "INTERSECTION"
    inliers = sample.get("num_inliers")
    if inliers is not None and inliers < inlier_num_threshold_min:
        return "INLIERS"
    return None


def run_post_filtering(supercategories, categories, prompts, human_sample_dir, save_dir, IoU_threshold_min, intersection_volume_ratio_threshold_max,
                       inlier_num_threshold_min, enable_aggregate_total_prompts, parallel_num=1, parallel_idx=0):
    """Writes the JSON files and returns dict(to_save, REJECTED_FROM_IoU, REJECTED_FROM_INTERSECTION, REJECTED_FROM_INLIERS, NUM_MESH)."""
    rejected = dict.fromkeys(REASONS, 0)
    n_meshes = 0
    kept = {}                                      # JSON file (relative to save_dir, without ".json") -> rows, in first-seen order
    for pth in list_human_pths(human_sample_dir, supercategories, categories, prompts, enable_aggregate_total_prompts):
        sample = parse_sample_path(pth)
        base_prompt = sample.prompt.split(",")[0]
        if sample.prompt.replace(base_prompt, "") not in ACCEPTED_SUFFIXES:
            continue
        target = (sample.supercategory, sample.category, sample.asset_id, "total" if enable_aggregate_total_prompts else base_prompt)
        rows = kept.setdefault(target, [])         # listed even when nothing survives: the file is written empty
        with open(pth, "rb") as fh:
            payload = pickle.load(fh)
        if isinstance(payload, str):               # a sentinel, not a mesh
            continue
        n_meshes += 1
        reason = rejection_reason(payload, IoU_threshold_min, intersection_volume_ratio_threshold_max, inlier_num_threshold_min)
        if reason is not None:
            rejected[reason] += 1
            continue
        rows.append([sample.view_id, sample.mask_id, sample.prompt, sample.inpaint_id])

    for (supercategory, category, asset_id, stem), rows in kept.items():
        out_dir = f"{save_dir}/{supercategory}/{category}/{asset_id}"
        print(out_dir)
        os.makedirs(out_dir, exist_ok=True)
        with open(f"{out_dir}/{stem}.json", "w") as fh:
            json.dump(rows, fh, indent=1)

    # the reference's summary, label for label (its numbering skips 2 and it spells INLINERS)
    banner = "================ POST-FILTERING RESULTS ================"
    report = ["\n", banner, f"1. REJECTED FROM IoU: {rejected['IoU']}", f"3. REJECTED FROM INTERSECTION: {rejected['INTERSECTION']}",
              f"4. REJECTED FROM INLINERS: {rejected['INLIERS']}", "\n", f"5. INITIAL MESHES: {n_meshes}",
              f"6. LEFTOVER MESHES: {n_meshes - sum(rejected.values())}", banner, "\n"]
    for line in report:
        print(line)
    by_key = {(k[:3] if enable_aggregate_total_prompts else k): rows for k, rows in kept.items()}
    return dict(to_save=by_key, REJECTED_FROM_IoU=rejected["IoU"], REJECTED_FROM_INTERSECTION=rejected["INTERSECTION"],
                REJECTED_FROM_INLIERS=rejected["INLIERS"], NUM_MESH=n_meshes)


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("--supercategories", type=str, nargs="+")
    parser.add_argument("--categories", type=str, nargs="+")
    parser.add_argument("--prompts", type=str, nargs="+")
    parser.add_argument("--human_sample_dir", type=str, default="results/generation/human_sample")
    parser.add_argument("--save_dir", type=str, default="results/coma/human_postfilterings")
    parser.add_argument("--IoU_threshold_min", type=float, default=0.7)
    parser.add_argument("--intersection_volume_ratio_threshold_max", type=float, default=0.05)
    parser.add_argument("--inlier_num_threshold_min", type=int, default=1)
    parser.add_argument("--enable_aggregate_total_prompts", action="store_true")
    parser.add_argument("--skip_done", action="store_true")
    parser.add_argument("--seed", type=int, default=DEFAULT_SEED)
    parser.add_argument("--parallel_num", type=int, default=1)
    parser.add_argument("--parallel_idx", type=int, default=0)
    return parser


def main(args):
    for name in ("supercategories", "categories", "prompts"):
        if getattr(args, name) is not None:
            setattr(args, name, [x.lower() for x in getattr(args, name)])
    from utils.reproducibility import seed_everything
    seed_everything(args.seed)
    return run_post_filtering(supercategories=args.supercategories, categories=args.categories, prompts=args.prompts,
                              human_sample_dir=args.human_sample_dir, save_dir=args.save_dir, IoU_threshold_min=args.IoU_threshold_min,
                              intersection_volume_ratio_threshold_max=args.intersection_volume_ratio_threshold_max,
                              inlier_num_threshold_min=args.inlier_num_threshold_min,
                              enable_aggregate_total_prompts=args.enable_aggregate_total_prompts, parallel_num=args.parallel_num,
                              parallel_idx=args.parallel_idx)


if __name__ == "__main__":
    main(build_parser().parse_args())
