#!/bin/bash
# Per-GPU fan-out of the depth optimisation (the reference's scripts/generation/optimize_depth.sh): one process per GPU, each taking
# slice --parallel_idx of --parallel_num of the sorted work list; processes share nothing but the file system.
# The accepted flags are the reference's explicit set -- anything else is an error, not forwarded -- plus the three additions of
# src/generation/optimize_depth.py (--asset_obj_root, --volume_resolution, --perturb_view_num).  --skip_done is on unless --no_skip_done
# is given.  --human_prefilter_dir is accepted and dropped, as the reference's script does.
set -e
gpu_ids=(0 1 2 3 4 5 6 7)
value_flags=" inpaint_dir asset_seg_dir human_initial_dir human_preds_dir camera_dir save_dir smplx_path maximum_candidates ransac_threshold triangulation_threshold num_epoch minimum_inliers lr w_collision w_multiview w_refview seed asset_obj_root volume_resolution perturb_view_num "
list_flags=" supercategories categories prompts "
bool_flags=" disable_lowres_switch_for_behave enable_aggregate_total_prompts no_initialize no_collision verbose "
args=()
skip_done=true
while [[ $# -gt 0 ]]; do
  name=${1#--}
  if [[ $1 == --gpus ]]; then
    shift; gpu_ids=()
    while [[ $# -gt 0 && $1 != --* ]]; do gpu_ids+=("$1"); shift; done
  elif [[ $1 == --no_skip_done ]]; then
    skip_done=false; shift
  elif [[ $1 == --human_prefilter_dir ]]; then
    shift 2
  elif [[ $1 == --* && $list_flags == *" $name "* ]]; then
    args+=("$1"); shift
    while [[ $# -gt 0 && $1 != --* ]]; do args+=("$1"); shift; done
  elif [[ $1 == --* && $value_flags == *" $name "* ]]; then
    [[ $# -ge 2 ]] || { echo "optimize_depth.sh: $1 needs a value" >&2; exit 2; }
    args+=("$1" "$2"); shift 2
  elif [[ $1 == --* && $bool_flags == *" $name "* ]]; then
    args+=("$1"); shift
  else
    echo "optimize_depth.sh: unknown argument '$1'" >&2; exit 2
  fi
done
[[ $skip_done == true ]] && args+=(--skip_done)
n=${#gpu_ids[@]}
i=0
pids=()
for g in "${gpu_ids[@]}"; do
  HIP_VISIBLE_DEVICES=$g python src/generation/optimize_depth.py "${args[@]}" --parallel_idx $i --parallel_num $n &
  pids+=($!)
  i=$((i + 1))
done
# a bare `wait` returns 0 whatever the children did: wait for each, and fail when one of them failed
rc=0
for p in "${pids[@]}"; do wait "$p" || rc=$?; done
exit $rc
