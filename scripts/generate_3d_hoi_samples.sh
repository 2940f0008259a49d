#!/bin/bash
# Same flags as the reference's scripts/generate_3d_hoi_samples.sh (--gpus --dataset_type --supercategory --category --no_skip_done):
# the 2D -> 3D lifting stages this repository has, in the reference's order.  predict_human (the third-party pose estimator) is not
# part of this repository: its pickles under results/generation/human_preds must already be there.
set -e
gpu_ids=(0 1 2 3 4 5 6 7)
skip_done=true
while [[ $# -gt 0 ]]; do
  case $1 in
    --gpus) shift; gpu_ids=(); while [[ $# -gt 0 && $1 != --* ]]; do gpu_ids+=("$1"); shift; done ;;
    --dataset_type) shift 2 ;;
    --supercategory) supercategory="$2"; shift 2 ;;
    --category) category="$2"; shift 2 ;;
    --no_skip_done) skip_done=false; shift 1 ;;
    *) echo "Unknown option: $1"; exit 1 ;;
  esac
done
sel=(--supercategories "$supercategory" --categories "$category")
py_skip=(); sh_skip=()
if [[ $skip_done == true ]]; then py_skip=(--skip_done); else sh_skip=(--no_skip_done); fi
n=${#gpu_ids[@]}

# one process per GPU over slices of the sorted work list, for the stages that have no launcher script of their own
fan_out() {
  local i=0 rc=0 pids=() p
  for g in "${gpu_ids[@]}"; do
    HIP_VISIBLE_DEVICES=$g python "$@" --parallel_idx $i --parallel_num $n &
    pids+=($!)
    i=$((i + 1))
  done
  for p in "${pids[@]}"; do wait "$p" || rc=$?; done   # a bare `wait` would lose a child's failure and the next stage would run
  return $rc
}

python src/generation/segment_human.py "${sel[@]}" "${py_skip[@]}"
echo "predict_human: skipped (not part of this repository); reading results/generation/human_preds as it is"
fan_out src/generation/initialize_depth.py "${sel[@]}" "${py_skip[@]}"
bash scripts/generation/optimize_depth.sh "${sel[@]}" --gpus "${gpu_ids[@]}" "${sh_skip[@]}"
fan_out src/generation/compute_metrics.py "${sel[@]}" "${py_skip[@]}"
