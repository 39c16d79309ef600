#!/bin/bash
# Run ON THE GPU BOX (via gpurun), at the end of a round: everything that is copied into profiles/ afterwards.
#   tools/ablate.sh render_fwd_merged.hip mstamps=-DVAMP_MERGED_STAMPS      (here, before the call: the stamps build)
#   bash tools/collect_round.sh r06 <out>      (on the GPU machine, about an hour; <out> = the folder to keep)
# Outputs: profiles_<tag>/ (tools/collect_profiles.sh) and pmc_<tag>/summary.txt (tools/pmc_passes.sh) where those scripts
# write them; under <out>: merged_timeline_<tag>.txt, pytest_gpu.log (the whole -m gpu suite), bench_<tag>.json (the
# bench.py --full line) and the logs of the steps.
TAG=${1:-r06}
OUT=${2:?usage: tools/collect_round.sh <tag> <output folder>}
mkdir -p "$OUT" && OUT=$(realpath "$OUT")
cd $GRAFT_REPO_ROOT
bash tools/collect_profiles.sh $TAG B > $OUT/collect.log 2>&1
cd $GRAFT_REPO_ROOT
bash tools/pmc_passes.sh $TAG B 1 > $OUT/pmc.log 2>&1
cd $GRAFT_REPO_ROOT
if [ -f vampire_amd/_lib/abl_mstamps.so ]; then
  VAMPIRE_HIP_LIB=$PWD/vampire_amd/_lib/abl_mstamps.so python tools/debug/merged_stamps.py B 1 $OUT/merged_timeline_$TAG.txt > $OUT/stamps.log 2>&1
fi
timeout 2400 python -m pytest tests -x -q -m gpu > $OUT/pytest_gpu.log 2>&1; grep -E "passed|failed|rror" $OUT/pytest_gpu.log | tail -3
python bench.py --full 2>/dev/null | tail -1 > $OUT/bench_$TAG.json; cut -c1-300 $OUT/bench_$TAG.json
