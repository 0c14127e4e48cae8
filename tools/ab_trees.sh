#!/bin/bash
# A/B two checked-out trees with their own bench.py on one box: [AB_ROUNDS=3] [AB_ARGS="--pairs"] tools/ab_trees.sh <dir> <dir> ...
# (interleaved; prints: tree value ms_per_step histogram scatter_per_pass tile_keys local_stage).  A bench that fails ends the script.
set -e
sides=(); for d in "$@"; do sides+=(--side "$d" "@$d"); done
python "$(dirname "$0")/ab.py" --rounds ${AB_ROUNDS:-3} --bench bench.py \
  --common "--full --steps 20 --warmup 3 --no-cpu-baseline --no-extra $AB_ARGS" "${sides[@]}"
