#!/bin/bash
# A/B of library variants on the key/value configuration (2^27 pairs): tools/ab_pairs_bench.sh <tag>...
set -e
REPO=${GRAFT_REPO_ROOT:-$(pwd)}
sides=(); for v in "$@"; do sides+=(--side "$v" "LSDSORT_LIB=$REPO/lsdradixsort_amd/liblsdsort$v.so"); done
python $REPO/tools/ab.py --rounds 3 --bench $REPO/bench.py \
  --common "--full --pairs --log2-keys 27 --steps 20 --warmup 3 --no-cpu-baseline --no-extra" "${sides[@]}"
