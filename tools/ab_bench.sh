#!/bin/bash
# A/B library variants with bench.py itself (same process shape as the driver's run): tools/ab_bench.sh <tag>...
set -e
REPO=${GRAFT_REPO_ROOT:-$(pwd)}
sides=(); for v in "$@"; do sides+=(--side "$v" "LSDSORT_LIB=$REPO/lsdradixsort_amd/liblsdsort$v.so"); done
python $REPO/tools/ab.py --rounds 2 --bench $REPO/bench.py "${sides[@]}"
