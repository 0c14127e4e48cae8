#!/bin/bash
# stage-1 time of library variants: tools/hist_variants.sh <tag>...   (first two lines of tools/hist_size_sweep.py each)
# Every run has its own time limit, and the first one that fails ends the script (awk reads the run to its end: no broken pipe).
set -eo pipefail
REPO=${GRAFT_REPO_ROOT:-$(pwd)}
for round in 1 2; do
  for v in "$@"; do
    echo "== $v"
    LSDSORT_LIB=$REPO/lsdradixsort_amd/liblsdsort$v.so timeout -k 10 300 python $REPO/tools/hist_size_sweep.py 2>/dev/null | awk 'NR <= 2'
  done
done
