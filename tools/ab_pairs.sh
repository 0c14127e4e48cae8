#!/bin/bash
# interleaved A/B of (library tag, tile config) pairs through bench.py: tools/ab_pairs.sh tag:cfg ...  ("" tag = product library)
set -e
REPO=${GRAFT_REPO_ROOT:-$(pwd)}
sides=(); for pair in "$@"; do sides+=(--side "$pair" "LSDSORT_LIB=$REPO/lsdradixsort_amd/liblsdsort${pair%%:*}.so --tile-config ${pair##*:}"); done
python $REPO/tools/ab.py --rounds 3 --bench $REPO/bench.py "${sides[@]}"
