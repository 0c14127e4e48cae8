#!/bin/bash
# A/B library variants on the hybrid form's stages with bench.py: tools/ab_local.sh <tag>...   ("" = the product)
set -e
REPO=${GRAFT_REPO_ROOT:-$(pwd)}
sides=(); for v in "$@"; do sides+=(--side "lib$v" "LSDSORT_LIB=$REPO/lsdradixsort_amd/liblsdsort$v.so"); done
python $REPO/tools/ab.py --rounds 2 --timeout 100 --bench $REPO/bench.py \
  --common "--full --steps 20 --warmup 3 --no-cpu-baseline --no-extra --no-live-traffic $AB_ARGS" "${sides[@]}"
