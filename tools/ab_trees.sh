#!/bin/bash
# A/B two checked-out trees with their own bench.py on one box: [AB_ROUNDS=3] [AB_ARGS="--pairs"] tools/ab_trees.sh <dir> <dir> ...
# (interleaved; prints: tree value ms_per_step histogram scatter_per_pass local_stage).  A bench that fails ends the script.
set -o pipefail
for round in $(seq ${AB_ROUNDS:-3}); do
  for d in "$@"; do
    out=$(cd "$d" && timeout -k 10 150 python bench.py --full --steps 20 --warmup 3 --no-cpu-baseline --no-extra $AB_ARGS 2>/dev/null | tail -1)
    status=$?
    if [ $status -ne 0 ] || [ -z "$out" ]; then echo "$d: bench.py failed (status $status), stopping" >&2; exit 1; fi
    echo "$d $(echo "$out" | python -c 'import sys,json; d=json.loads(sys.stdin.read()); s=d["stages_ms"]; print(d["value"], d["ms_per_step"], s["histogram"], s["scatter_per_pass"], s.get("local_stage"))')"
  done
done
