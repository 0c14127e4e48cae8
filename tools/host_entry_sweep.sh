#!/bin/bash
# the host entry's time over its feed chunk: every run under its own time limit, the first one that fails ends the script
set -eo pipefail
for c in 22 24 26 28; do echo "chunk 2^$c"; LSDSORT_FEED_CHUNK_LOG2=$c timeout -k 10 300 python tools/host_entry_perf.py 2>&1 | grep "n=2^28"; done
