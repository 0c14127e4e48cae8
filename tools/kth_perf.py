#!/usr/bin/env python3
"""K-th value timings (GPU box): one JSON line per case, the method of tools/perfkit.py.  float32
normal-distributed rows, smallest, with positions; device events around the call alone; the median of --reps calls on fresh inputs
after --warmup calls.  The sides ALTERNATE in one process, call by call, on the same rows:
  kth        lsdsort_kth_device at the given rank
  baseline   what a caller had before the entry: lsdsort_topk_device with k = rank + 1, smallest, whose last column is the answer.
             With --baseline-lib it is timed in a library built from the parent commit (only names that exist there are used:
             lsdsort_topk_workspace_bytes, lsdsort_topk_device, lsdsort_check_device); without, in this tree's library.
  torch      torch.kthvalue(x, rank + 1, dim=-1) (torch.median is this call at the lower-median rank), for the record:
             --torch-reps calls after one warm-up
The baseline is measured --spread-repeats times over (each a median of --reps calls, alternating with kth in the first):
"baseline_spread_ms" is the largest minus the smallest of those medians, and "baseline_ms" their median.  "ahead" says whether kth
is ahead of the baseline by more than that spread.
Cases: the lower-median rank of [64 x 2^22], [4096 x 131072], [1 x 2^28], [2^14 x 2^14], [2^20 x 256]; rank 1023 of [1 x 2^28].
Usage: python tools/kth_perf.py [--reps 20] [--warmup 3] [--spread-repeats 5] [--torch-reps 3] [--only NAME] [--baseline-lib PATH]
                                [--out FILE]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import lsdradixsort_amd as lsd
import perfkit

F32 = 2
BASELINE_ENTRIES = ("lsdsort_topk_workspace_bytes", "lsdsort_topk_device", "lsdsort_check_device")


def run_case(name, rows, cols, rank, a, base):
    n = rows * cols
    k = rank + 1
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.empty((rows, cols), dtype=torch.float32, device="cuda")
    out_k = torch.empty(rows, dtype=torch.float32, device="cuda")
    out_i = torch.empty(rows, dtype=torch.int32, device="cuda")
    top_k = torch.empty((rows, k), dtype=torch.float32, device="cuda")
    top_i = torch.empty((rows, k), dtype=torch.int32, device="cuda")
    L = lsd.lib()
    ws = torch.empty(L.lsdsort_kth_workspace_bytes(rows, cols), dtype=torch.uint8, device="cuda")
    ws_b = torch.empty(base.lsdsort_topk_workspace_bytes(rows, cols, k), dtype=torch.uint8, device="cuda")
    stream = int(torch.cuda.current_stream().cuda_stream)

    def kth():
        st = L.lsdsort_kth_device(x.data_ptr(), rows, cols, rank, F32, 0, out_k.data_ptr(), out_i.data_ptr(), ws.data_ptr(), ws.numel(),
                                  stream)
        assert st == 0, st

    def baseline():
        st = base.lsdsort_topk_device(x.data_ptr(), rows, cols, k, F32, 0, top_k.data_ptr(), top_i.data_ptr(), ws_b.data_ptr(),
                                      ws_b.numel(), stream)
        assert st == 0, st

    sides = {"kth": kth, "baseline": baseline}
    medians = perfkit.measure(sides, {"baseline"}, a.spread_repeats, a.reps, a.warmup, fresh=lambda: x.normal_(0.0, 1.0, generator=g))
    assert L.lsdsort_check_device(ws.data_ptr(), None) == 0 and base.lsdsort_check_device(ws_b.data_ptr(), None) == 0
    # once more, untimed, on the same rows: the two sides answer the same question
    kth()
    baseline()
    torch.cuda.synchronize()
    assert torch.equal(out_k, top_k[:, -1]) and torch.equal(out_i, top_i[:, -1]), "kth and the baseline disagree"
    b = medians["baseline"]
    kth_ms, (base_ms, spread) = medians["kth"][0], perfkit.spread_of(b)
    out = {"case": name, "rows": rows, "cols": cols, "rank": rank, "dtype": "float32", "largest": False, "positions": True,
           "reps": a.reps, "warmup": a.warmup, "kth_ms": kth_ms,
           "baseline": "lsdsort_topk_device k=rank+1" + (" (parent commit's library)" if a.baseline_lib else " (this tree's library)"),
           "baseline_ms": base_ms, "baseline_repeats_ms": b, "baseline_spread_ms": spread,
           "speedup_vs_baseline": base_ms / kth_ms, "ahead": bool(base_ms - kth_ms > spread),
           "kth_bytes_per_key_at_5p5TBs": perfkit.bytes_per_key(kth_ms, n), "kth_TBs_at_4B_per_key": 4.0 * n / (kth_ms * 1e-3) / 1e12,
           "workspace_bytes": ws.numel(), "baseline_workspace_bytes": ws_b.numel()}
    del top_k, top_i, ws_b
    torch.cuda.empty_cache()
    if a.torch_reps > 0:
        ts = []
        for i in range(1 + a.torch_reps):
            x.normal_(0.0, 1.0, generator=g)
            t = perfkit.one(lambda: torch.kthvalue(x, k, dim=-1))
            if i >= 1:
                ts.append(t)
            elif t > 2000.0:   # seconds per call: the warm-up call is the record
                ts.append(t)
                break
        out["torch_kthvalue_ms"] = float(np.median(ts))
        out["torch_reps"] = len(ts)
    return out


def lower_median(cols):
    return (cols - 1) // 2


CASES = {
    "rows_64x4194304_median": (64, 1 << 22, lower_median(1 << 22)),
    "rows_4096x131072_median": (4096, 131072, lower_median(131072)),
    "one_row_2p28_median": (1, 1 << 28, lower_median(1 << 28)),
    "one_row_2p28_rank1023": (1, 1 << 28, 1023),
    "rows_16384x16384_median": (1 << 14, 1 << 14, lower_median(1 << 14)),
    "rows_1048576x256_median": (1 << 20, 256, lower_median(256)),
}


def parser():
    ap = perfkit.parser(__doc__, spread_repeats=5, lib_flag="--baseline-lib")
    ap.add_argument("--torch-reps", type=int, default=3)
    return ap


def main():
    a = parser().parse_args()
    base = perfkit.bound_library(a.baseline_lib, BASELINE_ENTRIES)
    perfkit.run_cases(a, CASES, lambda name, rows, cols, rank: run_case(name, rows, cols, rank, a, base))


if __name__ == "__main__":
    main()
