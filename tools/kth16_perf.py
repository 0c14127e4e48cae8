#!/usr/bin/env python3
"""K-th value timings for 16-bit keys (GPU box): one JSON line per case, the method of tools/perfkit.py.  bfloat16
normal-distributed rows, smallest; device events around the call alone; the median of --reps calls on fresh inputs after --warmup
calls.  The sides ALTERNATE in one process, call by call, on the same rows:
  kth16              lsdsort_kth16_device at the given rank, with positions
  kth16_values_only  the same with a NULL index pointer (long rows: no count, pick or locate)
  baseline_topk16    what a caller had before the entry, detour A: lsdsort_topk16_device with k = rank + 1, smallest, whose last
                     column is the answer
  baseline_float32   detour B: the rows converted to float32 (into a buffer that exists already; the conversion IS in the time)
                     and lsdsort_kth_device on the copy
                     With --baseline-lib both baselines are timed in a library built from the parent commit (only names that exist
                     there are used: lsdsort_topk16_workspace_bytes, lsdsort_topk16_device, lsdsort_kth_workspace_bytes,
                     lsdsort_kth_device, lsdsort_check_device); without, in this tree's library.
  torch              torch.kthvalue(x, rank + 1, dim=-1) (torch.median is this call at the lower-median rank), for the record:
                     --torch-reps calls after one warm-up
Each baseline is measured --spread-repeats times over (each a median of --reps calls, alternating with the other sides in the
first): "<baseline>_spread_ms" is the largest minus the smallest of those medians, and "<baseline>_ms" their median.  "ahead" and
"values_only_ahead" say whether the side is ahead of the FASTER of the two baselines by more than that baseline's spread.
After the timed calls every side runs once more on the same rows and the tool asserts that they agree.
Cases: the lower-median rank of [128 x 128256], [4096 x 131072], [1 x 2^28], [2^14 x 2^14], [2^20 x 256]; rank 1023 of [1 x 2^28].
Usage: python tools/kth16_perf.py [--reps 20] [--warmup 3] [--spread-repeats 5] [--torch-reps 3] [--only NAME] [--baseline-lib PATH]
                                  [--out FILE]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import lsdradixsort_amd as lsd
import perfkit

F32, BF16 = 2, 3
BASELINES = ("baseline_topk16", "baseline_float32")
BASELINE_ENTRIES = ("lsdsort_topk16_workspace_bytes", "lsdsort_kth_workspace_bytes", "lsdsort_topk16_device", "lsdsort_kth_device",
                    "lsdsort_check_device")


def run_case(name, rows, cols, rank, a, base):
    n = rows * cols
    k = rank + 1
    g = torch.Generator(device="cuda").manual_seed(1)
    dev = {"device": "cuda"}
    x = torch.empty((rows, cols), dtype=torch.bfloat16, **dev)
    wide = torch.empty((rows, cols), dtype=torch.float32, **dev)   # detour B's temporary: rows x cols x 4 bytes
    out_k, out_i = torch.empty(rows, dtype=torch.bfloat16, **dev), torch.empty(rows, dtype=torch.int32, **dev)
    out_v = torch.empty(rows, dtype=torch.bfloat16, **dev)
    top_k, top_i = torch.empty((rows, k), dtype=torch.bfloat16, **dev), torch.empty((rows, k), dtype=torch.int32, **dev)
    f_k, f_i = torch.empty(rows, dtype=torch.float32, **dev), torch.empty(rows, dtype=torch.int32, **dev)
    L = lsd.lib()
    ws = torch.empty(L.lsdsort_kth16_workspace_bytes(rows, cols), dtype=torch.uint8, **dev)
    ws_a = torch.empty(base.lsdsort_topk16_workspace_bytes(rows, cols, k), dtype=torch.uint8, **dev)
    ws_b = torch.empty(base.lsdsort_kth_workspace_bytes(rows, cols), dtype=torch.uint8, **dev)
    stream = int(torch.cuda.current_stream().cuda_stream)

    def kth16():
        st = L.lsdsort_kth16_device(x.data_ptr(), rows, cols, rank, BF16, 0, out_k.data_ptr(), out_i.data_ptr(), ws.data_ptr(), ws.numel(),
                                    stream)
        assert st == 0, st

    def kth16_values_only():
        st = L.lsdsort_kth16_device(x.data_ptr(), rows, cols, rank, BF16, 0, out_v.data_ptr(), None, ws.data_ptr(), ws.numel(), stream)
        assert st == 0, st

    def baseline_topk16():
        st = base.lsdsort_topk16_device(x.data_ptr(), rows, cols, k, BF16, 0, top_k.data_ptr(), top_i.data_ptr(), ws_a.data_ptr(),
                                        ws_a.numel(), stream)
        assert st == 0, st

    def baseline_float32():
        wide.copy_(x)
        st = base.lsdsort_kth_device(wide.data_ptr(), rows, cols, rank, F32, 0, f_k.data_ptr(), f_i.data_ptr(), ws_b.data_ptr(),
                                     ws_b.numel(), stream)
        assert st == 0, st

    sides = {"kth16": kth16, "kth16_values_only": kth16_values_only, "baseline_topk16": baseline_topk16,
             "baseline_float32": baseline_float32}
    medians = perfkit.measure(sides, BASELINES, a.spread_repeats, a.reps, a.warmup, fresh=lambda: x.normal_(0.0, 1.0, generator=g))
    assert L.lsdsort_check_device(ws.data_ptr(), None) == 0
    for w in (ws_a, ws_b):
        assert base.lsdsort_check_device(w.data_ptr(), None) == 0
    # once more, untimed, on the same rows: every side answers the same question
    for fn in sides.values():
        fn()
    torch.cuda.synchronize()
    assert L.lsdsort_check_device(ws.data_ptr(), None) == 0
    bits = lambda t: t.view(torch.int16)
    assert torch.equal(bits(out_k), bits(top_k[:, -1].contiguous())) and torch.equal(out_i, top_i[:, -1]), "kth16 and top-k disagree"
    assert torch.equal(bits(out_v), bits(out_k)), "values only and with positions disagree"
    assert torch.equal(out_k.float().view(torch.int32), f_k.view(torch.int32)) and torch.equal(out_i, f_i), "kth16 and float32 disagree"
    out = {"case": name, "rows": rows, "cols": cols, "rank": rank, "dtype": "bfloat16", "largest": False, "reps": a.reps,
           "warmup": a.warmup, "kth16_ms": medians["kth16"][0], "kth16_values_only_ms": medians["kth16_values_only"][0],
           "baseline_library": "parent commit's" if a.baseline_lib else "this tree's"}
    best = None
    for side, what in (("baseline_topk16", "lsdsort_topk16_device k=rank+1"), ("baseline_float32", "float32 copy + lsdsort_kth_device")):
        b = medians[side]
        out[side] = what
        ms, spread = perfkit.spread_of(b)
        out[side + "_ms"], out[side + "_repeats_ms"], out[side + "_spread_ms"] = ms, b, spread
        if best is None or out[side + "_ms"] < out[best + "_ms"]:
            best = side
    base_ms, spread = out[best + "_ms"], out[best + "_spread_ms"]
    out.update({"faster_baseline": best, "gated": cols > 16384,
                "speedup_vs_faster_baseline": base_ms / out["kth16_ms"], "ahead": bool(base_ms - out["kth16_ms"] > spread),
                "values_only_speedup_vs_faster_baseline": base_ms / out["kth16_values_only_ms"],
                "values_only_ahead": bool(base_ms - out["kth16_values_only_ms"] > spread),
                "speedup_vs_float32": out["baseline_float32_ms"] / out["kth16_ms"],
                "kth16_bytes_per_key_at_5p5TBs": perfkit.bytes_per_key(out["kth16_ms"], n),
                "kth16_values_only_bytes_per_key_at_5p5TBs": perfkit.bytes_per_key(out["kth16_values_only_ms"], n),
                "workspace_bytes": ws.numel(), "baseline_topk16_workspace_bytes": ws_a.numel(),
                "baseline_float32_workspace_bytes": ws_b.numel() + 4 * n})
    del top_k, top_i, ws_a, ws_b, wide
    torch.cuda.empty_cache()
    if a.torch_reps > 0:
        ts = []
        try:
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
        except RuntimeError as e:   # torch has no such kernel for this dtype or size: say so, for the record
            out["torch_kthvalue_error"] = str(e).splitlines()[0][:200]
    return out


def lower_median(cols):
    return (cols - 1) // 2


CASES = {
    "rows_128x128256_median": (128, 128256, lower_median(128256)),
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
