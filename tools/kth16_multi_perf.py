#!/usr/bin/env python3
"""Multi-rank k-th value timings for 16-bit keys (GPU box): one JSON line per case, the method of tools/perfkit.py.
bfloat16 normal-distributed rows, smallest; device events around the call alone; the median of --reps calls on fresh inputs after
--warmup calls.  The sides ALTERNATE in one process, call by call, on the same rows:
  multi              lsdsort_kth16_multi_device with the case's ranks and an index buffer: ONE call
  multi_values       the same with a NULL index pointer (long rows: two reads of the row, no count, pick or locate)
  baseline           what a caller had before the entry: one lsdsort_kth16_device call per rank with an index buffer, timed as
                     one window
  baseline_values    the same with a NULL index pointer
With --baseline-lib the baselines run in a library built from the parent commit (only names that exist there are used:
lsdsort_kth16_workspace_bytes, lsdsort_kth16_device, lsdsort_check_device); without, in this tree's library.
Each baseline is measured --spread-repeats times over (each a median of --reps windows, alternating with the other sides in the
first): "<baseline>_spread_ms" is the largest minus the smallest of those medians, and "<baseline>_ms" their median.  "ahead" and
"values_ahead" say whether a side is ahead of ITS baseline by more than that baseline's spread; "gated" whether the shape counts for
the acceptance (long rows; the short tiers read the row once either way and are recorded only).  After the timing all sides run
once more, untimed, on the same rows, and the tool asserts that they agree bit for bit, values and positions.
Rank sets: the adjacent pair around the median (m = 2), the quartiles (m = 3), and the eight percentiles 1, 5, 25, 50, 75, 95, 99
and 99.9 (m = 8).  Shapes: [128 x 128256], [4096 x 131072], [1 x 2^28] (long rows) and [2^14 x 2^14], [2^20 x 256] (short rows).
The bytes-per-key figures divide a time by 5.5 TB/s: byte ACCOUNTING of a time, not a measured traffic.
Usage: python tools/kth16_multi_perf.py [--reps 20] [--warmup 3] [--spread-repeats 5] [--only SHAPE] [--baseline-lib PATH] [--out FILE]"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import lsdradixsort_amd as lsd
import perfkit

BF16 = 3
BASELINES = ("baseline", "baseline_values")
BASELINE_ENTRIES = ("lsdsort_kth16_workspace_bytes", "lsdsort_kth16_device", "lsdsort_check_device")


def rank_sets(cols):
    percentiles = (0.01, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99, 0.999)
    return {"median_pair": [(cols - 1) // 2, cols // 2],
            "quartiles": [cols // 4, cols // 2, 3 * cols // 4],
            "percentiles8": [min(cols - 1, int(p * (cols - 1))) for p in percentiles]}


def run_case(shape, set_name, rows, cols, ranks, a, base):
    n, m = rows * cols, len(ranks)
    g = torch.Generator(device="cuda").manual_seed(1)
    dev = {"device": "cuda"}
    x = torch.empty((rows, cols), dtype=torch.bfloat16, **dev)
    out_k, out_i = torch.empty((rows, m), dtype=torch.bfloat16, **dev), torch.empty((rows, m), dtype=torch.int32, **dev)
    out_v = torch.empty((rows, m), dtype=torch.bfloat16, **dev)
    one_k, one_i = torch.empty((m, rows), dtype=torch.bfloat16, **dev), torch.empty((m, rows), dtype=torch.int32, **dev)
    one_v = torch.empty((m, rows), dtype=torch.bfloat16, **dev)
    L = lsd.lib()
    c_ranks = (ctypes.c_size_t * m)(*ranks)
    ws = torch.empty(L.lsdsort_kth16_multi_workspace_bytes(rows, cols, m), dtype=torch.uint8, **dev)
    ws_b = torch.empty(base.lsdsort_kth16_workspace_bytes(rows, cols), dtype=torch.uint8, **dev)
    stream = int(torch.cuda.current_stream().cuda_stream)

    def multi():
        st = L.lsdsort_kth16_multi_device(x.data_ptr(), rows, cols, c_ranks, m, BF16, 0, out_k.data_ptr(), out_i.data_ptr(),
                                          ws.data_ptr(), ws.numel(), stream)
        assert st == 0, st

    def multi_values():
        st = L.lsdsort_kth16_multi_device(x.data_ptr(), rows, cols, c_ranks, m, BF16, 0, out_v.data_ptr(), None, ws.data_ptr(), ws.numel(),
                                          stream)
        assert st == 0, st

    def baseline():
        for j, rank in enumerate(ranks):
            st = base.lsdsort_kth16_device(x.data_ptr(), rows, cols, rank, BF16, 0, one_k[j].data_ptr(), one_i[j].data_ptr(),
                                           ws_b.data_ptr(), ws_b.numel(), stream)
            assert st == 0, st

    def baseline_values():
        for j, rank in enumerate(ranks):
            st = base.lsdsort_kth16_device(x.data_ptr(), rows, cols, rank, BF16, 0, one_v[j].data_ptr(), None, ws_b.data_ptr(),
                                           ws_b.numel(), stream)
            assert st == 0, st

    sides = {"multi": multi, "multi_values": multi_values, "baseline": baseline, "baseline_values": baseline_values}
    medians = perfkit.measure(sides, BASELINES, a.spread_repeats, a.reps, a.warmup, fresh=lambda: x.normal_(0.0, 1.0, generator=g))
    assert L.lsdsort_check_device(ws.data_ptr(), None) == 0 and base.lsdsort_check_device(ws_b.data_ptr(), None) == 0
    # once more, untimed, on the same rows: the sides answer the same question, bit for bit
    for fn in sides.values():
        fn()
    torch.cuda.synchronize()
    assert L.lsdsort_check_device(ws.data_ptr(), None) == 0 and base.lsdsort_check_device(ws_b.data_ptr(), None) == 0
    bits = lambda t: t.contiguous().view(torch.int16)
    assert torch.equal(bits(out_k), bits(one_k.t())), "multi and the baseline disagree in a value"
    assert torch.equal(out_i, one_i.t()), "multi and the baseline disagree in a position"
    assert torch.equal(bits(out_v), bits(out_k)) and torch.equal(bits(one_v), bits(one_k)), "values only and with positions disagree"
    b, bv = medians["baseline"], medians["baseline_values"]
    multi_ms, values_ms = medians["multi"][0], medians["multi_values"][0]
    (base_ms, spread), (base_v_ms, spread_v) = perfkit.spread_of(b), perfkit.spread_of(bv)
    which = " (parent commit's library)" if a.baseline_lib else " (this tree's library)"
    return {"shape": shape, "ranks": set_name, "rows": rows, "cols": cols, "num_ranks": m, "rank_values": ranks, "dtype": "bfloat16",
            "largest": False, "reps": a.reps, "warmup": a.warmup, "gated": cols > 16384,
            "multi_ms": multi_ms, "multi_values_ms": values_ms,
            "baseline": f"{m} x lsdsort_kth16_device with positions" + which, "baseline_ms": base_ms, "baseline_repeats_ms": b,
            "baseline_spread_ms": spread,
            "baseline_values": f"{m} x lsdsort_kth16_device, NULL index pointer" + which, "baseline_values_ms": base_v_ms,
            "baseline_values_repeats_ms": bv, "baseline_values_spread_ms": spread_v,
            "speedup_vs_baseline": base_ms / multi_ms, "ahead": bool(base_ms - multi_ms > spread),
            "values_speedup_vs_baseline": base_v_ms / values_ms, "values_ahead": bool(base_v_ms - values_ms > spread_v),
            "multi_bytes_per_key_at_5p5TBs": perfkit.bytes_per_key(multi_ms, n),
            "multi_values_bytes_per_key_at_5p5TBs": perfkit.bytes_per_key(values_ms, n),
            "workspace_bytes": ws.numel(), "baseline_workspace_bytes": ws_b.numel()}


SHAPES = {
    "rows_128x128256": (128, 128256),
    "rows_4096x131072": (4096, 131072),
    "one_row_2p28": (1, 1 << 28),
    "rows_16384x16384": (1 << 14, 1 << 14),
    "rows_1048576x256": (1 << 20, 256),
}


def parser():
    return perfkit.parser(__doc__, spread_repeats=5, lib_flag="--baseline-lib")


def main():
    a = parser().parse_args()
    base = perfkit.bound_library(a.baseline_lib, BASELINE_ENTRIES)
    perfkit.run_cases(a, SHAPES, lambda shape, rows, cols: (run_case(shape, set_name, rows, cols, ranks, a, base)
                                                            for set_name, ranks in rank_sets(cols).items()))


if __name__ == "__main__":
    main()
