#!/usr/bin/env python3
"""Multi-rank k-th value timings (GPU box): one JSON line per case, the method of tools/perfkit.py.  float32 normal-distributed
rows, smallest, with positions; device events around the call alone; the median of --reps calls on fresh inputs after --warmup
calls.  The sides ALTERNATE in one process, call by call, on the same rows:
  multi      lsdsort_kth_multi_device with the case's ranks: ONE call
  baseline   what a caller had before the entry: one lsdsort_kth_device call per rank, timed as one window.  With --baseline-lib
             it runs in a library built from the parent commit (only names that exist there are used:
             lsdsort_kth_workspace_bytes, lsdsort_kth_device, lsdsort_check_device); without, in this tree's library.
The baseline is measured --spread-repeats times over (each a median of --reps windows, alternating with multi in the first):
"baseline_spread_ms" is the largest minus the smallest of those medians, and "baseline_ms" their median.  "ahead" says whether
multi is ahead of the baseline by more than that spread.  After the timing both sides run once more, untimed, on the same rows, and
the tool asserts that they agree bit for bit, values and positions.
Rank sets: the adjacent pair around the median (m = 2), the quartiles (m = 3), and the eight percentiles 1, 5, 25, 50, 75, 95, 99
and 99.9 (m = 8).  Shapes: [64 x 2^22], [4096 x 131072], [1 x 2^28] (long rows) and [2^14 x 2^14], [2^20 x 256] (short rows).
Usage: python tools/kth_multi_perf.py [--reps 20] [--warmup 3] [--spread-repeats 5] [--only SHAPE] [--baseline-lib PATH] [--out FILE]"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import lsdradixsort_amd as lsd
import perfkit

F32 = 2
BASELINE_ENTRIES = ("lsdsort_kth_workspace_bytes", "lsdsort_kth_device", "lsdsort_check_device")


def rank_sets(cols):
    percentiles = (0.01, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99, 0.999)
    return {"median_pair": [(cols - 1) // 2, cols // 2],
            "quartiles": [cols // 4, cols // 2, 3 * cols // 4],
            "percentiles8": [min(cols - 1, int(p * (cols - 1))) for p in percentiles]}


def run_case(shape, set_name, rows, cols, ranks, a, base):
    n, m = rows * cols, len(ranks)
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.empty((rows, cols), dtype=torch.float32, device="cuda")
    out_k = torch.empty((rows, m), dtype=torch.float32, device="cuda")
    out_i = torch.empty((rows, m), dtype=torch.int32, device="cuda")
    one_k = torch.empty((m, rows), dtype=torch.float32, device="cuda")
    one_i = torch.empty((m, rows), dtype=torch.int32, device="cuda")
    L = lsd.lib()
    c_ranks = (ctypes.c_size_t * m)(*ranks)
    ws = torch.empty(L.lsdsort_kth_multi_workspace_bytes(rows, cols, m), dtype=torch.uint8, device="cuda")
    ws_b = torch.empty(base.lsdsort_kth_workspace_bytes(rows, cols), dtype=torch.uint8, device="cuda")
    stream = int(torch.cuda.current_stream().cuda_stream)

    def multi():
        st = L.lsdsort_kth_multi_device(x.data_ptr(), rows, cols, c_ranks, m, F32, 0, out_k.data_ptr(), out_i.data_ptr(), ws.data_ptr(),
                                        ws.numel(), stream)
        assert st == 0, st

    def baseline():
        for j, rank in enumerate(ranks):
            st = base.lsdsort_kth_device(x.data_ptr(), rows, cols, rank, F32, 0, one_k[j].data_ptr(), one_i[j].data_ptr(), ws_b.data_ptr(),
                                         ws_b.numel(), stream)
            assert st == 0, st

    sides = {"multi": multi, "baseline": baseline}
    medians = perfkit.measure(sides, {"baseline"}, a.spread_repeats, a.reps, a.warmup, fresh=lambda: x.normal_(0.0, 1.0, generator=g))
    assert L.lsdsort_check_device(ws.data_ptr(), None) == 0 and base.lsdsort_check_device(ws_b.data_ptr(), None) == 0
    # once more, untimed, on the same rows: the two sides answer the same question, bit for bit
    multi()
    baseline()
    torch.cuda.synchronize()
    assert torch.equal(out_k.view(torch.int32), one_k.t().contiguous().view(torch.int32)), "multi and the baseline disagree in a value"
    assert torch.equal(out_i, one_i.t()), "multi and the baseline disagree in a position"
    b = medians["baseline"]
    multi_ms, (base_ms, spread) = medians["multi"][0], perfkit.spread_of(b)
    return {"shape": shape, "ranks": set_name, "rows": rows, "cols": cols, "num_ranks": m, "rank_values": ranks, "dtype": "float32",
            "largest": False, "positions": True, "reps": a.reps, "warmup": a.warmup, "multi_ms": multi_ms,
            "baseline": f"{m} x lsdsort_kth_device" + (" (parent commit's library)" if a.baseline_lib else " (this tree's library)"),
            "baseline_ms": base_ms, "baseline_repeats_ms": b, "baseline_spread_ms": spread,
            "speedup_vs_baseline": base_ms / multi_ms, "ahead": bool(base_ms - multi_ms > spread),
            "multi_TBs_at_4B_per_key": 4.0 * n / (multi_ms * 1e-3) / 1e12, "multi_bytes_per_key_at_5p5TBs": perfkit.bytes_per_key(multi_ms, n),
            "workspace_bytes": ws.numel(), "baseline_workspace_bytes": ws_b.numel()}


SHAPES = {
    "rows_64x4194304": (64, 1 << 22),
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
