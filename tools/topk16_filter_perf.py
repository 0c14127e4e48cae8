#!/usr/bin/env python3
"""Timings of the per-row-k entries for 16-bit keys (GPU box): one JSON line per case and mode, the method of tools/perfkit.py.
bfloat16 normal-distributed rows, largest, 16-byte aligned; device events around the call alone; the median of --reps calls on fresh
inputs after --warmup calls.  The sides ALTERNATE in one process, call by call, on the same rows.  Three modes per shape:
  perrow_k (the gate)   k_r drawn per row from {1, 20, 50, 100, 1000}, capped at cols - 1.
      filter            lsdsort_topk16_filter_device, fill -inf, into a second buffer
      filter_in_place   the same with d_out == d_keys (timed last: it changes the rows)
      baseline          what a caller had before: lsdsort_topk16_device(k = k_max), a gather of column k_r - 1, torch.where
  uniform_k (recorded)  k_r = 50 in every row.
      filter            as above
      baseline          lsdsort_kth16_device at rank 49, values only, then torch.where
  perrow_rank (recorded) the lower-median rank in every row, from the device array.
      perrow, perrow_values_only       lsdsort_kth16_perrow_device with and without positions
      baseline, baseline_values_only   lsdsort_kth16_device at that rank
With --baseline-lib the baselines' library calls are made in a library built from the parent commit (only names that exist there
are used); without, in this tree's library.  Each baseline is measured --spread-repeats times over (each a median of --reps calls,
alternating with the other sides in the first): "<baseline>_spread_ms" is the largest minus the smallest of those medians and
"<baseline>_ms" their median.  "verdict" is "ahead" where the side is faster than its baseline by more than that spread, "behind"
where it is slower by more than it, else "within spread".  After the timed calls every side runs once more on the same rows and
the tool asserts that they agree, bit for bit.
Shapes: [128 x 128256], [4096 x 131072], [1 x 2^28], [2^14 x 2^14], [2^20 x 256].
Usage: python tools/topk16_filter_perf.py [--reps 20] [--warmup 3] [--spread-repeats 5] [--only NAME] [--modes a,b] [--baseline-lib PATH]
                                          [--out profiles/topk16_filter_perf.jsonl]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import lsdradixsort_amd as lsd
import perfkit

BF16 = 3
NEG_INF_BITS = 0xFF80
BASELINE_ENTRIES = ("lsdsort_topk16_workspace_bytes", "lsdsort_kth16_workspace_bytes", "lsdsort_topk16_device", "lsdsort_kth16_device",
                    "lsdsort_check_device")


def measured(sides, baselines, x, g, a):
    return perfkit.measure(sides, baselines, a.spread_repeats, a.reps, a.warmup, fresh=lambda: x.normal_(0.0, 1.0, generator=g))


def report(out, medians, pairs, n):
    for side, baseline in pairs:
        b = medians[baseline]
        base_ms, spread = perfkit.spread_of(b)
        out[baseline + "_ms"], out[baseline + "_repeats_ms"], out[baseline + "_spread_ms"] = base_ms, b, spread
        ms = medians[side][0]
        out[side + "_ms"] = ms
        out[side + "_speedup"] = base_ms / ms
        out[side + "_verdict"] = perfkit.verdict(ms, base_ms, spread)
        out[side + "_bytes_per_key_at_5p5TBs"] = perfkit.bytes_per_key(ms, n)
    return out


def run_filter(name, mode, rows, cols, a, base):
    n = rows * cols
    dev = {"device": "cuda"}
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.empty((rows, cols), dtype=torch.bfloat16, **dev)
    out_f, out_b = torch.empty_like(x), torch.empty_like(x)
    assert x.data_ptr() % 16 == 0 and out_f.data_ptr() % 16 == 0
    if mode == "perrow_k":
        choice = torch.tensor([1, 20, 50, 100, 1000], dtype=torch.int32, **dev).clamp(max=cols - 1)
        d_k = choice[torch.randint(0, 5, (rows,), generator=g, **dev)].contiguous()
    else:
        d_k = torch.full((rows,), min(50, cols - 1), dtype=torch.int32, **dev)
    k_max = int(d_k.max())
    col = (d_k.long() - 1).unsqueeze(1)
    neg_inf = torch.tensor(float("-inf"), dtype=torch.bfloat16, **dev)
    L = lsd.lib()
    ws = torch.empty(L.lsdsort_topk16_filter_workspace_bytes(rows, cols), dtype=torch.uint8, **dev)
    stream = int(torch.cuda.current_stream().cuda_stream)

    def filter_():
        st = L.lsdsort_topk16_filter_device(x.data_ptr(), rows, cols, d_k.data_ptr(), BF16, 1, NEG_INF_BITS, out_f.data_ptr(), ws.data_ptr(),
                                            ws.numel(), stream)
        assert st == 0, st

    def filter_in_place():
        st = L.lsdsort_topk16_filter_device(x.data_ptr(), rows, cols, d_k.data_ptr(), BF16, 1, NEG_INF_BITS, x.data_ptr(), ws.data_ptr(),
                                            ws.numel(), stream)
        assert st == 0, st

    if mode == "perrow_k":
        top_k = torch.empty((rows, k_max), dtype=torch.bfloat16, **dev)
        ws_b = torch.empty(base.lsdsort_topk16_workspace_bytes(rows, cols, k_max), dtype=torch.uint8, **dev)
        what = "lsdsort_topk16_device k=k_max, values only + gather + torch.where"

        def baseline():
            st = base.lsdsort_topk16_device(x.data_ptr(), rows, cols, k_max, BF16, 1, top_k.data_ptr(), None, ws_b.data_ptr(), ws_b.numel(),
                                            stream)
            assert st == 0, st
            torch.where(x < top_k.gather(1, col), neg_inf, x, out=out_b)
    else:
        thr = torch.empty(rows, dtype=torch.bfloat16, **dev)
        ws_b = torch.empty(base.lsdsort_kth16_workspace_bytes(rows, cols), dtype=torch.uint8, **dev)
        what = "lsdsort_kth16_device rank=k-1, values only + torch.where"

        def baseline():
            st = base.lsdsort_kth16_device(x.data_ptr(), rows, cols, k_max - 1, BF16, 1, thr.data_ptr(), None, ws_b.data_ptr(), ws_b.numel(),
                                           stream)
            assert st == 0, st
            torch.where(x < thr.unsqueeze(1), neg_inf, x, out=out_b)

    sides = {"filter": filter_, "baseline": baseline, "filter_in_place": filter_in_place}   # in place last: it changes the rows
    medians = measured(sides, {"baseline"}, x, g, a)
    assert L.lsdsort_check_device(ws.data_ptr(), None) == 0 and base.lsdsort_check_device(ws_b.data_ptr(), None) == 0
    # once more, untimed, on the same rows: every side answers the same question
    x.normal_(0.0, 1.0, generator=g)
    for fn in sides.values():
        fn()
    torch.cuda.synchronize()
    assert L.lsdsort_check_device(ws.data_ptr(), None) == 0
    bits = lambda t: t.view(torch.int16)
    assert torch.equal(bits(out_f), bits(out_b)), "the filter and the baseline disagree"
    assert torch.equal(bits(x), bits(out_f)), "in place and out of place disagree"
    kept = int((out_f[0] != neg_inf).sum())
    out = {"case": name, "mode": mode, "rows": rows, "cols": cols, "dtype": "bfloat16", "largest": True, "k_max": k_max,
           "kept_in_row_0": kept, "k_of_row_0": int(d_k[0]), "reps": a.reps, "warmup": a.warmup, "gated": mode == "perrow_k",
           "baseline": what, "baseline_library": "parent commit's" if a.baseline_lib else "this tree's",
           "workspace_bytes": ws.numel(), "baseline_workspace_bytes": ws_b.numel()}
    return report(out, medians, (("filter", "baseline"), ("filter_in_place", "baseline")), n)


def run_rank(name, rows, cols, a, base):
    n = rows * cols
    rank = (cols - 1) // 2
    dev = {"device": "cuda"}
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.empty((rows, cols), dtype=torch.bfloat16, **dev)
    d_ranks = torch.full((rows,), rank, dtype=torch.int32, **dev)
    outs = {s: (torch.empty(rows, dtype=torch.bfloat16, **dev), torch.empty(rows, dtype=torch.int32, **dev))
            for s in ("perrow", "perrow_values_only", "baseline", "baseline_values_only")}
    L = lsd.lib()
    ws = torch.empty(L.lsdsort_kth16_perrow_workspace_bytes(rows, cols), dtype=torch.uint8, **dev)
    ws_b = torch.empty(base.lsdsort_kth16_workspace_bytes(rows, cols), dtype=torch.uint8, **dev)
    stream = int(torch.cuda.current_stream().cuda_stream)

    def perrow(side, with_idx):
        def fn():
            k, i = outs[side]
            st = L.lsdsort_kth16_perrow_device(x.data_ptr(), rows, cols, d_ranks.data_ptr(), BF16, 1, k.data_ptr(),
                                               i.data_ptr() if with_idx else None, ws.data_ptr(), ws.numel(), stream)
            assert st == 0, st
        return fn

    def single(side, with_idx):
        def fn():
            k, i = outs[side]
            st = base.lsdsort_kth16_device(x.data_ptr(), rows, cols, rank, BF16, 1, k.data_ptr(), i.data_ptr() if with_idx else None,
                                           ws_b.data_ptr(), ws_b.numel(), stream)
            assert st == 0, st
        return fn

    sides = {"perrow": perrow("perrow", True), "baseline": single("baseline", True),
             "perrow_values_only": perrow("perrow_values_only", False), "baseline_values_only": single("baseline_values_only", False)}
    medians = measured(sides, {"baseline", "baseline_values_only"}, x, g, a)
    for fn in sides.values():
        fn()
    torch.cuda.synchronize()
    assert L.lsdsort_check_device(ws.data_ptr(), None) == 0 and base.lsdsort_check_device(ws_b.data_ptr(), None) == 0
    bits = lambda t: t.view(torch.int16)
    for s in ("perrow_values_only", "baseline", "baseline_values_only"):
        assert torch.equal(bits(outs[s][0]), bits(outs["perrow"][0])), s
    assert torch.equal(outs["perrow"][1], outs["baseline"][1]), "positions disagree"
    out = {"case": name, "mode": "perrow_rank", "rows": rows, "cols": cols, "rank": rank, "dtype": "bfloat16", "largest": True,
           "reps": a.reps, "warmup": a.warmup, "gated": False, "baseline": "lsdsort_kth16_device at the same rank",
           "baseline_library": "parent commit's" if a.baseline_lib else "this tree's", "workspace_bytes": ws.numel()}
    return report(out, medians, (("perrow", "baseline"), ("perrow_values_only", "baseline_values_only")), n)


CASES = {
    "rows_128x128256": (128, 128256),
    "rows_4096x131072": (4096, 131072),
    "one_row_2p28": (1, 1 << 28),
    "rows_16384x16384": (1 << 14, 1 << 14),
    "rows_1048576x256": (1 << 20, 256),
}
MODES = ("perrow_k", "uniform_k", "perrow_rank")


def parser():
    ap = perfkit.parser(__doc__, spread_repeats=5, lib_flag="--baseline-lib")
    ap.add_argument("--modes", default=",".join(MODES))
    return ap


def main():
    a = parser().parse_args()
    modes = a.modes.split(",")
    assert all(m in MODES for m in modes), modes
    base = perfkit.bound_library(a.baseline_lib, BASELINE_ENTRIES)

    def run(name, rows, cols):
        for mode in modes:
            yield run_rank(name, rows, cols, a, base) if mode == "perrow_rank" else run_filter(name, mode, rows, cols, a, base)

    perfkit.run_cases(a, CASES, run)


if __name__ == "__main__":
    main()
