#!/usr/bin/env python3
"""16-bit row-sort timings (GPU box): one JSON line per shape, the method of tools/perfkit.py.  bfloat16 normal-distributed
"logits", descending, with positions; device events around the call alone; the median of --reps calls on fresh inputs after
--warmup calls.  The sides ALTERNATE in one process, call by call, on the same rows:
  native     lsdsort_rows16_device under lsdsort_set_rows16_route(1)
  widen      lsdsort_rows16_device under lsdsort_set_rows16_route(0)
  baseline   what a caller had before the entry: lsdsort_topk16_device with k = cols, largest (its sort route).  With
             --baseline-lib it is timed in a library built from the parent commit (only names that exist there are used:
             lsdsort_topk16_workspace_bytes, lsdsort_topk16_device, lsdsort_check_device); without, in this tree's library.
  torch      torch.sort(x, dim=-1, descending=True, stable=True), for the record
The baseline is measured --spread-repeats times over (each a median of --reps calls, alternating with the other sides):
"baseline_spread_ms" is the largest minus the smallest of those medians, and "baseline_ms" their median.
Shapes: [32 x 32000], [128 x 128256], [1024 x 131072], [2^14 x 2^14], [2^17 x 1024], [2^20 x 256].
Usage: python tools/rows16_perf.py [--reps 20] [--warmup 3] [--spread-repeats 5] [--only NAME] [--baseline-lib PATH] [--out FILE]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import lsdradixsort_amd as lsd
import perfkit

BF16 = 3
BASELINE_ENTRIES = ("lsdsort_topk16_workspace_bytes", "lsdsort_topk16_device", "lsdsort_check_device")


def run_shape(name, rows, cols, a, base):
    n = rows * cols
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.empty((rows, cols), dtype=torch.bfloat16, device="cuda")
    out_k = torch.empty_like(x)
    out_i = torch.empty((rows, cols), dtype=torch.int32, device="cuda")
    L = lsd.lib()
    ws = torch.empty(L.lsdsort_rows16_workspace_bytes(rows, cols), dtype=torch.uint8, device="cuda")
    ws_b = torch.empty(base.lsdsort_topk16_workspace_bytes(rows, cols, cols), dtype=torch.uint8, device="cuda")
    stream = int(torch.cuda.current_stream().cuda_stream)

    def rows16(route):
        def call():
            assert L.lsdsort_set_rows16_route(route) == 0
            st = L.lsdsort_rows16_device(x.data_ptr(), rows, cols, BF16, 1, out_k.data_ptr(), out_i.data_ptr(), ws.data_ptr(), ws.numel(),
                                         stream)
            assert st == 0, st
        return call

    def baseline():
        st = base.lsdsort_topk16_device(x.data_ptr(), rows, cols, cols, BF16, 1, out_k.data_ptr(), out_i.data_ptr(), ws_b.data_ptr(),
                                        ws_b.numel(), stream)
        assert st == 0, st

    sides = {"native": rows16(1), "widen": rows16(0), "baseline": baseline}
    if not a.no_torch:
        sides["torch"] = lambda: torch.sort(x, dim=-1, descending=True, stable=True)
    medians = perfkit.measure(sides, {"baseline"}, a.spread_repeats, a.reps, a.warmup, fresh=lambda: x.normal_(0.0, 1.0, generator=g))
    L.lsdsort_set_rows16_route(-1)
    assert L.lsdsort_check_device(ws.data_ptr(), None) == 0 and base.lsdsort_check_device(ws_b.data_ptr(), None) == 0
    b = medians["baseline"]
    base_ms, spread = perfkit.spread_of(b)
    out = {"shape": name, "rows": rows, "cols": cols, "dtype": "bfloat16", "descending": True, "positions": True,
           "reps": a.reps, "warmup": a.warmup, "native_ms": medians["native"][0], "widen_ms": medians["widen"][0],
           "baseline": "lsdsort_topk16_device k=cols" + (" (parent commit's library)" if a.baseline_lib else " (this tree's library)"),
           "baseline_ms": base_ms, "baseline_repeats_ms": b, "baseline_spread_ms": spread,
           "native_bytes_per_key_at_5p5TBs": perfkit.bytes_per_key(medians["native"][0], n),
           "speedup_native_vs_baseline": base_ms / medians["native"][0],
           "speedup_native_vs_widen": medians["widen"][0] / medians["native"][0], "workspace_bytes": ws.numel()}
    if "torch" in sides:
        out["torch_sort_ms"] = medians["torch"][0]
    return out


SHAPES = {
    "rows_32x32000": (32, 32000),
    "rows_128x128256": (128, 128256),
    "rows_1024x131072": (1024, 131072),
    "rows_16384x16384": (1 << 14, 1 << 14),
    "rows_131072x1024": (1 << 17, 1024),
    "rows_1048576x256": (1 << 20, 256),
}


def parser():
    ap = perfkit.parser(__doc__, spread_repeats=5, lib_flag="--baseline-lib")
    ap.add_argument("--no-torch", action="store_true")
    return ap


def main():
    a = parser().parse_args()
    base = perfkit.bound_library(a.baseline_lib, BASELINE_ENTRIES)
    perfkit.run_cases(a, SHAPES, lambda name, rows, cols: run_shape(name, rows, cols, a, base))


if __name__ == "__main__":
    main()
