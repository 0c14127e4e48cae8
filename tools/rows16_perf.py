#!/usr/bin/env python3
"""16-bit row-sort timings (GPU box): one JSON line per shape, the method of tools/topk16_perf.py.  bfloat16 normal-distributed
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
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import lsdradixsort_amd as lsd

BF16 = 3
c_size, c_int, c_ptr = ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p


def baseline_library(path):
    """the three entries of the baseline leg, bound in the library at `path` (None: this tree's)"""
    if path is None:
        return lsd.lib()
    L = ctypes.CDLL(os.path.abspath(path))
    L.lsdsort_topk16_workspace_bytes.restype, L.lsdsort_topk16_workspace_bytes.argtypes = c_size, [c_size, c_size, c_size]
    L.lsdsort_topk16_device.restype = c_int
    L.lsdsort_topk16_device.argtypes = [c_ptr, c_size, c_size, c_size, c_int, c_int, c_ptr, c_ptr, c_ptr, c_size, c_ptr]
    L.lsdsort_check_device.restype, L.lsdsort_check_device.argtypes = c_int, [c_ptr, c_ptr]
    return L


def one(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


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
    medians = {side: [] for side in sides}
    for repeat in range(a.spread_repeats):
        ts = {side: [] for side in sides}
        for i in range(a.warmup + a.reps):
            x.normal_(0.0, 1.0, generator=g)
            for side, fn in sides.items():   # the sides alternate, call by call, on the same rows
                if repeat > 0 and side != "baseline":
                    continue                  # the further repeats measure the baseline's spread
                t = one(fn)
                if i >= a.warmup:
                    ts[side].append(t)
        for side in sides:
            if ts[side]:
                medians[side].append(float(np.median(ts[side])))
    L.lsdsort_set_rows16_route(-1)
    assert L.lsdsort_check_device(ws.data_ptr(), None) == 0 and base.lsdsort_check_device(ws_b.data_ptr(), None) == 0
    b = medians["baseline"]
    out = {"shape": name, "rows": rows, "cols": cols, "dtype": "bfloat16", "descending": True, "positions": True,
           "reps": a.reps, "warmup": a.warmup, "native_ms": medians["native"][0], "widen_ms": medians["widen"][0],
           "baseline": "lsdsort_topk16_device k=cols" + (" (parent commit's library)" if a.baseline_lib else " (this tree's library)"),
           "baseline_ms": float(np.median(b)), "baseline_repeats_ms": b, "baseline_spread_ms": max(b) - min(b),
           "native_bytes_per_key_at_5p5TBs": medians["native"][0] * 1e-3 * 5.5e12 / n,
           "speedup_native_vs_baseline": float(np.median(b)) / medians["native"][0],
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--spread-repeats", type=int, default=5)
    ap.add_argument("--only", default=None)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    base = baseline_library(a.baseline_lib)
    sink = open(a.out, "a") if a.out else None
    for name, (rows, cols) in SHAPES.items():
        if a.only and a.only != name:
            continue
        line = json.dumps(run_shape(name, rows, cols, a, base))
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
