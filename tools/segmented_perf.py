#!/usr/bin/env python3
"""Segmented sort timings (GPU box): one JSON line per shape, device-event timing of the sort alone on a fresh copy of the
keys each rep (warm-up first, median and min of the timed reps: perfkit.timed), next to what it is compared with:
  [2^14 x 2^14]            workgroup tier   GPULSDRadixSort of the same 2^28 keys as one array; torch.sort(dim=-1)
  [2^20 x 256]             wave tier        torch.sort(dim=-1)
  1e6 lognormal segments   wave/workgroup   torch.sort(dim=-1) of a row-padded copy (rows of the largest segment)
  [64 x 2^22]              large tier       GPULSDRadixSort(algorithm=STAGED) of the 2^28 keys as one array; torch.sort(dim=-1)
  [32 x 131072] float32 descending + indices: large tier vs torch.sort(dim=-1, descending=True, stable=True)
Usage: python tools/segmented_perf.py [--reps 20] [--warmup 3] [--only NAME]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import lsdradixsort_amd as lsd
import perfkit
from perfkit import timed


def shape_rows(name, rows, cols, reps, warmup, whole_algo=None, dtype=torch.int32, descending=False, indices=False):
    n = rows * cols
    g = torch.Generator(device="cuda").manual_seed(1)
    if dtype == torch.float32:
        src = torch.randn(n, device="cuda", generator=g)
    else:
        src = torch.randint(-(1 << 31), 1 << 31, (n,), dtype=torch.int32, device="cuda", generator=g)
    off = torch.arange(0, rows + 1, dtype=torch.int64, device="cuda").mul_(cols).to(torch.int32)
    key_type = "float32" if dtype == torch.float32 else "uint32"
    ws = torch.empty(lsd.segmented_workspace_bytes(n, rows, indices), dtype=torch.uint8, device="cuda")
    iota = torch.arange(cols, dtype=torch.int32, device="cuda").repeat(rows) if indices else None
    work = src.clone()
    vals = iota.clone() if indices else None

    def fresh():
        work.copy_(src)
        if indices:
            vals.copy_(iota)

    seg_ms = timed(lambda: lsd.GPUSortSegmented(work, off, d_vals=vals, key_type=key_type, descending=descending, workspace=ws),
                   fresh, reps, warmup)
    out = {"shape": name, "n": n, "segments": rows, "segmented_ms": seg_ms[0], "segmented_min_ms": seg_ms[1],
           "segmented_gkeys_s": n / seg_ms[0] / 1e6}
    ref = src.view(rows, cols) if dtype == torch.float32 else (src.to(torch.int64) & 0xFFFFFFFF).view(rows, cols)
    t_ms = timed(lambda: torch.sort(ref, dim=-1, descending=descending, stable=True), None, reps, warmup)
    out["torch_sort_ms"] = t_ms[0]
    out["torch_sort_dtype"] = str(ref.dtype)
    if dtype == torch.int32:   # torch on the int32 bits too (signed order: the same work)
        t32 = timed(lambda: torch.sort(src.view(rows, cols), dim=-1, stable=True), None, reps, warmup)
        out["torch_sort_int32_ms"] = t32[0]
    if whole_algo is not None:
        wws = lsd.alloc_workspace(n, 8, False, whole_algo)
        w_ms = timed(lambda: lsd.GPULSDRadixSort(work, 8, algorithm=whole_algo, workspace=wws), fresh, reps, warmup)
        out["whole_array_ms"] = w_ms[0]
        out["whole_array_algorithm"] = "staged" if whole_algo == lsd.LSDSORT_ALGO_STAGED else "default"
    return out


def shape_lognormal(reps, warmup):
    rng = np.random.default_rng(6)
    sizes = np.maximum(0, rng.lognormal(np.log(100) - 0.5, 1.0, 10 ** 6)).astype(np.int64)
    off_np = np.concatenate([[0], np.cumsum(sizes)])
    n = int(off_np[-1])
    off = torch.from_numpy(off_np.astype(np.int32)).cuda()
    src = torch.randint(-(1 << 31), 1 << 31, (n,), dtype=torch.int32, device="cuda")
    ws = torch.empty(lsd.segmented_workspace_bytes(n, sizes.size), dtype=torch.uint8, device="cuda")
    work = src.clone()

    def fresh():
        work.copy_(src)

    seg_ms = timed(lambda: lsd.GPUSortSegmented(work, off, workspace=ws), fresh, reps, warmup)
    classes = {"wave": int(((sizes >= 2) & (sizes <= 1024)).sum()), "workgroup": int(((sizes > 1024) & (sizes <= 16384)).sum()),
               "large": int((sizes > 16384).sum())}
    out = {"shape": "lognormal_1e6_mean100", "n": n, "segments": int(sizes.size), "classes": classes, "segmented_ms": seg_ms[0],
           "segmented_min_ms": seg_ms[1], "segmented_gkeys_s": n / seg_ms[0] / 1e6}
    width = int(sizes.max())
    if sizes.size * width <= (1 << 29):
        padded = torch.full((sizes.size, width), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
        out["torch_sort_padded_ms"] = timed(lambda: torch.sort(padded, dim=-1, stable=True), None, reps, warmup)[0]
        out["torch_padded_shape"] = [int(sizes.size), width]
    else:
        out["torch_sort_padded_ms"] = None
        out["torch_padded_note"] = f"row-padded copy would be {sizes.size} x {width}: not run"
    return out


def parser():
    return perfkit.parser(__doc__, out=False)


def main():
    a = parser().parse_args()
    shapes = {
        "rows_16384x16384": lambda: shape_rows("rows_16384x16384", 1 << 14, 1 << 14, a.reps, a.warmup, whole_algo=lsd.LSDSORT_ALGO_ONESWEEP),
        "rows_1048576x256": lambda: shape_rows("rows_1048576x256", 1 << 20, 256, a.reps, a.warmup),
        "lognormal_1e6_mean100": lambda: shape_lognormal(a.reps, a.warmup),
        "rows_64x4194304": lambda: shape_rows("rows_64x4194304", 64, 1 << 22, a.reps, a.warmup, whole_algo=lsd.LSDSORT_ALGO_STAGED),
        "rows_32x131072_f32_desc_idx": lambda: shape_rows("rows_32x131072_f32_desc_idx", 32, 131072, a.reps, a.warmup,
                                                          dtype=torch.float32, descending=True, indices=True),
    }
    perfkit.run_cases(a, {name: () for name in shapes}, lambda name: shapes[name]())


if __name__ == "__main__":
    main()
