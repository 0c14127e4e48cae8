#!/usr/bin/env python3
"""Top-k timings (GPU box): one JSON line per shape.  Device-event timing of the call alone on fresh inputs each rep (warm-up
first, median and min of the timed reps), next to the two things it is compared with, timed in the same process:
  sort path    what a caller had before the entry: the rows sorted whole with their positions, then cut to k columns --
               GPUSortSegmented with an index payload (the kernel work of sort_rows; its copy and index set-up are NOT in the
               time), and for one row GPUSortTyped with an index payload
  torch.topk   (x, k, dim=-1, largest=True, sorted=True)
Shapes: [1 x 2^28] uniform float32 k=1024; [64 x 2^22] uniform k=100; [4096 x 131072] normal float32 k=50; [2^14 x 2^14] k=32;
[2^20 x 256] k=8; [1 x 2^28] all equal and shared-top-24-bit keys k=1024.
Usage: python tools/topk_perf.py [--reps 20] [--warmup 3] [--only NAME] [--no-baselines]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import lsdradixsort_amd as lsd
import perfkit
from perfkit import timed


def fill_uniform(x, g):
    x.uniform_(0.0, 1.0, generator=g)


def fill_normal(x, g):
    x.normal_(0.0, 1.0, generator=g)


def fill_equal(x, g):
    x.fill_(0.7310586)


def fill_shared24(x, g):
    low = torch.randint(0, 256, x.shape, dtype=torch.int32, device=x.device, generator=g)
    x.view(torch.int32).copy_(low | 0x3F123400)


def run_shape(name, rows, cols, k, fill, reps, warmup, baselines=True):
    n = rows * cols
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.empty((rows, cols), dtype=torch.float32, device="cuda")
    ws = torch.empty(lsd.topk_workspace_bytes(rows, cols, k), dtype=torch.uint8, device="cuda")
    ms = timed(lambda: lsd.GPUTopK(x, k, key_type="float32", largest=True, workspace=ws), lambda: fill(x, g), reps, warmup)
    assert lsd.lib().lsdsort_check_device(ws.data_ptr(), None) == 0
    out = {"shape": name, "rows": rows, "cols": cols, "k": k, "topk_ms": ms[0], "topk_min_ms": ms[1],
           "topk_bytes_per_key_at_5p5TBs": perfkit.bytes_per_key(ms[0], n), "workspace_bytes": ws.numel()}
    if not baselines:
        return out
    del ws
    t_ms = timed(lambda: torch.topk(x, k, dim=-1, largest=True, sorted=True), lambda: fill(x, g), reps, warmup)
    out["torch_topk_ms"] = t_ms[0]
    work = torch.empty_like(x)
    iota = torch.arange(cols, dtype=torch.int32, device="cuda").repeat(rows)
    vals = torch.empty_like(iota)

    def fresh():
        fill(x, g)
        work.copy_(x)
        vals.copy_(iota)

    if rows == 1:
        sws = lsd.alloc_workspace(n, 8, True)
        s_ms = timed(lambda: lsd.GPUSortTyped(work.view(-1), "float32", descending=True, d_vals=vals, workspace=sws), fresh, reps, warmup)
        out["sort_path"] = "GPUSortTyped + index payload"
    else:
        off = torch.arange(0, rows + 1, dtype=torch.int64, device="cuda").mul_(cols).to(torch.int32)
        sws = torch.empty(lsd.segmented_workspace_bytes(n, rows, True), dtype=torch.uint8, device="cuda")
        s_ms = timed(lambda: lsd.GPUSortSegmented(work.view(-1), off, d_vals=vals, key_type="float32", descending=True, workspace=sws),
                     fresh, reps, warmup)
        out["sort_path"] = "GPUSortSegmented + index payload"
    out["sort_path_ms"] = s_ms[0]
    out["speedup_vs_sort_path"] = s_ms[0] / ms[0]
    out["speedup_vs_torch_topk"] = t_ms[0] / ms[0]
    return out


SHAPES = {
    "one_row_2p28_uniform_k1024": (1, 1 << 28, 1024, fill_uniform),
    "rows_64x4194304_uniform_k100": (64, 1 << 22, 100, fill_uniform),
    "rows_4096x131072_normal_k50": (4096, 131072, 50, fill_normal),
    "rows_16384x16384_k32": (1 << 14, 1 << 14, 32, fill_uniform),
    "rows_1048576x256_k8": (1 << 20, 256, 8, fill_uniform),
    "one_row_2p28_all_equal_k1024": (1, 1 << 28, 1024, fill_equal),
    "one_row_2p28_shared_top24_k1024": (1, 1 << 28, 1024, fill_shared24),
}


def parser():
    ap = perfkit.parser(__doc__, out=False)
    ap.add_argument("--no-baselines", action="store_true")
    return ap


def main():
    a = parser().parse_args()
    perfkit.run_cases(a, SHAPES, lambda name, *shape: run_shape(name, *shape, a.reps, a.warmup, baselines=not a.no_baselines))


if __name__ == "__main__":
    main()
