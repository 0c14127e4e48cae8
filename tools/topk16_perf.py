#!/usr/bin/env python3
"""16-bit top-k timings (GPU box): one JSON line per shape, the method of tools/perfkit.py.  Device-event timing of the call
alone on fresh inputs each rep (warm-up first, median and min of the timed reps), next to the two things it is compared with,
timed in the same process on the same bfloat16 rows, largest first, with indices:
  float32 path   what a caller did before the entry: x.float() followed by GPUTopK(..., "float32") -- the conversion IS in the time
  torch.topk     (x, k, dim=-1, largest=True, sorted=True) on the bfloat16 tensor
Shapes (all normal-distributed bfloat16 "logits"): [128 x 128256] k=50; [4096 x 131072] k=50; [1 x 2^28] k=1024;
[2^14 x 2^14] k=32; [2^20 x 256] k=8.
Usage: python tools/topk16_perf.py [--reps 20] [--warmup 3] [--only NAME] [--no-baselines]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import lsdradixsort_amd as lsd
import perfkit
from perfkit import timed


def run_shape(name, rows, cols, k, reps, warmup, baselines=True):
    n = rows * cols
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.empty((rows, cols), dtype=torch.bfloat16, device="cuda")

    def fresh():
        x.normal_(0.0, 1.0, generator=g)

    ws = torch.empty(lsd.topk16_workspace_bytes(rows, cols, k), dtype=torch.uint8, device="cuda")
    ms = timed(lambda: lsd.GPUTopK16(x, k, key_type="bfloat16", largest=True, workspace=ws), fresh, reps, warmup)
    assert lsd.lib().lsdsort_check_device(ws.data_ptr(), None) == 0
    out = {"shape": name, "rows": rows, "cols": cols, "k": k, "dtype": "bfloat16", "topk16_ms": ms[0], "topk16_min_ms": ms[1],
           "topk16_bytes_per_key_at_5p5TBs": perfkit.bytes_per_key(ms[0], n), "workspace_bytes": ws.numel()}
    if not baselines:
        return out
    del ws
    ws32 = torch.empty(lsd.topk_workspace_bytes(rows, cols, k), dtype=torch.uint8, device="cuda")
    f_ms = timed(lambda: lsd.GPUTopK(x.float(), k, key_type="float32", largest=True, workspace=ws32), fresh, reps, warmup)
    assert lsd.lib().lsdsort_check_device(ws32.data_ptr(), None) == 0
    del ws32
    t_ms = timed(lambda: torch.topk(x, k, dim=-1, largest=True, sorted=True), fresh, reps, warmup)
    out["float32_path"] = "x.float() + GPUTopK float32"
    out["float32_path_ms"] = f_ms[0]
    out["torch_topk_ms"] = t_ms[0]
    out["speedup_vs_float32_path"] = f_ms[0] / ms[0]
    out["speedup_vs_torch_topk"] = t_ms[0] / ms[0]
    return out


SHAPES = {
    "rows_128x128256_k50": (128, 128256, 50),
    "rows_4096x131072_k50": (4096, 131072, 50),
    "one_row_2p28_k1024": (1, 1 << 28, 1024),
    "rows_16384x16384_k32": (1 << 14, 1 << 14, 32),
    "rows_1048576x256_k8": (1 << 20, 256, 8),
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
