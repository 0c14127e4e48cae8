#!/usr/bin/env python3
"""Time per sort of 2^28 keys that a sort which TRIES the hybrid form's half variant does not finish that way:

    tools/fallback_perf.py bucket_of_12000   uniform keys with one bucket of 12000: the hybrid form with a full-key pass B
    tools/fallback_perf.py half_zeros        half of the keys zero: the sample refuses, the ordinary form runs
    tools/fallback_perf.py uniform           the flagship's keys, for comparison

Run from the root of the tree to be measured (it imports that tree's package); prints one line: the input, ms per sort (HIP events
around --steps sorts, each on a fresh copy of the keys made outside the timed span), and the form and half word read back."""
import argparse
import os
import sys

sys.path.insert(0, os.getcwd())

import torch

import lsdradixsort_amd as lsd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("input", choices=["bucket_of_12000", "half_zeros", "uniform"])
    ap.add_argument("--log2-keys", type=int, default=28)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    n = 1 << a.log2_keys
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    keys = torch.randint(-(1 << 31), (1 << 31) - 1, (n,), dtype=torch.int32, device="cuda", generator=gen)
    if a.input == "bucket_of_12000":
        hot = 12000 - (n >> 15)
        keys[n - hot:] = (keys[:hot] & 0x1FFFF) | (5 << 17)
    elif a.input == "half_zeros":
        keys = torch.where(((keys >> 13) & 1) != 0, keys, torch.zeros_like(keys))
    ws = lsd.alloc_workspace(n, 8)
    copies = [keys.clone() for _ in range(a.steps)]
    for _ in range(a.warmup):
        lsd.GPULSDRadixSort(keys.clone(), 8, workspace=ws, check_fault=True)
    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    begin.record()
    for d in copies:
        lsd.GPULSDRadixSort(d, 8, workspace=ws)
    end.record()
    torch.cuda.synchronize()
    assert lsd.lib().lsdsort_check_device(ws.data_ptr(), None) == 0
    last = copies[-1]
    u = last.to(torch.int64) & 0xFFFFFFFF
    assert bool((u[1:] >= u[:-1]).all()), "not sorted"
    print(f"{a.input} ms_per_sort {begin.elapsed_time(end) / a.steps:.4f} hybrid {lsd.workspace_form(ws)} half {lsd.workspace_half(ws)}")


if __name__ == "__main__":
    main()
