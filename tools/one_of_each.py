#!/usr/bin/env python3
"""One of each kind of sort and of row selection (top-k, 16-bit top-k, sort_rows16, k-th value; each in every size class), once,
for a kernel trace (GPU box):
    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/one_of_each.py
Kernel names and call counts of two builds of the library can then be compared row by row (profiles/device_refactor)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import lsdradixsort_amd as lsd

g = torch.Generator(device="cuda"); g.manual_seed(7)
def keys(n, lo=-(1 << 31), hi=(1 << 31) - 1): return torch.randint(lo, hi, (n,), dtype=torch.int32, device="cuda", generator=g)
def iota(n): return torch.arange(n, dtype=torch.int32, device="cuda")

lsd.GPULSDRadixSort(keys(1 << 28), 8, check_fault=True)                                 # hybrid form, keys
lsd.GPULSDRadixSort(keys(1 << 24), 8, check_fault=True)                                 # four-pass form
lsd.GPULSDRadixSort(keys(1 << 27), 8, d_vals=iota(1 << 27), check_fault=True)           # hybrid form, pairs
lsd.GPULSDRadixSort(keys(1 << 28), 4, check_fault=True)                                 # 4-bit digits
lsd.GPULSDRadixSort(keys(1 << 24), 8, algorithm=lsd.LSDSORT_ALGO_STAGED, check_fault=True)
lsd.GPUSortTyped(keys(1 << 28), "int32", descending=True, check_fault=True)             # typed: the store turns the keys back
lsd.GPUSortTyped(keys(1 << 27), "int32", d_vals=iota(1 << 27), check_fault=True)
lsd.GPULSDRadixSort(keys(400_000_000), 8, check_fault=True)                             # 2^16 buckets
lsd.GPULSDRadixSort((keys(1 << 27) >> 9) << 9, 8, check_fault=True)                     # a dead low digit
k = torch.cat([keys(1 << 27), keys(1 << 27, 0, 1 << 20)]); lsd.GPULSDRadixSort(k, 8, check_fault=True)   # buckets for the list
k = torch.cat([keys(1 << 26), keys(1 << 26, 0, 1 << 20)]); lsd.GPULSDRadixSort(k, 8, d_vals=iota(1 << 27), check_fault=True)
lsd.GPULSDRadixSort(keys(10000), 8, check_fault=True)                                   # one launch
lsd.GPULSDRadixSort(keys(10000), 8, d_vals=iota(10000), check_fault=True)
n = 1 << 27
k64 = torch.randint(-(1 << 63), (1 << 63) - 1, (n,), dtype=torch.int64, device="cuda", generator=g)
lsd.GPUSortWide(k64.clone(), check_fault=True)                                          # uint64 keys
lsd.GPUSortWide(k64.clone(), torch.arange(n, dtype=torch.int64, device="cuda"), check_fault=True)   # records
lsd.GPUSortWide(keys(n), torch.arange(n, dtype=torch.int64, device="cuda"), check_fault=True)
lsd.sort_rows(keys(1 << 28).view(1 << 14, 1 << 14))                                     # segmented: workgroup tier
lsd.sort_rows(keys(1 << 28).view(1 << 20, 256), return_indices=True)                    # wave tier, pairs
lsd.sort_rows(keys(1 << 28).view(64, 1 << 22))                                          # large tier
lsd.sort_rows(keys(1 << 26).view(1 << 13, 1 << 13), return_indices=True)                # workgroup tier, pairs
lsd.topk_rows(keys(1 << 28).view(1 << 14, 1 << 14), 32)
lsd.topk_rows(keys(1 << 28).view(1 << 20, 256), 8)
lsd.topk_rows(keys(1 << 28), 1024)
lsd.topk_rows(keys(1 << 24).view(1 << 12, 1 << 12), 4000)                               # the sort route
def keys16(n): return torch.randint(-(1 << 15), (1 << 15) - 1, (n,), dtype=torch.int16, device="cuda", generator=g)
lsd.topk16_rows(keys16(1 << 26).view(1 << 12, 1 << 14), 32)                             # 16-bit top-k: workgroup tier
lsd.topk16_rows(keys16(1 << 26).view(1 << 18, 256), 8)                                  # wave tier
lsd.topk16_rows(keys16(1 << 26).view(64, 1 << 20), 1024)                                # long rows
lsd.topk16_rows(keys16(1 << 24).view(1 << 12, 1 << 12), 4000)                           # the sort route
lsd.sort_rows16(keys16(1 << 26).view(1 << 12, 1 << 14), return_indices=True)            # rows of 16-bit keys: workgroup tier
lsd.sort_rows16(keys16(1 << 26).view(1 << 18, 256), return_indices=True)                # wave tier
lsd.sort_rows16(keys16(1 << 26).view(512, 1 << 17), return_indices=True)                # long tier
lsd.sort_rows16(keys16(1 << 26).view(16, 1 << 22), return_indices=True)                 # widen route
lsd.median_rows(keys(1 << 26).view(1 << 12, 1 << 14))                                   # k-th value: workgroup tier
lsd.median_rows(keys(1 << 26).view(1 << 18, 256))                                       # wave tier
lsd.median_rows(keys(1 << 26).view(64, 1 << 20))                                        # long rows
torch.cuda.synchronize()
print("one of each: done")
