#!/usr/bin/env python3
"""64-bit keys / payloads (lsdsort_keys64_device, lsdsort_records_device) on the GPU box: Gitems/s at 2^27 items.

  wide_perf.py                                   uint64 ascending, the four shapes
  wide_perf.py --key-type int64 | float64        the same bit patterns compared as int64 / float64 (64-bit-key shapes only)
  wide_perf.py --descending
  wide_perf.py --small-ids                       int64 values in [0, 2^31): the typical index tensor (constant high word)
  wide_perf.py --shapes keys,64/64 --reps 20     a subset, more repetitions

Each repetition sorts a fresh copy; the time is device events around the sort alone, after one untimed warm-up per shape.
Printed per shape: median, min and max over the repetitions (the spread says what a difference between two runs is worth).
With the default key type and order the library is called exactly as before these options existed."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import lsdradixsort_amd as lsd

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--key-type", choices=("uint64", "int64", "float64"), default="uint64")
ap.add_argument("--descending", action="store_true")
ap.add_argument("--small-ids", action="store_true", help="64-bit keys drawn from [0, 2^31)")
ap.add_argument("--log2n", type=int, default=27)
ap.add_argument("--reps", type=int, default=8)
ap.add_argument("--shapes", default="keys,64/64,64/32,32/64", help="comma list of keys, 64/64, 64/32, 32/64")
args = ap.parse_args()

assert torch.cuda.is_available(), "wide_perf.py measures on the GPU: there is no device here"
typed = args.key_type != "uint64" or args.descending
kwargs = {"key_type": args.key_type, "descending": args.descending} if typed else {}
n = 1 << args.log2n
g = torch.Generator(device="cuda"); g.manual_seed(1)
if args.small_ids:
    k64 = torch.randint(0, 1 << 31, (n,), dtype=torch.int64, device="cuda", generator=g)
else:
    k64 = torch.randint(-(1 << 63), (1 << 63) - 1, (n,), dtype=torch.int64, device="cuda", generator=g)
k32 = torch.randint(-(1 << 31), (1 << 31) - 1, (n,), dtype=torch.int32, device="cuda", generator=g)
v64 = torch.arange(n, dtype=torch.int64, device="cuda")
v32 = torch.arange(n, dtype=torch.int32, device="cuda")
shapes = {"keys": ("keys", k64, None), "64/64": ("keys + 64-bit payloads", k64, v64), "64/32": ("keys + 32-bit payloads", k64, v32),
          "32/64": ("uint32 keys + 64-bit payloads", k32, v64)}
label = ("small-ids " if args.small_ids else "") + args.key_type + (" descending" if args.descending else "")
for shape in args.shapes.split(","):
    name, k, v = shapes[shape]
    if k is k32 and (typed or args.small_ids):
        continue   # 32-bit keys with 64-bit payloads sort as uint32 ascending only
    kb = 64 if k.dtype == torch.int64 else 32
    vb = 0 if v is None else (64 if v.dtype == torch.int64 else 32)
    ws = torch.empty(int(lsd.lib().lsdsort_wide_workspace_bytes(n, 8, kb, vb)), dtype=torch.uint8, device="cuda")
    ts = []
    for i in range(args.reps + 1):
        kk, vv = k.clone(), (v.clone() if v is not None else None)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        lsd.GPUSortWide(kk, vv, workspace=ws, **kwargs)
        t1.record()
        torch.cuda.synchronize()
        if i:   # the first call is the warm-up
            ts.append(t0.elapsed_time(t1))
    t = statistics.median(ts)
    print(f"{(label + ' ' + name if kb == 64 else name):44s} n=2^{args.log2n}: median {t:7.3f} ms  min {min(ts):7.3f}  max {max(ts):7.3f}  "
          f"{n / t / 1e6:6.2f} Gitems/s  workspace {ws.numel() / n:.1f} B/item", flush=True)
