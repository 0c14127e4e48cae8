#!/usr/bin/env python3
"""16-bit sort timings (GPU box): one JSON line per shape.  Device-event timing of the call alone on fresh inputs each rep
(warm-up first, median and min of the timed reps), the routes next to what they are compared with, timed in the same process:
  count        lsdsort_keys16_device on the count route (keys only): count the 65536 values, scan, fill
  widen        lsdsort_keys16_device on the widen route: map to uint32, the ordinary sort (two live passes), narrow
  caller       what a caller had before the entry: x.to(int32) + GPUSortTyped("int32") + the narrowing copy
  torch.sort   (x) -- with payloads torch.sort returns the positions, which is what the payload rows carry
Keys only: 2^12 .. 2^24 and 2^28 uniform bfloat16 bit patterns, 2^28 all-equal keys, 2^28 normal-distributed bfloat16 values.
Pairs: 2^24 and 2^27 uniform patterns.  bytes_per_key_at_5p5TBs puts a time into the unit of DESIGN.md's byte accounting.
Usage: python tools/keys16_perf.py [--reps 20] [--warmup 3] [--only NAME] [--no-baselines] [--out FILE]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import lsdradixsort_amd as lsd
import perfkit
from perfkit import timed


def fill_uniform(x, g):
    """uniform 16-bit patterns (as bfloat16: every exponent, NaNs included)"""
    x.view(torch.int16).random_(-(1 << 15), 1 << 15, generator=g)


def fill_equal(x, g):
    x.fill_(0.7310586)


def fill_normal(x, g):
    """normal-distributed VALUES: most keys share a few exponents, so a few hundred counters take nearly all the adds"""
    step = 1 << 24
    for first in range(0, x.numel(), step):
        part = x[first:first + step]
        part.copy_(torch.randn(part.numel(), dtype=torch.float32, device=x.device, generator=g))


def timed_on_route(route, fn, fresh, reps, warmup):
    """timed() with the route forced around the whole measurement: the setter is outside every timed region"""
    lsd.set_keys16_route(route)
    try:
        return timed(fn, fresh, reps, warmup)
    finally:
        lsd.set_keys16_route(-1)


def run_shape(name, n, pairs, fill, reps, warmup, baselines=True):
    g = torch.Generator(device="cuda").manual_seed(1)
    src = torch.empty(n, dtype=torch.bfloat16, device="cuda")
    x = torch.empty_like(src)
    iota = torch.arange(n, dtype=torch.int32, device="cuda") if pairs else None
    vals = torch.empty_like(iota) if pairs else None
    ws = torch.empty(lsd.keys16_workspace_bytes(n, pairs), dtype=torch.uint8, device="cuda")

    def fresh():
        fill(src, g)
        x.copy_(src)
        if pairs:
            vals.copy_(iota)

    def check():
        assert lsd.lib().lsdsort_keys16_check_device(ws.data_ptr(), n, int(pairs), None) == 0

    sort = lambda: lsd.GPUSort16(x, key_type="bfloat16", d_vals=vals, workspace=ws)
    out = {"shape": name, "n": n, "pairs": bool(pairs), "workspace_bytes": ws.numel()}
    if not pairs:
        ms = timed_on_route(1, sort, fresh, reps, warmup)
        check()
        out.update(count_ms=ms[0], count_min_ms=ms[1], count_bytes_per_key_at_5p5TBs=perfkit.bytes_per_key(ms[0], n),
                   count_GBps_of_6B_per_key=6.0 * n / (ms[0] * 1e-3) / 1e9)
    ms = timed_on_route(0, sort, fresh, reps, warmup)
    check()
    out.update(widen_ms=ms[0], widen_min_ms=ms[1], widen_bytes_per_key_at_5p5TBs=perfkit.bytes_per_key(ms[0], n))
    if not baselines:
        return out
    del ws
    torch.cuda.empty_cache()
    # the caller's route before this entry
    sws = lsd.alloc_workspace(n, 8, pairs)
    result = [None]

    def caller():
        wide = x.view(torch.int16).to(torch.int32)
        lsd.GPUSortTyped(wide, "int32", d_vals=vals, workspace=sws)
        result[0] = wide.to(torch.int16)

    ms = timed(caller, fresh, reps, warmup)
    out.update(caller_ms=ms[0], caller_min_ms=ms[1])
    del sws
    result[0] = None
    torch.cuda.empty_cache()

    def torch_sort():
        result[0] = torch.sort(x, stable=bool(pairs)) if pairs else torch.sort(x).values

    ms = timed(torch_sort, fresh, reps, warmup)
    out.update(torch_sort_ms=ms[0], torch_sort_min_ms=ms[1])
    best = out["widen_ms"] if pairs else out["count_ms"]
    out["speedup_vs_caller"] = out["caller_ms"] / best
    out["speedup_vs_torch_sort"] = out["torch_sort_ms"] / best
    return out


SHAPES = {
    "keys_2p12_uniform": (1 << 12, False, fill_uniform),     # 2^12 .. 2^23: where the automatic rule's threshold is read off
    "keys_2p13_uniform": (1 << 13, False, fill_uniform),
    "keys_2p14_uniform": (1 << 14, False, fill_uniform),
    "keys_2p15_uniform": (1 << 15, False, fill_uniform),
    "keys_2p16_uniform": (1 << 16, False, fill_uniform),
    "keys_2p17_uniform": (1 << 17, False, fill_uniform),
    "keys_2p18_uniform": (1 << 18, False, fill_uniform),
    "keys_2p19_uniform": (1 << 19, False, fill_uniform),
    "keys_2p20_uniform": (1 << 20, False, fill_uniform),
    "keys_2p21_uniform": (1 << 21, False, fill_uniform),
    "keys_2p22_uniform": (1 << 22, False, fill_uniform),
    "keys_2p23_uniform": (1 << 23, False, fill_uniform),
    "keys_2p24_uniform": (1 << 24, False, fill_uniform),
    "keys_2p28_uniform": (1 << 28, False, fill_uniform),
    "keys_2p28_all_equal": (1 << 28, False, fill_equal),
    "keys_2p28_normal": (1 << 28, False, fill_normal),
    "pairs_2p24_uniform": (1 << 24, True, fill_uniform),
    "pairs_2p27_uniform": (1 << 27, True, fill_uniform),
}


def parser():
    ap = perfkit.parser(__doc__, only_help="comma-separated shape names")
    ap.add_argument("--no-baselines", action="store_true")
    return ap


def main():
    a = parser().parse_args()
    perfkit.run_cases(a, SHAPES, lambda name, *shape: run_shape(name, *shape, a.reps, a.warmup, baselines=not a.no_baselines),
                      match="list")


if __name__ == "__main__":
    main()
