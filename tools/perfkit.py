"""The measuring convention of the tools/*_perf.py scripts, once.  A tool stays a script: it defines its cases, its sides and its
result dict, and calls these.  Nothing here touches the device at import.

Timing: device events around the call alone (`one`), on inputs made outside the timed region.  Two forms of loop:
  timed     ONE callable: warm-up calls, then the median and the smallest of --reps calls, each on fresh inputs
  measure   SEVERAL sides that ALTERNATE in one process, call by call, on the same inputs; the loop is repeated and a side has one
            median per repeat it ran in.  Which sides are repeated is the tool's to say, by name, in `repeated`:
              --spread-repeats family   repeat 0 runs every side, the further repeats only the baselines, for their spread
              --rounds family           every side runs in every repeat (repeated=None)
              gate-1 family             the --rounds family with the order of the sides given per repeat (temper16_perf.py)
A baseline's "spread" is the largest minus the smallest of its repeat medians, its time their median (`spread_of`).  A side is
"ahead" of a baseline where it is faster by MORE than that spread, "behind" where it is slower by more than it, else "within
spread" (`verdict`)."""
import argparse
import ctypes
import json
import os

import numpy as np
import torch

# byte ACCOUNTING of a time, not a measured traffic: the bytes per key that 5.5 TB/s would move in that time
ACCOUNTING_BYTES_PER_S = 5.5e12


def bytes_per_key(ms, n):
    return ms * 1e-3 * ACCOUNTING_BYTES_PER_S / n


def one(fn, prepare=None):
    """milliseconds of fn() by device events; prepare() runs before the first synchronise, outside the timed region"""
    if prepare:
        prepare()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def timed(fn, fresh, reps, warmup):
    """fresh() refills the inputs outside the timed region; fn() is timed: (median, min) of the reps after the warm-up"""
    ts = [one(fn, fresh) for _ in range(warmup + reps)][warmup:]
    return float(np.median(ts)), float(np.min(ts))


def measure(sides, repeated, repeats, reps, warmup, fresh=None, prepare=None, order=None):
    """side -> the medians of the repeats it ran in.  Within an iteration fresh() runs first, then the sides call by call in the
    dict's order (or in order(repeat)'s); prepare[side]() runs before that side's call, untimed.  Repeat 0 runs every side, the
    further repeats the sides in `repeated` (None: all).  Warm-up iterations are executed and not recorded."""
    prepare = prepare or {}
    medians = {side: [] for side in sides}
    for repeat in range(repeats):
        names = [side for side in (order(repeat) if order else sides) if repeat == 0 or repeated is None or side in repeated]
        ts = {side: [] for side in names}
        for i in range(warmup + reps):
            if fresh:
                fresh()
            for side in names:
                t = one(sides[side], prepare.get(side))
                if i >= warmup:
                    ts[side].append(t)
        for side in names:
            if ts[side]:
                medians[side].append(float(np.median(ts[side])))
    return medians


def spread_of(medians):
    """(the median of the repeat medians, the largest minus the smallest of them)"""
    return float(np.median(medians)), max(medians) - min(medians)


def verdict(side_ms, base_ms, spread):
    return "ahead" if base_ms - side_ms > spread else ("behind" if side_ms - base_ms > spread else "within spread")


def bound_library(path, names):
    """The entries `names` bound in the library at `path`, for a baseline timed in a parent commit's build (None: this tree's
    library, every entry bound).  The signatures are THIS tree's (lsdradixsort_amd._lib.SIGNATURES): name only entries that exist
    in the parent and whose signature has not changed since."""
    import lsdradixsort_amd as lsd
    from lsdradixsort_amd._lib import SIGNATURES

    if path is None:
        return lsd.lib()
    L = ctypes.CDLL(os.path.abspath(path))
    for name in names:
        restype, argtypes = SIGNATURES[name]   # KeyError: no entry of include/lsdsort.h
        fn = getattr(L, name)                  # AttributeError: the library at `path` does not export it
        fn.restype, fn.argtypes = restype, argtypes
    return L


def parser(doc, reps=20, warmup=3, spread_repeats=None, rounds=None, out=True, lib_flag=None, only_help="run this case alone"):
    """The shared flags a tool asks for, with the tool's defaults; the tool adds its own to what this returns."""
    ap = argparse.ArgumentParser(description=doc, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=reps)
    ap.add_argument("--warmup", type=int, default=warmup)
    if spread_repeats is not None:
        ap.add_argument("--spread-repeats", type=int, default=spread_repeats)
    if rounds is not None:
        ap.add_argument("--rounds", type=int, default=rounds)
    ap.add_argument("--only", default=None, help=only_help)
    if lib_flag:
        ap.add_argument(lib_flag, default=None, help="time the baselines in this library, built from the parent commit")
    if out:
        ap.add_argument("--out", default=None, help="append the result lines to this file as well")
    return ap


def run_cases(a, cases, run, match="exact"):
    """Walk the case table: run(name, *cases[name]) for every name --only selects ("exact": the name; "list": one of its
    comma-separated names; "substring": a part of the name).  run returns one result dict or yields several; each is printed as
    one JSON line, appended to --out where given, and followed by an empty_cache()."""
    selected = {"exact": lambda name: a.only == name, "list": lambda name: name in a.only.split(","),
                "substring": lambda name: a.only in name}[match]
    sink = open(a.out, "a") if getattr(a, "out", None) else None
    for name, args in cases.items():
        if a.only and not selected(name):
            continue
        results = run(name, *args)
        for result in [results] if isinstance(results, dict) else results:
            line = json.dumps(result)
            print(line, flush=True)
            if sink:
                sink.write(line + "\n")
                sink.flush()
            torch.cuda.empty_cache()
