#!/usr/bin/env python3
"""Timings of unique and run-length encode (GPU box): one JSON line per case and variant, the method of tools/perfkit.py.
Device events around the call alone, on the same keys for every side; the sides ALTERNATE in one process, call by call, in --rounds
rounds (six) of --warmup + --reps calls each.  A side's time is the median of its round medians, its spread the largest minus the
smallest of them.
Cases: uint32 at 2^24 / 2^26 / 2^28 keys with 2^16 distinct values ("few"), with about n/4 (uniform below n/2, "quarter") and all
distinct ("distinct", a permutation); int64 at 2^26 keys, uniform below n/2.  Variants: "counts" (counts only) and "inverse" (counts
and the inverse map).
  unique        lsdsort_unique_device into preallocated outputs and workspace
  torch_unique  (a) torch.unique(x, sorted=True, return_counts=True[, return_inverse=True])
  sort_rle      (b) what a caller of this library has at the parent commit: a copy, this library's sort on it (with the positions
                as payload for the inverse), torch.unique_consecutive(return_counts=True[, return_inverse=True]) and, for the
                inverse, the scatter through the sorted positions
  sort          (recorded) the copy and the library's sort alone, as `unique` runs them: its share of the call
  rle           (recorded) lsdsort_rle_device with counts on the keys sorted beforehand
  torch_rle     (recorded) torch.unique_consecutive(return_counts=True) on the same sorted keys
  copy          (recorded) a device copy of the keys: the rate the run-length phases' byte accounting is multiplied with
"verdict" is "ahead" where `unique` is faster than the FASTER of (a) and (b) by more than that baseline's spread, "behind" where it
is slower by more than it, else "within spread".  The gate is the nine uint32 cases of the "counts" variant; everything else is
recorded.  After the timed calls the entry's result is compared with torch.unique's.
Byte accounting of the run-length phases as timed here (counts, no starts), per key of width w bytes with d distinct values among
n: two reads of the keys (2 w) and per run the word and the count, (w + 4) d / n.
Usage: python tools/unique_perf.py [--rounds 6] [--reps 5] [--warmup 2] [--only NAME] [--variant counts|inverse]
                                   [--out profiles/unique_perf.jsonl]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import lsdradixsort_amd as lsd
import perfkit

KEY_CODE = {"uint32": 0, "int64": 4}


def make_keys(n, key_type, kind):
    g = torch.Generator(device="cuda").manual_seed(n % 1000 + len(kind))
    if kind == "distinct":
        return torch.randperm(n, device="cuda", generator=g, dtype=torch.int64).to(torch.int32 if key_type == "uint32" else torch.int64)
    high = (1 << 16) if kind == "few" else n // 2
    dtype = torch.int32 if key_type == "uint32" else torch.int64
    return torch.randint(0, high, (n,), device="cuda", generator=g, dtype=dtype)


def run(name, n, key_type, kind, variant, a):
    L = lsd.lib()
    dev = {"device": "cuda"}
    x = make_keys(n, key_type, kind)      # non-negative: uint32 order is int32 order, torch's
    w = x.element_size()
    code = KEY_CODE[key_type]
    inverse = variant == "inverse"
    stream = int(torch.cuda.current_stream().cuda_stream)
    out = torch.empty_like(x)
    counts = torch.empty(n, dtype=torch.int32, **dev)
    inv = torch.empty(n, dtype=torch.int32, **dev) if inverse else None
    num = torch.zeros(1, dtype=torch.int32, **dev)
    ws = torch.empty(L.lsdsort_unique_workspace_bytes(n, code, int(inverse)), dtype=torch.uint8, **dev)
    ws_rle = torch.empty(L.lsdsort_rle_workspace_bytes(n, 8 * w), dtype=torch.uint8, **dev)
    copy = torch.empty_like(x)
    pos = torch.empty(n, dtype=torch.int32, **dev)
    if w == 4:
        ws_sort = torch.empty(L.lsdsort_workspace_bytes(n, 8, int(inverse)), dtype=torch.uint8, **dev)
    else:
        ws_sort = torch.empty(L.lsdsort_wide_workspace_bytes(n, 8, 64, 32 * int(inverse)), dtype=torch.uint8, **dev)
    in_order = torch.sort(x).values.contiguous()
    kept = {}

    def unique():
        st = L.lsdsort_unique_device(x.data_ptr(), n, code, 0, out.data_ptr(), counts.data_ptr(), None, inv.data_ptr() if inverse else None,
                                     num.data_ptr(), ws.data_ptr(), ws.numel(), stream)
        assert st == 0, st

    def torch_unique():
        kept["a"] = torch.unique(x, sorted=True, return_counts=True, return_inverse=inverse)

    def sort():
        copy.copy_(x)
        if inverse:
            torch.arange(n, out=pos)
        payload = pos.data_ptr() if inverse else None
        if w == 4:
            st = L.lsdsort_keys_device(copy.data_ptr(), payload, ws_sort.data_ptr(), ws_sort.numel(), n, 8, code, 0, stream)
        else:
            st = L.lsdsort_keys64_device(copy.data_ptr(), payload, 32 * int(inverse), ws_sort.data_ptr(), ws_sort.numel(), n, 8, code, 0, stream)
        assert st == 0, st

    def sort_rle():
        sort()
        got = torch.unique_consecutive(copy, return_counts=True, return_inverse=inverse)
        if inverse:
            full = torch.empty(n, dtype=torch.int64, **dev)
            full[pos.long()] = got[1]
            got = (got[0], full, got[2])
        kept["b"] = got

    def rle():
        st = L.lsdsort_rle_device(in_order.data_ptr(), n, 8 * w, out.data_ptr(), counts.data_ptr(), None, num.data_ptr(), ws_rle.data_ptr(),
                                  ws_rle.numel(), stream)
        assert st == 0, st

    def torch_rle():
        kept["c"] = torch.unique_consecutive(in_order, return_counts=True)

    sides = {"unique": unique, "torch_unique": torch_unique, "sort_rle": sort_rle, "sort": sort, "rle": rle, "torch_rle": torch_rle,
             "copy": lambda: copy.copy_(x)}
    rounds = perfkit.measure(sides, None, a.rounds, a.reps, a.warmup)   # every side in every round
    # once more, untimed: the entry against torch.unique
    unique()
    torch.cuda.synchronize()
    assert L.lsdsort_unique_check_device(ws.data_ptr(), n, code, int(inverse), None) == 0
    ref = torch.unique(x, sorted=True, return_counts=True, return_inverse=inverse)
    m = int(num.item())
    agreed = m == ref[0].numel() and torch.equal(out[:m], ref[0]) and torch.equal(counts[:m].long(), ref[-1])
    if inverse:
        agreed = agreed and torch.equal(inv.long(), ref[1])
    assert agreed, "lsdsort_unique_device disagrees with torch.unique"
    res = {"case": name, "variant": variant, "n": n, "key_type": key_type, "kind": kind, "distinct": m, "rounds": a.rounds, "reps": a.reps,
           "warmup": a.warmup, "workspace_bytes": ws.numel(), "agrees_with_torch": bool(agreed)}
    for side, r in rounds.items():
        ms, spread = perfkit.spread_of(r)
        res[side + "_ms"], res[side + "_rounds_ms"], res[side + "_spread_ms"] = ms, r, spread
    faster = min(("torch_unique", "sort_rle"), key=lambda side: res[side + "_ms"])
    res["faster_baseline"] = faster
    res["speedup"] = res[faster + "_ms"] / res["unique_ms"]
    res["speedup_torch_unique"] = res["torch_unique_ms"] / res["unique_ms"]
    res["speedup_sort_rle"] = res["sort_rle_ms"] / res["unique_ms"]
    res["verdict"] = perfkit.verdict(res["unique_ms"], res[faster + "_ms"], res[faster + "_spread_ms"])
    res["gated"] = key_type == "uint32" and variant == "counts"
    res["sort_share"] = res["sort_ms"] / res["unique_ms"]
    res["rle_speedup_torch"] = res["torch_rle_ms"] / res["rle_ms"]
    res["copy_GBps"] = 2 * w * n / (res["copy_ms"] * 1e-3) / 1e9          # read and written
    res["rle_bytes_per_key"] = 2 * w + (w + 4) * m / n
    res["rle_at_copy_rate_ms"] = res["rle_bytes_per_key"] * n / (res["copy_GBps"] * 1e9) * 1e3
    return res


def cases():
    out = {}
    for log in (24, 26, 28):
        for kind in ("few", "quarter", "distinct"):
            out[f"uint32_2^{log}_{kind}"] = (1 << log, "uint32", kind)
    out["int64_2^26_quarter"] = (1 << 26, "int64", "quarter")
    return out


def parser():
    ap = perfkit.parser(__doc__, reps=5, warmup=2, rounds=6, only_help="run the cases whose name contains this")
    ap.add_argument("--variant", default=None, choices=("counts", "inverse"))
    return ap


def main():
    a = parser().parse_args()
    perfkit.run_cases(a, cases(), lambda name, n, key_type, kind: (run(name, n, key_type, kind, variant, a)
                                                                   for variant in ("counts", "inverse") if not a.variant or a.variant == variant),
                      match="substring")


if __name__ == "__main__":
    main()
