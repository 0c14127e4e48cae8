#!/usr/bin/env python3
"""Timings of reduce by key (GPU box): one JSON line per case and operation, the method of tools/perfkit.py.
Device events around the call alone, on the same keys and values for every side; the sides ALTERNATE in one process, call by call,
in --rounds rounds (six) of --warmup + --reps calls each.  A side's time is the median of its round medians, its spread the largest
minus the smallest of them.
Cases: uint32 keys at 2^24 / 2^26 / 2^28 with 2^16 distinct values ("few"), with about n/4 (uniform below n/2, "quarter") and all
distinct ("distinct", a permutation); int64 keys at 2^26, uniform below n/2 (recorded only).  Operations: "f32_sum" (float32 values,
integer-valued in [-100, 100], so that every sum is exact and the sides can be compared bit for bit) and "i32_max".
  reduce_by_key   lsdsort_reduce_by_key_device with counts, into preallocated outputs and workspace
  unique_scatter  (a) what a caller has at the parent commit: lsdsort_unique_device with the inverse map, then index_add_ /
                  scatter_reduce_(include_self=False) into a zeroed array (full length: the number of groups is on the device)
  sort_scatter    (b) a copy of keys and values, this library's pair sort with the values as payload,
                  torch.unique_consecutive(return_inverse=True, return_counts=True) and the same scatter on the sorted values
  sort            (recorded) the copies and the pair sort alone: the share of the by-key call that is not the three phases
  runs            (recorded) lsdsort_reduce_runs_device with counts on keys and values sorted beforehand
  torch_runs      (recorded) torch.unique_consecutive(return_inverse=True, return_counts=True) + the scatter on the same sorted arrays
  copy            (recorded) a device copy of the keys: the rate the byte accounting is multiplied with
"verdict" is "ahead" where `reduce_by_key` is faster than the FASTER of (a) and (b) by more than that baseline's spread, "behind"
where it is slower by more than it, else "within spread".  The gate is the eighteen uint32 rows; the int64 rows are recorded.  After
the timed calls the entry's keys, aggregates and counts are compared with baseline (a)'s and torch.unique's counts.
Byte accounting of the three phases as timed here (with counts), per key of width w bytes with d groups among n: two reads of keys
and values, 2 (w + 4), and per group the word, the aggregate and the count, (w + 8) d / n.
Usage: python tools/reduce_by_key_perf.py [--rounds 6] [--reps 5] [--warmup 2] [--only NAME] [--op f32_sum|i32_max]
                                          [--out profiles/reduce_by_key_perf.jsonl]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import lsdradixsort_amd as lsd
import perfkit
from lsdradixsort_amd import errors as E

KEY_CODE = {"uint32": E.LSDSORT_KEY_U32, "int64": E.LSDSORT_KEY_I64}
OPS = {"f32_sum": (torch.float32, E.LSDSORT_VAL_F32, E.LSDSORT_REDUCE_SUM), "i32_max": (torch.int32, E.LSDSORT_VAL_I32, E.LSDSORT_REDUCE_MAX)}


def make_keys(n, key_type, kind):
    g = torch.Generator(device="cuda").manual_seed(n % 1000 + len(kind))
    dtype = torch.int32 if key_type == "uint32" else torch.int64
    if kind == "distinct":
        return torch.randperm(n, device="cuda", generator=g, dtype=torch.int64).to(dtype)
    high = (1 << 16) if kind == "few" else n // 2
    return torch.randint(0, high, (n,), device="cuda", generator=g, dtype=dtype)


def scatter(index, v, op, n):
    """What a caller does with an inverse map: into a zeroed array of full length (the number of groups is a device word)."""
    out = torch.zeros(n, dtype=v.dtype, device="cuda")
    if op == "f32_sum":
        return out.index_add_(0, index, v)
    return out.scatter_reduce_(0, index.long(), v, "amax", include_self=False)


def run(name, n, key_type, kind, op, a):
    L = lsd.lib()
    dev = {"device": "cuda"}
    x = make_keys(n, key_type, kind)      # non-negative: uint32 order is int32 order, torch's
    w = x.element_size()
    code = KEY_CODE[key_type]
    dtype, val_type, op_code = OPS[op]
    g = torch.Generator(device="cuda").manual_seed(7 + n % 1000)
    v = torch.randint(-100, 101, (n,), device="cuda", generator=g, dtype=torch.int32).to(dtype)
    stream = int(torch.cuda.current_stream().cuda_stream)
    out = torch.empty_like(x)
    agg = torch.empty_like(v)
    counts = torch.empty(n, dtype=torch.int32, **dev)
    num = torch.zeros(1, dtype=torch.int32, **dev)
    ws = torch.empty(L.lsdsort_reduce_by_key_workspace_bytes(n, code), dtype=torch.uint8, **dev)
    ws_runs = torch.empty(L.lsdsort_reduce_runs_workspace_bytes(n, 8 * w), dtype=torch.uint8, **dev)
    ws_unique = torch.empty(L.lsdsort_unique_workspace_bytes(n, code, 1), dtype=torch.uint8, **dev)
    u_out = torch.empty_like(x)
    u_inv = torch.empty(n, dtype=torch.int32, **dev)
    u_num = torch.zeros(1, dtype=torch.int32, **dev)
    copy = torch.empty_like(x)
    vcopy = torch.empty_like(v)
    if w == 4:
        ws_sort = torch.empty(L.lsdsort_workspace_bytes(n, 8, 1), dtype=torch.uint8, **dev)
    else:
        ws_sort = torch.empty(L.lsdsort_wide_workspace_bytes(n, 8, 64, 32), dtype=torch.uint8, **dev)
    order = torch.sort(x, stable=True).indices
    in_order, v_in_order = x[order].contiguous(), v[order].contiguous()
    del order
    r_out, r_agg = torch.empty_like(x), torch.empty_like(v)
    kept = {}

    def reduce_by_key():
        st = L.lsdsort_reduce_by_key_device(x.data_ptr(), v.data_ptr(), n, code, 0, val_type, op_code, out.data_ptr(), agg.data_ptr(),
                                            counts.data_ptr(), num.data_ptr(), ws.data_ptr(), ws.numel(), stream)
        assert st == 0, st

    def unique_scatter():
        st = L.lsdsort_unique_device(x.data_ptr(), n, code, 0, u_out.data_ptr(), None, None, u_inv.data_ptr(), u_num.data_ptr(),
                                     ws_unique.data_ptr(), ws_unique.numel(), stream)
        assert st == 0, st
        kept["a"] = scatter(u_inv, v, op, n)

    def sort():
        copy.copy_(x)
        vcopy.copy_(v)
        if w == 4:
            st = L.lsdsort_keys_device(copy.data_ptr(), vcopy.data_ptr(), ws_sort.data_ptr(), ws_sort.numel(), n, 8, code, 0, stream)
        else:
            st = L.lsdsort_keys64_device(copy.data_ptr(), vcopy.data_ptr(), 32, ws_sort.data_ptr(), ws_sort.numel(), n, 8, code, 0, stream)
        assert st == 0, st

    def sort_scatter():
        sort()
        keys, inverse, sizes = torch.unique_consecutive(copy, return_inverse=True, return_counts=True)
        kept["b"] = (keys, scatter(inverse, vcopy, op, n), sizes)

    def runs():
        st = L.lsdsort_reduce_runs_device(in_order.data_ptr(), v_in_order.data_ptr(), n, 8 * w, val_type, op_code, r_out.data_ptr(),
                                          r_agg.data_ptr(), counts.data_ptr(), num.data_ptr(), ws_runs.data_ptr(), ws_runs.numel(), stream)
        assert st == 0, st

    def torch_runs():
        keys, inverse, sizes = torch.unique_consecutive(in_order, return_inverse=True, return_counts=True)
        kept["c"] = (keys, scatter(inverse, v_in_order, op, n), sizes)

    sides = {"reduce_by_key": reduce_by_key, "unique_scatter": unique_scatter, "sort_scatter": sort_scatter, "sort": sort, "runs": runs,
             "torch_runs": torch_runs, "copy": lambda: copy.copy_(x)}
    rounds = perfkit.measure(sides, None, a.rounds, a.reps, a.warmup)   # every side in every round
    # once more, untimed: the entry against baseline (a), and the runs entry against the entry
    runs()
    torch.cuda.synchronize()
    m_runs = int(num.item())
    reduce_by_key()
    unique_scatter()
    torch.cuda.synchronize()
    assert L.lsdsort_reduce_by_key_check_device(ws.data_ptr(), n, code, None) == 0
    m = int(num.item())
    sizes = torch.unique(x, sorted=True, return_counts=True)[1]
    agreed = m == int(u_num.item()) == sizes.numel() == m_runs and torch.equal(out[:m], u_out[:m]) and torch.equal(agg[:m], kept["a"][:m]) \
        and torch.equal(counts[:m].long(), sizes) and torch.equal(r_out[:m], out[:m]) and torch.equal(r_agg[:m], agg[:m])
    assert agreed, "lsdsort_reduce_by_key_device disagrees with unique + scatter"
    kept.clear()
    res = {"case": name, "op": op, "n": n, "key_type": key_type, "kind": kind, "groups": m, "rounds": a.rounds, "reps": a.reps,
           "warmup": a.warmup, "workspace_bytes": ws.numel(), "agrees_with_baseline": bool(agreed)}
    for side, r in rounds.items():
        ms, spread = perfkit.spread_of(r)
        res[side + "_ms"], res[side + "_rounds_ms"], res[side + "_spread_ms"] = ms, r, spread
    faster = min(("unique_scatter", "sort_scatter"), key=lambda side: res[side + "_ms"])
    res["faster_baseline"] = faster
    res["speedup"] = res[faster + "_ms"] / res["reduce_by_key_ms"]
    res["speedup_unique_scatter"] = res["unique_scatter_ms"] / res["reduce_by_key_ms"]
    res["speedup_sort_scatter"] = res["sort_scatter_ms"] / res["reduce_by_key_ms"]
    res["verdict"] = perfkit.verdict(res["reduce_by_key_ms"], res[faster + "_ms"], res[faster + "_spread_ms"])
    res["gated"] = key_type == "uint32"
    res["sort_share"] = res["sort_ms"] / res["reduce_by_key_ms"]
    res["runs_speedup_torch"] = res["torch_runs_ms"] / res["runs_ms"]
    res["copy_GBps"] = 2 * w * n / (res["copy_ms"] * 1e-3) / 1e9          # read and written
    res["runs_bytes_per_key"] = 2 * (w + 4) + (w + 8) * m / n
    res["runs_at_copy_rate_ms"] = res["runs_bytes_per_key"] * n / (res["copy_GBps"] * 1e9) * 1e3
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
    ap.add_argument("--op", default=None, choices=tuple(OPS))
    return ap


def main():
    a = parser().parse_args()
    perfkit.run_cases(a, cases(), lambda name, n, key_type, kind: (run(name, n, key_type, kind, op, a)
                                                                   for op in OPS if not a.op or a.op == op),
                      match="substring")


if __name__ == "__main__":
    main()
