#!/usr/bin/env python3
"""Timings of the top-p filter for 16-bit rows (GPU box): one JSON line per shape, the method of tools/perfkit.py.
bfloat16 normal logits scaled by 4, 16-byte aligned, p_r drawn per row from {0.5, 0.8, 0.9, 0.95, 0.99}; device events around the
call alone; the median of --reps calls on fresh rows after --warmup calls.  The sides ALTERNATE in one process, call by call, on the
same rows:
  filter            lsdsort_topp16_filter_device, fill -inf, into a second buffer
  baseline          (the gate) what a caller had before: lsdsort_rows16_device descending with positions, float32 softmax, cumsum,
                    the mask cumsum - probs >= p, -inf filled in, scattered back through the positions
  torch             (recorded) the same with torch.sort in place of the library's row sort
  filter_in_place   the filter with d_out == d_keys (timed last: it changes the rows)
With --baseline-lib the baseline's library call is made in a library built from the parent commit; without, in this tree's library.
The baseline is measured --spread-repeats times over (each a median of --reps calls, alternating with the other sides in the first):
"baseline_spread_ms" is the largest minus the smallest of those medians and "baseline_ms" their median.  "verdict" is "ahead" where
the side is faster than the baseline by more than that spread, "behind" where it is slower by more than it, else "within spread".
After the timed calls every side runs once more on the same rows, and up to --check-rows rows of every side's output go through the
acceptance rule of the tests in float64: the output is every key at least as good as its worst kept value T, and T is consistent with
p +- 2^-12 of the row's mass.  The filter must pass; the sort-based sides cut the sorted row at a position, so among the duplicates of
T they keep some and drop others: for them the rule leaves the duplicates of T open, and what they get is recorded ("accepted").
Shapes: [128 x 128256], [4096 x 131072], [2^14 x 2^14], [2^20 x 256].
Usage: python tools/topp16_filter_perf.py [--reps 20] [--warmup 3] [--spread-repeats 5] [--only NAME] [--baseline-lib PATH]
                                          [--check-rows 256] [--out profiles/topp16_filter_perf.jsonl]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import lsdradixsort_amd as lsd
import perfkit

BF16 = 3
NEG_INF_BITS = 0xFF80
TOLERANCE = 2.0 ** -12
BASELINE_ENTRIES = ("lsdsort_rows16_workspace_bytes", "lsdsort_rows16_device", "lsdsort_check_device")


def fresh(x, g):
    x.normal_(0.0, 4.0, generator=g)


def sortable(t):
    """the library's order with largest as an int32 per key: smaller is better"""
    b = t.view(torch.int16).to(torch.int32) & 0xFFFF
    return (b ^ torch.where(b >= 0x8000, 0xFFFF, 0x8000)) ^ 0xFFFF


def accepted(x, out, p, neg_inf, whole_ties=True):
    """the acceptance rule of the tests for finite rows without -inf, in float64, all rows at once.  whole_ties=False is the rule
    for the sort-based sides: they cut the sorted row at a POSITION, so of the duplicates of the worst kept value T some stay and
    some go; everything better than T stays, everything worse goes, and T is held to the same mass tolerance"""
    s = sortable(x)
    kept = out != neg_inf
    assert bool(kept.any(dim=1).all()), "a row keeps nothing"
    thr = torch.where(kept, s, -1).amax(dim=1, keepdim=True)
    want = torch.where(s <= thr, x, neg_inf)
    same = (want.view(torch.int16) == out.view(torch.int16)) if whole_ties else ((want.view(torch.int16) == out.view(torch.int16)) | (s == thr))
    if not bool(same.all()):
        return False
    v = x.double()
    w = torch.exp(v - v.amax(dim=1, keepdim=True))
    z = w.sum(dim=1)
    better = (w * (s < thr)).sum(dim=1)
    upto = (w * (s <= thr)).sum(dim=1)
    best, worst = thr[:, 0] == s.amin(dim=1), thr[:, 0] == s.amax(dim=1)
    pd = p.double()
    ok = ((better < (pd + TOLERANCE) * z) | best) & ((upto >= (pd - TOLERANCE) * z) | worst)
    return bool(ok.all())


def run(name, rows, cols, a, base):
    n = rows * cols
    dev = {"device": "cuda"}
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.empty((rows, cols), dtype=torch.bfloat16, **dev)
    out_f, out_b, out_t = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    assert x.data_ptr() % 16 == 0 and out_f.data_ptr() % 16 == 0
    choice = torch.tensor([0.5, 0.8, 0.9, 0.95, 0.99], dtype=torch.float32, **dev)
    d_p = choice[torch.randint(0, 5, (rows,), generator=g, **dev)].contiguous()
    p_col = d_p.unsqueeze(1)
    neg_inf = torch.tensor(float("-inf"), dtype=torch.bfloat16, **dev)
    L = lsd.lib()
    ws = torch.empty(L.lsdsort_topp16_filter_workspace_bytes(rows, cols), dtype=torch.uint8, **dev)
    ws_b = torch.empty(base.lsdsort_rows16_workspace_bytes(rows, cols), dtype=torch.uint8, **dev)
    sorted_keys = torch.empty_like(x)
    positions = torch.empty((rows, cols), dtype=torch.int32, **dev)
    stream = int(torch.cuda.current_stream().cuda_stream)

    def filter_():
        st = L.lsdsort_topp16_filter_device(x.data_ptr(), rows, cols, d_p.data_ptr(), BF16, NEG_INF_BITS, out_f.data_ptr(), ws.data_ptr(),
                                            ws.numel(), stream)
        assert st == 0, st

    def filter_in_place():
        st = L.lsdsort_topp16_filter_device(x.data_ptr(), rows, cols, d_p.data_ptr(), BF16, NEG_INF_BITS, x.data_ptr(), ws.data_ptr(),
                                            ws.numel(), stream)
        assert st == 0, st

    def mask_and_scatter(keys, index, out):
        probs = torch.softmax(keys.float(), dim=-1)
        mask = torch.cumsum(probs, dim=-1) - probs >= p_col
        out.scatter_(1, index, keys.masked_fill(mask, float("-inf")))

    def baseline():
        st = base.lsdsort_rows16_device(x.data_ptr(), rows, cols, BF16, 1, sorted_keys.data_ptr(), positions.data_ptr(), ws_b.data_ptr(),
                                        ws_b.numel(), stream)
        assert st == 0, st
        mask_and_scatter(sorted_keys, positions.long(), out_b)

    def torch_():
        keys, index = torch.sort(x, dim=-1, descending=True)
        mask_and_scatter(keys, index, out_t)

    sides = {"filter": filter_, "baseline": baseline, "torch": torch_, "filter_in_place": filter_in_place}   # in place last
    medians = perfkit.measure(sides, {"baseline"}, a.spread_repeats, a.reps, a.warmup, fresh=lambda: fresh(x, g))
    assert L.lsdsort_check_device(ws.data_ptr(), None) == 0 and base.lsdsort_check_device(ws_b.data_ptr(), None) == 0
    # once more, untimed, on the same rows: every side answers the same question, under the acceptance rule
    fresh(x, g)
    original = x.clone()
    for fn in sides.values():
        fn()
    torch.cuda.synchronize()
    assert L.lsdsort_check_device(ws.data_ptr(), None) == 0
    assert torch.equal(x.view(torch.int16), out_f.view(torch.int16)), "in place and out of place disagree"
    pick = torch.linspace(0, rows - 1, min(rows, a.check_rows), **dev).long()
    agreed = {side: accepted(original[pick], o[pick], d_p[pick], neg_inf, whole_ties=side == "filter")
              for side, o in (("filter", out_f), ("baseline", out_b), ("torch", out_t))}
    assert agreed["filter"], "the filter's output is not accepted"
    same = float((out_f.view(torch.int16) == out_b.view(torch.int16)).all(dim=1).float().mean())
    b = medians["baseline"]
    base_ms, spread = perfkit.spread_of(b)
    out = {"case": name, "rows": rows, "cols": cols, "dtype": "bfloat16", "sigma": 4.0, "p": choice.tolist(), "reps": a.reps, "warmup": a.warmup,
           "baseline": "lsdsort_rows16_device descending with positions + float32 softmax, cumsum, mask, scatter",
           "baseline_library": "parent commit's" if a.baseline_lib else "this tree's", "workspace_bytes": ws.numel(),
           "baseline_workspace_bytes": ws_b.numel(), "kept_in_row_0": int((out_f[0] != neg_inf).sum()), "p_of_row_0": float(d_p[0]),
           "accepted": agreed, "rows_checked": int(pick.numel()), "rows_bit_equal_to_baseline": same,
           "baseline_ms": base_ms, "baseline_repeats_ms": b, "baseline_spread_ms": spread, "torch_ms": medians["torch"][0]}
    for side in ("filter", "filter_in_place"):
        ms = medians[side][0]
        out[side + "_ms"] = ms
        out[side + "_speedup"] = base_ms / ms
        out[side + "_verdict"] = perfkit.verdict(ms, base_ms, spread)
        out[side + "_bytes_per_key_at_5p5TBs"] = perfkit.bytes_per_key(ms, n)
    return out


CASES = {
    "rows_128x128256": (128, 128256),
    "rows_4096x131072": (4096, 131072),
    "rows_16384x16384": (1 << 14, 1 << 14),
    "rows_1048576x256": (1 << 20, 256),
}


def parser():
    ap = perfkit.parser(__doc__, spread_repeats=5, lib_flag="--baseline-lib")
    ap.add_argument("--check-rows", type=int, default=256)
    return ap


def main():
    a = parser().parse_args()
    base = perfkit.bound_library(a.baseline_lib, BASELINE_ENTRIES)
    perfkit.run_cases(a, CASES, lambda name, rows, cols: run(name, rows, cols, a, base))


if __name__ == "__main__":
    main()
