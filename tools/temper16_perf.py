#!/usr/bin/env python3
"""Timings of the per-row temperature and min-p of the 16-bit sampling chain (GPU box): one JSON line per shape, the method of
tools/perfkit.py.  bfloat16 normal logits scaled by 4, 16-byte aligned; u uniform per row, T from {0.5, 0.7, 1, 1.3} by row,
p = 0.9, mp = 0.05; device events around the call alone; the median of --reps calls on fresh rows after --warmup calls.  The sides
ALTERNATE in one process, call by call, on the same rows.  Every baseline is measured --spread-repeats times over: its spread is the
largest minus the smallest of those medians.

1. the entries without the new arguments against the PARENT commit's library (--parent-lib, loaded into the same process):
     old_filter / parent_filter    lsdsort_topp16_filter_device out of place, p = 0.9
     old_draw / parent_draw        lsdsort_sample16_device
   gate: this commit is not behind the parent by more than the parent's own spread.  --gate1-rounds N measures these four sides
   ALONE, N rounds over (each round a median of --reps calls, the four sides alternating call by call, the order of the two
   libraries swapped from round to round): "<side>_rounds_ms" are the N medians, "<side>_ms" their median, and the parent's
   spread is the largest minus the smallest of ITS N medians.
2. the new capability against what a caller had at the parent commit, lossless:
     ex_draw                       lsdsort_sample16_ex_device with T
     multinomial_T, cumsum_T       torch.multinomial(softmax(x.float() / T[:, None])); float32 softmax, cumsum, searchsorted
     ex_filter, ex_filter_inplace  lsdsort_topp16_filter_ex_device with p, mp and T
     sort_filter                   lsdsort_rows16_device descending with positions, float32 tempered softmax, cumsum, the two masks, scatter
   gate: ahead of the (faster) baseline by more than that baseline's spread.  After the timing both sides go through the float64
   acceptance rule of tests/_temper16.py on up to --check-rows rows.
3. recorded without a gate:
     ex_filter_ones, ex_draw_ones  the ex entries with T all ones (min-p NULL) next to old_filter / old_draw
     minp_alone / minp_torch       min-p with top-p off against x.masked_fill(x.float() < m + T * log(mp), -inf)
     lossy_draw                    (x.float() / T).to(bfloat16), then lsdsort_sample16_device
     chain / chain_torch           top-k (50), ex filter, ex draw in place on a copy made outside the timed region, against top-k by
                                   torch.topk, the sort-based filter above and multinomial
Usage: python tools/temper16_perf.py [--parent-lib PATH] [--gate1-rounds N] [--reps 20] [--warmup 3] [--spread-repeats 5] [--only NAME] [--check-rows 256]
                                     [--out profiles/temper16_perf.jsonl]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import lsdradixsort_amd as lsd
import perfkit
from perfkit import spread_of, verdict

BF16 = 3
NEG_INF_BITS = 0xFF80
BASELINES = ("parent_filter", "parent_draw", "multinomial_T", "cumsum_T", "sort_filter")
PARENT_ENTRIES = ("lsdsort_topp16_filter_device", "lsdsort_sample16_device", "lsdsort_prepare_device")


def run(name, rows, cols, a, parent):
    import _temper16 as tm

    dev = {"device": "cuda"}
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.empty((rows, cols), dtype=torch.bfloat16, **dev)
    y, out = torch.empty_like(x), torch.empty_like(x)
    d_u = torch.empty((rows,), dtype=torch.float32, **dev)
    d_t = torch.tensor([0.5, 0.7, 1.0, 1.3], dtype=torch.float32, **dev).repeat((rows + 3) // 4)[:rows].contiguous()
    ones = torch.ones((rows,), dtype=torch.float32, **dev)
    d_p = torch.full((rows,), 0.9, dtype=torch.float32, **dev)
    d_mp = torch.full((rows,), 0.05, dtype=torch.float32, **dev)
    d_k = torch.full((rows,), 50, dtype=torch.int32, **dev)
    index = torch.empty((rows,), dtype=torch.int32, **dev)
    L = lsd.lib()
    ws_d = torch.empty(L.lsdsort_sample16_workspace_bytes(rows, cols), dtype=torch.uint8, **dev)
    ws_p = torch.empty(L.lsdsort_topp16_filter_workspace_bytes(rows, cols), dtype=torch.uint8, **dev)
    ws_k = torch.empty(L.lsdsort_topk16_filter_workspace_bytes(rows, cols), dtype=torch.uint8, **dev)
    stream = int(torch.cuda.current_stream().cuda_stream)
    kept = {}

    def fresh():
        x.normal_(0.0, 4.0, generator=g)
        d_u.uniform_(0.0, 1.0, generator=g)

    def ok(st):
        assert st == 0, st

    def old_filter(lib=L):
        ok(lib.lsdsort_topp16_filter_device(x.data_ptr(), rows, cols, d_p.data_ptr(), BF16, NEG_INF_BITS, out.data_ptr(), ws_p.data_ptr(), ws_p.numel(), stream))

    def old_draw(lib=L, keys=x):
        ok(lib.lsdsort_sample16_device(keys.data_ptr(), rows, cols, d_u.data_ptr(), BF16, index.data_ptr(), None, ws_d.data_ptr(), ws_d.numel(), stream))

    def ex_filter(src, dst, p, mp, t):
        ok(L.lsdsort_topp16_filter_ex_device(src.data_ptr(), rows, cols, p, mp, t, BF16, NEG_INF_BITS, dst.data_ptr(), ws_p.data_ptr(), ws_p.numel(), stream))

    def ex_draw(keys, t):
        ok(L.lsdsort_sample16_ex_device(keys.data_ptr(), rows, cols, d_u.data_ptr(), t, BF16, index.data_ptr(), None, ws_d.data_ptr(), ws_d.numel(), stream))

    def multinomial_T(keys=x):
        kept["multinomial"] = torch.multinomial(torch.softmax(keys.float() / d_t[:, None], dim=-1), 1)

    def cumsum_T():
        kept["cumsum"] = torch.searchsorted(torch.cumsum(torch.softmax(x.float() / d_t[:, None], dim=-1), dim=-1), d_u.unsqueeze(1), right=True)

    def sort_filter(keys=x):
        ordered, idx = lsd.GPUSortRows16(keys, key_type="bfloat16", descending=True, return_indices=True)
        probs = torch.softmax(ordered.float() / d_t[:, None], dim=-1)
        mask = (torch.cumsum(probs, dim=-1) - probs >= d_p[:, None]) | (probs < d_mp[:, None] * probs[:, :1])
        kept["sort_filter"] = torch.empty_like(ordered).scatter_(-1, idx.long(), ordered.masked_fill(mask, float("-inf")))

    def minp_torch():
        v = x.float()
        kept["minp_torch"] = x.masked_fill(v < v.amax(dim=-1, keepdim=True) + d_t[:, None] * torch.log(d_mp)[:, None], float("-inf"))

    def lossy_draw():
        old_draw(L, (x.float() / d_t[:, None]).to(torch.bfloat16))

    def chain():
        ok(L.lsdsort_topk16_filter_device(y.data_ptr(), rows, cols, d_k.data_ptr(), BF16, 1, NEG_INF_BITS, y.data_ptr(), ws_k.data_ptr(), ws_k.numel(), stream))
        ex_filter(y, y, d_p.data_ptr(), d_mp.data_ptr(), d_t.data_ptr())
        ex_draw(y, d_t.data_ptr())

    def chain_torch():
        kth = torch.topk(y, 50, dim=-1).values[:, -1:]
        sort_filter(y.masked_fill(y < kth, float("-inf")))
        multinomial_T(kept["sort_filter"])

    sides = {"old_filter": old_filter, "old_draw": old_draw}
    if parent is not None:
        sides.update({"parent_filter": lambda: old_filter(parent), "parent_draw": lambda: old_draw(parent)})
    if a.gate1_rounds:
        assert parent is not None, "--gate1-rounds needs --parent-lib"
        swapped = ["parent_filter", "parent_draw", "old_filter", "old_draw"]
        rounds = perfkit.measure(sides, None, a.gate1_rounds, a.reps, a.warmup, fresh=fresh,
                                 order=lambda n: list(sides) if n % 2 == 0 else swapped)
        for w in (ws_d, ws_p):
            assert L.lsdsort_check_device(w.data_ptr(), None) == 0
        res = {"case": name, "rows": rows, "cols": cols, "dtype": "bfloat16", "sigma": 4.0, "reps": a.reps, "warmup": a.warmup, "p": 0.9,
               "gate1_rounds": a.gate1_rounds}
        for side, m in rounds.items():
            res[side + "_rounds_ms"], (res[side + "_ms"], res[side + "_spread_ms"]) = m, spread_of(m)
        for mine, base in (("old_filter", "parent_filter"), ("old_draw", "parent_draw")):
            res[mine + "_verdict"] = verdict(res[mine + "_ms"], res[base + "_ms"], res[base + "_spread_ms"])
        return res
    sides.update({
        "ex_draw": lambda: ex_draw(x, d_t.data_ptr()), "multinomial_T": multinomial_T, "cumsum_T": cumsum_T,
        "ex_filter": lambda: ex_filter(x, out, d_p.data_ptr(), d_mp.data_ptr(), d_t.data_ptr()),
        "ex_filter_inplace": lambda: ex_filter(y, y, d_p.data_ptr(), d_mp.data_ptr(), d_t.data_ptr()), "sort_filter": sort_filter,
        "ex_filter_ones": lambda: ex_filter(x, out, d_p.data_ptr(), None, ones.data_ptr()), "ex_draw_ones": lambda: ex_draw(x, ones.data_ptr()),
        "minp_alone": lambda: ex_filter(x, out, None, d_mp.data_ptr(), d_t.data_ptr()), "minp_torch": minp_torch, "lossy_draw": lossy_draw,
        "chain": chain, "chain_torch": chain_torch})
    copy = lambda: y.copy_(x)
    medians = perfkit.measure(sides, BASELINES, a.spread_repeats, a.reps, a.warmup, fresh=fresh,
                              prepare={"ex_filter_inplace": copy, "chain": copy, "chain_torch": copy})
    for w in (ws_d, ws_p, ws_k):
        assert L.lsdsort_check_device(w.data_ptr(), None) == 0
    # once more, untimed, on the same rows: both sides of the two gates under the float64 acceptance rule of the tests
    fresh()
    ex_draw(x, d_t.data_ptr())
    ex_filter(x, out, d_p.data_ptr(), d_mp.data_ptr(), d_t.data_ptr())
    cumsum_T()
    sort_filter()
    torch.cuda.synchronize()
    pick = np.unique(np.linspace(0, rows - 1, min(rows, a.check_rows)).astype(np.int64))
    host = lambda t: t[torch.from_numpy(pick).cuda()].cpu()
    bits = lambda t: host(t).view(torch.int16).numpy().view(np.uint16)
    keys, T, u = bits(x), host(d_t).numpy(), host(d_u).numpy()
    p, mp = np.full(pick.size, 0.9, dtype=np.float32), np.full(pick.size, 0.05, dtype=np.float32)
    agreed = {}

    def passes(check):
        try:
            check()
            return True
        except AssertionError:
            return False

    agreed["ex_draw"] = passes(lambda: tm.check_draws(host(index).numpy(), keys, u, T, "bfloat16"))
    agreed["cumsum_T"] = passes(lambda: tm.check_draws(host(kept["cumsum"].view(-1).clamp(max=cols - 1)).numpy(), keys, u, T, "bfloat16"))
    agreed["ex_filter"] = passes(lambda: tm.check_rows(bits(out), keys, p, mp, T, "bfloat16", fill=NEG_INF_BITS))
    agreed["sort_filter"] = passes(lambda: tm.check_rows(bits(kept["sort_filter"]), keys, p, mp, T, "bfloat16", fill=NEG_INF_BITS))
    assert agreed["ex_draw"] and agreed["ex_filter"], agreed
    kept.clear()
    res = {"case": name, "rows": rows, "cols": cols, "dtype": "bfloat16", "sigma": 4.0, "reps": a.reps, "warmup": a.warmup,
           "T": [0.5, 0.7, 1.0, 1.3], "p": 0.9, "mp": 0.05, "k": 50, "accepted": agreed, "rows_checked": int(pick.size)}
    for side, m in medians.items():
        res[side + "_ms"], spread = spread_of(m)
        if side in BASELINES:
            res[side + "_repeats_ms"], res[side + "_spread_ms"] = m, spread
    if parent is not None:
        for mine, base in (("old_filter", "parent_filter"), ("old_draw", "parent_draw")):
            res[mine + "_verdict"] = verdict(res[mine + "_ms"], res[base + "_ms"], res[base + "_spread_ms"])
    faster = min(("multinomial_T", "cumsum_T"), key=lambda side: res[side + "_ms"])
    res["faster_draw_baseline"] = faster
    res["ex_draw_verdict"] = verdict(res["ex_draw_ms"], res[faster + "_ms"], res[faster + "_spread_ms"])
    res["ex_draw_speedup"] = res[faster + "_ms"] / res["ex_draw_ms"]
    for side in ("ex_filter", "ex_filter_inplace"):
        res[side + "_verdict"] = verdict(res[side + "_ms"], res["sort_filter_ms"], res["sort_filter_spread_ms"])
        res[side + "_speedup"] = res["sort_filter_ms"] / res[side + "_ms"]
    return res


CASES = {
    "rows_128x128256": (128, 128256),
    "rows_4096x131072": (4096, 131072),
    "rows_16384x16384": (1 << 14, 1 << 14),
    "rows_1048576x256": (1 << 20, 256),
}


def parser():
    ap = perfkit.parser(__doc__, spread_repeats=5, lib_flag="--parent-lib")
    ap.add_argument("--gate1-rounds", type=int, default=0)
    ap.add_argument("--check-rows", type=int, default=256)
    return ap


def main():
    a = parser().parse_args()
    parent = perfkit.bound_library(a.parent_lib, PARENT_ENTRIES) if a.parent_lib else None
    assert parent is None or parent.lsdsort_prepare_device() == 0
    perfkit.run_cases(a, CASES, lambda name, rows, cols: run(name, rows, cols, a, parent))


if __name__ == "__main__":
    main()
