#!/usr/bin/env python3
"""Timings of logprob16 -- log-probabilities and ranks of given tokens of 16-bit logit rows (GPU box): one JSON line per shape and
case, the method of tools/perfkit.py.  bfloat16 normal logits scaled by 4, 16-byte aligned, a temperature per row in [0.5, 1.5],
ids uniform over the row; device events around the call alone; the median of --reps calls on fresh rows after --warmup calls.  The
sides ALTERNATE in one process, call by call, on the same rows, ids and temperatures.
Case a, slots = 1, no ranks:
  logprob           lsdsort_logprob16_device, d_logprob alone
  baseline          torch.log_softmax(x.float() / T[:, None], -1).gather(-1, ids)
  draw_logprob      (recorded) lsdsort_sample16_ex_device with d_logprob on the same rows: the same reads
Case b, slots = 21, with ranks and the lse:
  logprob           lsdsort_logprob16_device with d_rank and d_lse
  baseline          the gather above and the ranks, in the faster of two forms, both timed:
                    "broadcast" (x.float()[:, None, :] > v[..., None]).sum(-1), "loop" one (x.float() > v[:, s:s + 1]).sum(-1) per slot
                    (x.float() is made once per call and shared with the log_softmax)
  logprob_no_ranks  (recorded) the entry without d_rank and d_lse
The baseline is what a caller has at the parent commit.  It is measured --spread-repeats times over (each a median of --reps calls,
alternating with the other sides in the first): "baseline_spread_ms" is the largest minus the smallest of those medians and
"baseline_ms" their median.  "verdict" is "ahead" where `logprob` is faster than the baseline by more than that spread, "behind"
where it is slower by more than it, else "within spread".  After the timed calls the entry runs once more and up to --check-rows rows
go through float64: every logprob within 2^-11 + 2^-22 |(x - m) / T|, every rank equal to the count, every lse within
2^-11 + 2^-22 |m / T|.  Time x 5.5 TB/s per key stands next to the byte accounting (2 B/key for rows of up to 16384 keys, 4 B/key above).
Shapes: [128 x 128256], [4096 x 131072], [2^14 x 2^14], [2^20 x 256]; recorded without a gate: [8192 x 128256], case a.
Usage: python tools/logprob16_perf.py [--reps 20] [--warmup 3] [--spread-repeats 5] [--only NAME] [--case a|b] [--check-rows 256]
                                      [--out profiles/logprob16_perf.jsonl]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import lsdradixsort_amd as lsd
import perfkit

BF16 = 3
TOL = 2.0 ** -11
BROADCAST_LIMIT = 24 << 30       # bytes of the broadcast form's boolean intermediate above which it is not attempted


def checked(x, ids, T, logprob, rank, lse):
    """the tests' tolerances in float64 for finite rows, all picked rows at once: (logprob ok, rank ok or None, lse ok or None)"""
    v = x.double()
    t = T.double()[:, None]
    m = v.amax(dim=1, keepdim=True)
    at = v.gather(1, ids.long())
    total = torch.logsumexp((v - m) / t, dim=1, keepdim=True)
    want = (at - m) / t - total
    ok = bool(((logprob.double() - want).abs() <= TOL + 2.0 ** -22 * ((at - m) / t).abs()).all())
    ok_rank = None if rank is None else bool(torch.equal(rank.long(), torch.stack([(v > at[:, s:s + 1]).sum(-1) for s in range(ids.shape[1])], dim=1)))
    ok_lse = None if lse is None else bool(((lse.double() - (m / t + total)[:, 0]).abs() <= TOL + 2.0 ** -22 * (m / t)[:, 0].abs()).all())
    return ok, ok_rank, ok_lse


def run(name, rows, cols, case, a):
    n = rows * cols
    slots = 1 if case == "a" else 21
    dev = {"device": "cuda"}
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.empty((rows, cols), dtype=torch.bfloat16, **dev)
    assert x.data_ptr() % 16 == 0
    ids = torch.empty((rows, slots), dtype=torch.int32, **dev)
    ids64 = torch.empty((rows, slots), dtype=torch.int64, **dev)
    d_t = torch.empty((rows,), dtype=torch.float32, **dev)
    d_u = torch.empty((rows,), dtype=torch.float32, **dev)
    logprob = torch.empty((rows, slots), dtype=torch.float32, **dev)
    rank = torch.empty((rows, slots), dtype=torch.int32, **dev)
    lse = torch.empty((rows,), dtype=torch.float32, **dev)
    index = torch.empty((rows,), dtype=torch.int32, **dev)
    drawn = torch.empty((rows,), dtype=torch.float32, **dev)
    L = lsd.lib()
    ws = torch.empty(L.lsdsort_logprob16_workspace_bytes(rows, cols, slots), dtype=torch.uint8, **dev)
    ws_d = torch.empty(L.lsdsort_sample16_workspace_bytes(rows, cols), dtype=torch.uint8, **dev)
    stream = int(torch.cuda.current_stream().cuda_stream)
    kept = {}

    def fresh():
        x.normal_(0.0, 4.0, generator=g)
        ids64.random_(0, cols, generator=g)
        ids.copy_(ids64)
        d_t.uniform_(0.5, 1.5, generator=g)
        d_u.uniform_(0.0, 1.0, generator=g)

    def entry(with_rest):
        st = L.lsdsort_logprob16_device(x.data_ptr(), rows, cols, ids.data_ptr(), slots, d_t.data_ptr(), BF16, logprob.data_ptr(),
                                        rank.data_ptr() if with_rest else None, lse.data_ptr() if with_rest else None, ws.data_ptr(), ws.numel(), stream)
        assert st == 0, st

    def draw():
        st = L.lsdsort_sample16_ex_device(x.data_ptr(), rows, cols, d_u.data_ptr(), d_t.data_ptr(), BF16, index.data_ptr(), drawn.data_ptr(),
                                          ws_d.data_ptr(), ws_d.numel(), stream)
        assert st == 0, st

    def gather_of(f):
        kept["logprob"] = torch.log_softmax(f / d_t[:, None], -1).gather(-1, ids64)

    def base_a():
        gather_of(x.float())

    def base_broadcast():
        f = x.float()
        gather_of(f)
        v = f.gather(-1, ids64)
        kept["rank"] = (f[:, None, :] > v[..., None]).sum(-1)

    def base_loop():
        f = x.float()
        gather_of(f)
        v = f.gather(-1, ids64)
        kept["rank"] = torch.stack([(f > v[:, s:s + 1]).sum(-1) for s in range(slots)], dim=1)

    if case == "a":
        sides = {"logprob": lambda: entry(False), "baseline": base_a, "draw_logprob": draw}
        baselines = ("baseline",)
    else:
        sides = {"logprob": lambda: entry(True), "baseline_loop": base_loop, "logprob_no_ranks": lambda: entry(False)}
        if n * slots <= BROADCAST_LIMIT:
            sides["baseline_broadcast"] = base_broadcast
        baselines = tuple(s for s in ("baseline_loop", "baseline_broadcast") if s in sides)
    medians = perfkit.measure(sides, baselines, a.spread_repeats, a.reps, a.warmup, fresh=fresh)
    kept.clear()
    torch.cuda.empty_cache()
    # once more, untimed: the entry's three outputs through float64
    fresh()
    entry(True)
    torch.cuda.synchronize()
    assert L.lsdsort_check_device(ws.data_ptr(), None) == 0
    pick = torch.linspace(0, rows - 1, min(rows, a.check_rows), **dev).long()
    agreed = checked(x[pick], ids[pick], d_t[pick], logprob[pick], rank[pick], lse[pick])
    assert all(agreed), f"the entry is not within its tolerances: {agreed}"
    out = {"case": name, "variant": case, "rows": rows, "cols": cols, "slots": slots, "dtype": "bfloat16", "sigma": 4.0, "reps": a.reps,
           "warmup": a.warmup, "workspace_bytes": ws.numel(), "rows_checked": int(pick.numel()), "within_tolerance": list(agreed)}
    for side in baselines:
        b = medians[side]
        ms, spread = perfkit.spread_of(b)
        out[side + "_ms"], out[side + "_repeats_ms"], out[side + "_spread_ms"] = ms, b, spread
    faster = min(baselines, key=lambda side: out[side + "_ms"])
    out["faster_baseline"] = faster
    for side in sides:
        if side not in baselines:
            out[side + "_ms"] = medians[side][0]
    out["speedup"] = out[faster + "_ms"] / out["logprob_ms"]
    out["bytes_per_key_at_5p5TBs"] = perfkit.bytes_per_key(out["logprob_ms"], n)
    out["verdict"] = perfkit.verdict(out["logprob_ms"], out[faster + "_ms"], out[faster + "_spread_ms"])
    return out


CASES = {
    "rows_128x128256": (128, 128256, "ab"),
    "rows_4096x131072": (4096, 131072, "ab"),
    "rows_16384x16384": (1 << 14, 1 << 14, "ab"),
    "rows_1048576x256": (1 << 20, 256, "ab"),
    "prompt_8192x128256": (8192, 128256, "a"),      # recorded without a gate
}


def parser():
    ap = perfkit.parser(__doc__, spread_repeats=5)
    ap.add_argument("--case", default=None, choices=("a", "b"))
    ap.add_argument("--check-rows", type=int, default=256)
    return ap


def main():
    a = parser().parse_args()
    perfkit.run_cases(a, CASES, lambda name, rows, cols, cases: (run(name, rows, cols, case, a) for case in cases
                                                                 if not a.case or a.case == case))


if __name__ == "__main__":
    main()
