#!/usr/bin/env python3
"""Timings of the draw for 16-bit logit rows (GPU box): one JSON line per shape, the method of tools/perfkit.py.
bfloat16 normal logits scaled by 4, 16-byte aligned, u_r uniform per row; device events around the call alone; the median of --reps
calls on fresh rows after --warmup calls.  The sides ALTERNATE in one process, call by call, on the same rows and the same u:
  sample            lsdsort_sample16_device without d_logprob
  sample_logprob    the same with d_logprob
  multinomial       (baseline a) torch.multinomial(torch.softmax(x.float(), -1), 1)
  cumsum            (baseline b) softmax(x.float()), cumsum, searchsorted(u, right=True)
  chain             (recorded) lsdsort_topk16_filter_device, lsdsort_topp16_filter_device, lsdsort_sample16_device in place on a copy
                    made outside the timed region (k = 50, p = 0.9)
  chain_multinomial (recorded) the same two filters, then baseline a
The baselines are what a caller has at the parent commit, which holds nothing for this step.  Each baseline is measured
--spread-repeats times over (each a median of --reps calls, alternating with the other sides in the first): "<baseline>_spread_ms" is
the largest minus the smallest of those medians and "<baseline>_ms" their median.  The GATE is against the FASTER of the two:
"verdict" is "ahead" where `sample` is faster than it by more than that baseline's spread, "behind" where it is slower by more than
it, else "within spread".  After the timed calls `sample` and `cumsum` run once more on the same rows, and up to --check-rows rows of
each go through the acceptance rule of the tests in float64: the index has mass and is consistent with u +- 2^-12 of the row's mass.
`sample` must pass; what `cumsum` gets is recorded.  Time x 5.5 TB/s per key stands next to the byte accounting (2 B/key for rows of
up to 16384 keys, about 4 B/key above).
Shapes: [128 x 128256], [4096 x 131072], [2^14 x 2^14], [2^20 x 256].
Usage: python tools/sample16_perf.py [--reps 20] [--warmup 3] [--spread-repeats 5] [--only NAME] [--check-rows 256]
                                     [--out profiles/sample16_perf.jsonl]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import lsdradixsort_amd as lsd
import perfkit

BF16 = 3
NEG_INF_BITS = 0xFF80
TOLERANCE = 2.0 ** -12
BASELINES = ("multinomial", "cumsum")


def accepted(x, index, u):
    """the acceptance rule of the tests for finite rows, in float64, all rows at once"""
    v = x.double()
    w = torch.exp(v - v.amax(dim=1, keepdim=True))
    inc = torch.cumsum(w, dim=1)
    z = inc[:, -1]
    i = index.long().view(-1, 1)
    if not bool(((i >= 0) & (i < x.shape[1])).all()):
        return False
    wi, upto = w.gather(1, i)[:, 0], inc.gather(1, i)[:, 0]
    uc = torch.nan_to_num(u.double(), nan=0.0).clamp(0.0, 1.0)
    return bool(((wi > 0) & (upto - wi <= (uc + TOLERANCE) * z) & (upto >= (uc - TOLERANCE) * z)).all())


def run(name, rows, cols, a):
    n = rows * cols
    dev = {"device": "cuda"}
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.empty((rows, cols), dtype=torch.bfloat16, **dev)
    y = torch.empty_like(x)
    assert x.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0
    d_u = torch.empty((rows,), dtype=torch.float32, **dev)
    d_k = torch.full((rows,), 50, dtype=torch.int32, **dev)
    d_p = torch.full((rows,), 0.9, dtype=torch.float32, **dev)
    index = torch.empty((rows,), dtype=torch.int32, **dev)
    logprob = torch.empty((rows,), dtype=torch.float32, **dev)
    L = lsd.lib()
    ws = torch.empty(L.lsdsort_sample16_workspace_bytes(rows, cols), dtype=torch.uint8, **dev)
    ws_k = torch.empty(L.lsdsort_topk16_filter_workspace_bytes(rows, cols), dtype=torch.uint8, **dev)
    ws_p = torch.empty(L.lsdsort_topp16_filter_workspace_bytes(rows, cols), dtype=torch.uint8, **dev)
    stream = int(torch.cuda.current_stream().cuda_stream)
    kept = {}

    def fresh():
        x.normal_(0.0, 4.0, generator=g)
        d_u.uniform_(0.0, 1.0, generator=g)

    def draw(keys, lp):
        st = L.lsdsort_sample16_device(keys.data_ptr(), rows, cols, d_u.data_ptr(), BF16, index.data_ptr(), lp, ws.data_ptr(), ws.numel(), stream)
        assert st == 0, st

    def filters():
        st = L.lsdsort_topk16_filter_device(y.data_ptr(), rows, cols, d_k.data_ptr(), BF16, 1, NEG_INF_BITS, y.data_ptr(), ws_k.data_ptr(),
                                            ws_k.numel(), stream)
        assert st == 0, st
        st = L.lsdsort_topp16_filter_device(y.data_ptr(), rows, cols, d_p.data_ptr(), BF16, NEG_INF_BITS, y.data_ptr(), ws_p.data_ptr(),
                                            ws_p.numel(), stream)
        assert st == 0, st

    def multinomial(keys=x):
        kept["multinomial"] = torch.multinomial(torch.softmax(keys.float(), dim=-1), 1)

    def cumsum():
        kept["cumsum"] = torch.searchsorted(torch.cumsum(torch.softmax(x.float(), dim=-1), dim=-1), d_u.unsqueeze(1), right=True)

    def chain():
        filters()
        draw(y, None)

    def chain_multinomial():
        filters()
        multinomial(y)

    sides = {"sample": lambda: draw(x, None), "sample_logprob": lambda: draw(x, logprob.data_ptr()), "multinomial": multinomial,
             "cumsum": cumsum, "chain": chain, "chain_multinomial": chain_multinomial}
    copy = lambda: y.copy_(x)
    medians = perfkit.measure(sides, BASELINES, a.spread_repeats, a.reps, a.warmup, fresh=fresh,
                              prepare={"chain": copy, "chain_multinomial": copy})
    for w in (ws, ws_k, ws_p):
        assert L.lsdsort_check_device(w.data_ptr(), None) == 0
    # once more, untimed, on the same rows: this side and baseline (b) under the acceptance rule
    fresh()
    draw(x, logprob.data_ptr())
    cumsum()
    torch.cuda.synchronize()
    assert L.lsdsort_check_device(ws.data_ptr(), None) == 0
    pick = torch.linspace(0, rows - 1, min(rows, a.check_rows), **dev).long()
    agreed = {"sample": accepted(x[pick], index[pick], d_u[pick]),
              "cumsum": accepted(x[pick], kept["cumsum"][pick].clamp(max=cols - 1), d_u[pick])}
    assert agreed["sample"], "the draw is not accepted"
    same = float((index.long() == kept["cumsum"].view(-1)).float().mean())
    kept.clear()
    out = {"case": name, "rows": rows, "cols": cols, "dtype": "bfloat16", "sigma": 4.0, "reps": a.reps, "warmup": a.warmup,
           "baselines": {"multinomial": "torch.multinomial(torch.softmax(x.float(), -1), 1)",
                         "cumsum": "torch.searchsorted(torch.cumsum(torch.softmax(x.float(), -1), -1), u[:, None], right=True)"},
           "workspace_bytes": ws.numel(), "accepted": agreed, "rows_checked": int(pick.numel()), "rows_equal_to_cumsum": same,
           "chain": {"k": 50, "p": 0.9}}
    for side in BASELINES:
        b = medians[side]
        ms, spread = perfkit.spread_of(b)
        out[side + "_ms"], out[side + "_repeats_ms"], out[side + "_spread_ms"] = ms, b, spread
    faster = min(BASELINES, key=lambda side: out[side + "_ms"])
    out["faster_baseline"] = faster
    for side in ("sample", "sample_logprob", "chain", "chain_multinomial"):
        out[side + "_ms"] = medians[side][0]
    for side in ("sample", "sample_logprob"):
        out[side + "_speedup"] = out[faster + "_ms"] / out[side + "_ms"]
        out[side + "_bytes_per_key_at_5p5TBs"] = perfkit.bytes_per_key(out[side + "_ms"], n)
    out["verdict"] = perfkit.verdict(out["sample_ms"], out[faster + "_ms"], out[faster + "_spread_ms"])
    out["chain_speedup"] = out["chain_multinomial_ms"] / out["chain_ms"]
    return out


CASES = {
    "rows_128x128256": (128, 128256),
    "rows_4096x131072": (4096, 131072),
    "rows_16384x16384": (1 << 14, 1 << 14),
    "rows_1048576x256": (1 << 20, 256),
}


def parser():
    ap = perfkit.parser(__doc__, spread_repeats=5)
    ap.add_argument("--check-rows", type=int, default=256)
    return ap


def main():
    a = parser().parse_args()
    perfkit.run_cases(a, CASES, lambda name, rows, cols: run(name, rows, cols, a))


if __name__ == "__main__":
    main()
