"""Oracle, acceptance rules and inputs of logprob16 -- log-probabilities, ranks and the log-sum-exp of given tokens of 16-bit logit
rows (a helper module: no fixtures, no pytest settings), for test_gpu_logprob16.py and test_logprob16_cpu.py.  It stands on
_temper16.py, _topp16.py and _sample16.py by import.

The oracle is numpy float64, per slot.  With v the row's values, w and m = `best` from _temper16.weights_of under the float32 T the
device reads, Z = sum(w), i the slot's id and x = v[i]:
  logprob  NaN for a padding id (i < 0 or i >= cols), for a NaN key and in a row without a number; otherwise
           (x == m ? 0 : greedy ? -inf : (x - m) / T) - ln Z -- _temper16.logprob64's expression, computed here once per row instead of
           once per slot (test_logprob16_cpu.py holds the two against each other).  An infinite logprob is compared exactly, a finite one
           within _temper16.logprob_tol's 2^-11 + 2^-22 |(x - m) / T|.
  rank     -1 for a padding id and a NaN key, otherwise the number of non-NaN values strictly greater than x: exact.
  lse      NaN for a greedy row and a row without a number, otherwise m / T + ln Z; an infinity exactly, a finite one within
           2^-11 + 2^-22 |m / T|: the product value(m) * k has the roundings of (x - m) * k, the ln Z term is the draw's.
The tolerances hold for |logit| <= 64, cols <= 2^17 and T greedy or at least 2^-10, the conditions of _temper16.py."""
import numpy as np

import _sample16 as sm
import _temper16 as tm
import _topp16 as tp
from _temper16 import COLS, ROWS, T_CYCLE, is_greedy, logprob64, logprob_tol, scale32, weights_of   # noqa: F401  (the suites' names)
from _topp16 import values64   # noqa: F401

TYPES = tp.TYPES
MAX_SLOTS = 32
SLOTS = (1, 2, 21, 32)
INT32_MIN = -2 ** 31
PADDING = (-1, INT32_MIN, -7)          # and cols, cols + 5, INT32_MAX: padding_ids
LSE_TOL = sm.LOGPROB_TOL


def padding_ids(cols):
    return list(PADDING) + [cols, cols + 5, 2 ** 31 - 1]


class RowOracle:
    """the float64 sums of one row under one T, computed once for all its slots"""

    def __init__(self, row, key_type, T=1.0):
        self.v = tp.values64(row, key_type)
        self.w, self.best = tm.weights_of(self.v, T)
        self.Z = float(self.w.sum())
        self.greedy = bool(tm.is_greedy(T))
        self.t = None if self.greedy else tm.t_eff(T)
        self.numbers = np.sort(self.v[~np.isnan(self.v)])

    def slots(self, ids):
        """(logprob, tol, rank) of the ids: float64, float64, int64"""
        ids = np.asarray(ids, dtype=np.int64)
        pad = (ids < 0) | (ids >= self.v.size)
        x = self.v[np.where(pad, 0, ids)]
        none = pad | np.isnan(x)
        logprob = np.full(ids.shape, np.nan)
        tol = np.full(ids.shape, sm.LOGPROB_TOL)
        rank = np.full(ids.shape, -1, dtype=np.int64)
        rank[~none] = self.numbers.size - np.searchsorted(self.numbers, x[~none], side="right")
        if self.best is None:
            return logprob, tol, rank
        with np.errstate(invalid="ignore", over="ignore"):
            if self.greedy:
                first = np.where(x == self.best, 0.0, -np.inf)
            else:
                first = np.where(x == self.best, 0.0, (x - self.best) / self.t)
                tol = tol + np.where(np.isfinite(first), 2.0 ** -22 * np.abs(first), 0.0)
        logprob[~none] = first[~none] - np.log(self.Z)
        return logprob, tol, rank

    def lse(self):
        """(lse, tol)"""
        if self.best is None or self.greedy:
            return float("nan"), LSE_TOL
        with np.errstate(invalid="ignore", over="ignore"):
            first = float(self.best) / self.t
        return first + float(np.log(self.Z)), LSE_TOL + (2.0 ** -22 * abs(first) if np.isfinite(first) else 0.0)


def close(got, want, tol):
    """the acceptance of one float: NaN for NaN, an infinity exactly, else within tol"""
    got, want = float(got), float(want)
    if np.isnan(want):
        return bool(np.isnan(got))
    if np.isinf(want):
        return got == want
    return bool(abs(got - want) <= tol)


def check_rows(logprob, rank, lse, keys, ids, T, key_type):
    """every word of the three outputs against the oracle: logprob [rows, slots] float32, rank [rows, slots] int32 or None, lse [rows]
    float32 or None; keys [rows, cols] bit patterns, ids [rows, slots], T [rows] float32 or None (1)"""
    rows, slots = ids.shape
    last = None
    for r in range(rows):
        t = 1.0 if T is None else T[r]
        if last is None or not np.array_equal(keys[r], keys[last[0]]) or np.float32(t).tobytes() != np.float32(last[1]).tobytes():
            o, last = RowOracle(keys[r], key_type, t), (r, t)
        want, tol, want_rank = o.slots(ids[r])
        for s in range(slots):
            assert close(logprob[r, s], want[s], tol[s]), (f"row {r} slot {s} of {keys.shape}, {key_type}, T = {t!r}, id {int(ids[r, s])}: "
                                                            f"logprob {float(logprob[r, s])!r}, float64 {want[s]!r} +- {tol[s]:.3g}")
        if rank is not None:
            bad = np.flatnonzero(np.asarray(rank[r], dtype=np.int64) != want_rank)
            assert bad.size == 0, (f"row {r} of {keys.shape}, {key_type}: rank {int(rank[r, bad[0]])} of id {int(ids[r, bad[0]])} in slot {bad[0]}, "
                                   f"want {int(want_rank[bad[0]])}")
        if lse is not None:
            want_lse, lse_tol = o.lse()
            assert close(lse[r], want_lse, lse_tol), f"row {r} of {keys.shape}, {key_type}, T = {t!r}: lse {float(lse[r])!r}, float64 {want_lse!r}"


def mixed_ids(keys, slots, key_type, seed):
    """[rows, slots] int32: per row a shuffle of position 0, cols - 1, the row's argmax, a NaN's position, a -inf's position (where the
    row holds one), padding ids of every kind, and random positions; the first `slots` of them -- the shuffle differs from row to row,
    so every kind occurs at every slot count over a few rows"""
    rows, cols = keys.shape
    rng = np.random.default_rng(seed)
    v = tp.values64(keys, key_type)
    out = np.empty((rows, slots), dtype=np.int32)
    pads = padding_ids(cols)
    for r in range(rows):
        number = ~np.isnan(v[r])
        must = [0, cols - 1, pads[r % len(pads)], int(rng.integers(0, cols))]
        if number.any():
            must.append(int(np.flatnonzero(number & (v[r] == v[r][number].max()))[-1]))
        for found in (np.flatnonzero(~number), np.flatnonzero(np.isneginf(v[r]))):
            if found.size:
                must.append(int(found[rng.integers(0, found.size)]))
        pool = np.array(must + pads + rng.integers(0, cols, MAX_SLOTS).tolist(), dtype=np.int64)
        head = rng.permutation(len(must))
        order = np.concatenate([head, len(must) + rng.permutation(pool.size - len(must))])
        if slots < len(must):      # short slot counts: rotate through the musts by row
            order = np.roll(order[:len(must)], r)
        out[r] = pool[order][:slots].astype(np.int64).clip(INT32_MIN, 2 ** 31 - 1)
    return out


def cycle_t(rows, shift=0):
    return tm.cycle_t(rows, shift)
