"""Oracle, acceptance rule and inputs of the draw for 16-bit logit rows (a helper module: no fixtures, no pytest settings), for
test_gpu_sample16.py and test_sample16_cpu.py.  It stands on _topp16.py (values, bit patterns, input families, M) and _rowk16.py.

The oracle is numpy float64, per POSITION: w_i = 0 for a NaN, 1 at the largest non-NaN value m of the row and exp(x_i - m) elsewhere
(_topp16.groups' weights, not grouped); C_i = the sum of w in front of position i; Z the total; u_c = the float32 u clipped to [0, 1],
a NaN taken as 0.  The exact index is the i with C_i <= u_c Z < C_i + w_i, for u_c = 1 the last key that has mass, and -1 for a row
without a number.

The device works in float32 and truncated fixed point with the top-p filter's masses, so a returned index i is ACCEPTED iff
w_i > 0, C_i <= (u_c + M) Z and C_i + w_i >= (u_c - M) Z with M = 2^-12 (for |logit| <= 64 and cols <= 2^17: _topp16's budget word
for word; the float64 product u Z adds nothing visible).  On SHARP rows exactly one index is acceptable, so acceptance is equality
with the oracle.  The logprob (x_i - m) - ln Z of the index the device returned is compared with float64 within LOGPROB_TOL = 2^-11:
x - m in float32 is off by at most 7.6e-6, ln Z with Z off by at most 6e-5 relative, the float32 log, conversion and final rounding
below 1.2e-5; together below 8e-5."""
import numpy as np

import _long_plan as lp
import _topp16 as tp

M = tp.M
LOGPROB_TOL = 2.0 ** -11
TYPES = tp.TYPES
SHARP_SETS = tp.SHARP_SETS
HEAVY = 48             # heavy keys of a sharp row: the lightest level of every set still holds 0.5 % of such a row
U_CYCLE = np.array([0.0, -0.0, 2.0 ** -149, 1e-30, 0.1, 0.5, 0.9, 1.0 - 2.0 ** -24, 1.0, 1.5, -1.0, np.nan], dtype=np.float32)


def weights(row, key_type):
    """one row of bit patterns -> (v, w, best): values and weights per position in float64, and the largest number (None: none)"""
    v = tp.values64(row, key_type)
    number = ~np.isnan(v)
    w = np.zeros(v.shape)
    if not number.any():
        return v, w, None
    best = v[number].max()
    with np.errstate(invalid="ignore", over="ignore"):
        w[number] = np.where(v[number] == best, 1.0, np.exp(v[number] - best))
    return v, w, best


def cdf(row, key_type):
    """(w, C, Z): the weight of every position, the mass in front of it, the total"""
    v, w, best = weights(row, key_type)
    inc = np.cumsum(w)
    return w, inc - w, float(inc[-1]) if w.size else 0.0


def clip_u(u):
    u = np.float32(u)
    return 0.0 if np.isnan(u) else float(min(max(u, np.float32(0)), np.float32(1)))


def exact_from(w, C, Z, u):
    if Z == 0.0:
        return -1
    u = clip_u(u)
    mass = np.flatnonzero(w > 0)
    if u >= 1.0:
        return int(mass[-1])
    hit = np.flatnonzero((C[mass] <= u * Z) & (u * Z < C[mass] + w[mass]))
    return int(mass[hit[0]]) if hit.size else int(mass[-1])


def acceptable_from(w, C, Z, u, m=M):
    if Z == 0.0:
        return [-1]
    u = clip_u(u)
    return [int(i) for i in np.flatnonzero((w > 0) & (C <= (u + m) * Z) & (C + w >= (u - m) * Z))]


def exact_index(row, u, key_type):
    """the float64 oracle's index for one row"""
    return exact_from(*cdf(row, key_type), u)


def acceptable(row, u, key_type, m=M):
    """every index the acceptance rule admits for one row; [-1] for a row without a number"""
    return acceptable_from(*cdf(row, key_type), u, m)


def logprob64(row, i, key_type):
    """the float64 log-probability of position i of one row (NaN for i == -1)"""
    if i < 0:
        return float("nan")
    v, w, best = weights(row, key_type)
    return (0.0 if v[i] == best else float(v[i] - best)) - float(np.log(w.sum()))


def _per_row(keys, key_type):
    """(r, w, C, Z) per row, the float64 sums computed once for a run of equal rows"""
    last = None
    for r in range(keys.shape[0]):
        if last is None or not np.array_equal(keys[r], keys[last]):
            sums, last = cdf(keys[r], key_type), r
        yield (r,) + sums


def check_rows(index, keys, u, key_type, logprob=None, m=M):
    """every returned index is accepted, and every returned logprob is within LOGPROB_TOL of float64 for the index returned"""
    for r, w, C, Z in _per_row(keys, key_type):
        ok = acceptable_from(w, C, Z, u[r], m)
        assert int(index[r]) in ok, (f"row {r} of {keys.shape}, {key_type}, u = {u[r]!r}: index {int(index[r])} is not consistent with u +- {m}: "
                                     f"acceptable {ok[:4]}{' ..' if len(ok) > 4 else ''}")
        if logprob is not None:
            want = logprob64(keys[r], int(index[r]), key_type)
            got = float(logprob[r])
            assert (np.isnan(want) and np.isnan(got)) or abs(got - want) <= LOGPROB_TOL, \
                f"row {r} of {keys.shape}, {key_type}: logprob {got!r} of index {int(index[r])}, float64 {want!r}"


def exact_rows(keys, u, key_type):
    """the float64 oracle's indices of every row: [rows] int64"""
    return np.array([exact_from(w, C, Z, u[r]) for r, w, C, Z in _per_row(keys, key_type)], dtype=np.int64)


def assert_sharp(keys, u, key_type):
    """every (row, u) has exactly one acceptable index, the float64 oracle's"""
    for r, w, C, Z in _per_row(keys, key_type):
        ok = acceptable_from(w, C, Z, u[r])
        assert ok == [exact_from(w, C, Z, u[r])], (r, u[r], ok)


def cycle_u(rows, shift=0):
    """[rows] float32: U_CYCLE shifted by the row index, so that the eight rows of one wave-tier workgroup differ"""
    return U_CYCLE[(np.arange(rows) + shift) % U_CYCLE.size]


def chunk_len(rows, cols):
    """the chunk length the library's plan gives rows above 16384 keys: about 2048 chunks over the array, at least 16384 keys, a
    multiple of the 4096-key tile (_long_plan.py restates the plan)"""
    return lp.chunks_for(rows, cols)[0]


def placement_positions(cols, chunk):
    """Position 0, cols - 1 and, for EVERY head = 0 .. 7 (the keys in front of a row's first 16-byte line: the rows of one array
    differ in it), the last head key and the first body key, both sides of the first 8-key load, of the 512-key lane round, of the
    1024-key wave tile and of the chunk boundary (head + b - 1, head + b)."""
    at = {0, cols - 1}
    for head in range(8):
        for b in (0, 8, 512, 1024, chunk):
            at |= {head + b - 1, head + b}
    return sorted(p for p in at if 0 <= p < cols)


def sharp_rows(name, cols, key_type, seed, placement=False, rows=None, nans=True):
    """(keys [n, cols], u [n] float32, at [n]): one row -- the same row -- per heavy key, u the midpoint of that key's interval, at
    its position.  n = min(HEAVY, cols) heavy keys drawn from the level set (neighbouring bit patterns: nearly equal masses) lie
    among keys of zero or negligible mass: -inf, NaNs of both signs, a filler at -60.  Every heavy key holds at least 0.5 % of the
    row against an acceptance window of 2 M = 0.05 %.  `placement`: the heavy keys take placement_positions first; without `nans` the light keys are -inf and the filler alone
    (torch's softmax turns a row that holds a NaN into NaNs)."""
    levels = SHARP_SETS[name]
    rng = np.random.default_rng(seed)
    n = min(HEAVY, cols)
    ninf, pinf = tp.NEG_INF[key_type], tp.POS_INF[key_type]
    filler = int(tp.bits_of_values(np.array([-60.0]), key_type)[0])
    assert tp.FILL not in (ninf, filler)
    light = np.array([ninf, ninf, filler, filler, pinf + 1, ninf + 1, 0x7FFF, 0xFFFF], dtype=np.uint16)[:8 if nans else 4]
    row = light[rng.integers(0, light.size, cols)]
    forced = placement_positions(cols, chunk_len(rows or n, cols)) if placement else []
    assert len(forced) <= n
    free = np.setdiff1d(np.arange(cols), forced)
    at = np.sort(np.concatenate([np.array(forced, dtype=np.int64), rng.permutation(free)[:n - len(forced)]])).astype(np.int64)
    for attempt in range(100):                                          # rejection: no draw is the tests' fill word, none too light
        heavy = levels[rng.integers(0, levels.size, n)]
        row[at] = heavy
        w, C, Z = cdf(row, key_type)
        if not (heavy == tp.FILL).any() and (w[at] / Z >= 0.005).all():
            break
    assert (w[at] / Z >= 0.005).all() and np.delete(w, at).sum() < 1e-20 * Z and not (row == tp.FILL).any()
    u = ((2 * C[at] + w[at]) / (2 * Z)).astype(np.float32)
    return np.tile(row, (n, 1)), u, at
