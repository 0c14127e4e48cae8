"""Oracle, acceptance rules and inputs of the per-row temperature and min-p of the 16-bit sampling chain (a helper module: no
fixtures, no pytest settings), for test_gpu_temper16.py and test_temper16_cpu.py.  It stands on _topp16.py and _sample16.py by import.

The oracle is numpy float64.  T32 is the float32 the device reads.  The device's scale is c = float32(log2(e) / float64(T32)) with T32
above 2^64 taken as 2^64; the row is GREEDY where !(T32 > 0) or that float32 c is +inf.  The oracle's weights are w = 0 for a NaN, 1 at
the largest number m of the row, 0 elsewhere in a greedy row, and exp((x - m) / T) = exp2((x - m) * log2(e) / float64(T32)) elsewhere.
With T = 1 every function here gives what _topp16 / _sample16 give, bit for bit.

Top-p under T: _topp16's rule with these weights.  The mass tolerance stays M = 2^-12 for |logit| <= 64, cols <= 2^17 and T greedy or
>= 2^-10: a key contributes to the sums only while |(x - m) c| <= 32 (below that w < 2^-46, lost to the truncation anyway); there
the exponent carries three float32 roundings -- the subtraction, c and the product --, at most 32 * 3 * 2^-24 absolute or 4e-6
relative in w, below the 1.2e-5 of _topp16's budget, which the truncation term cols * 2^-32 dominates.

min-p: theta = value(m) + T ln(mp) in float64 from the float32 mp (T above 2^64 as 2^64; greedy: theta = value(m)); a key is kept iff
it is at least as good as m, or it is a number with value >= theta.  The device computes theta in float32 with the error bound
B = 2^-22 (|value(m)| + |T ln mp|) (keys16_map.hpp), so keys whose value lies within 4 B of theta may go either way and everything else
is bit for bit.  Both filters: the stricter threshold.  A returned row is ACCEPTED iff it is "every key at least as good as its worst
kept value, the fill word elsewhere" and that value is the stricter of an acceptable top-p and an acceptable min-p threshold.

The draw under T: _sample16's rule with these weights; the logprob is within 2^-11 + 2^-22 |(x_i - m) / T| of float64."""
import numpy as np

import _sample16 as sm
import _topp16 as tp
from _rowk16 import sortable16_np

M = tp.M
FILL = tp.FILL
TYPES = tp.TYPES
LOG2E = 1.4426950408889634
T_MAX = 2.0 ** 64
B_FACTOR = 2.0 ** -22
T_CYCLE = np.array([0.0, -1.0, np.nan, 2.0 ** -149, 2.0 ** -10, 0.05, 0.5, 0.7, 1.0, 1.3, 4.0, 100.0, 2.0 ** 65, np.inf], dtype=np.float32)
MP_SET = np.array([np.nan, -1.0, 0.0, 2.0 ** -149, 1e-9, 0.01, 0.05, 0.3, 1.0 - 2.0 ** -24, 1.0, 2.0, np.inf], dtype=np.float32)
# the cycles run by row index with pairwise coprime lengths (p 11, mp 13, T 14: MP_SET has 12 members, one of them comes twice), so
# that the eight rows of a wave-tier workgroup differ and every pair of values meets
MP_CYCLE = np.concatenate([MP_SET, MP_SET[6:7]])
assert np.gcd(MP_CYCLE.size, T_CYCLE.size) == 1 and np.gcd(tp.P_CYCLE.size, MP_CYCLE.size) == 1 and np.gcd(tp.P_CYCLE.size, T_CYCLE.size) == 1


def cycle_t(rows, shift=0):
    return T_CYCLE[(np.arange(rows) + shift) % T_CYCLE.size]


def cycle_mp(rows, shift=0):
    return MP_CYCLE[(np.arange(rows) + shift) % MP_CYCLE.size]


# ---- the temperature -----------------------------------------------------------------------------------------------------------------
def scale32(T):
    """the device's float32 scale c of a temperature, as a float: +inf for a greedy row"""
    T = np.float32(T)
    if not T > 0:
        return float("inf")
    with np.errstate(over="ignore"):
        return float(np.float32(LOG2E / min(float(T), T_MAX)))


def is_greedy(T):
    return np.isinf(scale32(T))


def t_eff(T):
    """the temperature the arithmetic uses for a row that is not greedy"""
    return min(float(np.float32(T)), T_MAX)


def weights_of(v, T):
    """values (float64, any shape, one row) -> (w, best): the weights under T and the largest number (None: none)"""
    number = ~np.isnan(v)
    w = np.zeros(v.shape)
    if not number.any():
        return w, None
    best = v[number].max()
    if is_greedy(T):
        w[number] = np.where(v[number] == best, 1.0, 0.0)
    else:
        with np.errstate(invalid="ignore", over="ignore"):
            w[number] = np.where(v[number] == best, 1.0, np.exp((v[number] - best) / t_eff(T)))
    return w, best


# ---- top-p under T ----------------------------------------------------------------------------------------------------------------------
def groups(row, key_type, T=1.0):
    """_topp16.groups under T: (s, mass, A, Z)"""
    s, first, count = np.unique(sortable16_np(row, key_type, True), return_index=True, return_counts=True)
    w, best = weights_of(tp.values64(row[first], key_type), T)
    mass = count * w
    A = np.cumsum(mass) - mass
    return s, mass, A, float(mass.sum())


def topp_exact_at(g, p):
    """index into s of the float64 oracle's threshold"""
    s, mass, A, Z = g
    kept = A < float(np.float32(p)) * Z
    kept[0] = True
    return int(np.flatnonzero(kept).max())


def topp_acceptable_at(g, p, m=M):
    s, mass, A, Z = g
    p = float(np.float32(p))
    at = np.arange(s.size)
    return [int(j) for j in np.flatnonzero(((A < (p + m) * Z) | (at == 0)) & ((A + mass >= (p - m) * Z) | (at == s.size - 1)))]


def exact_threshold(row, p, key_type, T=1.0):
    g = groups(row, key_type, T)
    return int(g[0][topp_exact_at(g, p)])


def acceptable(row, p, key_type, T=1.0, m=M):
    g = groups(row, key_type, T)
    return [int(g[0][j]) for j in topp_acceptable_at(g, p, m)]


# ---- min-p --------------------------------------------------------------------------------------------------------------------------------
def minp_on(mp):
    return bool(np.float32(mp) > 0)


def theta_of(best, T, mp):
    """(theta, 4 B) in float64 for a row whose best number is `best`; mp > 0"""
    if is_greedy(T):
        return float(best), 0.0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        step = t_eff(T) * np.log(np.float64(np.float32(mp)))
        theta = float(best) + step
        band = 4 * B_FACTOR * (abs(float(best)) + abs(step))
    return float(theta), float(band) if np.isfinite(band) else 0.0


def minp_range_at(row, key_type, T, mp, s):
    """(lo, hi, exact, in_band): the indices into the distinct sortable values s (best first) of the strictest and of the most
    generous worst kept value the band admits, of the float64 oracle's, and how many keys of the row lie within the band"""
    first = np.unique(sortable16_np(row, key_type, True), return_index=True)[1]
    v = tp.values64(row[first], key_type)
    number = ~np.isnan(v)
    if not number.any():
        return 0, 0, 0, 0
    best = v[number].max()
    at_m = int(np.flatnonzero(number & (v == best)).min())      # m: the best of the keys with the largest value (+0.0 before -0.0)
    theta, band = theta_of(best, T, mp)
    with np.errstate(invalid="ignore"):
        def worst(limit):
            kept = number & (v >= limit)
            return max(at_m, int(np.flatnonzero(kept).max())) if kept.any() else at_m
        lo, hi, exact = worst(theta + band), worst(theta - band), worst(theta)
        vr = tp.values64(row, key_type)
        in_band = int((~np.isnan(vr) & (np.abs(vr - theta) <= band) & (sortable16_np(row, key_type, True) > s[at_m])).sum()) if band > 0 else 0
    return lo, hi, exact, in_band


# ---- the filter with p, mp and T -------------------------------------------------------------------------------------------------------------
def _off(p):
    return p is None or tp.is_off(p)


def filter_row(row, p, mp, T, key_type, fill=FILL):
    """the float64 oracle's output for one row: p and mp may be None (off)"""
    mp_live = mp is not None and minp_on(mp)
    if _off(p) and not mp_live:
        return row.copy()
    g = groups(row, key_type, T)
    s = g[0]
    at = s.size - 1
    if not _off(p):
        at = min(at, topp_exact_at(g, p))
    if mp_live:
        at = min(at, minp_range_at(row, key_type, T, mp, s)[2])
    return np.where(sortable16_np(row, key_type, True) <= s[at], row, np.uint16(fill))


def filter_np(keys, p, mp, T, key_type, fill=FILL):
    """[rows, cols] -> the oracle's output; p, mp, T: [rows] arrays or None"""
    rows = keys.shape[0]
    return np.stack([filter_row(keys[r], None if p is None else p[r], None if mp is None else mp[r], 1.0 if T is None else T[r], key_type, fill)
                     for r in range(rows)])


def check_row(got, row, p, mp, T, key_type, fill=FILL, m=M):
    """None where the returned row is accepted, else what is wrong"""
    mp_live = mp is not None and minp_on(mp)
    if _off(p) and not mp_live:
        return None if np.array_equal(got, row) else "a row with both filters off differs from the input"
    kept = got != fill
    if not kept.any():
        return "no key was kept"
    sr = sortable16_np(row, key_type, True)
    worst = int(sr[kept].max())
    want = np.where(sr <= worst, row, np.uint16(fill))
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        return f"not every key at least as good as {worst:#x} and only those: {bad.size} words differ, first at {bad[0]}"
    g = groups(row, key_type, T)
    s = g[0]
    at = int(np.searchsorted(s, worst))
    from_p = [s.size - 1] if _off(p) else topp_acceptable_at(g, p, m)
    lo, hi = (s.size - 1, s.size - 1) if not mp_live else minp_range_at(row, key_type, T, mp, s)[:2]
    if not any(min(jp, jm) == at for jp in from_p for jm in range(lo, hi + 1)):
        return (f"the worst kept value {worst:#x} (value {at} of {s.size}) is not the stricter of a top-p threshold in {from_p[:4]} "
                f"(p = {p!r}) and a min-p threshold in [{lo}, {hi}] (mp = {mp!r}) under T = {T!r}")
    return None


def check_rows(got, keys, p, mp, T, key_type, fill=FILL):
    for r in range(keys.shape[0]):
        why = check_row(got[r], keys[r], None if p is None else p[r], None if mp is None else mp[r], 1.0 if T is None else T[r], key_type, fill)
        assert why is None, f"row {r} of {keys.shape}, {key_type}: {why}"


def rows_in_band(keys, mp, T, key_type):
    """how many rows have a key within 4 B of their theta (rows whose min-p is off: none)"""
    hit = 0
    for r in range(keys.shape[0]):
        if minp_on(mp[r]):
            s = np.unique(sortable16_np(keys[r], key_type, True))
            hit += minp_range_at(keys[r], key_type, T[r], mp[r], s)[3] > 0
    return hit


# ---- sharp inputs -----------------------------------------------------------------------------------------------------------------------------
def sharp_topp_rows(name, cols, key_type, T, seed):
    """_topp16.sharp_rows with p at the midpoint of each value's mass UNDER T; values whose mass under T is not above 1 % of the row
    are left out (a low temperature starves the lower levels)"""
    keys, _ = tp.sharp_rows(name, cols, key_type, seed)
    s, mass, A, Z = groups(keys[0], key_type, T)
    use = np.flatnonzero(mass / Z > 0.01)
    p = ((2 * A + mass) / (2 * Z)).astype(np.float32)[use]
    return keys[:use.size].copy(), p


def assert_sharp_topp(keys, p, T, key_type):
    for r in range(keys.shape[0]):
        ok = acceptable(keys[r], p[r], key_type, T[r])
        assert ok == [exact_threshold(keys[r], p[r], key_type, T[r])], (r, p[r], T[r], ok)


SHARP_T = np.array([0.5, 1.0, 2.0, 1.3], dtype=np.float32)


def sharp_minp_rows(name, cols, key_type, seed):
    """(keys [n, cols], mp [n] float32, T [n] float32): the same row of _topp16.SHARP_SETS levels n times; row j has
    mp = exp((midpoint - m) / T) for the j-th pair of neighbouring VALUES occurring in the row, T from SHARP_T by j.  A pair whose
    midpoint is not further than 4 B from both of its values -- the denormals next to zero, which no float32 theta tells apart -- is
    left out: assert_sharp_minp holds for every row returned."""
    keys, _ = tp.sharp_rows(name, cols, key_type, seed)
    row = keys[0]
    v = np.unique(tp.values64(row, key_type))[::-1]                     # distinct values, best first (-0.0 == +0.0)
    best = v[0]
    rows_mp, rows_t = [], []
    for j in range(v.size - 1):
        T = SHARP_T[j % SHARP_T.size]
        mid = (v[j] + v[j + 1]) / 2
        mp = np.float32(np.exp((mid - best) / float(T)))
        if not mp > 0:
            continue
        theta, band = theta_of(best, T, mp)
        if v[j] - theta > band and theta - v[j + 1] > band:
            rows_mp.append(mp)
            rows_t.append(T)
    n = len(rows_mp)
    return np.tile(row, (n, 1)), np.array(rows_mp, dtype=np.float32), np.array(rows_t, dtype=np.float32)


def assert_sharp_minp(keys, mp, T, key_type):
    """no key lies within 4 B of theta: the acceptance rule admits exactly the oracle's threshold"""
    for r in range(keys.shape[0]):
        s = np.unique(sortable16_np(keys[r], key_type, True))
        lo, hi, exact, in_band = minp_range_at(keys[r], key_type, T[r], mp[r], s)
        assert lo == hi == exact and in_band == 0, (r, mp[r], T[r], lo, hi, exact, in_band)


# ---- the draw under T --------------------------------------------------------------------------------------------------------------------------
def cdf(row, key_type, T=1.0):
    """_sample16.cdf under T: (w, C, Z) per position"""
    w, best = weights_of(tp.values64(row, key_type), T)
    inc = np.cumsum(w)
    return w, inc - w, float(inc[-1]) if w.size else 0.0


def exact_index(row, u, key_type, T=1.0):
    return sm.exact_from(*cdf(row, key_type, T), u)


def acceptable_index(row, u, key_type, T=1.0, m=M):
    return sm.acceptable_from(*cdf(row, key_type, T), u, m)


def logprob64(row, i, key_type, T=1.0):
    if i < 0:
        return float("nan")
    v = tp.values64(row, key_type)
    w, best = weights_of(v, T)
    if v[i] == best:
        first = 0.0
    elif is_greedy(T):
        first = float("-inf")
    else:
        first = float(v[i] - best) / t_eff(T)
    return first - float(np.log(w.sum()))


def logprob_tol(row, i, key_type, T=1.0):
    """2^-11 + 2^-22 |(x_i - m) / T|"""
    v = tp.values64(row, key_type)
    w, best = weights_of(v, T)
    if i < 0 or v[i] == best or is_greedy(T):
        return sm.LOGPROB_TOL
    return sm.LOGPROB_TOL + 2.0 ** -22 * abs(float(v[i] - best) / t_eff(T))


def check_draws(index, keys, u, T, key_type, logprob=None, m=M):
    """every returned index is accepted under T, every returned logprob within its bound for the index returned"""
    for r in range(keys.shape[0]):
        t = 1.0 if T is None else T[r]
        ok = acceptable_index(keys[r], u[r], key_type, t, m)
        i = int(index[r])
        assert i in ok, f"row {r} of {keys.shape}, {key_type}, u = {u[r]!r}, T = {t!r}: index {i} is not consistent with u +- {m}: {ok[:4]}"
        if logprob is not None:
            want, got = logprob64(keys[r], i, key_type, t), float(logprob[r])
            assert (np.isnan(want) and np.isnan(got)) or abs(got - want) <= logprob_tol(keys[r], i, key_type, t), \
                f"row {r} of {keys.shape}, {key_type}, T = {t!r}: logprob {got!r} of index {i}, float64 {want!r}"


def sharp_draw_rows(name, cols, key_type, T, seed, placement=False):
    """_sample16.sharp_rows' row with u at the midpoint of each heavy key's interval UNDER T: (keys, u, at).  Heavy keys that hold less
    than 0.5 % of the row under T are left out."""
    keys, _, at = sm.sharp_rows(name, cols, key_type, seed, placement=placement)
    w, C, Z = cdf(keys[0], key_type, T)
    use = at[w[at] / Z >= 0.005]
    u = ((2 * C[use] + w[use]) / (2 * Z)).astype(np.float32)
    return keys[:use.size].copy(), u, use


def assert_sharp_draw(keys, u, T, key_type):
    for r in range(keys.shape[0]):
        ok = acceptable_index(keys[r], u[r], key_type, T[r])
        assert ok == [exact_index(keys[r], u[r], key_type, T[r])], (r, u[r], T[r], ok)


def greedy_rows(cols, key_type, ties, seed):
    """one row of normal logits whose maximum occurs `ties` times (min(ties, cols)); returns (row, positions of the maximum)"""
    rng = np.random.default_rng(seed)
    row = tp.bits_of_values(np.clip(rng.standard_normal(cols) * 4, -30, 30), key_type)
    top = tp.bits_of_values(np.array([40.0]), key_type)[0]
    at = np.sort(rng.permutation(cols)[:min(ties, cols)])
    row[at] = top
    return tp.without_fill(row[None, :])[0], at


# ---- the inputs the GPU suite runs, for the band condition on the CPU ------------------------------------------------------------------------
COLS = (1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 16383, 16384, 16385, 20001, 70001, 131073)
ROWS = (1, 3, 9, 17, 64)


def family_cases(cols, key_type):
    """(name, keys, p, mp, T) for every family of _topp16.families at this row length: the row count runs through ROWS from family
    to family (and from length to length), the three cycles start at shifts of their own.  This is a reduction against the sibling
    suites, which cross every row count with every length for every family: here every (length, row count) pair occurs, but with
    one family each -- the float64 oracle of a [64 x 131073] case costs a second, and six families times five counts would not
    stay within a few seconds per test."""
    at = COLS.index(cols)
    made = {}
    for f, name in enumerate(sorted(tp.families(1, 1, key_type, seed=0))):
        rows = ROWS[(at + f) % len(ROWS)]
        if rows not in made:
            made[rows] = tp.families(rows, cols, key_type, seed=1000 * rows + cols)
        yield name, made[rows][name], tp.cycle_p(rows, at + f), cycle_mp(rows, 3 * at + f), cycle_t(rows, 5 * at + 2 * f)
