"""Oracle, acceptance rule and inputs of the top-p filter for 16-bit rows (a helper module: no fixtures, no pytest settings), for
test_gpu_topp16.py and test_topp16_cpu.py.

The oracle is numpy float64.  A row is grouped by distinct sortable value (the map of include/lsdsort.h with largest, restated in
_rowk16.py: smaller is better); per value j, best first: mass_j = count_j * w_j with w = 0 for a NaN, 1 at the largest non-NaN value m
and exp(x - m) elsewhere, A_j = the mass of the strictly better values, Z the total.  Value j is kept iff A_j < p Z or j == 0.

The device works in float32 and truncated fixed point, so a returned row is ACCEPTED iff (1) it is np.where(sortable(x) <=
sortable(T), x, fill) bit for bit for T its worst kept value, which occurs in the row, and (2) T is consistent with p +- M:
A(T) < (p + M) Z or T is the best value, and A(T) + mass(T) >= (p - M) Z or T is the worst value.  M = 2^-12 for |logit| <= 64 and
cols <= 2^17: the float32 x - m is off by at most 128 * 2^-24 in the exponent, the log2 e scaling and v_exp_f32 add about 1.2e-5
relative, truncation at most cols * 2^-32 <= 3.1e-5 of Z >= 1; the sum is below 6e-5 and M is four times that.  Rows whose filter is
off -- !(p < 1) -- are compared with the input bit for bit.  On SHARP rows (every distinct value carries mass far above M, p at the
midpoint of a value's mass) exactly one T is acceptable, so acceptance is equality with the float64 oracle."""
import numpy as np

from _rowk16 import sortable16_np

M = 2.0 ** -12
FILL = 0x7E7E          # the fill word of the tests: it occurs nowhere in their inputs (without_fill)
TYPES = ("float16", "bfloat16")
NEG_INF = {"float16": 0xFC00, "bfloat16": 0xFF80}
POS_INF = {"float16": 0x7C00, "bfloat16": 0x7F80}
P_CYCLE = np.array([0.0, 1e-30, 0.1, 0.5, 0.9, 0.99, 1.0 - 2.0 ** -24, 1.0, 1.5, -1.0, np.nan], dtype=np.float32)
# neighbours one bit pattern apart on both sides of the 5-bit, 8-bit and 11-bit digit boundaries; +-0, denormals and the sign
# crossing; three values
SHARP_SETS = {
    "near two": np.array([0x3FDF, 0x3FE0, 0x3FFF, 0x4000, 0x4001, 0x3F00, 0x3EFF, 0x4020, 0x401F, 0x3F80, 0x3F7F, 0x3F81], dtype=np.uint16),
    "around zero": np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x3C00, 0xBC00, 0x3BFF, 0xBC01], dtype=np.uint16),
    "three": np.array([0x4000, 0x3FFF, 0x3F80], dtype=np.uint16),
}


def values64(bits, key_type):
    """uint16 bit patterns -> their values as float64"""
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    if key_type == "float16":
        return bits.view(np.float16).astype(np.float64)
    with np.errstate(invalid="ignore"):   # signalling NaNs
        return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)


def bits_of_values(values, key_type):
    """float values -> the uint16 bit patterns of the type, rounded to nearest even"""
    values = np.ascontiguousarray(values, dtype=np.float32)
    if key_type == "float16":
        return values.astype(np.float16).view(np.uint16)
    u = values.view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def groups(row, key_type):
    """one row of bit patterns -> (s, mass, A, Z): the distinct sortable values best first, the mass of each, the mass strictly
    better than each, and the total, in float64"""
    s, first, count = np.unique(sortable16_np(row, key_type, True), return_index=True, return_counts=True)
    v = values64(row[first], key_type)
    number = ~np.isnan(v)
    w = np.zeros(v.shape)
    if number.any():
        best = v[number].max()
        with np.errstate(invalid="ignore"):
            w[number] = np.where(v[number] == best, 1.0, np.exp(v[number] - best))
    mass = count * w
    A = np.cumsum(mass) - mass
    return s, mass, A, float(mass.sum())


def is_off(p):
    return not (np.float32(p) < np.float32(1))


def exact_threshold(row, p, key_type):
    """sortable(T) of the float64 oracle for one row whose filter is on"""
    s, mass, A, Z = groups(row, key_type)
    kept = A < float(np.float32(p)) * Z
    kept[0] = True
    return int(s[np.flatnonzero(kept).max()])


def acceptable(row, p, key_type, m=M):
    """the sortable values of every T the acceptance rule admits for one row whose filter is on"""
    s, mass, A, Z = groups(row, key_type)
    p = float(np.float32(p))
    at = np.arange(s.size)
    ok = ((A < (p + m) * Z) | (at == 0)) & ((A + mass >= (p - m) * Z) | (at == s.size - 1))
    return [int(x) for x in s[ok]]


def filter_np(keys, p, key_type, fill=FILL):
    """the float64 oracle's output, bit for bit: keys [rows, cols] uint16, p [rows] float32"""
    out = keys.copy()
    for r in range(keys.shape[0]):
        if not is_off(p[r]):
            s = sortable16_np(keys[r], key_type, True)
            out[r] = np.where(s <= exact_threshold(keys[r], p[r], key_type), keys[r], np.uint16(fill))
    return out


def check_row(got, row, p, key_type, fill=FILL, m=M):
    """None where the returned row `got` is accepted for the input `row` (which holds no `fill`) and p, else what is wrong"""
    if is_off(p):
        return None if np.array_equal(got, row) else "a row whose filter is off differs from the input"
    kept = got != fill
    if not kept.any():
        return "no key was kept"
    s = sortable16_np(row, key_type, True)
    T = int(s[kept].max())
    want = np.where(s <= T, row, np.uint16(fill))
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        return f"not every key at least as good as T = {T:#x} and only those: {bad.size} words differ, first at {bad[0]}"
    ok = acceptable(row, p, key_type, m)
    if T not in ok:
        return f"T = {T:#x} (sortable) is not consistent with p = {p!r} +- {m}: acceptable {[hex(x) for x in ok[:4]]}"
    return None


def check_rows(got, keys, p, key_type, fill=FILL, m=M):
    for r in range(keys.shape[0]):
        why = check_row(got[r], keys[r], p[r], key_type, fill, m)
        assert why is None, f"row {r} of {keys.shape}, {key_type}, p = {p[r]!r}: {why}"


def without_fill(keys, fill=FILL):
    keys = keys.copy()
    keys[keys == fill] ^= np.uint16(1)
    return keys


def cycle_p(rows, shift=0):
    """[rows] float32: P_CYCLE shifted by the row index, so that the eight rows of one wave-tier workgroup differ"""
    return P_CYCLE[(np.arange(rows) + shift) % P_CYCLE.size]


def sharp_rows(name, cols, key_type, seed):
    """(keys [n, cols], p [n] float32): one row per distinct value j of a row drawn uniformly from the level set with every level
    present, p the midpoint (A_j + A_j+1) / (2 Z) of that value's mass.  cols >= the number of levels."""
    levels = SHARP_SETS[name]
    rng = np.random.default_rng(seed)
    row = levels[rng.integers(0, levels.size, cols)]
    row[rng.permutation(cols)[:levels.size]] = levels
    s, mass, A, Z = groups(row, key_type)
    p = ((2 * A + mass) / (2 * Z)).astype(np.float32)
    return np.tile(row, (s.size, 1)), p


def assert_sharp(keys, p, key_type):
    """every (row, p) has exactly one acceptable T, the float64 oracle's"""
    for r in range(keys.shape[0]):
        ok = acceptable(keys[r], p[r], key_type)
        assert ok == [exact_threshold(keys[r], p[r], key_type)], (r, p[r], ok)


def normal_rows(rows, cols, key_type, sigma, seed):
    """normal logits scaled by sigma, clamped to +-64"""
    rng = np.random.default_rng(seed)
    return without_fill(bits_of_values(np.clip(rng.standard_normal((rows, cols)) * sigma, -64, 64), key_type))


def families(rows, cols, key_type, seed):
    """name -> [rows, cols] bit patterns under the mass tolerance, none of them FILL"""
    rng = np.random.default_rng(seed)
    out = {f"normal sigma {sigma}": normal_rows(rows, cols, key_type, sigma, seed + sigma) for sigma in (1, 4, 16)}
    out["all equal"] = np.full((rows, cols), 0x3E37, dtype=np.uint16)
    out["shared top 11 bits"] = (np.uint16(0x3FC0) | rng.integers(0, 32, (rows, cols)).astype(np.uint16))
    lone = bits_of_values(rng.standard_normal((rows, cols)), key_type)
    lone[np.arange(rows), rng.integers(0, cols, rows)] = bits_of_values(np.array([40.0]), key_type)[0]   # a lone maximum far above the rest
    out["lone maximum"] = lone
    return {name: without_fill(keys) for name, keys in out.items()}


def special_rows(cols, key_type, seed):
    """[6, cols]: rows whose masses are 0 or 1 -- several +inf among numbers and NaNs, all -inf, NaNs of both signs around -inf
    and +inf, all NaN of both signs, one +NaN among -inf, +inf and -inf alone: the float64 oracle is exact on them"""
    rng = np.random.default_rng(seed)
    pinf, ninf = POS_INF[key_type], NEG_INF[key_type]
    nans = np.array([pinf + 1, ninf + 1, 0x7FFF, 0xFFFF], dtype=np.uint16)
    rows = []
    mixed = bits_of_values(rng.standard_normal(cols) * 4, key_type)
    mixed[rng.random(cols) < 0.2] = pinf
    mixed[rng.random(cols) < 0.1] = ninf
    pick = rng.random(cols) < 0.1
    mixed[pick] = nans[rng.integers(0, 4, int(pick.sum()))]
    mixed[rng.integers(0, cols)] = pinf
    rows.append(mixed)
    rows.append(np.full(cols, ninf, dtype=np.uint16))
    both = np.where(rng.random(cols) < 0.5, np.uint16(pinf), np.uint16(ninf))
    pick = rng.random(cols) < 0.3
    both[pick] = nans[rng.integers(0, 4, int(pick.sum()))]
    rows.append(both)
    rows.append(nans[rng.integers(0, 4, cols)])
    one = np.full(cols, ninf, dtype=np.uint16)
    one[rng.integers(0, cols)] = 0x7FFF
    rows.append(one)
    rows.append(np.where(rng.random(cols) < 0.5, np.uint16(pinf), np.uint16(ninf)))
    return without_fill(np.stack(rows).astype(np.uint16))
