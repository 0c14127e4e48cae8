"""Oracles and inputs of the per-row-k entries for 16-bit keys (a helper module: no fixtures, no pytest settings), for
test_gpu_kth16_rowk.py and test_kth16_rowk_cpu.py.

The oracle is numpy: the 16-bit sortable map of include/lsdsort.h restated, then np.argsort(kind="stable") per row.  The filter's
expected output is np.where(sortable(x) <= sortable(T_r), x, fill) with T_r item k_r - 1 of the row's stable sort; rows with
k_r == 0 or k_r >= cols (as uint32) are the input."""
import numpy as np

KEY_TYPES = {"uint16": 0, "int16": 1, "float16": 2, "bfloat16": 3}
ALL_TYPES = list(KEY_TYPES)
FILL = 0x7E7E          # the fill word of the filter tests: it occurs nowhere in their inputs (without_fill)
OFF = 0xFFFFFFFF       # an int32 -1 as the library reads it
# +-0, +-inf, NaNs of both signs (quiet, signalling, all ones), denormals, the largest finite values
SPECIALS = {
    "float16": np.array([0x0000, 0x8000, 0x7C00, 0xFC00, 0x7E00, 0xFE00, 0x7C01, 0xFC01, 0xFFFF, 0x7FFF, 0x0001, 0x8001, 0x03FF,
                         0x83FF, 0x7BFF, 0xFBFF], dtype=np.uint16),
    "bfloat16": np.array([0x0000, 0x8000, 0x7F80, 0xFF80, 0x7FC0, 0xFFC0, 0x7F81, 0xFF81, 0xFFFF, 0x7FFF, 0x0001, 0x8001, 0x007F,
                          0x807F, 0x7F7F, 0xFF7F], dtype=np.uint16),
}


def sortable16_np(u, key_type, largest):
    """the map of include/lsdsort.h restated: the uint16 whose unsigned order is the requested one"""
    u = u.astype(np.uint32)
    if key_type == "int16":
        u = u ^ np.uint32(0x8000)
    elif key_type in ("float16", "bfloat16"):
        u = u ^ np.where(u & np.uint32(0x8000), np.uint32(0xFFFF), np.uint32(0x8000))
    return ((u ^ np.uint32(0xFFFF)) if largest else u).astype(np.uint16)


def expected_np(keys, key_type, largest):
    """keys: [rows, cols] uint16 bits -> the full stable order of every row: (sorted keys, positions)"""
    order = np.argsort(sortable16_np(keys, key_type, largest), axis=1, kind="stable")
    return np.take_along_axis(keys, order, axis=1), order.astype(np.uint32)


def filter_on(k, cols):
    """which rows have their filter on: k as uint32"""
    k = np.asarray(k, dtype=np.uint32)
    return (k != 0) & (k < cols)


def filter_np(keys, k, key_type, largest, fill=FILL):
    """the filter's expected output, bit for bit: k [rows] uint32"""
    rows, cols = keys.shape
    s = sortable16_np(keys, key_type, largest)
    on = filter_on(k, cols)
    at = np.where(on, np.asarray(k, dtype=np.int64) - 1, cols - 1)
    thr = np.take_along_axis(np.sort(s, axis=1), at[:, None], axis=1)      # sortable(T_r); the row's worst key where the filter is off
    return np.where(s <= thr, keys, np.uint16(fill)).astype(np.uint16)


def without_fill(keys):
    """the keys with every FILL changed in its lowest bit: a kept key and a filled one can then never be confused"""
    keys = keys.copy()
    keys[keys == FILL] ^= np.uint16(1)
    return keys


def candidates_ranks(cols):
    return sorted({r for r in (0, 1, cols // 2, cols - 2, cols - 1) if 0 <= r < cols})


def candidates_k(cols):
    return [0, 1, 2, cols // 2, cols - 1, cols, cols + 5, OFF]


def cycle(values, rows, shift=0):
    """[rows] uint32: the values in a cycle shifted by the row index (and by `shift`), so that neighbouring rows -- the eight of one
    workgroup of the wave tier -- differ"""
    values = np.asarray(values, dtype=np.uint32)
    return values[(np.arange(rows) + shift) % values.size]


def shifts(values, rows):
    """the shifts at which `rows` rows see every one of the values"""
    return range(0, len(values), rows) if rows < len(values) else (0,)


def inputs(rows, cols, key_type, seed):
    """name -> [rows, cols] uint16 bit patterns, none of them FILL"""
    rng = np.random.default_rng(seed)

    def rnd(hi):
        return rng.integers(0, hi, (rows, cols), dtype=np.uint32).astype(np.uint16)

    out = {"uniform bits": rnd(1 << 16)}
    four = np.array([5, 0x0100, 0x7FFF, 0xFFF0], dtype=np.uint16)
    out["four values"] = four[rng.integers(0, 4, (rows, cols))]                  # tie runs across lanes, waves and chunks
    out["all equal"] = np.full((rows, cols), 0x9E37, dtype=np.uint16)            # the position must equal the rank; never filled
    out["shared top 11 bits"] = np.uint16(0xABC0) | rnd(32)                      # the second level decides; long rows are all ties
    out["shared top 8 bits"] = np.uint16(0xAB00) | rnd(256)
    lone = np.full((rows, cols), 0x4000, dtype=np.uint16)                        # one 0x0001 among 0x4000s: the select stops after
    lone[np.arange(rows), rng.integers(0, cols, rows)] = 0x0001                  # the first level or round, with a nonzero shift
    out["lone minimum"] = lone
    if key_type in SPECIALS:
        f = rnd(1 << 16).reshape(-1)
        pick = rng.random(rows * cols) < 0.3
        f[pick] = SPECIALS[key_type][rng.integers(0, SPECIALS[key_type].size, int(pick.sum()))]
        out["float specials"] = f.reshape(rows, cols)
    return {name: without_fill(keys) for name, keys in out.items()}
