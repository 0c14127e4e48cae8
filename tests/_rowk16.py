"""Oracles and inputs of the per-row-k entries for 16-bit keys (a helper module: no fixtures, no pytest settings), for
test_gpu_kth16_rowk.py and test_kth16_rowk_cpu.py.

The oracle is numpy: _key_oracle.py's restatement of the 16-bit sortable map, then np.argsort(kind="stable") per row.  The filter's
expected output is np.where(sortable(x) <= sortable(T_r), x, fill) with T_r item k_r - 1 of the row's stable sort; rows with
k_r == 0 or k_r >= cols (as uint32) are the input."""
import numpy as np

# the oracle's own pieces, under the names this module's users know them by (rk.KEY_TYPES, rk.expected_np, ...)
from _key_oracle import (
    ALL_TYPES16 as ALL_TYPES, KEY_TYPES16 as KEY_TYPES, SPECIALS16 as SPECIALS, expected_np, inputs16, sortable16_np,
)

FILL = 0x7E7E          # the fill word of the filter tests: it occurs nowhere in their inputs (without_fill)
OFF = 0xFFFFFFFF       # an int32 -1 as the library reads it


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
    """name -> [rows, cols] uint16 bit patterns: the families of _key_oracle.inputs16, none of them holding FILL"""
    return {name: without_fill(keys) for name, keys in inputs16(rows, cols, key_type, seed).items()}
