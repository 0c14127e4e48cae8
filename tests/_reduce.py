"""Reduce by key (csrc/reduce_by_key.hip), restated in numpy (a helper module: no fixtures, no pytest settings).

    oracle_reduce_runs(bits, vals, val_type, op)                        per run of equal adjacent words: keys, vals, counts
    oracle_reduce_by_key(bits, vals, key_type, descending, val_type, op) per distinct word, in the library's order
    sum_bound(bits, vals)                                               per run: the float64 sum and the bound of any summation order
    values(n, family, val_type)                                          the value inputs of the tests, by name
    key_families(n, w)                                                   tests/_unique.py's families and `runs_2T+3`

Keys are uint32 / uint64 bit patterns, values uint32 bit patterns throughout; `val_type` says how the value bits are read."""
import functools

import numpy as np

import _unique as un

VAL_TYPES = ("uint32", "int32", "float32")
VAL_CODE = {name: code for code, name in enumerate(VAL_TYPES)}   # lsdsort_val_type
OPS = ("sum", "min", "max")
OP_CODE = {name: code for code, name in enumerate(OPS)}          # lsdsort_reduce_op
U = 2.0 ** -24                                                   # unit roundoff of float32


def from_sortable_f32(t):
    """The inverse of _unique.sortable(bits, "float32")."""
    t = np.ascontiguousarray(t, dtype=np.uint32)
    top = np.uint32(1 << 31)
    return np.where(t >> np.uint32(31) != 0, t ^ top, ~t).astype(np.uint32)


def _starts(bits):
    return np.flatnonzero(un.heads_of(bits))


def reduce_at(vals, starts, val_type, op):
    """`op` over vals[starts[j] : starts[j + 1]], the value bits read as `val_type`; returns uint32 bits."""
    vals = np.ascontiguousarray(vals, dtype=np.uint32)
    if starts.size == 0:
        return np.zeros(0, dtype=np.uint32)
    if op == "sum":
        if val_type == "float32":
            with np.errstate(invalid="ignore", over="ignore"):
                return np.add.reduceat(vals.view(np.float32).astype(np.float64), starts).astype(np.float32).view(np.uint32)
        return np.add.reduceat(vals, starts, dtype=np.uint32)                           # mod 2^32, either sign
    pick = np.minimum if op == "min" else np.maximum
    if val_type == "uint32":
        return pick.reduceat(vals, starts)
    if val_type == "int32":
        return pick.reduceat(vals.view(np.int32), starts).view(np.uint32)
    return from_sortable_f32(pick.reduceat(un.sortable(vals, "float32"), starts))       # the library's float total order


def oracle_reduce_runs(bits, vals, val_type, op):
    """{keys, vals, counts} of the runs of equal adjacent words of `bits`."""
    bits = np.ascontiguousarray(bits)
    runs = un.oracle_rle(bits)
    return {"keys": runs["keys"], "vals": reduce_at(vals, _starts(bits), val_type, op), "counts": runs["counts"]}


def oracle_reduce_by_key(bits, vals, key_type, descending, val_type, op):
    """The same per distinct word, in the library's order: the stable argsort of the sortable keys, then the runs."""
    bits = np.ascontiguousarray(bits, dtype=un.word(un.width_of(key_type)))
    order = np.argsort(un.sortable(bits, key_type, descending), kind="stable")
    return oracle_reduce_runs(bits[order], np.ascontiguousarray(vals, dtype=np.uint32)[order], val_type, op)


def sum_bound(bits, vals):
    """(s64, bound) per run of `bits`: the float64 sum of the float32 values and gamma * sum|v| with gamma = (L-1)u / (1 - (L-1)u),
    the error bound of float32 summation in ANY order (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2)."""
    starts = _starts(np.ascontiguousarray(bits))
    v = np.ascontiguousarray(vals, dtype=np.uint32).view(np.float32).astype(np.float64)
    length = np.diff(np.append(starts, v.size)).astype(np.float64)
    gamma = (length - 1) * U / (1 - (length - 1) * U)
    return np.add.reduceat(v, starts), gamma * np.add.reduceat(np.abs(v), starts)


# ---- inputs ------------------------------------------------------------------------------------------------------------------
VALUE_FAMILIES = ("ones", "small_ints", "wrap", "specials", "normal")


@functools.lru_cache(maxsize=None)
def values(n, family, val_type, seed=0):
    """uint32 bits of `n` values of `val_type`, none of them the sentinel the outputs are pre-filled with.
    ones: 1 | small_ints: integer-valued, |v| <= 100 | wrap: int32 near +-2^31 | specials: _unique.F32_SPECIALS tiled | normal: float32
    normal numbers x 2^k, k in -10..10, both signs."""
    rng = np.random.default_rng(31 * n + 7 * len(family) + seed)
    if family == "ones":
        whole = np.ones(n, dtype=np.int64)
    elif family == "small_ints":
        whole = rng.integers(-100, 101, size=n)
    if family in ("ones", "small_ints"):
        out = whole.astype(np.float32).view(np.uint32) if val_type == "float32" else whole.astype(np.int32).view(np.uint32)
    elif family == "wrap":
        assert val_type != "float32"
        near = rng.integers(0, 100, size=n)
        out = np.where(rng.integers(0, 2, size=n) == 0, (1 << 31) - 1 - near, -(1 << 31) + near).astype(np.int32).view(np.uint32)
    elif family == "specials":
        assert val_type == "float32"
        out = np.tile(un.F32_SPECIALS, -(-n // un.F32_SPECIALS.size))[:n].copy()
        rng.shuffle(out)
    elif family == "normal":
        assert val_type == "float32"
        out = (rng.standard_normal(n) * np.exp2(rng.integers(-10, 11, size=n))).astype(np.float32).view(np.uint32)
    else:
        raise KeyError(family)
    out = np.ascontiguousarray(out, dtype=np.uint32).copy()
    out[out == np.uint32(un.SENT[32])] ^= np.uint32(1)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def key_families(n, w):
    """tests/_unique.py's run-length inputs and `runs_2T+3`: runs of 2 * TILE + 3 keys, so that whole tiles lie inside a run."""
    out = dict(un.families(n, w))
    out["runs_2T+3"] = un._clean(un._runs_of(2 * un.TILE + 3, n, w, 11), w)
    return out


@functools.lru_cache(maxsize=None)
def shuffled(n, w, name):
    """The key family `name`, shuffled: the by-key tests' input."""
    if name in un.families(n, w):
        return un.shuffled(n, w, name)
    bits = key_families(n, w)[name].copy()
    np.random.default_rng(n + len(name)).shuffle(bits)
    bits.setflags(write=False)
    return bits
