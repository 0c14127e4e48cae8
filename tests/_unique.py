"""Run-length encode and unique (csrc/unique.hip), restated in numpy (a helper module: no fixtures, no pytest settings).

    sortable(bits, key_type, descending)          the unsigned integers whose order is the library's order of the keys
    oracle_rle(bits)                              runs of equal adjacent words: keys, counts, starts
    oracle_unique(bits, key_type, descending)     distinct words in the library's order: keys, counts, first, inverse
    model_rle(bits, pos=None)                     the unit's own phases -- count | scan | emit -- tile by tile, wave by wave
    families(n, bits_per_key)                     the inputs of the tests, by name
    TILE, SCAN_ROUND, MAX_GRID, ...               csrc/run_tiles.hpp's constants, restated; unit_constants() reads them out of the source

Keys are handled as uint32 / uint64 bit patterns throughout; equality is equality of bits."""
import functools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = os.path.join(ROOT, "lsdradixsort_amd", "csrc", "unique.hip")
HEADER = os.path.join(ROOT, "lsdradixsort_amd", "csrc", "run_tiles.hpp")   # what the unit shares with reduce_by_key.hip

# ---- the constants of csrc/run_tiles.hpp, restated (tests/test_unique_cpu.py holds them to the source) ------------------------
THREADS = 256                      # kRunThreads
THREAD_KEYS = 16                   # kRunThreadKeys
TILE = THREADS * THREAD_KEYS       # kRunTile: keys of a workgroup
WAVE = 64
WAVES = THREADS // WAVE
SCAN_THREADS = 1024                # kRunScanThreads
SCAN_ROUND = 4 * SCAN_THREADS      # kRunScanRound: tile counts the one-workgroup scan takes per round
MAX_GRID = 2048                    # kRunMaxGrid: workgroups of the grid-stride copy kernel

SIZES = (1, 2, 3, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 5 * TILE + 7)
# One size past every loop's first round: the scan's second round starts at SCAN_ROUND tiles; the copy kernel's at
# MAX_GRID * THREADS 16-byte groups (far below BIG_N for either width).  BIG_DISTINCT: about 256 runs in every tile.
BIG_N = TILE * SCAN_ROUND + 5
BIG_DISTINCT = 2 * MAX_GRID * THREADS
assert BIG_N == (1 << 24) + 5 and BIG_DISTINCT == 1 << 20
assert -(-BIG_N // TILE) > SCAN_ROUND and BIG_DISTINCT > MAX_GRID * THREADS and BIG_N // 4 > MAX_GRID * THREADS

KEY_TYPES_32 = ("uint32", "int32", "float32")
KEY_TYPES_64 = ("uint64", "int64", "float64")
KEY_TYPES = KEY_TYPES_32 + KEY_TYPES_64
KEY_CODE = {name: code for code, name in enumerate(KEY_TYPES)}   # lsdsort_key_type

SENT = {32: 0x7E7E7E7E, 64: 0x7E7E7E7E7E7E7E7E}   # tests/_guarded.py: what the outputs are pre-filled with


def unit_constants():
    """{name: value} of the constexpr integers of run_tiles.hpp (the tile of unique.hip and reduce_by_key.hip) that are written as plain
    numbers."""
    text = open(HEADER).read()
    return {name: int(value) for name, value in re.findall(r"constexpr (?:int|uint32_t) (k\w+) = (\d+)u?;", text)}


def word(bits_per_key):
    return {32: np.uint32, 64: np.uint64}[bits_per_key]


def width_of(key_type):
    return 32 if key_type in KEY_TYPES_32 else 64


# ---- the oracle ----------------------------------------------------------------------------------------------------------------
def sortable(bits, key_type, descending=False):
    """The map of include/lsdsort.h (as tests/test_gpu_segmented.py and tests/test_gpu_containment.py restate it), either width."""
    w = width_of(key_type)
    u = word(w)
    bits = np.ascontiguousarray(bits, dtype=u)
    top = u(1 << (w - 1))
    if key_type.startswith("int"):
        t = bits ^ top
    elif key_type.startswith("float"):
        t = np.where(bits >> u(w - 1) != 0, ~bits, bits ^ top).astype(u)
    else:
        t = bits.copy()
    return (~t).astype(u) if descending else t


def heads_of(bits):
    """head(i) = i == 0 || bits[i] != bits[i - 1]"""
    heads = np.ones(bits.size, dtype=bool)
    heads[1:] = bits[1:] != bits[:-1]
    return heads


def oracle_rle(bits):
    """{keys, counts, starts} of the runs of equal adjacent words."""
    bits = np.ascontiguousarray(bits)
    starts = np.flatnonzero(heads_of(bits)).astype(np.uint32)
    counts = np.diff(np.append(starts, np.uint32(bits.size)).astype(np.int64)).astype(np.uint32)
    return {"keys": bits[starts], "counts": counts, "starts": starts}


def oracle_unique(bits, key_type, descending=False):
    """{keys, counts, first, inverse}: the distinct words in the library's order, how often each occurs, the lowest position that
    holds it, and for every position the index of its word."""
    bits = np.ascontiguousarray(bits, dtype=word(width_of(key_type)))
    order = np.argsort(sortable(bits, key_type, descending), kind="stable")
    in_order = bits[order]
    runs = oracle_rle(in_order)
    inverse = np.empty(bits.size, dtype=np.uint32)
    inverse[order] = (np.cumsum(heads_of(in_order)) - 1).astype(np.uint32)
    return {"keys": runs["keys"], "counts": runs["counts"], "first": order[runs["starts"]].astype(np.uint32), "inverse": inverse}


# ---- the unit's phases ---------------------------------------------------------------------------------------------------------
def model_rle(bits, pos=None, sentinel=0x7E7E7E7E):
    """count | scan | emit as unique.hip runs them.  A tile is TILE keys; thread t of a tile holds J groups of G = 16 bytes
    of keys, group j from (j * THREADS + t) * G on, so a tile's keys in position order are indexed (j, wave, lane, e).  Returns
    {num, keys, starts, counts[, first, inverse], tile_heads (scanned), rounds}; outputs are full length, pre-filled with the
    sentinel, and every store is guarded as in the kernel."""
    bits = np.ascontiguousarray(bits)
    n = bits.size
    G = 16 // bits.dtype.itemsize
    J = THREAD_KEYS // G
    tiles = max(-(-n // TILE), 1)
    # count: the flags of every tile, and one word per tile
    flags = np.zeros(tiles * TILE, dtype=bool)
    flags[:n] = heads_of(bits)
    flags = flags.reshape(tiles, J, WAVES, WAVE, G)
    tile_heads = flags.sum(axis=(1, 2, 3, 4)).astype(np.uint32)
    where = np.where(flags.reshape(tiles, TILE), np.arange(tiles * TILE, dtype=np.int64).reshape(tiles, TILE) + 1, 0)
    tile_last = where.max(axis=1).astype(np.uint32)                   # 1 + the position of the tile's last head, 0: none
    # scan: one workgroup, rounds of SCAN_ROUND words, the running total and the running last head carried
    carry, carry_last, rounds = 0, 0, 0
    for first in range(0, tiles, SCAN_ROUND):
        part = tile_heads[first:first + SCAN_ROUND].astype(np.int64)
        incl = np.cumsum(part)
        tile_heads[first:first + SCAN_ROUND] = (carry + incl - part).astype(np.uint32)
        carry += int(incl[-1])
        last = tile_last[first:first + SCAN_ROUND].astype(np.int64)
        incl_last = np.maximum(np.maximum.accumulate(last), carry_last)
        tile_last[first:first + SCAN_ROUND] = np.concatenate([[carry_last], incl_last[:-1]]).astype(np.uint32)
        carry_last = int(incl_last[-1])
        rounds += 1
    num = carry
    out = {"num": num, "tile_heads": tile_heads, "tile_last": tile_last, "rounds": rounds,
           "keys": np.full(n, sentinel if bits.dtype.itemsize == 4 else SENT[64], dtype=bits.dtype),
           "starts": np.full(n, sentinel, dtype=np.uint32), "counts": np.full(n, sentinel, dtype=np.uint32)}
    if pos is not None:
        out["first"] = np.full(n, sentinel, dtype=np.uint32)
        out["inverse"] = np.full(n, sentinel, dtype=np.uint32)
    if num == 0 or num > n:   # the fault: nothing is stored
        return out
    # emit: per group the thread's head count, the wave's inclusive scan, the waves' totals of every group, the tile's base
    count = flags.sum(axis=4)                                         # [tiles, J, WAVES, WAVE]
    incl = np.cumsum(count, axis=3)
    part = incl[:, :, :, WAVE - 1].reshape(tiles, J * WAVES)          # LDS: part[j * WAVES + wave]
    before = (np.cumsum(part, axis=1) - part).reshape(tiles, J, WAVES, 1)
    r = tile_heads.astype(np.int64).reshape(tiles, 1, 1, 1) + before + incl - count   # heads in front of the thread's group
    within = np.cumsum(flags, axis=4)                                 # heads of the group at or before e
    after = (r[..., None] + within).reshape(-1)[:n]                   # heads at positions <= i
    flat = flags.reshape(-1)[:n]
    i = np.flatnonzero(flat)
    rank = after[i] - 1
    ok = rank < n
    out["keys"][rank[ok]] = bits[i[ok]]
    out["starts"][rank[ok]] = i[ok]
    if pos is not None:
        out["first"][rank[ok]] = pos[i[ok]]
        inside = pos < n
        out["inverse"][pos[inside]] = (after - 1)[inside]
    # counts, by the emit kernel as well: every head stores the length of the run BEFORE it -- the head before it is the one it finds
    # in LDS at the rank below its own within the tile, and for the tile's first head the scanned tile_last; the scan stores the last
    # run's, from the last head of all to n
    tile_of = i // TILE
    q = rank - tile_heads[tile_of].astype(np.int64)
    head_before = np.where(q > 0, np.concatenate([[0], i[:-1]]) + 1, tile_last[tile_of].astype(np.int64))   # 1 + its position; 0: none
    ok = (rank >= 1) & (rank <= n) & (head_before >= 1) & (head_before <= i)
    out["counts"][rank[ok] - 1] = (i[ok] - (head_before[ok] - 1)).astype(np.uint32)
    out["counts"][num - 1] = n - (carry_last - 1)
    return out


def model_unique(bits, key_type, descending=False):
    """copy + positions | the stable sort | the run-length phases over the sorted copy."""
    bits = np.ascontiguousarray(bits, dtype=word(width_of(key_type)))
    order = np.argsort(sortable(bits, key_type, descending), kind="stable").astype(np.uint32)
    return model_rle(bits[order], pos=order)


# ---- inputs ------------------------------------------------------------------------------------------------------------------
F32_SPECIALS = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000,                    # +-0, +-inf
                         0x7FC00000, 0x7FC00001, 0x7F800001, 0xFFC00000, 0xFFC00001, 0xFF800001,   # three NaN payloads of each sign
                         0x3F800000, 0xBF800000, 0x00000001, 0x80000001, 0x7F7FFFFF, 0xFF7FFFFF],  # +-1, +-denormal, +-max
                        dtype=np.uint32)
F64_SPECIALS = np.array([0x0000000000000000, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000,
                         0x7FF8000000000000, 0x7FF8000000000001, 0x7FF0000000000001,
                         0xFFF8000000000000, 0xFFF8000000000001, 0xFFF0000000000001,
                         0x3FF0000000000000, 0xBFF0000000000000, 0x0000000000000001, 0x8000000000000001,
                         0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF], dtype=np.uint64)
# 64-bit words that differ only in the high or only in the low word, of both signs as int64
WORD_PAIRS = np.array([0x0000000100000005, 0x0000000200000005, 0x0000000100000006, 0xFFFFFFFF00000005, 0xFFFFFFFE00000005,
                       0xFFFFFFFF00000006, 0x0000000000000005, 0x0000000500000000, 0x8000000000000000, 0x8000000000000001,
                       0x8000000100000000, 0x7FFFFFFFFFFFFFFF, 0x7FFFFFFF00000000, 0x00000000FFFFFFFF, 0xFFFFFFFFFFFFFFFF],
                      dtype=np.uint64)


def specials(key_type):
    """The values of the float and word-difference cases for a key type, each several times over, shuffled."""
    w = width_of(key_type)
    base = F32_SPECIALS if w == 32 else np.concatenate([F64_SPECIALS, WORD_PAIRS])
    rng = np.random.default_rng(7 + w)
    bits = np.concatenate([base, base, base[::3], base[:5]])
    rng.shuffle(bits)
    return bits


def _clean(bits, w):
    """No word equals the sentinel the outputs are pre-filled with."""
    bits = np.ascontiguousarray(bits, dtype=word(w))
    bits[bits == word(w)(SENT[w])] ^= word(w)(1)
    bits.setflags(write=False)
    return bits


def _values(count, w, seed):
    """`count` distinct words of width w whose high and low halves both vary."""
    rng = np.random.default_rng(seed)
    if w == 32:
        return rng.permutation(1 << 20)[:count].astype(np.uint32) * np.uint32(4001) + np.uint32(17)
    lo = rng.permutation(1 << 20)[:count].astype(np.uint64)
    return (lo << np.uint64(40)) ^ (lo * np.uint64(2654435761)) ^ np.uint64(0x0000000300000000)


def _runs_of(length, n, w, seed):
    k = -(-n // length)
    return np.repeat(_values(k, w, seed), length)[:n]


@functools.lru_cache(maxsize=None)
def families(n, w, seed=0):
    """{name: words} -- the run-length inputs at size n and width w; runs of TILE, TILE - 1 and TILE + 1 put run edges on, before
    and after tile edges; `recurring` is unsorted: runs of three values come back again and again.  Another `seed` draws `random8`
    and `recurring` anew from the same values (tests/_replay.py)."""
    rng = np.random.default_rng(1000 * w + n + 7919 * seed)
    eight = _values(8, w, 3)
    three = _values(3, w, 4)
    lengths = rng.integers(1, 6, size=n)
    recurring = np.repeat(three[np.arange(n) % 3], lengths)[:n]
    two = _values(2, w, 5) if w == 32 else np.array([0x0000000100000005, 0x0000000200000005], dtype=np.uint64)   # the low words agree
    out = {
        "all_equal": np.full(n, _values(1, w, 6)[0], dtype=word(w)),
        "all_distinct": _values(n, w, 7) if n <= 1 << 20 else None,
        "alternating": two[np.arange(n) % 2],
        "runs_T": _runs_of(TILE, n, w, 8),
        "runs_T-1": _runs_of(TILE - 1, n, w, 9),
        "runs_T+1": _runs_of(TILE + 1, n, w, 10),
        "random8": eight[rng.integers(0, 8, size=n)],
        "recurring": recurring,
    }
    return {name: _clean(bits, w) for name, bits in out.items() if bits is not None}


@functools.lru_cache(maxsize=None)
def shuffled(n, w, name):
    """The family `name`, shuffled: the unique tests' input."""
    bits = families(n, w)[name].copy()
    np.random.default_rng(n + len(name)).shuffle(bits)
    bits.setflags(write=False)
    return bits


@functools.lru_cache(maxsize=None)
def big_keys(w):
    """BIG_N words with about BIG_DISTINCT distinct values (uniform below BIG_DISTINCT, spread over both halves of a 64-bit word)."""
    rng = np.random.default_rng(99 + w)
    v = rng.integers(0, BIG_DISTINCT, size=BIG_N, dtype=np.uint64)
    bits = (v * np.uint64(4001) + np.uint64(17)).astype(np.uint32) if w == 32 else (v << np.uint64(40)) ^ (v * np.uint64(2654435761))
    return _clean(bits, w)
