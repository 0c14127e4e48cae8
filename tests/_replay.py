"""Repeated runs of one device entry in ONE workspace and one set of buffers, eager and as a captured graph (a helper module: no
fixtures, no pytest settings).  tests/test_gpu_replay.py runs every cell of CELLS five times, each time on another key family, so that
a later run meets the state a different earlier run left; tests/test_replay_cpu.py holds this module to numpy.

    RUNS                                         the five (family, seed) of a cell, in order; run 0 is the warm-up and the captured call
    keys(n, key_type, run)                       the words of run `run`: the families of tests/_unique.py
    payload(n, run, k)                           payload array k of run `run`: positions above a base that no other run or array has
    oracle_sort / oracle_histograms / oracle_partition        numpy's stable argsort, bincount
    CELLS, ENTRIES, MODES                        what is run; cell_id(cell) names a cell

Keys are uint32 / uint64 bit patterns throughout; every comparison is of bits."""
import functools
import os
import re

import numpy as np

import _unique as un

ROOT = un.ROOT
HOST_HEADER = os.path.join(ROOT, "lsdradixsort_amd", "csrc", "lsd_host.hpp")
API = os.path.join(ROOT, "lsdradixsort_amd", "csrc", "lsdsort_api.hip")

TILE = un.TILE                       # 4096: a tile of the run-length phases, and the unit the sizes are named in
SMALL_SORT_CAP = 16384               # kLocalSortCap: up to here a plain uint32 sort is one launch (lsdsort_set_small_sort)
N2 = TILE + 1                        # two tiles
N3 = 2 * TILE + 1                    # three tiles: the size at which the second replay was seen to fail
N_CHAINED = SMALL_SORT_CAP + 1       # plain uint32 reaches the chained form unaided
N_PARITY = (1 << 18) + 77            # what tests/test_gpu_parity.py replays
SIZES = (N2, N3, N_CHAINED, N_PARITY)
assert SIZES == (4097, 8193, 16385, 262221)

# the families change from run to run and are fixed: two values | eight | n | one | eight, drawn anew
RUNS = (("alternating", 0), ("random8", 0), ("all_distinct", 0), ("all_equal", 0), ("random8", 1))
DISTINCT = {"alternating": 2, "random8": 8, "all_distinct": None, "all_equal": 1}   # None: every key
MODES = ("eager", "graph")           # five plain calls | warm-up, one capture, four replays

ALIGN = 256                          # lsd::kAlign, and lsd::kCtlBytes: unique's control block in front of its key copy
SENT = un.SENT


def host_constants():
    """{name: value} of lsd_host.hpp's constexpr sizes, and the small sort's cap as lsdsort_api.hip's comment states it."""
    out = {name: int(value) for name, value in re.findall(r"constexpr size_t (k\w+) = (\d+);", open(HOST_HEADER).read())}
    out["small_sort_cap"] = int(re.search(r"// Up to (\d+) items: one workgroup sorts them in its LDS", open(API).read()).group(1))
    return out


def _align(x):
    return -(-x // ALIGN) * ALIGN


def unique_sort_offset(n, w, positions):
    """Where the sort's workspace begins inside unique's: control block | key copy | positions | the sort's (csrc/unique.hip)."""
    return ALIGN + _align(n * w // 8) + (_align(4 * n) if positions else 0)


# ---- inputs ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def keys(n, key_type, run):
    """The words of run `run` at size n.  Floats: `all_distinct` holds +-0, +-inf, three NaN payloads of either sign, +-denormal."""
    w = un.width_of(key_type)
    name, seed = RUNS[run]
    bits = un.families(n, w, seed)[name]
    if name == "all_distinct" and key_type.startswith("float"):
        special = un.F32_SPECIALS if w == 32 else un.F64_SPECIALS
        bits = bits.copy()
        bits[np.arange(special.size) * (n // special.size) + 3] = special
        bits.setflags(write=False)
    return bits


@functools.lru_cache(maxsize=None)
def payload(n, run, k=0):
    """Payload array k of run `run`: the positions, above a base of its own -- a payload word left over from another run, or from
    the other array, is not a word of this one (what a sentinel is to an output)."""
    assert n <= 1 << 20 and 0 <= k < 4 and 0 <= run < len(RUNS)
    out = np.arange(n, dtype=np.uint32) + np.uint32((1 + 4 * run + k) << 20)
    out.setflags(write=False)
    return out


# ---- oracles -----------------------------------------------------------------------------------------------------------------
def oracle_sort(bits, key_type, descending, payloads=()):
    """(keys, [payloads]) in the library's order of the key type, ties in input order: numpy's stable argsort of the mapped keys."""
    order = np.argsort(un.sortable(bits, key_type, descending), kind="stable")
    return bits[order], [np.asarray(p)[order] for p in payloads]


def oracle_histograms(bits, radix_bits=8):
    """[32 / radix_bits][2^radix_bits] counts, digit 0 the lowest bits."""
    bins = 1 << radix_bits
    return np.stack([np.bincount(((bits >> np.uint32(radix_bits * g)) & np.uint32(bins - 1)).astype(np.int64), minlength=bins)
                     for g in range(32 // radix_bits)]).astype(np.uint32)


def msb_buckets(bits, msb_bits):
    return (bits >> np.uint32(32 - msb_bits)).astype(np.int64) if msb_bits else np.zeros(bits.size, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def splitters(n, log2_buckets):
    """2^log2_buckets - 1 ascending splitters, the same for every run of a cell (they travel in the captured launch): quantiles of
    the all-distinct run, so keys EQUAL to a splitter occur, and the runs of few values leave buckets empty."""
    in_order = np.sort(keys(n, "uint32", 2))
    count = (1 << log2_buckets) - 1
    return tuple(int(in_order[(i + 1) * n >> log2_buckets]) for i in range(count))


def splitter_buckets(bits, values):
    """bucket = number of splitters <= key"""
    return np.searchsorted(np.asarray(values, dtype=np.uint32), bits, side="right").astype(np.int64)


def oracle_partition(bits, bucket, buckets):
    """(keys by bucket, ties in input order; uint64 counts)"""
    return bits[np.argsort(bucket, kind="stable")], np.bincount(bucket, minlength=buckets).astype(np.uint64)


# ---- the cells -----------------------------------------------------------------------------------------------------------------
def _cell(entry, n, **how):
    return dict(entry=entry, n=n, **how)


def _cells():
    out = []
    # the typed 32-bit entry: no plan word, the key transform in the first and the last pass
    for n in (N3, N2):
        for key_type in ("int32", "float32"):
            for descending in (False, True):
                for payloads in (0, 1):
                    out.append(_cell("lsdsort_keys_device", n, key_type=key_type, descending=descending, payloads=payloads))
    out.append(_cell("lsdsort_keys_device", N_PARITY, key_type="int32", descending=True, payloads=1))
    # plain uint32: the chained form unaided, the chained form with the one-launch sort switched off, and the one-launch sort
    for n, small in ((N_CHAINED, True), (N3, False), (N3, True)):
        out.append(_cell("lsdsort_u32_device", n, small=small))
        out.append(_cell("lsdsort_pairs_u32_device", n, small=small))
    out.append(_cell("lsdsort_multi_u32_device", N3, payloads=2))
    # 64-bit keys: the sticky word's clear and two sorts in one graph
    for key_type, descending in (("float64", True), ("int64", False)):
        for val_bits in (0, 32):
            out.append(_cell("lsdsort_keys64_device", N3, key_type=key_type, descending=descending, val_bits=val_bits))
    out.append(_cell("lsdsort_unique_device", N3, key_type="int32", descending=True, outputs=("counts", "first", "inverse")))
    out.append(_cell("lsdsort_unique_device", N3, key_type="float64", descending=True, outputs=("counts", "first", "inverse")))
    out.append(_cell("lsdsort_unique_device", N3, key_type="int32", descending=True, outputs=("counts",)))   # no positions
    out.append(_cell("lsdsort_digit_histograms_u32_device", N3, radix_bits=8))                               # the caller's table
    for bits in (0, 1, 3):
        out.append(_cell("lsdsort_msb_partition_u32_device", N3, msb_bits=bits))
        out.append(_cell("lsdsort_splitter_partition_u32_device", N3, log2_buckets=bits))
    return out


CELLS = _cells()

# Every exported entry that reaches one of the clears a caller can capture (the sort's opening clear, the clear of the caller's table
# in the histogram entry, the partitions' opening clear, the wide sort's sticky word) has a row above.  A literal list: an entry that
# is added to the library with such a clear gets a row here, or tests/test_replay_cpu.py says so.
ENTRIES = (
    "lsdsort_keys_device",
    "lsdsort_u32_device",
    "lsdsort_pairs_u32_device",
    "lsdsort_multi_u32_device",
    "lsdsort_keys64_device",
    "lsdsort_unique_device",
    "lsdsort_digit_histograms_u32_device",
    "lsdsort_msb_partition_u32_device",
    "lsdsort_splitter_partition_u32_device",
)
# Entries that reach the same clears and have NO row, and why (tests/test_replay_cpu.py holds the two lists to the library's exports)
REACHED_THROUGH = {
    "lsdsort_u32_device_ex": "lsdsort_u32_device and lsdsort_pairs_u32_device are this call",
    "lsdsort_u32_device_prefixed": "lsdsort_u32_device with the half variant kept out",
    "lsdsort_u64_device": "lsdsort_keys64_device with uint64 keys",
    "lsdsort_records_device": "lsdsort_keys64_device with payloads, or the same sort_wide",
    "lsdsort_threshold_partition_u32_device": "the splitter partition with 64-bit thresholds: the same partition_impl",
    "lsdsort_keys16_device": "its widen route calls lsdsort_pairs_u32_device; its own clear is a kernel (tests/test_gpu_keys16.py)",
    "lsdsort_u32_device_timed": "records events and reads them back: not capturable",
    "lsdsort_u32": "host pointers: synchronises, not capturable",
    "lsdsort_u32_ex": "host pointers: synchronises, not capturable",
    "lsdsort_u32_loopback": "host pointers: synchronises, not capturable",
    "lsdsort_pairs_u32": "host pointers: synchronises, not capturable",
    "lsdsort_sharded_u32_device": "a collective step with host-side waits: not capturable",
    "lsdsort_sharded_u32_device_ex": "a collective step with host-side waits: not capturable",
}


def cell_id(cell):
    parts = [cell["entry"].replace("lsdsort_", "").replace("_device", ""), str(cell["n"])]
    for name, value in cell.items():
        if name in ("entry", "n"):
            continue
        if name == "descending":
            parts.append("descending" if value else "ascending")
        elif name == "small":
            parts.append("small_on" if value else "small_off")
        elif name == "outputs":
            parts.append("+".join(value))
        elif name == "key_type":
            parts.append(value)
        else:
            parts.append("%s%s" % (name, value))
    return "-".join(parts)
