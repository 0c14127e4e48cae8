"""CPU suite: run-length encode and unique (lsdsort_rle_device, lsdsort_unique_device; csrc/unique.hip) without a device -- the C-ABI
surface and the Python face, the argument checks of both entries in the header's order, the workspace figures, the numpy oracle
against np.unique and hand-written rows, the numpy restatement of the unit's phases (count | scan | emit) against the
oracle at every size the GPU suite runs, and the kernels' resources from hipcc's own remarks."""
import json
import os
import re

import numpy as np
import pytest

import _unique as un
from _faces import FakeCuda, lib as _lib, no_library
from _kernel_resources import hipcc, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "kernel_resources_unique.json")
ENTRIES = ("lsdsort_rle_workspace_bytes", "lsdsort_rle_device", "lsdsort_unique_workspace_bytes", "lsdsort_unique_device",
           "lsdsort_unique_check_device")
NAMES = ("GPURunLength", "GPUUnique", "rle_workspace_bytes", "unique_workspace_bytes", "unique", "unique_consecutive")
FAKE = 1 << 20   # an address that is never dereferenced: every call that gets it returns before a device is touched


# ---- surface ---------------------------------------------------------------------------------------------------------------------
def test_header_ctypes_table_makefile_and_faces_have_the_entries():
    import lsdradixsort_amd as lsd
    from lsdradixsort_amd import _lib as binding

    raw = open(os.path.join(ROOT, "include", "lsdsort.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"LSDSORT_API\s+[\w\s\*]+?\b" + name + r"\s*\(", text), name
        assert name in binding.SIGNATURES
        assert hasattr(_lib(), name)
    assert len(binding.SIGNATURES["lsdsort_rle_device"][1]) == 10 and len(binding.SIGNATURES["lsdsort_unique_device"][1]) == 12
    # the header says how equality is meant, next to the torch equivalents
    for words in ("BIT PATTERNS", "torch.unique_consecutive", "torch.unique", "-0.0 and +0.0 are two values"):
        assert words in raw, words
    for name in NAMES:
        assert callable(getattr(lsd, name)) and name in lsd.api.__all__, name
    makefile = open(os.path.join(ROOT, "lsdradixsort_amd", "csrc", "Makefile")).read()
    assert "unique" in re.search(r"^NAMES\s*:=(.*)$", makefile, flags=re.M).group(1).split()
    # no C++ wrapper yet: INTEGRATION.md names it as missing
    assert "lsdsort_unique_device" not in open(os.path.join(ROOT, "include", "lsdsort.hpp")).read()
    assert "lsdsort_unique_device" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_the_restated_constants_are_the_units():
    k = un.unit_constants()
    assert (k["kRunThreads"], k["kRunThreadKeys"], k["kRunScanThreads"], k["kRunMaxGrid"]) == (un.THREADS, un.THREAD_KEYS, un.SCAN_THREADS,
                                                                                               un.MAX_GRID)
    header = open(un.HEADER).read()
    assert "kRunTile = kRunThreads * kRunThreadKeys;" in header and "kRunScanRound = 4 * kRunScanThreads;" in header
    # the constants are csrc/run_tiles.hpp's: the unit defines none of them itself
    text = open(un.UNIT).read()
    assert not re.findall(r"constexpr[^;\n]*\bkRun\w+\s*=", text)
    # the grid cap the unit has: the grid-stride copy kernel's, and none on the per-tile kernels
    caps = re.findall(r"grid_for\(([^,()]+),\s*(\w+)\s*,\s*([^()]+?)\)\)", text)
    assert [cap for _, _, cap in caps] == ["kRunMaxGrid"], caps                     # the copy kernel's
    assert un.SIZES == (1, 2, 3, 4095, 4096, 4097, 8193, 20487)


# ---- argument checks -------------------------------------------------------------------------------------------------------------
def test_rle_argument_checks_in_entry_order():
    from lsdradixsort_amd import errors as E

    L = _lib()
    BIG = E.LSDSORT_MAX_KEYS

    def call(keys=FAKE, out=FAKE + 4096, counts=None, starts=None, num=FAKE + 8192, w=FAKE, wb=None, n=1000, bits=32):
        if wb is None:
            wb = L.lsdsort_rle_workspace_bytes(min(n, BIG), bits if bits in (32, 64) else 32)
        return L.lsdsort_rle_device(keys, n, bits, out, counts, starts, num, w, wb, None)

    # 1. the width, before everything else
    for bits in (0, 16, 31, 33, 128, -32):
        assert call(bits=bits, n=BIG + 1, keys=None, w=None) == E.LSDSORT_ERR_INVALID_ARG, bits
        assert call(bits=bits, n=0) == E.LSDSORT_ERR_INVALID_ARG, bits
    # 2. the size, before the empty call, the pointers and the workspace
    assert call(n=BIG + 1, keys=None, out=None, num=None, w=None) == E.LSDSORT_ERR_TOO_LARGE
    # 3. nothing to do, before the pointers and the workspace (without a count word there is not even the one store)
    for bits in (32, 64):
        assert call(n=0, bits=bits, keys=None, out=None, num=None, w=None, wb=0) == E.LSDSORT_OK
    # 4. the pointers and their alignment, before the workspace
    for bad in (dict(keys=None), dict(out=None), dict(num=None), dict(out=FAKE), dict(keys=FAKE + 2), dict(out=FAKE + 4098),
                dict(counts=FAKE + 2), dict(starts=FAKE + 1), dict(num=FAKE + 8193), dict(keys=FAKE + 4, bits=64),
                dict(out=FAKE + 4100, bits=64)):
        assert call(w=None, **bad) == E.LSDSORT_ERR_INVALID_ARG, bad
    # 5. the workspace: exactly the figure
    assert call(w=None) == E.LSDSORT_ERR_WORKSPACE
    assert call(w=FAKE + 128) == E.LSDSORT_ERR_WORKSPACE
    for bits in (32, 64):
        need = L.lsdsort_rle_workspace_bytes(1000, bits)
        assert need > 0 and call(bits=bits, wb=need - 1, counts=FAKE + 12288, starts=FAKE + 16384) == E.LSDSORT_ERR_WORKSPACE
    # 6. the device answers last; word alignment of the keys and an odd 4-byte alignment of the outputs are enough
    import torch

    if not torch.cuda.is_available():
        assert call() == E.LSDSORT_ERR_NO_DEVICE
        assert call(keys=FAKE + 4, out=FAKE + 4100, counts=FAKE + 12292, starts=FAKE + 16388, num=FAKE + 8196) == E.LSDSORT_ERR_NO_DEVICE
        assert call(keys=FAKE + 8, bits=64) == E.LSDSORT_ERR_NO_DEVICE
        assert call(n=0, num=FAKE + 8192) == E.LSDSORT_ERR_NO_DEVICE          # the one store of an empty call needs the device


def test_unique_argument_checks_in_entry_order():
    from lsdradixsort_amd import errors as E

    L = _lib()
    BIG = E.LSDSORT_MAX_KEYS

    def call(keys=FAKE, out=FAKE + 8192, counts=None, first=None, inverse=None, num=FAKE + 4096, w=FAKE, wb=None, n=1000, kt=0, desc=0):
        if wb is None:
            wb = L.lsdsort_unique_workspace_bytes(min(n, BIG), kt if 0 <= kt < 6 else 0, 1 if first or inverse else 0)
        return L.lsdsort_unique_device(keys, n, kt, desc, out, counts, first, inverse, num, w, wb, None)

    # 1. the key type, before everything else
    for kt in (-1, 6, 7, 100):
        assert call(kt=kt, n=BIG + 1, keys=None, w=None) == E.LSDSORT_ERR_INVALID_ARG, kt
        assert call(kt=kt, n=0) == E.LSDSORT_ERR_INVALID_ARG, kt
    # 2. the size
    assert call(n=BIG + 1, keys=None, out=None, num=None, w=None) == E.LSDSORT_ERR_TOO_LARGE
    # 3. nothing to do
    for kt in range(6):
        for desc in (0, 1):
            assert call(n=0, kt=kt, desc=desc, keys=None, out=None, num=None, w=None, wb=0) == E.LSDSORT_OK
    # 4. the pointers and their alignment; the keys themselves may take the result
    for bad in (dict(keys=None), dict(out=None), dict(num=None), dict(keys=FAKE + 2), dict(out=FAKE + 8194), dict(counts=FAKE + 2),
                dict(first=FAKE + 1), dict(inverse=FAKE + 3), dict(num=FAKE + 4097), dict(keys=FAKE + 4, kt=3), dict(out=FAKE + 8196, kt=5)):
        assert call(w=None, **bad) == E.LSDSORT_ERR_INVALID_ARG, bad
    assert call(out=FAKE, w=None) == E.LSDSORT_ERR_WORKSPACE
    # 5. the workspace: the figure for what is asked for
    assert call(w=None) == E.LSDSORT_ERR_WORKSPACE
    assert call(w=FAKE + 128) == E.LSDSORT_ERR_WORKSPACE
    for kt in range(6):
        for positions in (0, 1):
            need = L.lsdsort_unique_workspace_bytes(1000, kt, positions)
            assert need > 0 and call(kt=kt, wb=need - 1, inverse=FAKE + 16384 if positions else None) == E.LSDSORT_ERR_WORKSPACE
            if L.lsdsort_unique_workspace_bytes(1000, kt, 1) > L.lsdsort_unique_workspace_bytes(1000, kt, 0):
                assert call(kt=kt, wb=L.lsdsort_unique_workspace_bytes(1000, kt, 0), first=FAKE + 16384) == E.LSDSORT_ERR_WORKSPACE
    # 6. the device
    import torch

    if not torch.cuda.is_available():
        for kt in range(6):
            assert call(kt=kt, desc=kt & 1, counts=FAKE + 12292, first=FAKE + 16388, inverse=FAKE + 20484) == E.LSDSORT_ERR_NO_DEVICE
        assert call(out=FAKE) == E.LSDSORT_ERR_NO_DEVICE
    # the check entry: its own arguments first, an empty call is clean
    assert L.lsdsort_unique_check_device(None, 1000, 0, 0, None) == E.LSDSORT_ERR_WORKSPACE
    assert L.lsdsort_unique_check_device(FAKE, 1000, 6, 0, None) == E.LSDSORT_ERR_INVALID_ARG
    assert L.lsdsort_unique_check_device(FAKE, BIG + 1, 0, 0, None) == E.LSDSORT_ERR_TOO_LARGE
    assert L.lsdsort_unique_check_device(FAKE, 0, 4, 1, None) == E.LSDSORT_OK


def test_workspace_figures():
    from lsdradixsort_amd import errors as E

    L = _lib()
    ladder = [0, 1, 2, 3, un.TILE - 1, un.TILE, un.TILE + 1, 20487, (1 << 20) + 13, un.BIG_N, 1 << 28, E.LSDSORT_MAX_KEYS]
    for bits in (32, 64):
        prev = 0
        for n in ladder:
            b = L.lsdsort_rle_workspace_bytes(n, bits)
            tiles = max(-(-n // un.TILE), 1)
            assert b > 0 and b % 256 == 0 and b >= prev and b >= 256 + 8 * tiles, (n, bits, b, prev)
            prev = b
        assert L.lsdsort_rle_workspace_bytes(E.LSDSORT_MAX_KEYS + 1, bits) == 0
    for bits in (0, 16, 48, -1):
        assert L.lsdsort_rle_workspace_bytes(1000, bits) == 0
    for kt in range(6):
        wide = kt >= 3
        for positions in (0, 1):
            prev = 0
            for n in ladder:
                b = L.lsdsort_unique_workspace_bytes(n, kt, positions)
                inner = L.lsdsort_wide_workspace_bytes(n, 8, 64, 32 * positions) if wide else L.lsdsort_workspace_bytes(n, 8, positions)
                # control block, key copy, positions, the sort inside, the run-length arrays
                assert b > 0 and b % 256 == 0 and b >= prev, (n, kt, positions, b, prev)
                assert b >= 256 + (8 if wide else 4) * n + 4 * n * positions + inner + L.lsdsort_rle_workspace_bytes(n, 32) - 256, (n, kt)
                prev = b
            assert L.lsdsort_unique_workspace_bytes(E.LSDSORT_MAX_KEYS + 1, kt, positions) == 0
        for n in ladder:
            assert L.lsdsort_unique_workspace_bytes(n, kt, 1) >= L.lsdsort_unique_workspace_bytes(n, kt, 0)
            assert L.lsdsort_unique_workspace_bytes(n, kt, 7) == L.lsdsort_unique_workspace_bytes(n, kt, 1)   # a flag
    for kt in (-1, 6, 9):
        assert L.lsdsort_unique_workspace_bytes(1000, kt, 0) == 0


# ---- the oracle ------------------------------------------------------------------------------------------------------------------
def test_oracle_on_hand_written_rows():
    bits = np.array([5, 5, 7, 5, 5, 5, 9], dtype=np.uint32)
    r = un.oracle_rle(bits)
    assert r["keys"].tolist() == [5, 7, 5, 9] and r["counts"].tolist() == [2, 1, 3, 1] and r["starts"].tolist() == [0, 2, 3, 6]
    u = un.oracle_unique(bits, "uint32")
    assert u["keys"].tolist() == [5, 7, 9] and u["counts"].tolist() == [5, 1, 1] and u["first"].tolist() == [0, 2, 6]
    assert u["inverse"].tolist() == [0, 0, 1, 0, 0, 0, 2]
    d = un.oracle_unique(bits, "uint32", descending=True)
    assert d["keys"].tolist() == [9, 7, 5] and d["counts"].tolist() == [1, 1, 5] and d["first"].tolist() == [6, 2, 0]
    # int32: the sign bit sorts first; uint32: last
    bits = np.array([1, 0xFFFFFFFF, 0, 0x80000000, 1], dtype=np.uint32)
    assert un.oracle_unique(bits, "int32")["keys"].tolist() == [0x80000000, 0xFFFFFFFF, 0, 1]
    assert un.oracle_unique(bits, "uint32")["keys"].tolist() == [0, 1, 0x80000000, 0xFFFFFFFF]
    # one element; nothing
    assert un.oracle_rle(np.array([3], dtype=np.uint64))["counts"].tolist() == [1]
    assert un.oracle_rle(np.array([], dtype=np.uint32))["keys"].size == 0


@pytest.mark.parametrize("key_type", ["float32", "float64"])
def test_oracle_orders_floats_by_total_order_and_compares_bits(key_type):
    w = un.width_of(key_type)
    specials = un.F32_SPECIALS if w == 32 else un.F64_SPECIALS
    bits = np.concatenate([specials, specials[::-1]])
    u = un.oracle_unique(bits, key_type)
    assert u["keys"].size == specials.size and (u["counts"] == 2).all()          # -0.0 and +0.0, and every NaN payload, are values
    values = u["keys"].view(np.float32 if w == 32 else np.float64)
    nan = np.isnan(values)
    # -NaNs (three payloads), then the numbers ascending with -0.0 in front of +0.0, then +NaNs (three payloads)
    assert nan[:3].all() and nan[-3:].all() and not nan[3:-3].any()
    assert (np.signbit(values[:3])).all() and not np.signbit(values[-3:]).any()
    body = values[3:-3]
    assert (np.diff(body) >= 0).all() and np.isneginf(body[0]) and np.isposinf(body[-1])
    zero = np.flatnonzero(body == 0)
    assert zero.size == 2 and np.signbit(body[zero[0]]) and not np.signbit(body[zero[1]])
    top = specials.dtype.type(1 << (w - 1))
    assert u["keys"][:3].tolist() == sorted((specials[specials > top][np.isnan(specials[specials > top].view(values.dtype))]).tolist(),
                                            reverse=True)                          # larger payload = more negative
    # without -0.0 and NaN the result is numpy's, bit for bit
    plain = bits[~np.isnan(bits.view(values.dtype)) & (bits != top)]
    want, index, inverse, counts = np.unique(plain.view(values.dtype), return_index=True, return_inverse=True, return_counts=True)
    got = un.oracle_unique(plain, key_type)
    assert np.array_equal(got["keys"], want.view(bits.dtype)) and np.array_equal(got["counts"], counts)
    assert np.array_equal(got["first"], index) and np.array_equal(got["inverse"], inverse.reshape(-1))
    d = un.oracle_unique(bits, key_type, descending=True)
    assert np.array_equal(d["keys"], u["keys"][::-1]) and np.array_equal(d["inverse"], specials.size - 1 - u["inverse"])


def test_oracle_int64_keys_that_differ_in_one_word_only():
    bits = np.concatenate([un.WORD_PAIRS, un.WORD_PAIRS[::2]])
    for key_type, view in (("int64", np.int64), ("uint64", np.uint64)):
        want, index, inverse, counts = np.unique(bits.view(view), return_index=True, return_inverse=True, return_counts=True)
        got = un.oracle_unique(bits, key_type)
        assert got["keys"].size == un.WORD_PAIRS.size                              # all distinct: no word is dropped from the compare
        assert np.array_equal(got["keys"], want.view(np.uint64)) and np.array_equal(got["counts"], counts)
        assert np.array_equal(got["first"], index) and np.array_equal(got["inverse"], inverse.reshape(-1))


@pytest.mark.parametrize("w", [32, 64])
def test_oracle_against_numpy_on_the_families(w):
    for n in un.SIZES:
        for name in un.families(n, w):
            bits = un.shuffled(n, w, name)
            want, index, inverse, counts = np.unique(bits, return_index=True, return_inverse=True, return_counts=True)
            got = un.oracle_unique(bits, "uint%d" % w)
            assert np.array_equal(got["keys"], want) and np.array_equal(got["counts"], counts), (n, name)
            assert np.array_equal(got["first"], index) and np.array_equal(got["inverse"], inverse.reshape(-1)), (n, name)
            assert np.array_equal(got["keys"][got["inverse"]], bits) and np.array_equal(bits[got["first"]], got["keys"])


# ---- the unit's phases, restated -----------------------------------------------------------------------------------------------
def _assert_model_rle(bits, what):
    n = bits.size
    want = un.oracle_rle(bits)
    got = un.model_rle(bits)
    m = want["keys"].size
    assert got["num"] == m and got["rounds"] == max(-(-max(-(-n // un.TILE), 1) // un.SCAN_ROUND), 1), what
    for name in ("keys", "starts", "counts"):
        assert np.array_equal(got[name][:m], want[name]), (what, name)
        assert (got[name][m:] == un.SENT[8 * got[name].dtype.itemsize]).all(), (what, name, "written past the count")


@pytest.mark.parametrize("w", [32, 64])
def test_model_of_the_run_length_phases_against_the_oracle(w):
    seen = set()
    for n in un.SIZES:
        fam = un.families(n, w)
        assert set(fam) == {"all_equal", "all_distinct", "alternating", "runs_T", "runs_T-1", "runs_T+1", "random8", "recurring"}
        for name, bits in fam.items():
            _assert_model_rle(bits, (n, name))
            seen.add(un.oracle_rle(bits)["keys"].size)
    assert {1, un.SIZES[-1]} <= seen                                                # one run, and a run per key
    # run edges on, before and behind tile edges
    n = un.SIZES[-1]
    for name, length in (("runs_T", un.TILE), ("runs_T-1", un.TILE - 1), ("runs_T+1", un.TILE + 1)):
        starts = un.oracle_rle(un.families(n, w)[name])["starts"]
        assert starts[1] == length and {int(s) % un.TILE for s in starts[1:3]} == {(length * k) % un.TILE for k in (1, 2)}
    # the unsorted family: values come back
    r = un.oracle_rle(un.families(n, w)["recurring"])
    assert np.unique(r["keys"]).size == 3 and r["keys"].size > 1000


@pytest.mark.parametrize("key_type", un.KEY_TYPES)
@pytest.mark.parametrize("descending", [False, True])
def test_model_of_unique_against_the_oracle(key_type, descending):
    w = un.width_of(key_type)
    inputs = [(("specials",), un.specials(key_type))]
    inputs += [((n, name), un.shuffled(n, w, name)) for n in un.SIZES for name in ("alternating", "random8", "runs_T-1", "all_distinct")]
    for what, bits in inputs:
        want = un.oracle_unique(bits, key_type, descending)
        got = un.model_unique(bits, key_type, descending)
        m = want["keys"].size
        assert got["num"] == m, what
        for name in ("keys", "counts", "first"):
            assert np.array_equal(got[name][:m], want[name]), (what, name)
            assert (got[name][m:] == un.SENT[8 * got[name].dtype.itemsize]).all(), (what, name)
        assert np.array_equal(got["inverse"], want["inverse"]), what
        assert np.array_equal(got["keys"][got["inverse"]], bits), what


def test_model_at_the_size_past_every_first_round():
    """The scan's second round with its two carries, and more 16-byte groups than the copy kernel's grid has threads."""
    bits = np.sort(un.big_keys(32))
    assert bits.size == un.BIG_N
    want, index, counts = np.unique(bits, return_index=True, return_counts=True)
    assert want.size > un.MAX_GRID * un.THREADS and abs(want.size - un.BIG_DISTINCT) < un.BIG_DISTINCT // 8
    got = un.model_rle(bits)
    m = want.size
    assert got["num"] == m and got["rounds"] == 2 and got["tile_heads"].size == un.SCAN_ROUND + 1
    assert np.array_equal(got["keys"][:m], want) and np.array_equal(got["counts"][:m], counts) and np.array_equal(got["starts"][:m], index)
    assert (got["keys"][m:] == un.SENT[32]).all() and (got["counts"][m:] == un.SENT[32]).all()


# ---- the Python face ---------------------------------------------------------------------------------------------------------


def test_wrappers_check_their_tensors_before_the_library(no_library):
    import torch

    lsd = no_library
    for dtype in (torch.int32, torch.float32, torch.int64, torch.float64):
        t = torch.zeros(8, dtype=dtype)
        for call in (lsd.GPURunLength, lsd.GPUUnique, lsd.unique, lsd.unique_consecutive):
            with pytest.raises(TypeError):
                call(t)                                                          # a CPU tensor
    for call in (lsd.GPURunLength, lsd.GPUUnique, lsd.unique, lsd.unique_consecutive):
        with pytest.raises(TypeError):
            call([3, 1, 2])

    def fake(dtype, n=8):
        return torch.zeros(n, dtype=dtype).as_subclass(FakeCuda)

    for call in (lsd.GPURunLength, lsd.GPUUnique, lsd.unique, lsd.unique_consecutive):
        with pytest.raises(TypeError):
            call(fake(torch.int16))                                              # 16-bit keys are not served here
        with pytest.raises(TypeError):
            call(fake(torch.int32).view(2, 4))                                   # 1-D only
    for dtype, key_type in ((torch.float32, "int32"), (torch.float32, "float64"), (torch.int32, "int64"), (torch.int64, "float32"),
                            (torch.float64, "uint64")):
        with pytest.raises(TypeError):
            lsd.GPUUnique(fake(dtype), key_type=key_type)
    with pytest.raises(ValueError):
        lsd.GPUUnique(fake(torch.int32), key_type="int16")
    keys = fake(torch.int32)
    with pytest.raises(ValueError):
        lsd.GPURunLength(keys, out=keys)                                         # the runs cannot go where the keys are read
    with pytest.raises(ValueError):
        lsd.GPURunLength(keys, out=fake(torch.int32, 9))
    with pytest.raises(TypeError):
        lsd.GPUUnique(keys, out=fake(torch.float32))
    for name in ("counts", "starts"):
        with pytest.raises(ValueError):
            lsd.GPURunLength(keys, **{name: fake(torch.int32, 7)})
        with pytest.raises(TypeError):
            lsd.GPURunLength(keys, **{name: 1})
    for name in ("counts", "first", "inverse"):
        with pytest.raises(TypeError):
            lsd.GPUUnique(keys, **{name: fake(torch.int64)})
    for fn in (lsd.unique, lsd.unique_consecutive, lsd.GPUUnique, lsd.GPURunLength):
        assert "-0.0" in fn.__doc__ and "NaN" in fn.__doc__, fn.__name__          # the float difference is stated


# ---- kernel resources ------------------------------------------------------------------------------------------------------------
def test_kernels_no_scratch_no_spill_and_recorded_resources():
    if hipcc() is None:
        pytest.skip("no hipcc on this machine")
    res = kernel_resources("unique.hip")
    names = list(res)
    # the exact kernel set: count and emit per word, emit and copy with and without positions, one scan, one store
    sets = {"rle_count_kernel": 2, "rle_scan_kernel": 1, "rle_emit_kernel": 4, "run_store_kernel": 1, "unique_copy_kernel": 4}
    for must, times in sets.items():
        assert sum(must in name for name in names) == times, (must, names)
    assert len(names) == sum(sets.values()), names
    for name, r in res.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r)
    want = json.load(open(GOLDEN))["unique.hip"]
    assert sorted(res) == sorted(want), f"kernels gone: {sorted(set(want) - set(res))}, new: {sorted(set(res) - set(want))}"
    for name, w in want.items():
        assert res[name]["occupancy"] >= w["occupancy"], f"{name}: {res[name]['occupancy']} waves/SIMD, recorded {w['occupancy']}"
        assert res[name]["lds_bytes"] == w["lds_bytes"], f"{name}: {res[name]['lds_bytes']} B of static LDS, recorded {w['lds_bytes']}"


def test_the_unit_includes_four_files_only_and_has_no_inline_assembly():
    text = open(un.UNIT).read()
    assert re.findall(r"#include\s+(\S+)", text) == ['"../../include/lsdsort.h"', '"lsd_device.hpp"', '"lsd_host.hpp"', '"run_tiles.hpp"']
    unit = re.sub(r"//.*", "", text)
    shared = re.sub(r"//.*", "", open(un.HEADER).read())
    code = unit + shared   # what the unit compiles beside the three files it always had
    assert "asm" not in code
    # it reaches the sorts through their public device entries -- each call stands once, in the shared header -- and waits for no
    # other workgroup
    for call in ("lsdsort_keys_device(", "lsdsort_keys64_device(", "lsdsort_check_device(", "lsdsort_wide_check_device("):
        assert shared.count(call) == 1 and call not in unit, call
    for word in ("load_status", "store_status", "__hip_atomic", "hipMalloc", "hipStreamSynchronize", "hipDeviceSynchronize"):
        assert word not in code, word
