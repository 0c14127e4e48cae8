"""CPU suite: reduce by key (lsdsort_reduce_runs_device, lsdsort_reduce_by_key_device; csrc/reduce_by_key.hip) without a device -- the
C-ABI surface and the Python face, the argument checks of both entries in the header's order, the workspace figures, the numpy oracle
of tests/_reduce.py on hand-written rows and against np.unique + np.add.at, and the kernels' resources from hipcc's own remarks."""
import json
import os
import re

import numpy as np
import pytest

import _reduce as rd
import _unique as un
from _faces import FakeCuda, lib as _lib, no_library
from _kernel_resources import hipcc, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = os.path.join(ROOT, "lsdradixsort_amd", "csrc", "reduce_by_key.hip")
GOLDEN = os.path.join(ROOT, "tests", "golden", "kernel_resources_reduce.json")
ENTRIES = ("lsdsort_reduce_runs_workspace_bytes", "lsdsort_reduce_runs_device", "lsdsort_reduce_by_key_workspace_bytes",
           "lsdsort_reduce_by_key_device", "lsdsort_reduce_by_key_check_device")
NAMES = ("GPUReduceRuns", "GPUReduceByKey", "reduce_runs_workspace_bytes", "reduce_by_key_workspace_bytes", "reduce_by_key",
         "reduce_consecutive")
FAKE = 1 << 20   # an address that is never dereferenced: every call that gets it returns before a device is touched


def _header():
    raw = open(os.path.join(ROOT, "include", "lsdsort.h")).read()
    return raw, re.sub(r"/\*.*?\*/", "", raw, flags=re.S)


# ---- surface ---------------------------------------------------------------------------------------------------------------------
def test_header_ctypes_table_makefile_and_faces_have_the_entries():
    import lsdradixsort_amd as lsd
    from lsdradixsort_amd import _lib as binding

    raw, text = _header()
    for name in ENTRIES:
        assert re.search(r"LSDSORT_API\s+[\w\s\*]+?\b" + name + r"\s*\(", text), name
        assert name in binding.SIGNATURES
        assert hasattr(_lib(), name)
    args = {name: len(binding.SIGNATURES[name][1]) for name in ENTRIES}
    assert list(args.values()) == [2, 13, 2, 14, 4], args
    for name, count in args.items():   # the table has as many arguments as the header declares
        declared = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S).group(1)
        assert len(declared.split(",")) == count, name
    # the header says what the operations mean
    for words in ("mod 2^32", "TOTAL ORDER", "-NaN < -inf", "FIXED BY THE POSITIONS ALONE", "no identity element is ever added",
                  "IN INPUT ORDER", "MAY BE d_keys", "thrust::reduce_by_key"):
        assert words in raw, words
    for name in NAMES:
        assert callable(getattr(lsd, name)) and name in lsd.api.__all__, name
    makefile = open(os.path.join(ROOT, "lsdradixsort_amd", "csrc", "Makefile")).read()
    assert "reduce_by_key" in re.search(r"^NAMES\s*:=(.*)$", makefile, flags=re.M).group(1).split()
    # no C++ wrapper yet: INTEGRATION.md names it as missing
    assert "lsdsort_reduce_by_key_device" not in open(os.path.join(ROOT, "include", "lsdsort.hpp")).read()
    assert "lsdsort_reduce_by_key_device" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_enum_values_match_errors_py_and_the_helper():
    from lsdradixsort_amd import errors as E

    _, text = _header()
    for enum, count in (("lsdsort_reduce_op", 3), ("lsdsort_val_type", 3)):
        body = re.search(r"typedef\s+enum\s+%s\s*\{(.*?)\}\s*%s\s*;" % (enum, enum), text, flags=re.S).group(1)
        pairs = re.findall(r"(LSDSORT_\w+)\s*=\s*(-?\d+)", body)
        assert len(pairs) == count == len([item for item in body.split(",") if item.strip()]), enum
        for name, value in pairs:
            assert getattr(E, name) == int(value), name
    assert E.REDUCE_OPS == {"sum": E.LSDSORT_REDUCE_SUM, "min": E.LSDSORT_REDUCE_MIN, "max": E.LSDSORT_REDUCE_MAX} == rd.OP_CODE
    assert E.VAL_TYPES == {"uint32": E.LSDSORT_VAL_U32, "int32": E.LSDSORT_VAL_I32, "float32": E.LSDSORT_VAL_F32} == rd.VAL_CODE


# ---- argument checks -------------------------------------------------------------------------------------------------------------
def test_reduce_runs_argument_checks_in_entry_order():
    from lsdradixsort_amd import errors as E

    L = _lib()
    BIG = E.LSDSORT_MAX_KEYS

    def call(keys=FAKE, vals=FAKE + 4096, out=FAKE + 8192, out_vals=FAKE + 16384, counts=None, num=FAKE + 20480, w=FAKE, wb=None, n=1000,
             bits=32, vt=0, op=0):
        if wb is None:
            wb = L.lsdsort_reduce_runs_workspace_bytes(min(n, BIG), bits if bits in (32, 64) else 32)
        return L.lsdsort_reduce_runs_device(keys, vals, n, bits, vt, op, out, out_vals, counts, num, w, wb, None)

    # 1. the width, the value type and the operation, before everything else
    for bad in [dict(bits=b) for b in (0, 16, 31, 33, 128, -32)] + [dict(vt=v) for v in (-1, 3, 7)] + [dict(op=o) for o in (-1, 3, 9)]:
        assert call(n=BIG + 1, keys=None, w=None, **bad) == E.LSDSORT_ERR_INVALID_ARG, bad
        assert call(n=0, **bad) == E.LSDSORT_ERR_INVALID_ARG, bad
    # 2. the size, before the empty call, the pointers and the workspace
    assert call(n=BIG + 1, keys=None, vals=None, out=None, out_vals=None, num=None, w=None) == E.LSDSORT_ERR_TOO_LARGE
    # 3. nothing to do, before the pointers and the workspace (without a count word there is not even the one store)
    for bits in (32, 64):
        for vt in range(3):
            for op in range(3):
                assert call(n=0, bits=bits, vt=vt, op=op, keys=None, vals=None, out=None, out_vals=None, num=None, w=None, wb=0) == E.LSDSORT_OK
    # 4. the pointers, 5. their alignment, 6. the two aliases -- all before the workspace
    for bad in (dict(keys=None), dict(vals=None), dict(out=None), dict(out_vals=None), dict(num=None),
                dict(keys=FAKE + 2), dict(vals=FAKE + 4098), dict(out=FAKE + 8194), dict(out_vals=FAKE + 16385), dict(counts=FAKE + 2),
                dict(num=FAKE + 20481), dict(keys=FAKE + 4, bits=64), dict(out=FAKE + 8196, bits=64),
                dict(out=FAKE), dict(out_vals=FAKE + 4096), dict(out=FAKE, out_vals=FAKE + 4096)):
        assert call(w=None, **bad) == E.LSDSORT_ERR_INVALID_ARG, bad
    # a NULL or misaligned array is reported although an alias is there as well; an alias although the workspace is missing
    assert call(out=FAKE, num=None, w=None) == E.LSDSORT_ERR_INVALID_ARG
    # 7. the workspace: exactly the figure
    assert call(w=None) == E.LSDSORT_ERR_WORKSPACE
    assert call(w=FAKE + 128) == E.LSDSORT_ERR_WORKSPACE
    for bits in (32, 64):
        need = L.lsdsort_reduce_runs_workspace_bytes(1000, bits)
        assert need > 0 and call(bits=bits, wb=need - 1, counts=FAKE + 12288) == E.LSDSORT_ERR_WORKSPACE
    # 8. the device answers last; word alignment of the arrays is enough
    import torch

    if not torch.cuda.is_available():
        assert call() == E.LSDSORT_ERR_NO_DEVICE
        assert call(keys=FAKE + 4, vals=FAKE + 4100, out=FAKE + 8204, out_vals=FAKE + 16388, counts=FAKE + 12292, num=FAKE + 20484, vt=2,
                    op=2) == E.LSDSORT_ERR_NO_DEVICE
        assert call(keys=FAKE + 8, bits=64, vt=1, op=1) == E.LSDSORT_ERR_NO_DEVICE
        assert call(n=0, num=FAKE + 20480) == E.LSDSORT_ERR_NO_DEVICE         # the one store of an empty call needs the device


def test_reduce_by_key_argument_checks_in_entry_order():
    from lsdradixsort_amd import errors as E

    L = _lib()
    BIG = E.LSDSORT_MAX_KEYS

    def call(keys=FAKE, vals=FAKE + 4096, out=FAKE + 8192, out_vals=FAKE + 16384, counts=None, num=FAKE + 20480, w=FAKE, wb=None, n=1000,
             kt=0, desc=0, vt=0, op=0):
        if wb is None:
            wb = L.lsdsort_reduce_by_key_workspace_bytes(min(n, BIG), kt if 0 <= kt < 6 else 0)
        return L.lsdsort_reduce_by_key_device(keys, vals, n, kt, desc, vt, op, out, out_vals, counts, num, w, wb, None)

    # 1. the key type, the value type and the operation
    for bad in [dict(kt=k) for k in (-1, 6, 7, 100)] + [dict(vt=v) for v in (-1, 3)] + [dict(op=o) for o in (-1, 3)]:
        assert call(n=BIG + 1, keys=None, w=None, **bad) == E.LSDSORT_ERR_INVALID_ARG, bad
        assert call(n=0, **bad) == E.LSDSORT_ERR_INVALID_ARG, bad
    # 2. the size
    assert call(n=BIG + 1, keys=None, vals=None, out=None, out_vals=None, num=None, w=None) == E.LSDSORT_ERR_TOO_LARGE
    # 3. nothing to do
    for kt in range(6):
        for desc in (0, 1):
            assert call(n=0, kt=kt, desc=desc, vt=kt % 3, op=kt % 3, keys=None, vals=None, out=None, out_vals=None, num=None, w=None,
                        wb=0) == E.LSDSORT_OK
    # 4. the pointers and 5. their alignment
    for bad in (dict(keys=None), dict(vals=None), dict(out=None), dict(out_vals=None), dict(num=None), dict(keys=FAKE + 2),
                dict(vals=FAKE + 4097), dict(out=FAKE + 8194), dict(out_vals=FAKE + 16386), dict(counts=FAKE + 2), dict(num=FAKE + 20481),
                dict(keys=FAKE + 4, kt=3), dict(out=FAKE + 8196, kt=5)):
        assert call(w=None, **bad) == E.LSDSORT_ERR_INVALID_ARG, bad
    # 6. no alias is forbidden here: the inputs themselves may take the result
    assert call(out=FAKE, out_vals=FAKE + 4096, w=None) == E.LSDSORT_ERR_WORKSPACE
    # 7. the workspace
    assert call(w=None) == E.LSDSORT_ERR_WORKSPACE
    assert call(w=FAKE + 128) == E.LSDSORT_ERR_WORKSPACE
    for kt in range(6):
        need = L.lsdsort_reduce_by_key_workspace_bytes(1000, kt)
        assert need > 0 and call(kt=kt, wb=need - 1, counts=FAKE + 12288) == E.LSDSORT_ERR_WORKSPACE
        assert call(kt=kt, wb=L.lsdsort_reduce_runs_workspace_bytes(1000, 64)) == E.LSDSORT_ERR_WORKSPACE
    # 8. the device
    import torch

    if not torch.cuda.is_available():
        for kt in range(6):
            assert call(kt=kt, desc=kt & 1, vt=kt % 3, op=(kt + 1) % 3, counts=FAKE + 12292) == E.LSDSORT_ERR_NO_DEVICE
        assert call(out=FAKE, out_vals=FAKE + 4096) == E.LSDSORT_ERR_NO_DEVICE
    # the check entry: its own arguments first, an empty call is clean
    assert L.lsdsort_reduce_by_key_check_device(None, 1000, 0, None) == E.LSDSORT_ERR_WORKSPACE
    assert L.lsdsort_reduce_by_key_check_device(FAKE, 1000, 6, None) == E.LSDSORT_ERR_INVALID_ARG
    assert L.lsdsort_reduce_by_key_check_device(FAKE, BIG + 1, 0, None) == E.LSDSORT_ERR_TOO_LARGE
    assert L.lsdsort_reduce_by_key_check_device(FAKE, 0, 4, None) == E.LSDSORT_OK


def test_workspace_figures():
    from lsdradixsort_amd import errors as E

    L = _lib()
    ladder = [0, 1, 2, 3, un.TILE - 1, un.TILE, un.TILE + 1, 20487, (1 << 20) + 13, un.BIG_N, 1 << 28, E.LSDSORT_MAX_KEYS]
    for bits in (32, 64):
        prev = 0
        for n in ladder:
            b = L.lsdsort_reduce_runs_workspace_bytes(n, bits)
            tiles = max(-(-n // un.TILE), 1)
            assert b > 0 and b % 256 == 0 and b >= prev and b >= 256 + 12 * tiles, (n, bits, b, prev)   # control block, three tile arrays
            prev = b
        assert L.lsdsort_reduce_runs_workspace_bytes(E.LSDSORT_MAX_KEYS + 1, bits) == 0
    for bits in (0, 16, 48, -1):
        assert L.lsdsort_reduce_runs_workspace_bytes(1000, bits) == 0
    for kt in range(6):
        wide = kt >= 3
        prev = 0
        for n in ladder:
            b = L.lsdsort_reduce_by_key_workspace_bytes(n, kt)
            inner = L.lsdsort_wide_workspace_bytes(n, 8, 64, 32) if wide else L.lsdsort_workspace_bytes(n, 8, 1)
            assert b > 0 and b % 256 == 0 and b >= prev, (n, kt, b, prev)
            # the runs entry's figure (control block and tile arrays), the two copies, the sort inside
            assert b >= L.lsdsort_reduce_runs_workspace_bytes(n, 64 if wide else 32) + (8 if wide else 4) * n + 4 * n + inner, (n, kt)
            prev = b
        assert L.lsdsort_reduce_by_key_workspace_bytes(E.LSDSORT_MAX_KEYS + 1, kt) == 0
    for kt in (-1, 6, 9):
        assert L.lsdsort_reduce_by_key_workspace_bytes(1000, kt) == 0


# ---- the oracle ------------------------------------------------------------------------------------------------------------------
def _f32(*values):
    return np.array(values, dtype=np.float32).view(np.uint32)


def test_oracle_on_hand_written_rows():
    keys = np.array([5, 5, 7, 5, 5, 5, 9], dtype=np.uint32)
    vals = np.array([1, 2, 3, 4, 5, 6, 7], dtype=np.uint32)
    r = rd.oracle_reduce_runs(keys, vals, "uint32", "sum")
    assert r["keys"].tolist() == [5, 7, 5, 9] and r["vals"].tolist() == [3, 3, 15, 7] and r["counts"].tolist() == [2, 1, 3, 1]
    assert rd.oracle_reduce_runs(keys, vals, "uint32", "min")["vals"].tolist() == [1, 3, 4, 7]
    assert rd.oracle_reduce_runs(keys, vals, "uint32", "max")["vals"].tolist() == [2, 3, 6, 7]
    g = rd.oracle_reduce_by_key(keys, vals, "uint32", False, "uint32", "sum")
    assert g["keys"].tolist() == [5, 7, 9] and g["vals"].tolist() == [18, 3, 7] and g["counts"].tolist() == [5, 1, 1]
    d = rd.oracle_reduce_by_key(keys, vals, "uint32", True, "uint32", "max")
    assert d["keys"].tolist() == [9, 7, 5] and d["vals"].tolist() == [7, 3, 6]
    # int32 wrap: the sum is mod 2^32; min and max are signed for int32 and unsigned for uint32
    same = np.zeros(3, dtype=np.uint32)
    wrap = np.array([0x7FFFFFFF, 1, 0x80000000], dtype=np.uint32)            # INT_MAX, 1, INT_MIN
    assert rd.oracle_reduce_runs(same, wrap, "int32", "sum")["vals"].tolist() == [0]
    assert rd.oracle_reduce_runs(same[:2], wrap[:2], "int32", "sum")["vals"].tolist() == [0x80000000]
    assert rd.oracle_reduce_runs(same, wrap, "int32", "min")["vals"].tolist() == [0x80000000]
    assert rd.oracle_reduce_runs(same, wrap, "int32", "max")["vals"].tolist() == [0x7FFFFFFF]
    assert rd.oracle_reduce_runs(same, wrap, "uint32", "min")["vals"].tolist() == [1]
    assert rd.oracle_reduce_runs(same, wrap, "uint32", "max")["vals"].tolist() == [0x80000000]
    # a run of one -0.0, and a NaN payload alone, keep their bits under all three operations
    keys = np.array([1, 2, 3, 3], dtype=np.uint64)
    vals = np.array([0x80000000, 0x7FC00001, 0x3F800000, 0x40000000], dtype=np.uint32)
    for op in rd.OPS:
        got = rd.oracle_reduce_runs(keys, vals, "float32", op)["vals"]
        assert got[:2].tolist() == [0x80000000, 0x7FC00001], op
    assert rd.oracle_reduce_runs(keys, vals, "float32", "sum")["vals"][2] == _f32(3.0)[0]
    # +inf with -inf in one group: the sum is a NaN, min and max are the two
    keys = np.zeros(3, dtype=np.uint32)
    vals = _f32(np.inf, 1.0, -np.inf)
    assert np.isnan(rd.oracle_reduce_runs(keys, vals, "float32", "sum")["vals"].view(np.float32)[0])
    assert rd.oracle_reduce_runs(keys, vals, "float32", "min")["vals"].tolist() == [0xFF800000]
    assert rd.oracle_reduce_runs(keys, vals, "float32", "max")["vals"].tolist() == [0x7F800000]
    assert rd.oracle_reduce_runs(keys[:2], vals[:2], "float32", "sum")["vals"].tolist() == [0x7F800000]
    # the float total order: -NaN below -inf, +NaN above +inf, -0.0 below +0.0
    vals = np.array([0x00000000, 0x80000000, 0x7FC00000, 0xFFC00000, 0x7F800000, 0xFF800000], dtype=np.uint32)
    keys = np.zeros(6, dtype=np.uint32)
    assert rd.oracle_reduce_runs(keys, vals, "float32", "min")["vals"].tolist() == [0xFFC00000]
    assert rd.oracle_reduce_runs(keys, vals, "float32", "max")["vals"].tolist() == [0x7FC00000]
    assert rd.oracle_reduce_runs(keys[:2], vals[:2], "float32", "min")["vals"].tolist() == [0x80000000]
    assert rd.oracle_reduce_runs(keys[:2], vals[:2], "float32", "max")["vals"].tolist() == [0x00000000]
    assert np.array_equal(rd.from_sortable_f32(un.sortable(un.F32_SPECIALS, "float32")), un.F32_SPECIALS)
    # nothing
    empty = rd.oracle_reduce_runs(np.array([], dtype=np.uint32), np.array([], dtype=np.uint32), "int32", "sum")
    assert empty["keys"].size == empty["vals"].size == empty["counts"].size == 0


@pytest.mark.parametrize("w", [32, 64])
def test_oracle_against_numpy_on_the_families(w):
    for n in un.SIZES:
        fam = rd.key_families(n, w)
        assert set(fam) == set(un.families(n, w)) | {"runs_2T+3"}
        for name in fam:
            bits = rd.shuffled(n, w, name)
            keys, inverse, counts = np.unique(bits, return_inverse=True, return_counts=True)
            inverse = inverse.reshape(-1)
            v = rd.values(n, "small_ints", "int32")
            got = rd.oracle_reduce_by_key(bits, v, "uint%d" % w, False, "int32", "sum")
            want = np.zeros(keys.size, dtype=np.int64)
            np.add.at(want, inverse, v.view(np.int32).astype(np.int64))
            assert np.array_equal(got["keys"], keys) and np.array_equal(got["counts"], counts), (n, name)
            assert np.array_equal(got["vals"].view(np.int32), want), (n, name)
            for op, at, start in (("min", np.minimum.at, np.iinfo(np.int64).max), ("max", np.maximum.at, np.iinfo(np.int64).min)):
                want = np.full(keys.size, start, dtype=np.int64)
                at(want, inverse, v.view(np.int32).astype(np.int64))
                assert np.array_equal(rd.oracle_reduce_by_key(bits, v, "uint%d" % w, False, "int32", op)["vals"].view(np.int32), want), (n, name, op)
            # float sums of integer-valued values are exact, so they agree with the integer sums
            f = rd.values(n, "small_ints", "float32")
            assert np.abs(f.view(np.float32)).sum(dtype=np.float64) < 2 ** 24
            got = rd.oracle_reduce_by_key(bits, f, "uint%d" % w, False, "float32", "sum")["vals"].view(np.float32)
            want = np.zeros(keys.size, dtype=np.float64)
            np.add.at(want, inverse, f.view(np.float32).astype(np.float64))
            assert np.array_equal(got, want.astype(np.float32)), (n, name)
    # whole tiles lie inside a run
    starts = un.oracle_rle(rd.key_families(un.SIZES[-1], w)["runs_2T+3"])["starts"]
    assert starts.tolist() == [0, 2 * un.TILE + 3, 4 * un.TILE + 6]


def test_value_families():
    n = 5 * un.TILE + 7
    assert (rd.values(n, "ones", "float32") == 0x3F800000).all() and (rd.values(n, "ones", "int32") == 1).all()
    small = rd.values(n, "small_ints", "int32").view(np.int32)
    assert small.min() == -100 and small.max() == 100
    assert np.array_equal(rd.values(n, "small_ints", "float32").view(np.float32), small.astype(np.float32))
    wrap = rd.values(n, "wrap", "int32").view(np.int32).astype(np.int64)
    assert (np.abs(wrap) >= (1 << 31) - 100).all() and (wrap > 0).any() and (wrap < 0).any()
    assert set(rd.values(n, "specials", "float32").tolist()) == set(un.F32_SPECIALS.tolist())
    normal = rd.values(n, "normal", "float32").view(np.float32)
    assert np.isfinite(normal).all() and (normal > 0).any() and (normal < 0).any() and np.abs(normal).max() > 512 > 1 / 512 > np.abs(normal).min()
    for family, val_type in (("ones", "float32"), ("small_ints", "int32"), ("wrap", "int32"), ("specials", "float32"), ("normal", "float32")):
        assert not (rd.values(n, family, val_type) == un.SENT[32]).any()
    # the bound of any summation order: zero for a run of one, about L * u * sum|v| for a run of L
    s64, bound = rd.sum_bound(np.array([1, 2, 2, 2], dtype=np.uint32), _f32(1.5, 1.0, 2.0, 4.0))
    assert s64.tolist() == [1.5, 7.0] and bound[0] == 0 and bound[1] == 2 * rd.U / (1 - 2 * rd.U) * 7.0


# ---- the Python face ---------------------------------------------------------------------------------------------------------


def test_wrappers_check_their_tensors_before_the_library(no_library):
    import torch

    lsd = no_library
    calls = (lsd.GPUReduceRuns, lsd.GPUReduceByKey, lsd.reduce_by_key, lsd.reduce_consecutive)
    for dtype in (torch.int32, torch.float32, torch.int64, torch.float64):
        t = torch.zeros(8, dtype=dtype)
        for call in calls:
            with pytest.raises(TypeError):
                call(t, torch.zeros(8, dtype=torch.int32))                        # CPU tensors
    for call in calls:
        with pytest.raises(TypeError):
            call([3, 1, 2], [1, 1, 1])

    def fake(dtype, n=8):
        return torch.zeros(n, dtype=dtype).as_subclass(FakeCuda)

    keys, vals = fake(torch.int32), fake(torch.float32)
    for call in calls:
        with pytest.raises(TypeError):
            call(fake(torch.int16), vals)                                         # 16-bit keys are not served here
        with pytest.raises(TypeError):
            call(keys.view(2, 4), vals)                                           # 1-D only
        with pytest.raises(TypeError):
            call(keys, torch.zeros(8))                                            # the values on the CPU
        for dtype in (torch.int64, torch.float64, torch.float16, torch.int16):
            with pytest.raises(TypeError):
                call(keys, fake(dtype))                                           # 32-bit values only
        with pytest.raises(TypeError):
            call(keys, vals.view(2, 4))
        with pytest.raises(ValueError):
            call(keys, fake(torch.float32, 9))                                    # as long as the keys
        for op in ("mean", "prod", 0, None):
            with pytest.raises(ValueError):
                call(keys, vals, op=op)
    for dtype, key_type in ((torch.float32, "int32"), (torch.int32, "int64"), (torch.int64, "float32"), (torch.float64, "uint64")):
        with pytest.raises(TypeError):
            lsd.GPUReduceByKey(fake(dtype), vals, key_type=key_type)
    with pytest.raises(ValueError):
        lsd.GPUReduceByKey(keys, vals, key_type="int16")
    # the runs cannot go where the inputs are read; by key they may (the library is reached then: the fixture's AssertionError)
    with pytest.raises(ValueError):
        lsd.GPUReduceRuns(keys, vals, out_keys=keys)
    with pytest.raises(ValueError):
        lsd.GPUReduceRuns(keys, vals, out_vals=vals)
    with pytest.raises(AssertionError):
        lsd.GPUReduceByKey(keys, vals, out_keys=keys, out_vals=vals)
    for call in (lsd.GPUReduceRuns, lsd.GPUReduceByKey):
        with pytest.raises(ValueError):
            call(keys, vals, out_keys=fake(torch.int32, 9))
        with pytest.raises(ValueError):
            call(keys, vals, out_vals=fake(torch.float32, 7))
        with pytest.raises(TypeError):
            call(keys, vals, out_keys=fake(torch.float32))
        with pytest.raises(TypeError):
            call(keys, vals, out_vals=fake(torch.int32))                          # the aggregates have the values' dtype
        with pytest.raises(ValueError):
            call(keys, vals, counts=fake(torch.int32, 7))
        with pytest.raises(TypeError):
            call(keys, vals, counts=1)
        with pytest.raises(TypeError):
            call(keys, vals, counts=fake(torch.int64))
    for fn in calls:
        assert "-0.0" in fn.__doc__ and "NaN" in fn.__doc__, fn.__name__          # the float rules are stated


# ---- kernel resources ------------------------------------------------------------------------------------------------------------
def test_kernels_no_scratch_no_spill_and_recorded_resources():
    if hipcc() is None:
        pytest.skip("no hipcc on this machine")
    res = kernel_resources("reduce_by_key.hip")
    names = list(res)
    # the exact kernel set: count and emit per word and operation, one scan per operation, copy per word, one store
    sets = {"rbk_count_kernel": 6, "rbk_scan_kernel": 3, "rbk_emit_kernel": 6, "rbk_copy_kernel": 2, "run_store_kernel": 1}
    for must, times in sets.items():
        assert sum(must in name for name in names) == times, (must, names)
    assert len(names) == sum(sets.values()), names
    for op in ("AddWords", "AddFloats", "LeastWord"):
        assert sum(op in name for name in names) == 5, op
    for name, r in res.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r)
    want = json.load(open(GOLDEN))["reduce_by_key.hip"]
    assert sorted(res) == sorted(want), f"kernels gone: {sorted(set(want) - set(res))}, new: {sorted(set(res) - set(want))}"
    for name, w in want.items():
        assert res[name]["occupancy"] >= w["occupancy"], f"{name}: {res[name]['occupancy']} waves/SIMD, recorded {w['occupancy']}"
        assert res[name]["lds_bytes"] == w["lds_bytes"], f"{name}: {res[name]['lds_bytes']} B of static LDS, recorded {w['lds_bytes']}"


def test_the_unit_includes_four_files_only_and_has_no_inline_assembly():
    text = open(UNIT).read()
    assert re.findall(r"#include\s+(\S+)", text) == ['"../../include/lsdsort.h"', '"lsd_device.hpp"', '"lsd_host.hpp"', '"run_tiles.hpp"']
    unit = re.sub(r"//.*", "", text)
    header = open(un.HEADER).read()
    shared = re.sub(r"//.*", "", header)
    code = unit + shared   # what the unit compiles beside the three files it always had
    assert "asm" not in code
    # it reaches the sorts through their public device entries -- each call stands once, in the shared header -- waits for no other
    # workgroup, and clears with kernels only
    for call in ("lsdsort_keys_device(", "lsdsort_keys64_device(", "lsdsort_check_device(", "lsdsort_wide_check_device("):
        assert shared.count(call) == 1 and call not in unit, call
    for word in ("load_status", "store_status", "__hip_atomic", "hipMalloc", "hipMemset", "hipStreamSynchronize", "hipDeviceSynchronize",
                 "atomicAdd", "atomicMin", "atomicMax"):
        assert word not in code, word
    # the tile is unique.hip's, out of the header both include: tests/_unique.py's sizes are this unit's edges too
    k = {name: int(value) for name, value in re.findall(r"constexpr (?:int|uint32_t) (k\w+) = (\d+)u?;", header)}
    assert (k["kRunThreads"], k["kRunThreadKeys"], k["kRunScanThreads"], k["kRunMaxGrid"]) == (un.THREADS, un.THREAD_KEYS, un.SCAN_THREADS,
                                                                                               un.MAX_GRID)
    assert "kRunTile = kRunThreads * kRunThreadKeys;" in header and "kRunScanRound = 4 * kRunScanThreads;" in header
    assert not re.findall(r"constexpr[^;\n]*\bkRun\w+\s*=", text)                  # the unit defines none of them itself
    # the grid cap the unit has: the grid-stride copy kernel's, and none on the per-tile kernels
    caps = re.findall(r"grid_for\(([^,()]+),\s*(\w+)\s*,\s*([^()]+?)\)\)", text)
    assert [cap for _, _, cap in caps] == ["kRunMaxGrid"], caps
