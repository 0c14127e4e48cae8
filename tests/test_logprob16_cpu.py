"""CPU suite: log-probabilities and ranks of given tokens of 16-bit logit rows (logprob16.hip) -- its C-ABI surface
(lsdsort_logprob16_device and its workspace figure), its argument checks without a device, the Python face's own argument errors
(GPULogprob16, logprobs16_rows, top_logprobs16_rows), the float64 oracle of tests/_logprob16.py on hand-computed rows, and the
resources of every kernel of the unit from hipcc's own remarks."""
import json
import math
import os
import re

import numpy as np
import pytest

import _logprob16 as lg
import _temper16 as tm
import _topp16 as tp
from _faces import FakeCuda, lib as _lib, no_library
from _kernel_resources import hipcc, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "kernel_resources_logprob16.json")
U16, I16, F16, BF16 = range(4)
ENTRIES = ("lsdsort_logprob16_workspace_bytes", "lsdsort_logprob16_device")
NAMES = ("GPULogprob16", "logprob16_workspace_bytes", "logprobs16_rows", "top_logprobs16_rows")
MAX_SLOTS = 32


def test_header_ctypes_table_and_package_have_the_entries():
    import ctypes

    import lsdradixsort_amd as lsd
    from lsdradixsort_amd import _lib as binding

    header = open(os.path.join(ROOT, "include", "lsdsort.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"LSDSORT_API\s+[\w\s\*]+?\b" + name + r"\s*\(", text), name
        assert name in binding.SIGNATURES
        assert hasattr(_lib(), name)
    assert re.search(r"#define\s+LSDSORT_LOGPROB_MAX_SLOTS\s+32\b", text) and lsd.errors.LSDSORT_LOGPROB_MAX_SLOTS == MAX_SLOTS == lg.MAX_SLOTS
    entry = binding.SIGNATURES["lsdsort_logprob16_device"]
    assert entry[0] == binding.c_int and len(entry[1]) == 13 and entry[1][6] == binding.c_int
    assert all(entry[1][i] == binding.c_size for i in (1, 2, 4, 11)) and all(entry[1][i] == ctypes.c_void_p for i in (0, 3, 5, 7, 8, 9, 10, 12))
    assert binding.SIGNATURES[ENTRIES[0]] == (binding.c_size, [binding.c_size] * 3)
    doc = header[header.index("LOG-PROBABILITIES and RANKS"):header.index("lsdsort_logprob16_workspace_bytes(size_t")]
    for word in ("graph", "DETERMINISTIC", "in any batch", "lsdsort_sample16_ex_device", "THE BITS", "PADDING", "2^-11", "2^-22", "strictly greater",
                 "READ ONLY", "no fault bit", "-ln(ties)", "Every word", "GREEDY"):   # the contract's points
        assert word in doc, word
    for name in NAMES:
        assert callable(getattr(lsd, name)) and name in lsd.api.__all__, name
    init = open(os.path.join(ROOT, "lsdradixsort_amd", "__init__.py")).read()
    assert "GPULogprob16, logprob16_workspace_bytes, logprobs16_rows, top_logprobs16_rows," in init
    makefile = open(os.path.join(ROOT, "lsdradixsort_amd", "csrc", "Makefile")).read()
    assert "logprob16" in re.search(r"^NAMES\s*:=(.*)$", makefile, flags=re.M).group(1).split()
    assert "logprob16" not in open(os.path.join(ROOT, "include", "lsdsort.hpp")).read()     # no wrapper in the C++ face
    assert "lsdsort_logprob16_device" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_argument_checks_in_entry_order():
    from lsdradixsort_amd import errors as E

    L = _lib()
    rows, cols, slots = 10, 1000, 5
    fake = 1 << 20   # never dereferenced: every call below returns before a device is touched
    BIG = E.LSDSORT_MAX_KEYS

    def call(keys=fake, ids=fake + (1 << 12), T=fake + (1 << 13), lp=fake + (1 << 16), rank=fake + (1 << 17), lse=fake + (1 << 18), w=fake, wb=None,
             rows=rows, cols=cols, slots=slots, kt=BF16):
        if wb is None:
            wb = L.lsdsort_logprob16_workspace_bytes(rows, cols, slots)
        return L.lsdsort_logprob16_device(keys, rows, cols, ids, slots, T, kt, lp, rank, lse, w, wb, None)

    # 1. key type, before everything else: float16 and bfloat16 only
    for kt in (-1, U16, I16, 4, 5, 100):
        assert call(kt=kt, rows=BIG + 1, slots=0, keys=None, ids=None, lp=None, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG, kt
        assert call(kt=kt, rows=0, wb=0) == E.LSDSORT_ERR_INVALID_ARG, kt
        assert call(kt=kt) == E.LSDSORT_ERR_INVALID_ARG, kt
    # 2. slots, before the sizes and the empty call
    for bad in (0, MAX_SLOTS + 1, 64, 1 << 40):
        assert call(slots=bad, rows=BIG + 1, keys=None, ids=None, lp=None, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG, bad
        assert call(slots=bad, rows=0, wb=0) == E.LSDSORT_ERR_INVALID_ARG, bad
        assert call(slots=bad, wb=1 << 20) == E.LSDSORT_ERR_INVALID_ARG, bad
    # 3. sizes, before the empty call, the pointers and the workspace
    assert call(rows=BIG + 1, cols=1, keys=None, ids=None, lp=None, w=None, wb=0) == E.LSDSORT_ERR_TOO_LARGE
    assert call(rows=1 << 15, cols=1 << 15, keys=None, ids=fake + 1, lp=None, w=None, wb=0) == E.LSDSORT_ERR_TOO_LARGE
    assert call(rows=2, cols=BIG // 2 + 1, keys=fake + 1, lp=fake + 1, w=None, wb=0) == E.LSDSORT_ERR_TOO_LARGE
    # 4. nothing to do
    for kt in (F16, BF16):
        for n in (1, MAX_SLOTS):
            assert call(kt=kt, slots=n, rows=0, keys=None, ids=None, T=None, lp=None, rank=None, lse=None, w=None, wb=0) == E.LSDSORT_OK
            assert call(kt=kt, slots=n, cols=0, keys=fake + 1, ids=fake + 2, T=fake + 1, lp=fake + 3, rank=fake + 1, lse=fake + 2, w=None, wb=0) == E.LSDSORT_OK
    # 5. NULL or odd d_keys, before the ids and the outputs
    assert call(keys=None, ids=None, lp=None, w=None) == E.LSDSORT_ERR_INVALID_ARG
    for off in (1, 3, 7, 15):
        assert call(keys=fake + off, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG, off
    # 6. NULL or misaligned d_ids or d_logprob
    assert call(ids=None, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG
    assert call(lp=None, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG
    for off in (1, 2, 3, 6, 13):
        assert call(ids=fake + off, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG, off
        assert call(lp=fake + off, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG, off
    # 7. an optional array that is given and misaligned; NULL is "none" / "T = 1" and passes on to the workspace check: every NULL
    # combination of the three
    for off in (1, 2, 3, 6, 13):
        assert call(rank=fake + off, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG, off
        assert call(lse=fake + off, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG, off
        assert call(T=fake + off, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG, off
        assert call(rank=None, lse=None, T=fake + off, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG, off
    combos = [dict(zip(("T", "rank", "lse"), (fake + (1 << (13 + i)) if c >> i & 1 else None for i in range(3)))) for c in range(8)]
    for given in combos:
        assert call(w=None, **given) == E.LSDSORT_ERR_WORKSPACE, given
    # 8. workspace: exactly lsdsort_logprob16_workspace_bytes(rows, cols, slots)
    assert call(w=fake + 128) == E.LSDSORT_ERR_WORKSPACE
    need = L.lsdsort_logprob16_workspace_bytes(rows, cols, slots)
    assert need > 0 and call(wb=need - 1) == E.LSDSORT_ERR_WORKSPACE
    for src in (2, 6, 14):
        assert call(keys=fake + src, w=None) == E.LSDSORT_ERR_WORKSPACE, src               # any 2-byte alignment of the keys
    assert call(rows=3, cols=70001, slots=21, wb=L.lsdsort_logprob16_workspace_bytes(3, 70001, 21) - 1) == E.LSDSORT_ERR_WORKSPACE
    # 9. the device
    import torch

    if not torch.cuda.is_available():
        for kt in (F16, BF16):
            for given in combos:
                assert call(kt=kt, **given) == E.LSDSORT_ERR_NO_DEVICE, given
            assert call(kt=kt, rows=3, cols=70001, slots=MAX_SLOTS) == E.LSDSORT_ERR_NO_DEVICE
        assert call(keys=fake + 14, ids=fake + 12, lp=fake + 4, cols=1001, slots=1) == E.LSDSORT_ERR_NO_DEVICE


def figure(rows, cols, slots):
    """the control block, 4 B per row, and for rows above 16384 keys 8 B per chunk of the chunk cap min(2048, ceil(cols / 16384)) and
    4 B per slot; every array rounded up to 256 bytes"""
    up = lambda x: -(-x // 256) * 256
    long_rows = cols > 16384
    sums = rows * min(2048, -(-cols // 16384)) * 8 if long_rows else 0
    return up(up(up(256 + rows * 4) + sums) + (rows * slots * 4 if long_rows else 0))


PINNED = {(1, 1, 1): 512, (10, 1000, 5): 512, (64, 1000, 32): 512, (65, 16384, 32): 768, (3, 16385, 1): 1024, (3, 70001, 21): 1024,
          (128, 128256, 21): 19712, (8192, 128256, 1): 590080, (4096, 131072, 32): 803072}


def test_workspace_figure():
    from lsdradixsort_amd import errors as E

    L = _lib()
    BIG = E.LSDSORT_MAX_KEYS
    f = L.lsdsort_logprob16_workspace_bytes
    ladder = [1, 2, 7, 8, 9, 1000, 1024, 1025, 16384, 16385, 65536, 131073, (1 << 20) + 13, 1 << 24, BIG]
    row_ladder = [1, 2, 3, 64, 65, 513, 4096, 4097, 1 << 15, 1 << 20, BIG]
    slot_ladder = [1, 2, 21, MAX_SLOTS]
    seen = 0
    for rows in row_ladder:
        for slots in slot_ladder:
            prev = 0
            for cols in ladder:
                if rows * cols > BIG:
                    assert f(rows, cols, slots) == 0, (rows, cols, slots)
                    continue
                b = f(rows, cols, slots)
                assert b > 0 and b % 256 == 0 and b >= prev, (rows, cols, slots, b, prev)  # monotonic in cols
                assert b == figure(rows, cols, slots), (rows, cols, slots, b, figure(rows, cols, slots))
                assert b <= 1024 + rows * (8 + 4 * slots) + rows * cols // 1024, (rows, cols, slots, b)   # O(rows * slots), never O(rows * cols)
                prev = b
                seen += 1
    assert seen > 240
    for cols in ladder:                                                                   # monotonic in rows and in slots
        for slots in slot_ladder:
            prev = 0
            for rows in row_ladder:
                if rows * cols <= BIG:
                    b = f(rows, cols, slots)
                    assert b >= prev, (rows, cols, slots)
                    prev = b
        for rows in row_ladder:
            if rows * cols <= BIG:
                sizes = [f(rows, cols, slots) for slots in range(1, MAX_SLOTS + 1)]
                assert sizes == sorted(sizes), (rows, cols)
    assert f(3, 70001, 32) > f(3, 70001, 1) > f(3, 16384, 1) and f(2, 1 << 24, 1) > f(1, 1 << 24, 1)
    for slots in (0, MAX_SLOTS + 1, 64, 1 << 40):                                         # a bad `slots`
        assert f(10, 1000, slots) == 0 and f(3, 70001, slots) == 0 and f(0, 0, slots) == 0, slots
    assert f(0, 1000, 1) % 256 == 0 and f(10, 0, 1) % 256 == 0
    assert f(BIG + 1, 1, 1) == 0 and f(1, BIG + 1, 1) == 0 and f(BIG + 1, 0, 1) == 0
    assert f(2, BIG // 2 + 1, 1) == 0 and f(1 << 15, 1 << 15, 1) == 0
    assert f(1, BIG, 32) > 0 and f(BIG, 1, 32) > 0
    for (rows, cols, slots), want in PINNED.items():
        assert f(rows, cols, slots) == want == figure(rows, cols, slots), (rows, cols, slots, f(rows, cols, slots), want)
    # the figure has no argument for the optional outputs: one workspace serves a call with and without ranks and the lse
    assert L.lsdsort_logprob16_workspace_bytes.argtypes == [L.lsdsort_logprob16_workspace_bytes.argtypes[0]] * 3


def test_wrappers_check_their_arguments_before_the_library(no_library):
    import torch

    lsd = no_library

    def fake(dtype, shape=(2, 4)):
        return torch.zeros(shape, dtype=dtype).as_subclass(FakeCuda)

    ids2 = fake(torch.int32, (2, 3))
    for dtype in (torch.float16, torch.bfloat16):
        ok = str(dtype).replace("torch.", "")
        with pytest.raises(TypeError):
            lsd.GPULogprob16(torch.zeros((2, 4), dtype=dtype), ids2, key_type=ok)        # a CPU tensor
        with pytest.raises(TypeError):
            lsd.logprobs16_rows(torch.zeros((2, 4), dtype=dtype), ids2)
        with pytest.raises(TypeError):
            lsd.top_logprobs16_rows(torch.zeros((2, 4), dtype=dtype), 2)
        other = "float16" if ok == "bfloat16" else "bfloat16"
        with pytest.raises(TypeError):
            lsd.GPULogprob16(fake(dtype), ids2, key_type=other)                          # a key type that does not fit the dtype
        for key_type in ("int16", "uint16", "float32", "half", ""):
            with pytest.raises(ValueError):
                lsd.GPULogprob16(fake(dtype), ids2, key_type=key_type)                   # a key type this entry does not have
        with pytest.raises(TypeError):
            lsd.GPULogprob16(fake(dtype, (2, 2, 2)), ids2, key_type=ok)                  # 1-D or 2-D only
        for bad in (torch.zeros((2, 3), dtype=torch.int32), fake(torch.int64, (2, 3)), fake(torch.float32, (2, 3)), [[0, 1], [2, 3]], 1, None,
                    fake(torch.int32, (2, 6))[:, ::2], fake(torch.int32, (2, 1, 3))):
            with pytest.raises(TypeError):
                lsd.GPULogprob16(fake(dtype), bad, key_type=ok)                          # d_ids: a contiguous 1-D or 2-D int32 CUDA tensor
        for shape in ((3, 3), (1, 3), (3,), (2, 0), (2, MAX_SLOTS + 1)):
            with pytest.raises(ValueError):
                lsd.GPULogprob16(fake(dtype), fake(torch.int32, shape), key_type=ok)     # one row of 1 .. 32 ids per row
        for T in (fake(torch.float32, (3,)), fake(torch.float64, (2,)), torch.zeros(2, dtype=torch.float32), 0.7):
            with pytest.raises((TypeError, ValueError)):
                lsd.GPULogprob16(fake(dtype), ids2, key_type=ok, d_temperature=T)
        for out in (fake(torch.float32, (2, 4)), fake(torch.float64, (2, 3)), torch.zeros((2, 3), dtype=torch.float32)):
            with pytest.raises((TypeError, ValueError)):
                lsd.GPULogprob16(fake(dtype), ids2, key_type=ok, out=out)
        for ranks in (fake(torch.int32, (2, 4)), fake(torch.int64, (2, 3)), torch.zeros((2, 3), dtype=torch.int32), 1, "yes", None):
            with pytest.raises((TypeError, ValueError)):
                lsd.GPULogprob16(fake(dtype), ids2, key_type=ok, ranks=ranks)
        for total in (fake(torch.float32, (3,)), fake(torch.float64, (2,)), torch.zeros(2, dtype=torch.float32), 1, "yes", None):
            with pytest.raises((TypeError, ValueError)):
                lsd.GPULogprob16(fake(dtype), ids2, key_type=ok, lse=total)
        x = fake(dtype, (3, 2, 4))
        for ids in (fake(torch.int16, (3, 2)), fake(torch.float32, (3, 2)), [[0, 1]] * 3, torch.zeros((3, 2), dtype=torch.int64), None):
            with pytest.raises(TypeError, match="^ids: "):
                lsd.logprobs16_rows(x, ids)
        for shape in ((3,), (2, 3), (3, 2, 4, 1), (6,), (3, 3, 5)):
            with pytest.raises(ValueError, match="^ids: "):
                lsd.logprobs16_rows(x, fake(torch.int64, shape))
        with pytest.raises(TypeError, match="^temperature: "):
            lsd.logprobs16_rows(x, fake(torch.int64, (3, 2)), temperature="0.7")
        with pytest.raises(ValueError, match="^temperature: "):
            lsd.logprobs16_rows(x, fake(torch.int64, (3, 2)), temperature=[0.7] * 5)
        with pytest.raises(TypeError):
            lsd.logprobs16_rows(fake(dtype, ()), fake(torch.int64, ()))                  # at least one dimension
        for n in (0, -1, 2.0, True, "3", None):
            with pytest.raises(ValueError, match="^n: "):
                lsd.top_logprobs16_rows(x, n)
        # empty shapes: nothing to do, the library is not reached
        for shape, id_shape in (((0, 4), (0, 3)), ((3, 0), (3, 2)), ((2, 0, 5), (2, 0)), ((2, 3, 5), (2, 3, 0))):
            got, rank, total = lsd.logprobs16_rows(fake(dtype, shape), fake(torch.int64, id_shape), return_ranks=True, return_lse=True)
            assert got.shape == rank.shape == id_shape and got.dtype == total.dtype == torch.float32 and rank.dtype == torch.int64
            assert total.shape == shape[:-1] and torch.isnan(got).all() and (rank == -1).all() and torch.isnan(total).all()
            assert lsd.logprobs16_rows(fake(dtype, shape), fake(torch.int32, id_shape)).shape == id_shape
    for dtype in (torch.int16, torch.float32, torch.int32):
        with pytest.raises(TypeError):
            lsd.logprobs16_rows(fake(dtype), fake(torch.int64, (2,)))
        with pytest.raises(TypeError):
            lsd.GPULogprob16(fake(dtype), ids2, key_type="bfloat16")
        with pytest.raises(TypeError):
            lsd.top_logprobs16_rows(fake(dtype), 2)


# ---- the oracle itself -----------------------------------------------------------------------------------------------------------
def _row(values, key_type="bfloat16"):
    return tp.bits_of_values(np.array(values, dtype=np.float32), key_type)


def _oracle(row, ids, key_type, T=1.0):
    o = lg.RowOracle(row, key_type, T)
    return o.slots(np.array(ids)) + o.lse()


@pytest.mark.parametrize("key_type", lg.TYPES)
def test_the_oracle_on_hand_computed_rows(key_type):
    pinf, ninf = tp.POS_INF[key_type], tp.NEG_INF[key_type]
    one = _row([1.0], key_type)[0]
    # [0, -ln 2, -ln 4] has the masses 1, 1/2, 1/4 of 7/4 up to the 16-bit roundings of the logarithms (below 1 %)
    row = _row([0.0, -math.log(2), -math.log(4)], key_type)
    lp, tol, rank, lse, lse_tol = _oracle(row, [0, 1, 2, 2, 0], key_type)
    assert np.allclose(lp, np.log(np.array([4, 2, 1, 1, 4]) / 7), atol=0.02) and rank.tolist() == [0, 1, 2, 2, 0] and abs(lse - math.log(1.75)) < 0.02
    assert tol[0] == 2.0 ** -11 and tol[2] == 2.0 ** -11 + 2.0 ** -22 * abs(lp[2] - lp[0]) and lse_tol == 2.0 ** -11
    lp2, _, rank2, lse2, _ = _oracle(row, [0, 1, 2], key_type, T=0.5)                     # T = 1/2 squares the masses: 1, 1/4, 1/16 of 21/16
    assert np.allclose(lp2, np.log(np.array([16, 4, 1]) / 21), atol=0.04) and rank2.tolist() == [0, 1, 2] and abs(lse2 - math.log(21 / 16)) < 0.04
    # the fast oracle against _temper16.logprob64 / logprob_tol, slot by slot
    mixed = np.concatenate([_row([3.0, -2.5, 0.0, 40.0, -60.0, 1.5, 1.5], key_type), np.array([ninf, 0x7FFF, 0x8000], dtype=np.uint16)])
    for T in lg.T_CYCLE:
        lp, tol, rank, _, _ = _oracle(mixed, list(range(mixed.size)), key_type, T)
        for i in range(mixed.size):
            if i == 8:
                assert np.isnan(lp[i]) and rank[i] == -1                                  # a NaN key: NaN whatever T (logprob64 does not know it)
                continue
            assert lg.close(lp[i], lg.logprob64(mixed, i, key_type, T), 1e-12), (T, i, lp[i])
            assert tol[i] == lg.logprob_tol(mixed, i, key_type, T) or np.isinf(lp[i]), (T, i)
        assert rank.tolist() == [1, 6, 4, 0, 7, 2, 2, 8, -1, 4]                           # -0.0 ties with +0.0; the NaN counts for nothing
    # a row of one key: logprob 0, rank 0, lse = x / T; greedy: lse NaN
    for T, want_lse in ((1.0, -5.0), (0.5, -10.0), (0.0, float("nan"))):
        lp, _, rank, lse, _ = _oracle(_row([-5.0], key_type), [0], key_type, T)
        assert lp.tolist() == [0.0] and rank.tolist() == [0] and lg.close(lse, want_lse, 0.0)
    # a row of -inf: uniform over its keys, every rank 0, lse -inf
    lp, _, rank, lse, _ = _oracle(np.full(5, ninf, dtype=np.uint16), [0, 4], key_type)
    assert lp.tolist() == [-math.log(5)] * 2 and rank.tolist() == [0, 0] and lse == float("-inf")
    # a row with +inf: the infinities share the mass, a number under them has -inf, -inf has -inf; lse +inf
    row = np.array([_row([3.0], key_type)[0], pinf, 0x7FFF, pinf, ninf], dtype=np.uint16)
    lp, _, rank, lse, _ = _oracle(row, [1, 3, 0, 4, 2], key_type, T=0.7)
    assert lp[:4].tolist() == [-math.log(2), -math.log(2), float("-inf"), float("-inf")] and np.isnan(lp[4])
    assert rank.tolist() == [0, 0, 2, 3, -1] and lse == float("inf")
    # +-0.0 tie: equal values, equal logprobs, equal ranks
    row = np.array([0x0000, 0x8000, one, 0x8000, _row([-1.0], key_type)[0]], dtype=np.uint16)
    lp, _, rank, _, _ = _oracle(row, [0, 1, 3, 2, 4], key_type)
    assert lp[0] == lp[1] == lp[2] and rank.tolist() == [1, 1, 1, 0, 4]
    # a NaN id target, and the padding ids -1, cols and INT32_MIN: NaN and -1, and no other slot is disturbed
    row = np.array([one, 0x7FFF, ninf + 1, one], dtype=np.uint16)
    lp, _, rank, lse, _ = _oracle(row, [1, 2, -1, 4, lg.INT32_MIN, 0, 3, 2 ** 31 - 1], key_type)
    assert np.isnan(lp[[0, 1, 2, 3, 4, 7]]).all() and lp[5] == lp[6] == -math.log(2) and rank.tolist() == [-1, -1, -1, -1, -1, 0, 0, -1]
    assert abs(lse - (1.0 + math.log(2))) < 1e-12
    assert set(lg.padding_ids(4)) >= {-1, 4, lg.INT32_MIN}
    # a row of NaNs: NaN in every slot, rank -1, lse NaN
    lp, _, rank, lse, _ = _oracle(np.array([0xFFFF, 0x7FFF, ninf + 1, pinf + 1], dtype=np.uint16), [0, 3, -1], key_type)
    assert np.isnan(lp).all() and rank.tolist() == [-1, -1, -1] and math.isnan(lse)
    # greedy rows with 1 and 3 ties: -ln(ties) on the maximum's duplicates, -inf elsewhere, lse NaN; the ranks do not know T
    for ties in (1, 3):
        row, at = tm.greedy_rows(50, key_type, ties, seed=ties)
        other = int(np.setdiff1d(np.arange(50), at)[0])
        for T in (0.0, -1.0, float("nan"), 2.0 ** -149):
            lp, _, rank, lse, _ = _oracle(row, [int(at[0]), int(at[-1]), other], key_type, T)
            assert lp[0] == lp[1] == -math.log(ties) and lp[2] == float("-inf") and math.isnan(lse), (ties, T)
            assert rank[:2].tolist() == [0, 0] and rank[2] >= ties
        assert np.array_equal(_oracle(row, list(range(50)), key_type, 0.0)[2], _oracle(row, list(range(50)), key_type, 1.3)[2])
    # check_rows: the oracle's own answer passes; a logprob off by more than its tolerance, a rank off by one, a finite lse for a greedy
    # row and a finite logprob where -inf is due do not
    keys = np.stack([_row([1.0, 0.0, float("-inf"), -3.0], key_type)] * 2)
    ids = np.array([[0, 3, 2], [1, -1, 0]], dtype=np.int32)
    T = np.array([0.7, 0.0], dtype=np.float32)
    want = [_oracle(keys[r], ids[r], key_type, T[r]) for r in range(2)]
    lp = np.stack([w[0] for w in want]).astype(np.float32)
    rank = np.stack([w[2] for w in want]).astype(np.int32)
    lse = np.array([w[3] for w in want], dtype=np.float32)
    lg.check_rows(lp, rank, lse, keys, ids, T, key_type)
    lg.check_rows(lp, None, None, keys, ids, T, key_type)
    for r, s, value in ((0, 1, lp[0, 1] + 1.2 * want[0][1][1]), (0, 2, -1e30), (1, 1, 0.0), (1, 0, 0.0), (0, 0, float("nan"))):
        bad = lp.copy()
        bad[r, s] = value
        with pytest.raises(AssertionError):
            lg.check_rows(bad, rank, lse, keys, ids, T, key_type)
    bad = rank.copy()
    bad[0, 1] += 1
    with pytest.raises(AssertionError):
        lg.check_rows(lp, bad, lse, keys, ids, T, key_type)
    for r, value in ((1, 1.0), (0, lse[0] + 2 * want[0][4]), (0, float("nan"))):
        bad = lse.copy()
        bad[r] = value
        with pytest.raises(AssertionError):
            lg.check_rows(lp, rank, bad, keys, ids, T, key_type)


@pytest.mark.parametrize("key_type", lg.TYPES)
def test_mixed_ids_hold_every_kind(key_type):
    """over the rows of one case: position 0, cols - 1, the argmax, a NaN's and a -inf's position, every padding id, at every slot count"""
    keys = tp.special_rows(513, key_type, seed=3)
    v = tp.values64(keys, key_type)
    for slots in lg.SLOTS:
        seen = set()
        for seed in range(24 // slots + 2):
            ids = lg.mixed_ids(keys, slots, key_type, seed)
            assert ids.shape == (keys.shape[0], slots) and ids.dtype == np.int32
            for r in range(keys.shape[0]):
                for i in ids[r].tolist():
                    kind = "pad" if not 0 <= i < 513 else "nan" if np.isnan(v[r, i]) else "-inf" if np.isneginf(v[r, i]) else "number"
                    seen |= {kind, "first" if i == 0 else "last" if i == 512 else None, i if i in lg.padding_ids(513) else None}
        assert seen >= {"pad", "nan", "-inf", "number", "first", "last"} | (set(lg.padding_ids(513)) if slots > 2 else set()), (slots, seen)


# ---- kernel resources ------------------------------------------------------------------------------------------------------------
def test_kernels_no_scratch_no_spill_and_recorded_resources():
    if hipcc() is None:
        pytest.skip("no hipcc on this machine")
    res = kernel_resources("logprob16.hip")
    names = list(res)
    once = ("logprob16_clear_kernel", "logprob16_best_kernel", "logprob16_sum_kernel", "logprob16_finish_kernel")
    for must in once:
        assert sum(must in name for name in names) == 1, (must, names)
    assert sum("logprob16_short_kernel" in name for name in names) == 2, names             # wavefront / workgroup
    assert len(names) == len(once) + 2, names
    for name, r in res.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r)
    want = json.load(open(GOLDEN))["logprob16.hip"]
    assert sorted(res) == sorted(want), f"kernels gone: {sorted(set(want) - set(res))}, new: {sorted(set(res) - set(want))}"
    for name, w in want.items():
        assert res[name]["occupancy"] >= w["occupancy"], f"{name}: {res[name]['occupancy']} waves/SIMD, recorded {w['occupancy']}"
        assert res[name]["lds_bytes"] == w["lds_bytes"], f"{name}: {res[name]['lds_bytes']} B of static LDS, recorded {w['lds_bytes']}"


def test_the_unit_includes_the_shared_headers_only_and_has_no_inline_assembly():
    csrc = os.path.join(ROOT, "lsdradixsort_amd", "csrc")
    text = open(os.path.join(csrc, "logprob16.hip")).read()
    assert set(re.findall(r'#include "([^"]+)"', text)) == {"../../include/lsdsort.h", "keys16_map.hpp", "lsd_device.hpp", "lsd_host.hpp",
                                                             "mass_rows16.hpp", "radix_select.hpp"}
    code = re.sub(r"//.*", "", text)
    assert "asm" not in code
    for name in ("load_tile", "load_head", "locate_tile", "store_tile", "store_head", "same_phase", "StopNever16", "kNoKey", "kHeadBit",
                 "kNoChunk"):                                                              # select_tiles16.hpp's, not this unit's
        assert not re.search(r"\b" + name + r"\b", code), name
    # the mass functions live once, in keys16_map.hpp: this unit calls them and defines none
    for name in ("kMassShift =", "struct Values16", "bool is_number(", "float value_of(", "uint64_t mass_of(", "uint64_t mass_of_key(",
                 "float scale_of(", "float log_factor("):
        assert code.count(name) == 0, name
    for call in ("mass_of_key(", "value_of(", "is_number(", "scale_of(", "log_factor(", "chunk_cap_for(", "grid_for("):
        assert call in code, call
    assert "exp2" not in code and "expf" not in code                                       # no mass arithmetic of its own
    # the launches the GPU suite runs past their grid caps
    launch = re.compile(r"(\w+_kernel(?:<[^<>]*>)?)[>,(\s]*dim3\(grid_for\(([^,()]+),\s*(\w+)\s*,\s*(\w+)\s*\)\)")
    found = {k: (items.strip(), a, b) for k, items, a, b in launch.findall(text)}
    assert found["logprob16_short_kernel<1>"] == ("rows", "8", "16384") and found["logprob16_short_kernel<16>"] == ("rows", "1", "4096")
