"""CPU suite: the per-row-k entries for 16-bit keys (kth16_rowk.hip) -- their C-ABI surface (lsdsort_kth16_perrow_device,
lsdsort_topk16_filter_device and the two workspace figures), their argument checks without a device, the Python face's own argument
errors (GPUKth16PerRow, GPUTopK16Filter, topk16_filter_rows) and host conversions, the resources of every kernel of the unit from
hipcc's own remarks, and the launch lines of its four capped row loops."""
import json
import os
import re

import numpy as np
import pytest

import _row_rounds as rr
import _rowk16 as rk
from _faces import FakeCuda, lib as _lib, no_library
from _kernel_resources import hipcc, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "kernel_resources_kth16_rowk.json")
U16, I16, F16, BF16 = range(4)
ENTRIES = ("lsdsort_kth16_perrow_workspace_bytes", "lsdsort_kth16_perrow_device", "lsdsort_topk16_filter_workspace_bytes",
           "lsdsort_topk16_filter_device")
NAMES = ("GPUKth16PerRow", "kth16_perrow_workspace_bytes", "GPUTopK16Filter", "topk16_filter_workspace_bytes", "topk16_filter_rows")


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
    # the single-rank signature with the device array where it has the rank
    one, per = binding.SIGNATURES["lsdsort_kth16_device"], binding.SIGNATURES["lsdsort_kth16_perrow_device"]
    assert per[0] == one[0] and per[1][:3] == one[1][:3] and per[1][4:] == one[1][4:] and per[1][3] == binding.c_u32p
    flt = binding.SIGNATURES["lsdsort_topk16_filter_device"]
    assert flt[0] == binding.c_int and len(flt[1]) == 11 and flt[1][6] == ctypes.c_uint16
    for name in ENTRIES[::2]:
        assert binding.SIGNATURES[name] == (binding.c_size, [binding.c_size] * 2)
    assert "graph" in header[header.index("d_ranks[r]"):header.index("lsdsort_kth16_perrow_workspace_bytes(size_t")]   # the point of the entry
    for name in NAMES:
        assert callable(getattr(lsd, name)) and name in lsd.api.__all__, name
    makefile = open(os.path.join(ROOT, "lsdradixsort_amd", "csrc", "Makefile")).read()
    assert "kth16_rowk" in re.search(r"^NAMES\s*:=(.*)$", makefile, flags=re.M).group(1).split()
    # no wrapper in the C++ face: its guard demands a call from the existing harnesses
    assert "perrow" not in open(os.path.join(ROOT, "include", "lsdsort.hpp")).read()


def test_perrow_argument_checks_in_entry_order():
    from lsdradixsort_amd import errors as E

    L = _lib()
    rows, cols = 10, 1000
    fake = 1 << 20   # never dereferenced: every call below returns before a device is touched
    BIG = E.LSDSORT_MAX_KEYS

    def call(keys=fake, ranks=fake, out=fake, idx=fake, w=fake, wb=None, rows=rows, cols=cols, kt=BF16, largest=0):
        if wb is None:
            wb = L.lsdsort_kth16_perrow_workspace_bytes(rows, cols)
        return L.lsdsort_kth16_perrow_device(keys, rows, cols, ranks, kt, largest, out, idx, w, wb, None)

    # 1. key type, before everything else
    for kt in (-1, 4, 5, 100):
        assert call(kt=kt, rows=BIG + 1, keys=None, ranks=None, out=None, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG, kt
        assert call(kt=kt, rows=0, wb=0) == E.LSDSORT_ERR_INVALID_ARG, kt
    # 2. size, before the empty call, the pointers and the workspace
    assert call(rows=BIG + 1, cols=1, keys=None, ranks=None, out=None, w=None, wb=0) == E.LSDSORT_ERR_TOO_LARGE
    assert call(rows=1 << 15, cols=1 << 15, keys=None, ranks=fake + 1, out=None, w=None, wb=0) == E.LSDSORT_ERR_TOO_LARGE
    assert call(rows=2, cols=BIG // 2 + 1, keys=fake + 1, out=None, w=None, wb=0) == E.LSDSORT_ERR_TOO_LARGE
    # 3. nothing to do, before the pointers and the workspace
    for kt in (U16, I16, F16, BF16):
        for largest in (0, 1):
            assert call(kt=kt, largest=largest, rows=0, keys=None, ranks=None, out=None, idx=None, w=None, wb=0) == E.LSDSORT_OK
            assert call(kt=kt, largest=largest, cols=0, keys=fake + 1, ranks=fake + 2, out=fake + 1, w=None, wb=0) == E.LSDSORT_OK
    # 4. the keys and the values, before the ranks and the workspace: NULL, or odd
    assert call(keys=None, ranks=None, w=None) == E.LSDSORT_ERR_INVALID_ARG
    assert call(out=None, w=None) == E.LSDSORT_ERR_INVALID_ARG
    for off in (1, 3, 7, 15):
        assert call(keys=fake + off, w=None) == E.LSDSORT_ERR_INVALID_ARG, off
        assert call(out=fake + off, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG, off
    # 5. the ranks, after the keys and before the workspace: NULL, or not 4-byte aligned.  Their VALUES are the device's to check.
    assert call(ranks=None, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG
    for off in (1, 2, 3, 6, 13):
        assert call(ranks=fake + off, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG, off
    # 6. workspace: exactly lsdsort_kth16_perrow_workspace_bytes(rows, cols)
    assert call(w=None) == E.LSDSORT_ERR_WORKSPACE
    assert call(w=fake + 128) == E.LSDSORT_ERR_WORKSPACE                                # misaligned
    need = L.lsdsort_kth16_perrow_workspace_bytes(rows, cols)
    assert need > 0 and call(wb=need - 1) == E.LSDSORT_ERR_WORKSPACE
    assert call(idx=None, wb=need - 1) == E.LSDSORT_ERR_WORKSPACE                       # one figure, with or without indices
    for off in (2, 4, 6, 14):
        assert call(keys=fake + off, out=fake + 16 - off, ranks=fake + 4, w=None) == E.LSDSORT_ERR_WORKSPACE, off
    assert call(rows=3, cols=70001, wb=L.lsdsort_kth16_perrow_workspace_bytes(3, 70001) - 1) == E.LSDSORT_ERR_WORKSPACE
    # 7. without a gfx950 device the last check answers; with one, this test does not get here on bogus pointers
    import torch

    if not torch.cuda.is_available():
        for kt in (U16, I16, F16, BF16):
            for largest in (0, 1):
                for idx in (None, fake):
                    assert call(kt=kt, largest=largest, idx=idx) == E.LSDSORT_ERR_NO_DEVICE
                    assert call(kt=kt, largest=largest, idx=idx, rows=3, cols=70001) == E.LSDSORT_ERR_NO_DEVICE   # the long tier
        assert call(keys=fake + 14, out=fake + 6, ranks=fake + 12, cols=1001) == E.LSDSORT_ERR_NO_DEVICE


def test_filter_argument_checks_in_entry_order():
    from lsdradixsort_amd import errors as E

    L = _lib()
    rows, cols = 10, 1000
    fake = 1 << 20
    BIG = E.LSDSORT_MAX_KEYS

    def call(keys=fake, k=fake, out=fake + (1 << 16), w=fake, wb=None, rows=rows, cols=cols, kt=BF16, largest=1, fill=0xFF80):
        if wb is None:
            wb = L.lsdsort_topk16_filter_workspace_bytes(rows, cols)
        return L.lsdsort_topk16_filter_device(keys, rows, cols, k, kt, largest, fill, out, w, wb, None)

    # 1. key type
    for kt in (-1, 4, 5, 100):
        assert call(kt=kt, rows=BIG + 1, keys=None, k=None, out=None, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG, kt
        assert call(kt=kt, rows=0, wb=0) == E.LSDSORT_ERR_INVALID_ARG, kt
    # 2. sizes
    assert call(rows=BIG + 1, cols=1, keys=None, k=None, out=None, w=None, wb=0) == E.LSDSORT_ERR_TOO_LARGE
    assert call(rows=1 << 15, cols=1 << 15, keys=None, k=fake + 1, out=None, w=None, wb=0) == E.LSDSORT_ERR_TOO_LARGE
    assert call(rows=2, cols=BIG // 2 + 1, keys=fake + 1, out=None, w=None, wb=0) == E.LSDSORT_ERR_TOO_LARGE
    # 3. nothing to do
    for kt in (U16, I16, F16, BF16):
        for largest in (0, 1):
            assert call(kt=kt, largest=largest, rows=0, keys=None, k=None, out=None, w=None, wb=0) == E.LSDSORT_OK
            assert call(kt=kt, largest=largest, cols=0, keys=fake + 1, k=fake + 2, out=fake + 1, w=None, wb=0) == E.LSDSORT_OK
    # 4. NULL or odd d_keys or d_out; NULL or misaligned d_k
    assert call(keys=None, w=None) == E.LSDSORT_ERR_INVALID_ARG
    assert call(out=None, w=None) == E.LSDSORT_ERR_INVALID_ARG
    assert call(k=None, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG
    for off in (1, 3, 7, 15):
        assert call(keys=fake + off, w=None) == E.LSDSORT_ERR_INVALID_ARG, off
        assert call(out=fake + off, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG, off
    for off in (1, 2, 3, 6, 13):
        assert call(k=fake + off, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG, off
    # 5. workspace
    assert call(w=None) == E.LSDSORT_ERR_WORKSPACE
    assert call(w=fake + 128) == E.LSDSORT_ERR_WORKSPACE
    need = L.lsdsort_topk16_filter_workspace_bytes(rows, cols)
    assert need > 0 and call(wb=need - 1) == E.LSDSORT_ERR_WORKSPACE
    assert call(out=fake, wb=need - 1) == E.LSDSORT_ERR_WORKSPACE                       # in place passes check 4
    for src in (2, 6, 14):
        for dst in (0, 4, 10):
            assert call(keys=fake + src, out=fake + (1 << 16) + dst, w=None) == E.LSDSORT_ERR_WORKSPACE, (src, dst)   # alignments may differ
    assert call(rows=3, cols=70001, wb=L.lsdsort_topk16_filter_workspace_bytes(3, 70001) - 1) == E.LSDSORT_ERR_WORKSPACE
    # 6. the device
    import torch

    if not torch.cuda.is_available():
        for kt in (U16, I16, F16, BF16):
            for largest in (0, 1):
                for fill in (0, 0x7E7E, 0xFFFF):
                    assert call(kt=kt, largest=largest, fill=fill) == E.LSDSORT_ERR_NO_DEVICE
                assert call(kt=kt, largest=largest, rows=3, cols=70001) == E.LSDSORT_ERR_NO_DEVICE
        assert call(out=fake) == E.LSDSORT_ERR_NO_DEVICE                                # in place
        assert call(keys=fake + 14, out=fake + 6, k=fake + 12, cols=1001) == E.LSDSORT_ERR_NO_DEVICE


# (rows, cols) -> bytes, as the unit lays them out: control block 256, 16 B per row, and above 16384 keys per row 8 KiB of counters
# per row and (per-row entry only) 4 B per 16384 keys; every array rounded up to 256 bytes
PINNED = {
    "lsdsort_kth16_perrow_workspace_bytes": {(1, 1): 512, (10, 1000): 512, (17, 1000): 768, (3, 16384): 512, (3, 16385): 25344,
                                             (3, 70001): 25344, (128, 128256): 1054976, (1, (1 << 20) + 13): 9216,
                                             (4096, 131072): 33751296},
    "lsdsort_topk16_filter_workspace_bytes": {(1, 1): 512, (10, 1000): 512, (17, 1000): 768, (3, 16384): 512, (3, 16385): 25088,
                                              (3, 70001): 25088, (128, 128256): 1050880, (1, (1 << 20) + 13): 8704,
                                              (4096, 131072): 33620224},
}


@pytest.mark.parametrize("entry", sorted(PINNED))
def test_workspace_figure(entry):
    from lsdradixsort_amd import errors as E

    L = _lib()
    BIG = E.LSDSORT_MAX_KEYS
    f = getattr(L, entry)
    counts = 4 if "perrow" in entry else 0                                                # bytes per chunk count

    def bound(rows, cols):
        return 256 + rows * (16 + ((8192 + counts * -(-cols // 16384)) if cols > 16384 else 0)) + 765

    ladder = [1, 2, 7, 8, 9, 1000, 1024, 1025, 16384, 16385, 65536, 131073, (1 << 20) + 13, 1 << 24, BIG]
    row_ladder = [1, 2, 3, 64, 65, 513, 4096, 4097, 1 << 15, 1 << 20, BIG]
    seen = 0
    for rows in row_ladder:
        prev = 0
        for cols in ladder:
            if rows * cols > BIG:
                assert f(rows, cols) == 0, (rows, cols)
                continue
            b = f(rows, cols)
            assert b > 0 and b % 256 == 0 and b >= prev, (rows, cols, b, prev)            # monotonic in cols
            assert b <= bound(rows, cols), (rows, cols, b)
            if cols >= 16385:                                                             # O(rows), never O(rows * cols)
                assert 2 * b <= 2 * rows * cols, (rows, cols, b)
                assert cols < 65536 or 8 * b <= 2 * rows * cols, (rows, cols, b)
            else:
                assert b <= 256 + rows * 16 + 255, (rows, cols, b)
            prev = b
            seen += 1
    assert seen > 60
    for cols in ladder:                                                                   # monotonic in rows
        prev = 0
        for rows in row_ladder:
            if rows * cols <= BIG:
                b = f(rows, cols)
                assert b >= prev, (rows, cols)
                prev = b
    assert f(1, 16385) > f(1, 16384) and f(2, 1 << 24) > f(1, 1 << 24)
    assert f(0, 1000) % 256 == 0 and f(10, 0) % 256 == 0
    # O(rows): from 2 chunks per row to 5, three rows grow by their chunk counts at the most (and a rounding to 256)
    grown = f(3, 70001) - f(3, 16385)
    assert 0 <= grown <= 3 * counts * (-(-70001 // 16384) - -(-16385 // 16384)) + 255, grown
    # above the limits
    assert f(BIG + 1, 1) == 0 and f(1, BIG + 1) == 0 and f(BIG + 1, 0) == 0
    assert f(2, BIG // 2 + 1) == 0 and f(1 << 15, 1 << 15) == 0
    assert f(1, BIG) > 0 and f(BIG, 1) > 0
    for (rows, cols), want in PINNED[entry].items():
        assert f(rows, cols) == want, (rows, cols, f(rows, cols), want)
    if "perrow" in entry:                                                                 # kth16's layout
        for rows, cols in PINNED[entry]:
            assert f(rows, cols) == L.lsdsort_kth16_workspace_bytes(rows, cols), (rows, cols)


def test_wrappers_check_their_tensors_before_the_library(no_library):
    import torch

    lsd = no_library
    k = torch.zeros(1, dtype=torch.int32)
    for dtype, key_type in ((torch.int16, "int16"), (torch.int16, "uint16"), (torch.float16, "float16"), (torch.bfloat16, "bfloat16")):
        t = torch.zeros(8, dtype=dtype)
        with pytest.raises(TypeError):
            lsd.GPUKth16PerRow(t, k, key_type=key_type)                           # a CPU tensor
        with pytest.raises(TypeError):
            lsd.GPUTopK16Filter(t, k, key_type=key_type)
        with pytest.raises(TypeError):
            lsd.topk16_filter_rows(t, 3)
    for call in (lambda: lsd.GPUKth16PerRow([3, 1, 2], k), lambda: lsd.GPUTopK16Filter([3, 1, 2], k), lambda: lsd.topk16_filter_rows([3.0, 1.0], 1)):
        with pytest.raises(TypeError):
            call()


def test_dtype_key_type_per_row_arrays_fill_and_k(no_library):
    """Wrong dtype, a key type that does not fit, a 3-D or non-contiguous input, a per-row array that is no int32 CUDA tensor or has
    the wrong length, a fill outside 16 bits, an `out` of another shape or dtype, a k of the wrong kind or count -- checked on tensors
    that pass for CUDA tensors, so that the test needs no device."""
    import torch

    lsd = no_library

    def fake(dtype, shape=(2, 4)):
        return torch.zeros(shape, dtype=dtype).as_subclass(FakeCuda)

    k2 = fake(torch.int32, (2,))
    for dtype in (torch.int32, torch.float32, torch.int64, torch.uint8, torch.float64):
        with pytest.raises(TypeError):
            lsd.GPUKth16PerRow(fake(dtype), k2)
        with pytest.raises(TypeError):
            lsd.GPUTopK16Filter(fake(dtype), k2)
        with pytest.raises(TypeError):
            lsd.topk16_filter_rows(fake(dtype), 2)
    fits = {torch.int16: ("uint16", "int16"), torch.float16: ("float16",), torch.bfloat16: ("bfloat16",)}
    for dtype, mine in fits.items():
        ok = mine[0]
        for entry in (lsd.GPUKth16PerRow, lsd.GPUTopK16Filter):
            for key_type in ("uint16", "int16", "float16", "bfloat16"):
                if key_type not in mine:
                    with pytest.raises(TypeError):
                        entry(fake(dtype), k2, key_type=key_type)                 # a key type that does not fit the dtype
            for key_type in ("uint32", "float32", "half", ""):
                with pytest.raises(ValueError):
                    entry(fake(dtype), k2, key_type=key_type)                     # a key type this entry does not have
            with pytest.raises(TypeError):
                entry(fake(dtype, (2, 2, 2)), k2, key_type=ok)                    # 1-D or 2-D only
            with pytest.raises(TypeError):
                entry(fake(dtype, (4, 4)).t(), fake(torch.int32, (4,)), key_type=ok)   # contiguous only
            # the per-row array: an int32 CUDA tensor, contiguous, one entry per row
            for bad in (torch.zeros(2, dtype=torch.int32), fake(torch.int64, (2,)), fake(torch.int16, (2,)), [1, 2], 1, None,
                        fake(torch.int32, (4,))[::2]):
                with pytest.raises(TypeError):
                    entry(fake(dtype), bad, key_type=ok)
            for count in (0, 1, 3, 8):
                with pytest.raises(ValueError):
                    entry(fake(dtype), fake(torch.int32, (count,)), key_type=ok)
            with pytest.raises(ValueError):
                entry(fake(dtype, (4,)), k2, key_type=ok)                         # 1-D input: one row
        for fill in (-1, 0x10000, 1.5, "0", True):
            with pytest.raises(ValueError):
                lsd.GPUTopK16Filter(fake(dtype), k2, key_type=ok, fill=fill)
        other = torch.float16 if dtype != torch.float16 else torch.bfloat16
        for out in (fake(dtype, (2, 5)), fake(dtype, (8,)), fake(other), torch.zeros((2, 4), dtype=dtype)):
            with pytest.raises((TypeError, ValueError)):
                lsd.GPUTopK16Filter(fake(dtype), k2, key_type=ok, out=out)
        x = fake(dtype, (3, 2, 4))
        for k in (1.5, "3", None, True, fake(torch.float32, (6,)), fake(torch.int16, (6,))):
            with pytest.raises(TypeError):
                lsd.topk16_filter_rows(x, k)
        for k in ([1, 2], [1] * 7, fake(torch.int32, (5,)), fake(torch.int64, (2, 3, 4))):
            with pytest.raises(ValueError):
                lsd.topk16_filter_rows(x, k)
        with pytest.raises(TypeError):
            lsd.topk16_filter_rows(fake(dtype, ()), 1)                            # at least one dimension
        with pytest.raises(TypeError):
            lsd.topk16_filter_rows(fake(dtype, (4, 4)).t(), 1, inplace=True)      # in place: contiguous only
    with pytest.raises(ValueError):
        lsd.topk16_filter_rows(fake(torch.int16), 1, fill=40000)
    with pytest.raises(ValueError):
        lsd.topk16_filter_rows(fake(torch.int16), 1, fill=0.5)
    with pytest.raises(TypeError):
        lsd.GPUKth16PerRow(fake(torch.bfloat16), k2)                              # the default key type is int16


def test_host_conversions_of_fill_and_k(no_library):
    """What topk16_filter_rows hands the library for a host-side fill and k, worked out on the CPU: the fill as the 16-bit word of
    the tensor's dtype, k as an int32 vector with one entry per row, values outside int32 clamped into it (both ends are "off")."""
    import torch

    api = no_library.api
    bits = api._fill_bits16
    assert bits(torch.bfloat16, None, True) == 0xFF80 and bits(torch.bfloat16, None, False) == 0x7F80           # -inf, +inf
    assert bits(torch.float16, None, True) == 0xFC00 and bits(torch.float16, None, False) == 0x7C00
    assert bits(torch.int16, None, True) == 0x8000 and bits(torch.int16, None, False) == 0x7FFF                 # the worst value
    assert api._worst_bits16("uint16", True) == 0x0000 and api._worst_bits16("uint16", False) == 0xFFFF
    for key_type in rk.ALL_TYPES:                                                                                 # worst: last in its order
        for largest in (False, True):
            word = np.array([api._worst_bits16(key_type, largest)], dtype=np.uint16)
            numbers = np.arange(1 << 16, dtype=np.uint16)
            if key_type in rk.SPECIALS:                                                                           # NaNs rank beyond +-inf
                exp = (0x7C00, 0x03FF) if key_type == "float16" else (0x7F80, 0x007F)
                numbers = numbers[~(((numbers & exp[0]) == exp[0]) & ((numbers & exp[1]) != 0))]
            assert rk.sortable16_np(word, key_type, largest)[0] == rk.sortable16_np(numbers, key_type, largest).max(), (key_type, largest)
    assert bits(torch.int16, -7, True) == 0xFFF9 and bits(torch.int16, 32767, True) == 0x7FFF and bits(torch.int16, 3.0, False) == 3
    assert bits(torch.bfloat16, -1.0, True) == 0xBF80 and bits(torch.float16, -1.0, True) == 0xBC00
    assert bits(torch.bfloat16, float("-inf"), False) == 0xFF80 and bits(torch.float16, 0.0, True) == 0
    vec = api._k_per_row
    for k, want in ((50, [50] * 4), (0, [0] * 4), (-1, [-1] * 4), (1 << 40, [(1 << 31) - 1] * 4), (-(1 << 40), [-(1 << 31)] * 4),
                    ([1, 20, 0, -1], [1, 20, 0, -1]), ((5, 1 << 33, 7, 9), [5, (1 << 31) - 1, 7, 9]), (np.array([3, 2, 1, 0]), [3, 2, 1, 0]),
                    (torch.tensor([1, -1, 1 << 35, -(1 << 35)]), [1, -1, (1 << 31) - 1, -(1 << 31)]),
                    (torch.tensor([[4, 3], [2, 1]], dtype=torch.int32), [4, 3, 2, 1])):
        got = vec(k, 4, "cpu")
        assert got.dtype == torch.int32 and got.shape == (4,) and got.is_contiguous() and got.tolist() == want, (k, got)
    own = torch.tensor([9, 8, 7, 6], dtype=torch.int32)
    assert vec(own, 4, "cpu").data_ptr() == own.data_ptr()                                                        # used as it is
    # as the library reads them: a negative entry is a uint32 above every row length
    assert (vec([-1, -(1 << 40)], 2, "cpu").numpy().view(np.uint32) >= 1 << 31).all()
    for k in (torch.zeros(4), torch.zeros(4, dtype=torch.int16), 1.0, "4", None, True):
        with pytest.raises(TypeError):
            vec(k, 4, "cpu")
    for k in ([1, 2, 3], torch.zeros(5, dtype=torch.int32), []):
        with pytest.raises(ValueError):
            vec(k, 4, "cpu")


def test_the_numpy_oracle_on_a_worked_example():
    """the helper module's filter against a row worked out by hand: bfloat16, largest, k = 3 with a tie at the threshold"""
    row = np.array([[0x3F80, 0x4000, 0xBF80, 0x4000, 0x4040, 0x0000, 0x8000, 0x4000]], dtype=np.uint16)   # 1 2 -1 2 3 0 -0 2
    out = rk.filter_np(row, np.array([3], dtype=np.uint32), "bfloat16", True)
    assert out.tolist() == [[rk.FILL, 0x4000, rk.FILL, 0x4000, 0x4040, rk.FILL, rk.FILL, 0x4000]]        # 3 and every 2: four kept
    out = rk.filter_np(row, np.array([6], dtype=np.uint32), "bfloat16", True)
    assert out.tolist() == [[0x3F80, 0x4000, rk.FILL, 0x4000, 0x4040, 0x0000, rk.FILL, 0x4000]]          # +0.0 kept, -0.0 ranks below it
    for k in (0, 8, 13, rk.OFF):
        assert np.array_equal(rk.filter_np(row, np.array([k], dtype=np.uint32), "bfloat16", True), row)
    assert rk.cycle(rk.candidates_k(9), 9).tolist() == [0, 1, 2, 4, 8, 9, 14, rk.OFF, 0]
    assert [list(rk.shifts(rk.candidates_k(9), rows)) for rows in (1, 3, 9)] == [list(range(8)), [0, 3, 6], [0]]


def test_kernels_no_scratch_no_spill_and_recorded_resources():
    if hipcc() is None:
        pytest.skip("no hipcc on this machine")
    res = kernel_resources("kth16_rowk.hip")
    names = list(res)
    # count, pick and locate: the kernel templates of select_tiles16.hpp and radix_select.hpp, as Kth16Rowk
    once = ("count_rows16_kernelINS0_9Kth16RowkE", "pick_rows_kernelINS0_9Kth16RowkE", "locate_rows16_kernelINS0_9Kth16RowkE",
            "kth16r_value_kernel", "topk16f_apply_kernel")
    for must in once:
        assert sum(must in name for name in names) == 1, (must, names)
    for twice in ("kth16r_short_kernel", "topk16f_short_kernel", "kth16r_hist_kernel", "kth16r_clear_kernel"):
        assert sum(twice in name for name in names) == 2, (twice, names)              # wavefront / workgroup; two levels; rank / k
    assert sum("kth16r_scan_kernel" in name for name in names) == 3, names              # level 0 under two stop rules, level 1
    assert len(names) == len(once) + 4 * 2 + 3, names
    assert all("kth16r_" in name or "topk16f_" in name or "_kernelINS0_9Kth16RowkE" in name for name in names), names   # each names its unit
    for name, r in res.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r)
    want = json.load(open(GOLDEN))["kth16_rowk.hip"]
    assert sorted(res) == sorted(want), f"kernels gone: {sorted(set(want) - set(res))}, new: {sorted(set(res) - set(want))}"
    for name, w in want.items():
        assert res[name]["occupancy"] >= w["occupancy"], f"{name}: {res[name]['occupancy']} waves/SIMD, recorded {w['occupancy']}"
        assert res[name]["lds_bytes"] == w["lds_bytes"], f"{name}: {res[name]['lds_bytes']} B of static LDS, recorded {w['lds_bytes']}"
    # reading the rank from memory costs the short kernels nothing: kth16.hip's occupancy and static LDS; the filter needs no
    # per-wave counts and no more registers
    one16 = kernel_resources("kth16.hip")
    for waves in (1, 16):
        tag = "short_kernelILi%dEE" % waves
        single = next(r for name, r in one16.items() if tag in name)
        mine = next(r for name, r in res.items() if "kth16r_" + tag in name)
        flt = next(r for name, r in res.items() if "topk16f_" + tag in name)
        assert mine["occupancy"] >= single["occupancy"] and mine["lds_bytes"] == single["lds_bytes"], (waves, single, mine)
        assert flt["occupancy"] >= single["occupancy"] and flt["lds_bytes"] < single["lds_bytes"], (waves, single, flt)


# <kernel><template arguments> , dim3(grid_for(<items>, <per>, <cap>)): the form tests/test_row_rounds_cpu.py reads
LAUNCH = re.compile(r"(\w+_kernel(?:<[^<>]*>)?)[>,(\s]*dim3\(grid_for\(([^,()]+),\s*(\w+)\s*,\s*(\w+)\s*\)\)")
ROUNDS = {"WAVE": (131072 + 9, 9), "GROUP": (4096 + 3, 1025)}   # the shapes test_gpu_kth16_rowk.py runs past the caps


@pytest.mark.parametrize("kernel,per,cap,shape", [("kth16r_short_kernel<1>", 8, 16384, "WAVE"), ("kth16r_short_kernel<16>", 1, 4096, "GROUP"),
                                                  ("topk16f_short_kernel<1>", 8, 16384, "WAVE"), ("topk16f_short_kernel<16>", 1, 4096, "GROUP")])
def test_short_kernels_launch_lines_and_second_round_shapes(kernel, per, cap, shape):
    text = open(os.path.join(ROOT, "lsdradixsort_amd", "csrc", "kth16_rowk.hip")).read()
    found = {(items.strip(), a, b) for k, items, a, b in LAUNCH.findall(text) if k == kernel}
    assert found == {("rows", str(per), str(cap))}, f"{kernel} is launched with {sorted(found)}"
    assert re.search(r"cols <= \(size_t\)kWaveSegCap\b", text) and re.search(r"cols <= \(size_t\)kLocalSortCap\b", text)
    rows, cols = ROUNDS[shape]
    assert per * cap < rows, f"{shape}: one round of {kernel} covers {per * cap} >= {rows} rows"
    rest = rows % (per * cap)
    assert rest != 0 and (per == 1 or rest % per != 0), f"{shape}: the last round of {kernel} holds {rest} rows: no partly filled workgroup"
    assert per * cap == rr.STRIDE["wave" if per == 8 else "group"], f"{shape}: {kernel} strides by {per * cap}"
    assert (cols <= rr.TIERS["wave"]) == (per == 8) and cols <= rr.TIERS["group"]


def test_the_unit_includes_the_shared_headers_only_and_has_no_inline_assembly():
    """kth16_rowk.hip takes its tile helpers from select_tiles16.hpp: it includes the shared headers and none of the sibling units"""
    text = open(os.path.join(ROOT, "lsdradixsort_amd", "csrc", "kth16_rowk.hip")).read()
    assert set(re.findall(r'#include "([^"]+)"', text)) == {"../../include/lsdsort.h", "keys16_map.hpp", "lsd_device.hpp", "lsd_host.hpp",
                                                             "radix_select.hpp", "select_tiles16.hpp"}
    assert "asm" not in re.sub(r"//.*", "", text)                                          # no inline assembly
