"""CPU suite: the 16-bit k-th value selection's C-ABI surface (lsdsort_kth16_device and its workspace figure), its argument checks
without a device, the Python and C++ faces' own argument errors, and the resources of every kernel of kth16.hip from hipcc's own
remarks."""
import os
import re

import pytest

from _faces import FakeCuda, lib as _lib, no_library
from _kernel_resources import hipcc, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U16, I16, F16, BF16 = range(4)
ENTRIES = ("lsdsort_kth16_workspace_bytes", "lsdsort_kth16_device")
NAMES = ("GPUKth16", "kth16_workspace_bytes", "kthvalue16_rows", "median16_rows")


def test_header_ctypes_table_and_faces_have_the_entries():
    from lsdradixsort_amd import _lib as binding

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsdsort.h")).read(), flags=re.S)
    for name in ENTRIES:
        assert re.search(r"LSDSORT_API\s+[\w\s\*]+?\b" + name + r"\s*\(", text), name
        assert name in binding.SIGNATURES
        assert hasattr(_lib(), name)
    # top-k's signature with a rank where it has k, and the 32-bit entry's figure: the ctypes rows agree
    assert binding.SIGNATURES["lsdsort_kth16_device"] == binding.SIGNATURES["lsdsort_topk16_device"]
    assert binding.SIGNATURES["lsdsort_kth16_workspace_bytes"] == binding.SIGNATURES["lsdsort_kth_workspace_bytes"]
    hpp = open(os.path.join(ROOT, "include", "lsdsort.hpp")).read()
    assert re.search(r"inline\s+size_t\s+kth16_workspace_bytes\s*\(", hpp)
    for ctype in ("uint16_t", "int16_t"):
        assert re.search(r"inline\s+void\s+kth16_device\s*\(\s*const\s+%s\s*\*" % ctype, hpp), ctype
    body = hpp[hpp.index("inline void kth16_device(const uint16_t*"):]
    body = body[:body.index("{")]
    assert "lsdsort_key16_type key_type" in body and "bool largest = false" in body
    import lsdradixsort_amd as lsd

    for name in NAMES:
        assert callable(getattr(lsd, name)) and name in lsd.api.__all__, name


def test_argument_checks_in_entry_order():
    from lsdradixsort_amd import errors as E

    L = _lib()
    rows, cols, rank = 10, 1000, 7
    fake = 1 << 20   # never dereferenced: every call below returns before a device is touched
    BIG = E.LSDSORT_MAX_KEYS

    def call(keys=fake, out=fake, idx=fake, w=fake, wb=None, rows=rows, cols=cols, rank=rank, kt=BF16, largest=0):
        if wb is None:
            wb = L.lsdsort_kth16_workspace_bytes(rows, cols)
        return L.lsdsort_kth16_device(keys, rows, cols, rank, kt, largest, out, idx, w, wb, None)

    # 1. key type, before everything else
    for kt in (-1, 4, 5, 100):
        assert call(kt=kt, rows=BIG + 1, rank=cols, keys=None, out=None, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG, kt
        assert call(kt=kt, rows=0, wb=0) == E.LSDSORT_ERR_INVALID_ARG, kt
    # 2. size, before the empty call, the rank, the pointers and the workspace
    assert call(rows=BIG + 1, cols=1, rank=5, keys=None, out=None, w=None, wb=0) == E.LSDSORT_ERR_TOO_LARGE
    assert call(rows=1 << 15, cols=1 << 15, rank=1 << 15, keys=None, out=None, w=None, wb=0) == E.LSDSORT_ERR_TOO_LARGE
    assert call(rows=2, cols=BIG // 2 + 1, rank=BIG, keys=fake + 1, out=None, w=None, wb=0) == E.LSDSORT_ERR_TOO_LARGE
    # 3. nothing to do, before the rank (an empty row has no valid rank), the pointers and the workspace
    for kt in (U16, I16, F16, BF16):
        for largest in (0, 1):
            assert call(kt=kt, largest=largest, rows=0, rank=cols, keys=None, out=None, idx=None, w=None, wb=0) == E.LSDSORT_OK
            assert call(kt=kt, largest=largest, rows=0, rank=cols + 5, keys=fake + 1, out=None, w=None, wb=0) == E.LSDSORT_OK
            assert call(kt=kt, largest=largest, cols=0, rank=0, keys=None, out=None, idx=None, w=None, wb=0) == E.LSDSORT_OK
            assert call(kt=kt, largest=largest, cols=0, rank=9, keys=None, out=fake + 1, w=None, wb=0) == E.LSDSORT_OK
    # 4. the rank, before the pointers and the workspace
    assert call(rank=cols, keys=None, out=None, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG
    assert call(rank=cols + 1, keys=fake + 1, out=None, w=fake + 128, wb=0) == E.LSDSORT_ERR_INVALID_ARG
    assert call(rank=BIG, keys=None, out=None, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG
    assert call(rows=1, cols=1, rank=1, keys=None, out=None, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG
    # 5. the keys and the values, before the workspace: NULL, or odd
    assert call(keys=None, w=None) == E.LSDSORT_ERR_INVALID_ARG
    assert call(out=None, w=None) == E.LSDSORT_ERR_INVALID_ARG
    for off in (1, 3, 7, 15):
        assert call(keys=fake + off, w=None) == E.LSDSORT_ERR_INVALID_ARG, off
        assert call(out=fake + off, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG, off
    assert call(keys=fake + 6, out=fake + 5, w=None) == E.LSDSORT_ERR_INVALID_ARG
    # 6. workspace: exactly lsdsort_kth16_workspace_bytes(rows, cols)
    assert call(w=None) == E.LSDSORT_ERR_WORKSPACE
    assert call(w=fake + 128) == E.LSDSORT_ERR_WORKSPACE                                # misaligned
    need = L.lsdsort_kth16_workspace_bytes(rows, cols)
    assert need > 0 and call(wb=need - 1) == E.LSDSORT_ERR_WORKSPACE
    assert call(idx=None, wb=need - 1) == E.LSDSORT_ERR_WORKSPACE                       # one figure, with or without indices
    for off in (2, 4, 6, 10, 14):
        assert call(keys=fake + off, out=fake + 16 - off, w=None) == E.LSDSORT_ERR_WORKSPACE, off   # 2-byte alignment passes check 5
    long_need = L.lsdsort_kth16_workspace_bytes(3, 70001)
    assert call(rows=3, cols=70001, rank=70000, wb=long_need - 1) == E.LSDSORT_ERR_WORKSPACE
    assert call(rows=3, cols=70001, rank=70000, idx=None, wb=long_need - 1) == E.LSDSORT_ERR_WORKSPACE
    # 7. without a gfx950 device the last check answers; with one, this test does not get here on bogus pointers
    import torch

    if not torch.cuda.is_available():
        for kt in (U16, I16, F16, BF16):
            for largest in (0, 1):
                for idx in (None, fake):
                    assert call(kt=kt, largest=largest, idx=idx) == E.LSDSORT_ERR_NO_DEVICE
                    assert call(kt=kt, largest=largest, idx=idx, rows=3, cols=70001, rank=35000) == E.LSDSORT_ERR_NO_DEVICE   # the long tier
        assert call(keys=fake + 2) == E.LSDSORT_ERR_NO_DEVICE                           # 2-byte, not 16-byte aligned
        assert call(keys=fake + 14, out=fake + 6, cols=1001, rank=1000) == E.LSDSORT_ERR_NO_DEVICE
        assert call(rank=0) == E.LSDSORT_ERR_NO_DEVICE and call(rank=cols - 1) == E.LSDSORT_ERR_NO_DEVICE


def bound(rows, cols):
    """The figure as kth16.hip lays it out: control block, 16 B per row, and above 16384 keys per row 2048 counters per row and
    4 B per 16384 keys; every array rounded up to 256 bytes."""
    is_long = cols > 16384
    return 256 + rows * (16 + ((8192 + 4 * -(-cols // 16384)) if is_long else 0)) + 765


def test_workspace_figure():
    from lsdradixsort_amd import errors as E

    L = _lib()
    BIG = E.LSDSORT_MAX_KEYS
    f = L.lsdsort_kth16_workspace_bytes
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
            if cols >= 16385:                                                             # O(rows), never O(rows * cols):
                assert 2 * b <= 2 * rows * cols, (rows, cols, b)                          # half of the keys' bytes at the most
                assert cols < 65536 or 8 * b <= 2 * rows * cols, (rows, cols, b)          # an eighth from 65536 keys per row on
            else:
                assert b <= 256 + rows * 16 + 255, (rows, cols, b)                        # the short tiers: a row state, no more
            prev = b
            seen += 1
    assert seen > 60
    for cols in ladder:                                                                   # monotonic in rows
        prev = 0
        for rows in row_ladder:
            if rows * cols > BIG:
                continue
            b = f(rows, cols)
            assert b >= prev, (rows, cols)
            prev = b
    assert f(1, 16385) > f(1, 16384) and f(2, 1 << 24) > f(1, 1 << 24)
    assert f(0, 1000) % 256 == 0 and f(10, 0) % 256 == 0
    # above the limits
    assert f(BIG + 1, 1) == 0 and f(1, BIG + 1) == 0 and f(BIG + 1, 0) == 0
    assert f(2, BIG // 2 + 1) == 0 and f(1 << 15, 1 << 15) == 0
    assert f(1, BIG) > 0 and f(BIG, 1) > 0


def test_wrappers_check_their_tensors_before_the_library(no_library):
    import torch

    lsd = no_library
    for dtype, key_type in ((torch.int16, "int16"), (torch.int16, "uint16"), (torch.float16, "float16"), (torch.bfloat16, "bfloat16")):
        t = torch.zeros(8, dtype=dtype)
        with pytest.raises(TypeError):
            lsd.GPUKth16(t, 1, key_type=key_type)                                # a CPU tensor
        with pytest.raises(TypeError):
            lsd.kthvalue16_rows(t, 1)
        with pytest.raises(TypeError):
            lsd.median16_rows(t)
    with pytest.raises(TypeError):
        lsd.GPUKth16([3, 1, 2], 1)
    with pytest.raises(TypeError):
        lsd.kthvalue16_rows([3, 1, 2], 1)
    with pytest.raises(TypeError):
        lsd.median16_rows([3, 1, 2])


def test_dtype_key_type_rank_and_k(no_library):
    """Wrong dtype, a key type this entry does not have or that does not go with the dtype, a 3-D or non-contiguous input, a rank
    outside 0 .. cols - 1 and k outside 1 .. cols -- checked on tensors that pass for CUDA tensors, so that the test needs no
    device."""
    import torch

    lsd = no_library

    def fake(dtype, shape=(2, 4)):
        return torch.zeros(shape, dtype=dtype).as_subclass(FakeCuda)

    pairs = {torch.int16: "int16", torch.float16: "float16", torch.bfloat16: "bfloat16"}
    for dtype in (torch.int32, torch.float32, torch.int64, torch.float64, torch.uint8):
        for key_type in ("int16", "float16", "bfloat16"):
            with pytest.raises(TypeError):
                lsd.GPUKth16(fake(dtype), 1, key_type=key_type)
        with pytest.raises(TypeError):
            lsd.kthvalue16_rows(fake(dtype), 1)
        with pytest.raises(TypeError):
            lsd.median16_rows(fake(dtype))
    for dtype, own in pairs.items():
        for key_type in ("uint32", "int32", "float32", "uint64", "float64", "half", ""):
            with pytest.raises(ValueError):
                lsd.GPUKth16(fake(dtype), 1, key_type=key_type)                  # no such 16-bit type
        for key_type in ("uint16", "int16", "float16", "bfloat16"):
            fits = key_type == own or (dtype == torch.int16 and key_type == "uint16")
            if not fits:
                with pytest.raises(TypeError):
                    lsd.GPUKth16(fake(dtype), 1, key_type=key_type)              # a dtype / key_type mismatch
        with pytest.raises(TypeError):
            lsd.GPUKth16(fake(dtype, (2, 2, 2)), 1, key_type=own)                # 1-D or 2-D only
        with pytest.raises(TypeError):
            lsd.GPUKth16(fake(dtype, (4, 4)).t(), 1, key_type=own)               # contiguous only
        for rank in (-1, 4, 5, 100):
            with pytest.raises(ValueError):
                lsd.GPUKth16(fake(dtype), rank, key_type=own)
            with pytest.raises(ValueError):
                lsd.GPUKth16(fake(dtype, (4,)), rank, key_type=own, largest=True)
        for k in (-1, 0, 5, 100):
            with pytest.raises(ValueError):
                lsd.kthvalue16_rows(fake(dtype, (3, 2, 4)), k)
            with pytest.raises(ValueError):
                lsd.kthvalue16_rows(fake(dtype, (4,)), k)
        with pytest.raises(ValueError):
            lsd.median16_rows(fake(dtype, (3, 0)))
    with pytest.raises(TypeError):
        lsd.GPUKth16(fake(torch.float16), 1)                                     # the default key type is int16's
    # the 32-bit faces keep refusing 16-bit tensors
    for dtype in pairs:
        with pytest.raises(TypeError):
            lsd.GPUKth(fake(dtype), 1)
        with pytest.raises(TypeError):
            lsd.kthvalue_rows(fake(dtype), 1)
        with pytest.raises(TypeError):
            lsd.median_rows(fake(dtype))


def test_kth16_kernels_no_scratch_no_spill():
    if hipcc() is None:
        pytest.skip("no hipcc on this machine")
    res = kernel_resources("kth16.hip")
    names = list(res)
    # count, pick and locate: the kernel templates of select_tiles16.hpp and radix_select.hpp, as Kth16
    for must in ("kth16_clear_kernel", "count_rows16_kernelINS0_5Kth16E", "pick_rows_kernelINS0_5Kth16E", "locate_rows16_kernelINS0_5Kth16E",
                 "kth16_value_kernel"):
        assert sum(must in name for name in names) == 1, (must, names)
    assert sum("kth16_short_kernel" in name for name in names) == 2, names                # one wavefront, one workgroup
    assert sum("kth16_hist_kernel" in name for name in names) == 2, names                 # two digit levels
    assert 2 <= sum("kth16_scan_kernel" in name for name in names) <= 4, names            # two levels, two stop rules at the most
    assert all("kth16_" in name or "_kernelINS0_5Kth16E" in name for name in names), names   # every kernel names its unit
    for name, r in res.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r)
