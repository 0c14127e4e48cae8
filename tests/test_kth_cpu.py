"""CPU suite: the k-th value selection's C-ABI surface (lsdsort_kth_device and its workspace figure), its argument checks without
a device, the Python and C++ faces' own argument errors, and the resources of every kernel of kth.hip from hipcc's own remarks."""
import os
import re

import pytest

from _faces import FakeCuda, lib as _lib, no_library
from _kernel_resources import hipcc, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32, I32, F32 = range(3)
ENTRIES = ("lsdsort_kth_workspace_bytes", "lsdsort_kth_device")


def test_header_ctypes_table_and_faces_have_the_entries():
    from lsdradixsort_amd import _lib as binding

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsdsort.h")).read(), flags=re.S)
    for name in ENTRIES:
        assert re.search(r"LSDSORT_API\s+[\w\s\*]+?\b" + name + r"\s*\(", text), name
        assert name in binding.SIGNATURES
        assert hasattr(_lib(), name)
    # top-k's signature with a rank where it has k: the two ctypes rows agree
    assert binding.SIGNATURES["lsdsort_kth_device"] == binding.SIGNATURES["lsdsort_topk_device"]
    hpp = open(os.path.join(ROOT, "include", "lsdsort.hpp")).read()
    for ctype in ("uint32_t", "int32_t", "float"):
        assert re.search(r"inline\s+void\s+kth_device\s*\(\s*const\s+%s\s*\*" % ctype, hpp), ctype
    import lsdradixsort_amd as lsd

    for name in ("GPUKth", "kth_workspace_bytes", "kthvalue_rows", "median_rows"):
        assert callable(getattr(lsd, name)) and name in lsd.api.__all__, name


def test_argument_checks_in_entry_order():
    from lsdradixsort_amd import errors as E

    L = _lib()
    rows, cols, rank = 10, 1000, 7
    fake = 1 << 20   # never dereferenced: every call below returns before a device is touched
    BIG = E.LSDSORT_MAX_KEYS

    def call(keys=fake, out=fake, idx=fake, w=fake, wb=None, rows=rows, cols=cols, rank=rank, kt=F32, largest=0):
        if wb is None:
            wb = L.lsdsort_kth_workspace_bytes(rows, cols)
        return L.lsdsort_kth_device(keys, rows, cols, rank, kt, largest, out, idx, w, wb, None)

    # 1. key type, before everything else (the 64-bit key types are not this entry's either)
    for kt in (-1, 3, 4, 5, 100):
        assert call(kt=kt, rows=BIG + 1, rank=cols, keys=None, out=None, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG, kt
        assert call(kt=kt, rows=0, wb=0) == E.LSDSORT_ERR_INVALID_ARG, kt
    # 2. size, before the empty call, the rank, the pointers and the workspace
    assert call(rows=BIG + 1, cols=1, rank=5, keys=None, out=None, w=None, wb=0) == E.LSDSORT_ERR_TOO_LARGE
    assert call(rows=1 << 15, cols=1 << 15, rank=1 << 15, keys=None, out=None, w=None, wb=0) == E.LSDSORT_ERR_TOO_LARGE
    assert call(rows=2, cols=BIG // 2 + 1, rank=BIG, keys=fake + 1, out=None, w=None, wb=0) == E.LSDSORT_ERR_TOO_LARGE
    # 3. nothing to do, before the rank (an empty row has no valid rank), the pointers and the workspace
    for kt in (U32, I32, F32):
        for largest in (0, 1):
            assert call(kt=kt, largest=largest, rows=0, rank=cols, keys=None, out=None, idx=None, w=None, wb=0) == E.LSDSORT_OK
            assert call(kt=kt, largest=largest, rows=0, rank=cols + 5, keys=fake + 1, out=None, w=None, wb=0) == E.LSDSORT_OK
            assert call(kt=kt, largest=largest, cols=0, rank=0, keys=None, out=None, idx=None, w=None, wb=0) == E.LSDSORT_OK
            assert call(kt=kt, largest=largest, cols=0, rank=9, keys=None, out=fake + 2, w=None, wb=0) == E.LSDSORT_OK
    # 4. the rank, before the pointers and the workspace
    assert call(rank=cols, keys=None, out=None, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG
    assert call(rank=cols + 1, keys=fake + 2, out=None, w=fake + 128, wb=0) == E.LSDSORT_ERR_INVALID_ARG
    assert call(rank=BIG, keys=None, out=None, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG
    assert call(rows=1, cols=1, rank=1, keys=None, out=None, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG
    # 5. the keys and the values, before the workspace: NULL, or not 4-byte aligned
    assert call(keys=None, w=None) == E.LSDSORT_ERR_INVALID_ARG
    assert call(out=None, w=None) == E.LSDSORT_ERR_INVALID_ARG
    for off in (1, 2, 3):
        assert call(keys=fake + off, w=None) == E.LSDSORT_ERR_INVALID_ARG, off
        assert call(out=fake + off, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG, off
    assert call(keys=fake + 6, out=fake + 4, w=None) == E.LSDSORT_ERR_INVALID_ARG
    # 6. workspace: exactly lsdsort_kth_workspace_bytes(rows, cols)
    assert call(w=None) == E.LSDSORT_ERR_WORKSPACE
    assert call(w=fake + 128) == E.LSDSORT_ERR_WORKSPACE                                # misaligned
    need = L.lsdsort_kth_workspace_bytes(rows, cols)
    assert need > 0 and call(wb=need - 1) == E.LSDSORT_ERR_WORKSPACE
    assert call(idx=None, wb=need - 1) == E.LSDSORT_ERR_WORKSPACE                       # one figure, with or without indices
    assert call(keys=fake + 4, out=fake + 12, w=None) == E.LSDSORT_ERR_WORKSPACE        # 4-byte alignment passes check 5
    long_need = L.lsdsort_kth_workspace_bytes(3, 70001)
    assert call(rows=3, cols=70001, rank=70000, wb=long_need - 1) == E.LSDSORT_ERR_WORKSPACE
    # 7. without a gfx950 device the last check answers; with one, this test does not get here on bogus pointers
    import torch

    if not torch.cuda.is_available():
        for kt in (U32, I32, F32):
            for largest in (0, 1):
                for idx in (None, fake):
                    assert call(kt=kt, largest=largest, idx=idx) == E.LSDSORT_ERR_NO_DEVICE
        assert call(keys=fake + 4) == E.LSDSORT_ERR_NO_DEVICE                           # 4-byte, not 16-byte aligned
        assert call(keys=fake + 12, out=fake + 8, cols=1001, rank=1000) == E.LSDSORT_ERR_NO_DEVICE
        assert call(rank=0) == E.LSDSORT_ERR_NO_DEVICE and call(rank=cols - 1) == E.LSDSORT_ERR_NO_DEVICE
        assert call(rows=3, cols=70001, rank=35000) == E.LSDSORT_ERR_NO_DEVICE          # the long tier


def bound(rows, cols):
    """The figure as kth.hip lays it out: control block, 16 B per row, and above 16384 keys per row 2048 counters per row and
    4 B per 16384 keys (at most 2048 chunks per row); every array rounded up to 256 bytes."""
    is_long = cols > 16384
    chunks = min(2048, -(-cols // 16384))
    return 256 + rows * 16 + (rows * (8192 + 4 * chunks) if is_long else 0) + 3 * 255


def test_workspace_figure():
    from lsdradixsort_amd import errors as E

    L = _lib()
    BIG = E.LSDSORT_MAX_KEYS
    f = L.lsdsort_kth_workspace_bytes
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
            # the issue's bound: 8 B per 16384 keys where this layout takes 4
            assert b <= 256 + rows * (16 + 8192 + 8 * -(-cols // 16384)) + 3 * 255, (rows, cols, b)
            if cols >= 16385:                                                             # O(rows), never O(rows * cols):
                assert 4 * b <= 4 * rows * cols, (rows, cols, b)                          # a quarter of the keys' bytes at the most
                assert cols < 65536 or 16 * b <= 4 * rows * cols, (rows, cols, b)         # a sixteenth from 65536 keys per row on
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
    for dtype, key_type in ((torch.int32, "int32"), (torch.int32, "uint32"), (torch.float32, "float32")):
        t = torch.zeros(8, dtype=dtype)
        with pytest.raises(TypeError):
            lsd.GPUKth(t, 1, key_type=key_type)                                  # a CPU tensor
        with pytest.raises(TypeError):
            lsd.kthvalue_rows(t, 1)
        with pytest.raises(TypeError):
            lsd.median_rows(t)
    with pytest.raises(TypeError):
        lsd.GPUKth([3, 1, 2], 1)
    with pytest.raises(TypeError):
        lsd.kthvalue_rows([3, 1, 2], 1)
    with pytest.raises(TypeError):
        lsd.median_rows([3, 1, 2])


def test_dtype_key_type_rank_and_k(no_library):
    """Wrong dtype, a key type this entry does not have, a 3-D or non-contiguous input, a rank outside 0 .. cols - 1 and k outside
    1 .. cols -- checked on tensors that pass for CUDA tensors, so that the test needs no device."""
    import torch

    lsd = no_library

    def fake(dtype, shape=(2, 4)):
        return torch.zeros(shape, dtype=dtype).as_subclass(FakeCuda)

    for dtype in (torch.int16, torch.float16, torch.bfloat16, torch.int64, torch.float64, torch.uint8):
        with pytest.raises(TypeError):
            lsd.GPUKth(fake(dtype), 1)
        with pytest.raises(TypeError):
            lsd.kthvalue_rows(fake(dtype), 1)
        with pytest.raises(TypeError):
            lsd.median_rows(fake(dtype))
    for dtype in (torch.int32, torch.float32):
        for key_type in ("int16", "float16", "bfloat16", "uint64", "int64", "float64", "double", ""):
            with pytest.raises(ValueError):
                lsd.GPUKth(fake(dtype), 1, key_type=key_type)                    # a dtype / key_type mismatch: no such 32-bit type
        with pytest.raises(TypeError):
            lsd.GPUKth(fake(dtype, (2, 2, 2)), 1, key_type="float32")            # 1-D or 2-D only
        with pytest.raises(TypeError):
            lsd.GPUKth(fake(dtype, (4, 4)).t(), 1, key_type="float32")           # contiguous only
        for rank in (-1, 4, 5, 100):
            with pytest.raises(ValueError):
                lsd.GPUKth(fake(dtype), rank, key_type="float32")
            with pytest.raises(ValueError):
                lsd.GPUKth(fake(dtype, (4,)), rank, key_type="float32", largest=True)
    for key_type in ("uint32", "int32"):
        with pytest.raises(TypeError):
            lsd.GPUKth(fake(torch.float32), 1, key_type=key_type)                # a float32 tensor is float32 keys, nothing else
    with pytest.raises(TypeError):
        lsd.GPUKth(fake(torch.float32), 1)                                       # ... the default key type included
    for dtype in (torch.int32, torch.float32):
        for k in (-1, 0, 5, 100):
            with pytest.raises(ValueError):
                lsd.kthvalue_rows(fake(dtype, (3, 2, 4)), k)
            with pytest.raises(ValueError):
                lsd.kthvalue_rows(fake(dtype, (4,)), k)
        with pytest.raises(ValueError):
            lsd.median_rows(fake(dtype, (3, 0)))


def test_kth_kernels_no_scratch_no_spill():
    if hipcc() is None:
        pytest.skip("no hipcc on this machine")
    res = kernel_resources("kth.hip")
    names = list(res)
    once = ("kth_clear_kernel", "kth_count_kernel", "pick_rows_kernelINS0_3KthE", "kth_locate_kernel")   # the pick: radix_select.hpp's, as Kth
    for must in once:
        assert sum(must in name for name in names) == 1, (must, names)
    assert sum("kth_short_kernel" in name for name in names) == 2, names                  # one wavefront, one workgroup
    for must in ("kth_hist_kernel", "kth_scan_kernel"):                                   # three digit levels each
        assert sum(must in name for name in names) == 3, (must, names)
    assert len(names) == len(once) + 2 + 6, names
    assert all("kth_" in name or "_kernelINS0_3KthE" in name for name in names), names   # every kernel names its unit
    for name, r in res.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r)
