"""CPU suite: the 16-bit top-k's C-ABI surface (lsdsort_topk16_device and its workspace figure), its argument checks without a
device, the Python and C++ faces' own argument errors, and the resources of every kernel of topk16.hip from hipcc's own remarks."""
import os
import re

import pytest

from _faces import FakeCuda, lib as _lib, no_library
from _kernel_resources import hipcc, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U16, I16, F16, BF16 = range(4)
ENTRIES = ("lsdsort_topk16_workspace_bytes", "lsdsort_topk16_device")


def test_header_ctypes_table_and_faces_have_the_entries():
    from lsdradixsort_amd import _lib as binding

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsdsort.h")).read(), flags=re.S)
    for name in ENTRIES:
        assert re.search(r"LSDSORT_API\s+[\w\s\*]+?\b" + name + r"\s*\(", text), name
        assert name in binding.SIGNATURES
        assert hasattr(_lib(), name)
    # the 32-bit entry's signature with 16-bit keys: the two ctypes rows agree
    assert binding.SIGNATURES["lsdsort_topk16_device"] == binding.SIGNATURES["lsdsort_topk_device"]
    assert binding.SIGNATURES["lsdsort_topk16_workspace_bytes"] == binding.SIGNATURES["lsdsort_topk_workspace_bytes"]
    hpp = open(os.path.join(ROOT, "include", "lsdsort.hpp")).read()
    for ctype in ("uint16_t", "int16_t"):
        assert re.search(r"inline\s+void\s+topk16_device\s*\(\s*const\s+%s\s*\*" % ctype, hpp), ctype
    import lsdradixsort_amd as lsd

    for name in ("GPUTopK16", "topk16_rows", "topk16_workspace_bytes"):
        assert callable(getattr(lsd, name)) and name in lsd.api.__all__, name


def test_argument_checks_in_entry_order():
    from lsdradixsort_amd import errors as E

    L = _lib()
    rows, cols, k = 10, 1000, 7
    fake = 1 << 20   # never dereferenced: every call below returns before a device is touched
    BIG = E.LSDSORT_MAX_KEYS

    def call(keys=fake, out=fake, idx=fake, w=fake, wb=None, rows=rows, cols=cols, k=k, kt=BF16, largest=1):
        if wb is None:
            wb = L.lsdsort_topk16_workspace_bytes(rows, cols, k)
        return L.lsdsort_topk16_device(keys, rows, cols, k, kt, largest, out, idx, w, wb, None)

    # 1. key type, before everything else
    for kt in (-1, 4, 5, 100):
        assert call(kt=kt, rows=BIG + 1, keys=None, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG, kt
        assert call(kt=kt, k=cols + 1, wb=0) == E.LSDSORT_ERR_INVALID_ARG, kt
        assert call(kt=kt, rows=0, wb=0) == E.LSDSORT_ERR_INVALID_ARG, kt
    # 2. size, before k, the empty call, the pointers and the workspace
    assert call(rows=BIG + 1, cols=1, k=2, keys=None, out=None, w=None, wb=0) == E.LSDSORT_ERR_TOO_LARGE
    assert call(rows=1 << 15, cols=1 << 15, k=(1 << 15) + 1, keys=None, out=None, w=None, wb=0) == E.LSDSORT_ERR_TOO_LARGE
    assert call(rows=2, cols=BIG // 2 + 1, k=0, keys=None, out=None, w=None, wb=0) == E.LSDSORT_ERR_TOO_LARGE
    # 3. k above the row length, before the empty call, the pointers and the workspace
    assert call(k=cols + 1, keys=None, out=None, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG
    assert call(rows=0, k=cols + 1, keys=None, out=None, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG
    # 4. nothing to do, before the pointers and the workspace
    for kt in (U16, I16, F16, BF16):
        for largest in (0, 1):
            for empty in (dict(rows=0), dict(cols=0, k=0), dict(k=0)):
                assert call(kt=kt, largest=largest, keys=None, out=None, idx=None, w=None, wb=0, **empty) == E.LSDSORT_OK
    # 5. the keys and the values, before the workspace: NULL or odd
    assert call(keys=None, w=None) == E.LSDSORT_ERR_INVALID_ARG
    assert call(out=None, w=None) == E.LSDSORT_ERR_INVALID_ARG
    assert call(keys=fake + 1, w=None) == E.LSDSORT_ERR_INVALID_ARG                     # 2-byte alignment is the least
    assert call(out=fake + 1, w=None) == E.LSDSORT_ERR_INVALID_ARG
    assert call(keys=fake + 3, out=fake + 2, w=None) == E.LSDSORT_ERR_INVALID_ARG
    # 6. workspace: exactly lsdsort_topk16_workspace_bytes(rows, cols, k)
    assert call(w=None) == E.LSDSORT_ERR_WORKSPACE
    assert call(w=fake + 128) == E.LSDSORT_ERR_WORKSPACE                                # misaligned
    need = L.lsdsort_topk16_workspace_bytes(rows, cols, k)
    assert need > 0 and call(wb=need - 1) == E.LSDSORT_ERR_WORKSPACE
    assert call(idx=None, wb=need - 1) == E.LSDSORT_ERR_WORKSPACE                       # one figure, with or without indices
    assert call(keys=fake + 2, out=fake + 6, w=None) == E.LSDSORT_ERR_WORKSPACE         # even addresses pass check 5
    # 7. without a gfx950 device the last check answers; with one, this test does not get here on bogus pointers
    import torch

    if not torch.cuda.is_available():
        for kt in (U16, I16, F16, BF16):
            for largest in (0, 1):
                for idx in (None, fake):
                    assert call(kt=kt, largest=largest, idx=idx) == E.LSDSORT_ERR_NO_DEVICE
        assert call(keys=fake + 2) == E.LSDSORT_ERR_NO_DEVICE                           # 2-byte alignment is enough
        assert call(out=fake + 2) == E.LSDSORT_ERR_NO_DEVICE
        assert call(keys=fake + 14, out=fake + 6, cols=1001) == E.LSDSORT_ERR_NO_DEVICE
        assert call(k=cols) == E.LSDSORT_ERR_NO_DEVICE                                  # the sort route


def test_workspace_figure():
    from lsdradixsort_amd import errors as E

    L = _lib()
    BIG = E.LSDSORT_MAX_KEYS
    f = L.lsdsort_topk16_workspace_bytes
    ladder = [1, 2, 7, 8, 9, 1000, 1024, 1025, 16384, 16385, 65536, 131073, (1 << 20) + 13, 1 << 24, BIG]
    seen = 0
    for rows in (1, 2, 513, 4096, 1 << 20):
        for cols in ladder:
            if rows * cols > BIG:
                assert f(rows, cols, 1) == 0, (rows, cols)
                continue
            prev = 0
            for k in sorted(set(q for q in ladder + [3 * cols // 4, 3 * cols // 4 + 1, cols] if 1 <= q <= cols)):
                b = f(rows, cols, k)
                assert b > 0 and b % 256 == 0 and b >= prev, (rows, cols, k, b, prev)     # monotonic in k
                assert b >= L.lsdsort_segmented_workspace_bytes(rows * k, rows, 1), (rows, cols, k)
                assert b >= 8 * rows * k, (rows, cols, k)                                 # the winners and their positions
                prev = b
                seen += 1
    assert seen > 200
    for k in (1, 50, 1000):                                                               # monotonic in cols and in rows
        prev = 0
        for cols in [c for c in ladder if c >= k]:
            b = f(1, cols, k)
            assert b >= prev, (cols, k)
            prev = b
        prev = 0
        for rows in (1, 2, 3, 64, 65, 513, 4096, 4097, 1 << 15):
            b = f(rows, 16385, k)
            assert b > prev, (rows, k)
            prev = b
    assert f(0, 1000, 10) % 256 == 0 and f(10, 0, 0) % 256 == 0
    # above the limits
    assert f(BIG + 1, 1, 1) == 0 and f(1, BIG + 1, 1) == 0 and f(1, 1, BIG + 1) == 0
    assert f(2, BIG // 2 + 1, 1) == 0 and f(1 << 15, 1 << 15, 1) == 0
    assert f(1, BIG, BIG) > 0 and f(BIG, 1, 1) > 0


def test_wrappers_check_their_tensors_before_the_library(no_library):
    import torch

    lsd = no_library
    for dtype in (torch.int16, torch.float16, torch.bfloat16):
        t = torch.zeros(8, dtype=dtype)
        with pytest.raises(TypeError):
            lsd.GPUTopK16(t, 1, key_type=str(dtype).replace("torch.", ""))      # a CPU tensor
        with pytest.raises(TypeError):
            lsd.topk16_rows(t, 1)
    with pytest.raises(TypeError):
        lsd.GPUTopK16([3, 1, 2], 1)
    with pytest.raises(TypeError):
        lsd.topk16_rows(torch.zeros(8, dtype=torch.int32), 1)


def test_dtype_key_type_and_k(no_library):
    """Wrong dtype, a dtype / key_type mismatch and k outside 0 .. cols -- checked on tensors that pass for CUDA tensors, so that
    the test needs no device."""
    import torch

    lsd = no_library

    def fake(dtype, shape=(2, 4)):
        return torch.zeros(shape, dtype=dtype).as_subclass(FakeCuda)

    for dtype in (torch.int32, torch.float32, torch.int64, torch.uint8):
        with pytest.raises(TypeError):
            lsd.GPUTopK16(fake(dtype), 1)
        with pytest.raises(TypeError):
            lsd.topk16_rows(fake(dtype), 1)
    bad = [(torch.float16, "int16"), (torch.float16, "uint16"), (torch.bfloat16, "int16"), (torch.bfloat16, "float16"),
           (torch.float16, "bfloat16"), (torch.int16, "float16"), (torch.int16, "bfloat16")]
    for dtype, key_type in bad:
        with pytest.raises(TypeError):
            lsd.GPUTopK16(fake(dtype), 1, key_type=key_type)
    with pytest.raises(ValueError):
        lsd.GPUTopK16(fake(torch.int16), 1, key_type="int32")                   # no key type of this entry at all
    with pytest.raises(TypeError):
        lsd.GPUTopK16(fake(torch.int16, (2, 2, 2)), 1)                          # 1-D or 2-D only
    with pytest.raises(TypeError):
        lsd.GPUTopK16(fake(torch.int16, (4, 4)).t(), 1)                         # contiguous only
    for k in (-1, 5, 100):
        with pytest.raises(ValueError):
            lsd.GPUTopK16(fake(torch.int16), k)
        with pytest.raises(ValueError):
            lsd.GPUTopK16(fake(torch.bfloat16, (4,)), k, key_type="bfloat16")
        with pytest.raises(ValueError):
            lsd.topk16_rows(fake(torch.float16, (3, 2, 4)), k)


def test_topk16_kernels_no_scratch_no_spill():
    if hipcc() is None:
        pytest.skip("no hipcc on this machine")
    res = kernel_resources("topk16.hip")
    names = list(res)
    once = ("topk16_clear_kernel", "topk16_count_kernel", "topk16_write_kernel", "topk16_offsets_kernel", "topk16_widen_kernel",
            "topk16_finish_kernel")
    for must in once:
        assert sum(must in name for name in names) == 1, (must, names)
    for must in ("topk16_short_kernel", "topk16_hist_kernel", "topk16_scan_kernel"):     # two instantiations each
        assert sum(must in name for name in names) == 2, (must, names)
    assert len(names) == len(once) + 6, names
    for name, r in res.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r)
