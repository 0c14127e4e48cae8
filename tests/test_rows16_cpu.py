"""CPU suite: the 16-bit row sort's C-ABI surface (lsdsort_rows16_device, its workspace figure and its route setter), its argument
checks without a device, the Python and C++ faces' own argument errors, and the resources of every kernel of rows16.hip from hipcc's
own remarks."""
import os
import re

import pytest

from _faces import FakeCuda, lib as _lib, no_library
from _kernel_resources import hipcc, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U16, I16, F16, BF16 = range(4)
ENTRIES = ("lsdsort_rows16_workspace_bytes", "lsdsort_rows16_device", "lsdsort_set_rows16_route")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsdsort.h")).read(), flags=re.S)


def test_header_ctypes_table_and_faces_have_the_entries():
    from lsdradixsort_amd import _lib as binding
    from lsdradixsort_amd import errors as E

    text = _header()
    for name in ENTRIES:
        assert re.search(r"LSDSORT_API\s+[\w\s\*]+?\b" + name + r"\s*\(", text), name
        assert name in binding.SIGNATURES
        assert hasattr(_lib(), name)
    cap = int(re.search(r"#define\s+LSDSORT_ROWS16_NATIVE_MAX_COLS\s+(\d+)", text).group(1))
    assert cap >= 262144 and E.LSDSORT_ROWS16_NATIVE_MAX_COLS == cap
    hpp = open(os.path.join(ROOT, "include", "lsdsort.hpp")).read()
    assert re.search(r"inline\s+size_t\s+rows16_workspace_bytes\s*\(", hpp)
    for ctype in ("uint16_t", "int16_t"):
        assert re.search(r"inline\s+void\s+sort_rows16_device\s*\(\s*const\s+%s\s*\*" % ctype, hpp), ctype
    import lsdradixsort_amd as lsd

    for name in ("GPUSortRows16", "sort_rows16", "rows16_workspace_bytes", "set_rows16_route"):
        assert callable(getattr(lsd, name)) and name in lsd.api.__all__, name


def test_route_setter_takes_three_values():
    from lsdradixsort_amd import errors as E

    L = _lib()
    try:
        for route in (-1, 0, 1):
            assert L.lsdsort_set_rows16_route(route) == E.LSDSORT_OK
        for route in (-2, 2, 100):
            assert L.lsdsort_set_rows16_route(route) == E.LSDSORT_ERR_INVALID_ARG
    finally:
        L.lsdsort_set_rows16_route(-1)


def test_argument_checks_in_entry_order():
    from lsdradixsort_amd import errors as E

    L = _lib()
    rows, cols = 10, 1000
    fake = 1 << 20   # never dereferenced: every call below returns before a device is touched
    BIG = E.LSDSORT_MAX_KEYS

    def call(keys=fake, out=fake, idx=fake, w=fake, wb=None, rows=rows, cols=cols, kt=BF16, descending=1):
        if wb is None:
            wb = L.lsdsort_rows16_workspace_bytes(rows, cols)
        return L.lsdsort_rows16_device(keys, rows, cols, kt, descending, out, idx, w, wb, None)

    # 1. key type, before everything else
    for kt in (-1, 4, 5, 100):
        assert call(kt=kt, rows=BIG + 1, keys=None, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG, kt
        assert call(kt=kt, rows=0, wb=0) == E.LSDSORT_ERR_INVALID_ARG, kt
        assert call(kt=kt) == E.LSDSORT_ERR_INVALID_ARG, kt
    # 2. size, before the empty call, the pointers and the workspace
    assert call(rows=BIG + 1, cols=1, keys=None, out=None, w=None, wb=0) == E.LSDSORT_ERR_TOO_LARGE
    assert call(rows=BIG + 1, cols=0, keys=None, out=None, w=None, wb=0) == E.LSDSORT_ERR_TOO_LARGE
    assert call(rows=1 << 15, cols=1 << 15, keys=None, out=None, w=None, wb=0) == E.LSDSORT_ERR_TOO_LARGE
    assert call(rows=2, cols=BIG // 2 + 1, keys=None, out=None, w=None, wb=0) == E.LSDSORT_ERR_TOO_LARGE
    # 3. nothing to do, before the pointers and the workspace
    for kt in (U16, I16, F16, BF16):
        for descending in (0, 1):
            for empty in (dict(rows=0), dict(cols=0), dict(rows=0, cols=0)):
                assert call(kt=kt, descending=descending, keys=None, out=None, idx=None, w=None, wb=0, **empty) == E.LSDSORT_OK
    # 4. the keys and the values, before the workspace: NULL or odd
    assert call(keys=None, w=None) == E.LSDSORT_ERR_INVALID_ARG
    assert call(out=None, w=None) == E.LSDSORT_ERR_INVALID_ARG
    assert call(keys=fake + 1, w=None) == E.LSDSORT_ERR_INVALID_ARG                     # 2-byte alignment is the least
    assert call(out=fake + 1, w=None) == E.LSDSORT_ERR_INVALID_ARG
    assert call(keys=fake + 3, out=fake + 2, w=None) == E.LSDSORT_ERR_INVALID_ARG
    assert call(keys=fake + 1, out=fake + 1, w=None) == E.LSDSORT_ERR_INVALID_ARG       # in place, odd
    # 5. workspace: exactly lsdsort_rows16_workspace_bytes(rows, cols)
    assert call(w=None) == E.LSDSORT_ERR_WORKSPACE
    assert call(w=fake + 128) == E.LSDSORT_ERR_WORKSPACE                                # misaligned
    need = L.lsdsort_rows16_workspace_bytes(rows, cols)
    assert need > 0 and call(wb=need - 1) == E.LSDSORT_ERR_WORKSPACE
    assert call(idx=None, wb=need - 1) == E.LSDSORT_ERR_WORKSPACE                       # one figure, with or without indices
    assert call(keys=fake + 2, out=fake + 6, w=None) == E.LSDSORT_ERR_WORKSPACE         # even addresses pass check 4
    # 6. without a gfx950 device the last check answers; with one, this test does not get here on bogus pointers
    import torch

    if not torch.cuda.is_available():
        try:
            for route in (-1, 0, 1):
                assert L.lsdsort_set_rows16_route(route) == E.LSDSORT_OK
                for kt in (U16, I16, F16, BF16):
                    for descending in (0, 1):
                        for idx in (None, fake):
                            assert call(kt=kt, descending=descending, idx=idx) == E.LSDSORT_ERR_NO_DEVICE
                assert call(keys=fake + 2) == E.LSDSORT_ERR_NO_DEVICE                   # 2-byte alignment is enough
                assert call(out=fake + 2) == E.LSDSORT_ERR_NO_DEVICE
                assert call(keys=fake + 14, out=fake + 14, cols=1001) == E.LSDSORT_ERR_NO_DEVICE   # in place
                for cols_ in (5000, 20001, E.LSDSORT_ROWS16_NATIVE_MAX_COLS + 1):       # every size class
                    assert call(rows=2, cols=cols_) == E.LSDSORT_ERR_NO_DEVICE
        finally:
            L.lsdsort_set_rows16_route(-1)


def test_workspace_figure():
    from lsdradixsort_amd import errors as E

    L = _lib()
    BIG = E.LSDSORT_MAX_KEYS
    CAP = E.LSDSORT_ROWS16_NATIVE_MAX_COLS
    f = L.lsdsort_rows16_workspace_bytes
    seg = L.lsdsort_segmented_workspace_bytes
    cols_ladder = [1, 2, 7, 1000, 1023, 1024, 1025, 8192, 16383, 16384, 16385, 65535, 65536, 65537, 131072, CAP - 1, CAP, CAP + 1,
                   (1 << 20) + 13, 1 << 24, BIG]
    rows_ladder = [1, 2, 3, 8, 9, 64, 65, 513, 4096, 4097, 1 << 15, 1 << 20]
    seen = 0
    for rows in rows_ladder:
        prev = 0
        for cols in cols_ladder:
            if rows * cols > BIG:
                assert f(rows, cols) == 0, (rows, cols)
                continue
            b = f(rows, cols)
            assert b > 0 and b % 256 == 0 and b >= prev, (rows, cols, b, prev)           # monotonic in cols
            assert b >= 8 * rows * cols + seg(rows * cols, rows, 1), (rows, cols)         # the widen route's needs
            prev = b
            seen += 1
    assert seen > 100
    for cols in cols_ladder[:-3]:                                                         # monotonic in rows
        prev = 0
        for rows in rows_ladder:
            if rows * cols > BIG:
                break
            b = f(rows, cols)
            assert b >= prev and (b > prev or cols < 256), (rows, cols)                    # below: the rounding to 256 bytes
            prev = b
    try:                                                                                  # one figure whatever the route says
        for route in (0, 1):
            L.lsdsort_set_rows16_route(route)
            for rows, cols in ((3, 700), (3, 9000), (3, 40001), (1, CAP + 1)):
                L.lsdsort_set_rows16_route(-1)
                want = f(rows, cols)
                L.lsdsort_set_rows16_route(route)
                assert f(rows, cols) == want, (route, rows, cols)
    finally:
        L.lsdsort_set_rows16_route(-1)
    assert f(0, 1000) % 256 == 0 and f(10, 0) % 256 == 0
    # above the limits
    assert f(BIG + 1, 1) == 0 and f(1, BIG + 1) == 0 and f(BIG + 1, 0) == 0
    assert f(2, BIG // 2 + 1) == 0 and f(1 << 15, 1 << 15) == 0
    assert f(1, BIG) > 0 and f(BIG, 1) > 0


def test_wrappers_check_their_tensors_before_the_library(no_library):
    import torch

    lsd = no_library
    for dtype in (torch.int16, torch.float16, torch.bfloat16):
        t = torch.zeros(8, dtype=dtype)
        with pytest.raises(TypeError):
            lsd.GPUSortRows16(t, key_type=str(dtype).replace("torch.", ""))      # a CPU tensor
        with pytest.raises(TypeError):
            lsd.sort_rows16(t)
    with pytest.raises(TypeError):
        lsd.GPUSortRows16([3, 1, 2])
    with pytest.raises(TypeError):
        lsd.sort_rows16(torch.zeros(8, dtype=torch.int32))


def test_dtype_key_type_and_out(no_library):
    """Wrong dtype, a dtype / key_type mismatch and an `out` that does not fit -- checked on tensors that pass for CUDA tensors, so
    that the test needs no device."""
    import torch

    lsd = no_library

    def fake(dtype, shape=(2, 4)):
        return torch.zeros(shape, dtype=dtype).as_subclass(FakeCuda)

    for dtype in (torch.int32, torch.float32, torch.int64, torch.uint8):
        with pytest.raises(TypeError):
            lsd.GPUSortRows16(fake(dtype))
        with pytest.raises(TypeError):
            lsd.sort_rows16(fake(dtype))
    bad = [(torch.float16, "int16"), (torch.float16, "uint16"), (torch.bfloat16, "int16"), (torch.bfloat16, "float16"),
           (torch.float16, "bfloat16"), (torch.int16, "float16"), (torch.int16, "bfloat16")]
    for dtype, key_type in bad:
        with pytest.raises(TypeError):
            lsd.GPUSortRows16(fake(dtype), key_type=key_type)
    with pytest.raises(ValueError):
        lsd.GPUSortRows16(fake(torch.int16), key_type="int32")                   # no key type of this entry at all
    with pytest.raises(TypeError):
        lsd.GPUSortRows16(fake(torch.int16, (2, 2, 2)))                          # 1-D or 2-D only
    with pytest.raises(TypeError):
        lsd.GPUSortRows16(fake(torch.int16, (4, 4)).t())                         # contiguous only
    with pytest.raises(TypeError):
        lsd.GPUSortRows16(fake(torch.int16), out=fake(torch.float16))            # out: the keys' dtype
    with pytest.raises(TypeError):
        lsd.GPUSortRows16(fake(torch.int16), out=torch.zeros((2, 4), dtype=torch.int16))   # out: a CUDA tensor
    with pytest.raises(ValueError):
        lsd.GPUSortRows16(fake(torch.int16), out=fake(torch.int16, (4, 2)))      # out: the keys' shape
    with pytest.raises(TypeError):
        lsd.sort_rows16(fake(torch.int16, ()))                                   # at least one dimension


def test_rows16_kernels_no_scratch_no_spill():
    if hipcc() is None:
        pytest.skip("no hipcc on this machine")
    res = kernel_resources("rows16.hip")
    names = list(res)
    once = ("rows16_clear_kernel", "rows16_widen_kernel", "rows16_finish_kernel", "rows16_scan_kernel")
    for must in once:
        assert sum(must in name for name in names) == 1, (must, names)
    for must in ("rows16_local_kernel", "rows16_hist_kernel", "rows16_scatter_kernel"):   # two instantiations each
        assert sum(must in name for name in names) == 2, (must, names)
    assert len(names) == len(once) + 6, names
    for name, r in res.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r)
