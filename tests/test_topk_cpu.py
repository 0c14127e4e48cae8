"""CPU suite: the top-k selection's C-ABI surface, argument checks and workspace sizing without a device, and its kernels'
resources (ScratchSize 0, no VGPR spill) from hipcc's own remarks."""
import os
import re

import pytest

from _faces import lib as _lib
from _kernel_resources import hipcc, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lsdradixsort_amd", "csrc")
NEW = ("lsdsort_topk_workspace_bytes", "lsdsort_topk_device")


def test_header_and_ctypes_table_have_the_topk_entries():
    from lsdradixsort_amd import _lib as binding

    text = open(os.path.join(ROOT, "include", "lsdsort.h")).read()
    for name in NEW:
        assert re.search(r"LSDSORT_API\s+[\w\s\*]+?\b" + name + r"\s*\(", text), name
        assert name in binding.SIGNATURES
        assert hasattr(_lib(), name)
    hpp = open(os.path.join(ROOT, "include", "lsdsort.hpp")).read()
    assert re.search(r"inline\s+void\s+topk\s*\(", hpp) and "lsdsort_topk_device" in hpp
    import lsdradixsort_amd as lsd

    for name in ("GPUTopK", "topk_workspace_bytes", "topk_rows"):
        assert callable(getattr(lsd, name))
    assert "topk" in open(os.path.join(CSRC, "Makefile")).read()


def test_argument_checks_in_entry_order():
    from lsdradixsort_amd import errors as E

    L = _lib()
    rows, cols, k = 10, 1000, 5
    ws = L.lsdsort_topk_workspace_bytes(rows, cols, k)
    assert ws > 0
    fake = 1 << 20   # never dereferenced: every call below returns before a device is touched
    BIG = E.LSDSORT_MAX_KEYS

    def call(keys=fake, rows=rows, cols=cols, k=k, kt=0, largest=1, out=fake, idx=fake, w=fake, wb=ws):
        return L.lsdsort_topk_device(keys, rows, cols, k, kt, largest, out, idx, w, wb, None)

    # 1. key type, before everything else
    assert call(kt=3, rows=BIG + 1, keys=None, w=None) == E.LSDSORT_ERR_INVALID_ARG
    assert call(kt=-1) == E.LSDSORT_ERR_INVALID_ARG
    # 2. size, before k > cols, the zero sizes and the pointers
    assert call(rows=BIG + 1, cols=1, k=2, keys=None) == E.LSDSORT_ERR_TOO_LARGE
    assert call(rows=1, cols=BIG + 1, k=BIG + 2) == E.LSDSORT_ERR_TOO_LARGE
    assert call(rows=1 << 15, cols=1 << 15, k=0) == E.LSDSORT_ERR_TOO_LARGE          # rows * cols = 2^30
    assert call(rows=3, cols=(BIG + 1) // 2, keys=None) == E.LSDSORT_ERR_TOO_LARGE
    # 3. k > cols, before the zero sizes and the pointers
    assert call(k=cols + 1, keys=None, w=None) == E.LSDSORT_ERR_INVALID_ARG
    assert call(rows=0, k=cols + 1) == E.LSDSORT_ERR_INVALID_ARG
    assert call(cols=0, k=1) == E.LSDSORT_ERR_INVALID_ARG
    # 4. nothing to do, before the pointers and the workspace
    assert call(rows=0, keys=None, out=None, w=None) == E.LSDSORT_OK
    assert call(cols=0, k=0, keys=None, out=None, w=None) == E.LSDSORT_OK
    assert call(k=0, keys=None, out=None, w=None) == E.LSDSORT_OK
    # 5. pointers, before the workspace
    assert call(keys=None, w=None) == E.LSDSORT_ERR_INVALID_ARG
    assert call(out=None, w=None) == E.LSDSORT_ERR_INVALID_ARG
    # 6. workspace (a NULL index array is no error: values only)
    assert call(w=None) == E.LSDSORT_ERR_WORKSPACE
    assert call(idx=None, w=None) == E.LSDSORT_ERR_WORKSPACE
    assert call(w=fake + 4) == E.LSDSORT_ERR_WORKSPACE                                 # misaligned
    assert call(wb=ws - 1) == E.LSDSORT_ERR_WORKSPACE
    # 7. without a gfx950 device the last check answers; with one, this test does not get here on bogus pointers
    import torch

    if not torch.cuda.is_available():
        assert call() == E.LSDSORT_ERR_NO_DEVICE
        assert call(idx=None) == E.LSDSORT_ERR_NO_DEVICE
        assert call(rows=1, cols=1 << 28, k=1024, wb=L.lsdsort_topk_workspace_bytes(1, 1 << 28, 1024)) == E.LSDSORT_ERR_NO_DEVICE


def test_workspace_bytes_monotone_multiple_of_256_and_bounded():
    from lsdradixsort_amd import errors as E

    L = _lib()
    BIG = E.LSDSORT_MAX_KEYS
    rows_grid = [0, 1, 2, 7, 64, 513, 4096, 1 << 14, 1 << 20]
    cols_grid = [0, 1, 2, 100, 1023, 1024, 1025, 1365, 1366, 1367, 4096, 16383, 16384, 16385, 21846, 131072, 10 ** 6, (1 << 22) + 3,
                 1 << 26, 1 << 28]
    k_grid = [0, 1, 2, 63, 64, 65, 767, 768, 769, 1024, 1025, 12288, 12289, 16384, 16385, 98304, 98305, 10 ** 6, 1 << 26, 1 << 28]
    f = L.lsdsort_topk_workspace_bytes
    seen = 0
    for r in rows_grid:
        for c in cols_grid:
            if r * c > BIG:
                assert f(r, c, 1) == 0
                continue
            line = [f(r, c, k) for k in k_grid if r * k <= BIG]
            assert line == sorted(line), ("k", r, c, line)
            assert all(v > 0 and v % 256 == 0 for v in line), (r, c, line)
            seen += len(line)
    for r in rows_grid:
        for k in k_grid:
            line = [f(r, c, k) for c in cols_grid if r * c <= BIG and r * k <= BIG]
            assert line == sorted(line), ("cols", r, k, line)
    for c in cols_grid:
        for k in k_grid:
            line = [f(r, c, k) for r in rows_grid if r * c <= BIG and r * k <= BIG]
            assert line == sorted(line), ("rows", c, k, line)
    assert seen > 1000
    assert f(BIG + 1, 1, 1) == 0 and f(1, BIG + 1, 1) == 0 and f(1, 1, BIG + 1) == 0
    assert f(1 << 15, 1 << 15, 1) == 0 and f(1 << 15, 1, 1 << 15) == 0
    assert f(1, BIG, 1) > 0 and f(BIG, 1, 1) > 0
    # the select route's workspace does not grow with the row: counters and chunk counts only
    assert f(1, 1 << 28, 1024) < 1 << 20


def test_topk_kernels_no_scratch():
    if hipcc() is None:
        pytest.skip("no hipcc on this machine")
    res = kernel_resources("topk.hip")
    names = list(res)
    assert sum("topk" in name for name in names) >= 10 and all("topk" in name for name in names), names
    for name, r in res.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, f"{name}: scratch {r['scratch']} B/lane, {r['vgpr_spill']} VGPRs spilled"
