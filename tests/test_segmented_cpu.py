"""CPU suite: the segmented sort's C-ABI surface, argument checks and workspace sizing without a device, and its kernels'
resources (ScratchSize 0, no VGPR spill) from hipcc's own remarks."""
import os
import re

import pytest

from _faces import lib as _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lsdsort_segmented_workspace_bytes", "lsdsort_segmented_device")


def test_header_and_ctypes_table_have_the_segmented_entries():
    from lsdradixsort_amd import _lib as binding

    text = open(os.path.join(ROOT, "include", "lsdsort.h")).read()
    for name in NEW:
        assert re.search(r"LSDSORT_API\s+[\w\s\*]+?\b" + name + r"\s*\(", text), name
        assert name in binding.SIGNATURES
        assert hasattr(_lib(), name)
    assert "sort_segments" in open(os.path.join(ROOT, "include", "lsdsort.hpp")).read()
    import lsdradixsort_amd as lsd

    for name in ("GPUSortSegmented", "segmented_workspace_bytes", "sort_rows"):
        assert callable(getattr(lsd, name))


def test_argument_checks_in_entry_order():
    from lsdradixsort_amd import errors as E

    L = _lib()
    ws = L.lsdsort_segmented_workspace_bytes(1000, 10, 0)
    fake = 1 << 20   # never dereferenced: every call below returns before a device is touched
    call = lambda keys, vals, offs, segs, n, kt=0, desc=0, w=fake, wb=ws: L.lsdsort_segmented_device(keys, vals, offs, segs, n, kt, desc, w, wb, None)
    assert call(fake, None, fake, 10, 1000, kt=3) == E.LSDSORT_ERR_INVALID_ARG          # key type
    assert call(fake, None, fake, 10, E.LSDSORT_MAX_KEYS + 1) == E.LSDSORT_ERR_TOO_LARGE
    assert call(fake, None, fake, E.LSDSORT_MAX_KEYS + 1, 10) == E.LSDSORT_ERR_TOO_LARGE
    assert call(None, None, fake, 10, 1000) == E.LSDSORT_ERR_INVALID_ARG
    assert call(fake, None, None, 10, 1000) == E.LSDSORT_ERR_INVALID_ARG
    assert call(None, None, fake, 0, 1000) == E.LSDSORT_ERR_INVALID_ARG                # n > 0 needs keys
    assert call(fake, None, None, 10, 0) == E.LSDSORT_ERR_INVALID_ARG                  # segments need offsets
    assert call(None, None, None, 0, 0) == E.LSDSORT_OK
    assert call(fake, None, fake, 0, 1000) == E.LSDSORT_OK                             # nothing to sort
    assert call(fake, None, fake, 10, 0) == E.LSDSORT_OK
    assert call(fake, None, fake, 10, 1000, w=None) == E.LSDSORT_ERR_WORKSPACE
    assert call(fake, None, fake, 10, 1000, w=fake + 4) == E.LSDSORT_ERR_WORKSPACE     # misaligned
    assert call(fake, None, fake, 10, 1000, wb=ws - 1) == E.LSDSORT_ERR_WORKSPACE
    assert call(fake, fake, fake, 10, 1000) == E.LSDSORT_ERR_WORKSPACE                 # pairs need more
    # without a gfx950 device the last check answers; with one, this test does not get here on bogus pointers
    import torch

    if not torch.cuda.is_available():
        assert call(fake, None, fake, 10, 1000) == E.LSDSORT_ERR_NO_DEVICE


def test_workspace_bytes_monotone_and_bounded():
    from lsdradixsort_amd import errors as E

    L = _lib()
    ns = [0, 1, 2, 100, 1024, 1025, 4096, 4097, 16384, 16385, 10 ** 6, 1 << 28, E.LSDSORT_MAX_KEYS]
    ss = [0, 1, 2, 7, 1000, 10 ** 6, 1 << 28, E.LSDSORT_MAX_KEYS]
    for pairs in (0, 1):
        for s in ss:
            row = [L.lsdsort_segmented_workspace_bytes(n, s, pairs) for n in ns]
            assert row == sorted(row), (s, pairs, row)
        for n in ns:
            col = [L.lsdsort_segmented_workspace_bytes(n, s, pairs) for s in ss]
            assert col == sorted(col), (n, pairs, col)
        assert L.lsdsort_segmented_workspace_bytes(E.LSDSORT_MAX_KEYS + 1, 10, pairs) == 0
        assert L.lsdsort_segmented_workspace_bytes(10, E.LSDSORT_MAX_KEYS + 1, pairs) == 0
    n = 1 << 20
    assert L.lsdsort_segmented_workspace_bytes(n, 64, 1) >= L.lsdsort_segmented_workspace_bytes(n, 64, 0) + 4 * n
    assert L.lsdsort_segmented_workspace_bytes(n, 64, 0) % 256 == 0


@pytest.mark.parametrize("source", ["segmented.hip", "local_sort.hip"])
def test_segmented_kernels_no_scratch(source):
    from _kernel_resources import hipcc, kernel_resources

    if hipcc() is None:
        pytest.skip("no hipcc on this machine")
    seg = {name: r for name, r in kernel_resources(source).items() if "seg" in name}   # seg_*_kernel, segment_sort_kernel
    assert seg, "no segmented-sort kernel in " + source
    for name, r in seg.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, f"{name}: scratch {r['scratch']} B/lane, {r['vgpr_spill']} VGPRs spilled"
