"""CPU suite: the typed 64-bit sort's C-ABI surface (lsdsort_keys64_device), its argument checks without a device, the 32-bit
entries' refusal of the 64-bit key types, and the resources of every kernel of wide.hip from hipcc's own remarks."""
import os
import re

import pytest

from _faces import lib as _lib
from _kernel_resources import hipcc, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32, I32, F32, U64, I64, F64 = range(6)


def test_header_ctypes_table_and_faces_have_the_entry():
    from lsdradixsort_amd import _lib as binding

    text = open(os.path.join(ROOT, "include", "lsdsort.h")).read()
    assert re.search(r"LSDSORT_API\s+int\s+lsdsort_keys64_device\s*\(", text)
    for name, value in (("U64", 3), ("I64", 4), ("F64", 5)):
        assert re.search(r"LSDSORT_KEY_%s\s*=\s*%d\b" % (name, value), text), name
    assert "lsdsort_keys64_device" in binding.SIGNATURES
    assert hasattr(_lib(), "lsdsort_keys64_device")
    hpp = open(os.path.join(ROOT, "include", "lsdsort.hpp")).read()
    for ctype in ("uint64_t", "int64_t", "double"):
        assert re.search(r"inline\s+void\s+sort_device\s*\(\s*%s\s*\*" % ctype, hpp), ctype
    assert "sort_records_device" in hpp and "lsdsort_keys64_device" in hpp
    import lsdradixsort_amd as lsd

    assert callable(lsd.sort64) and "sort64" in lsd.api.__all__


def test_argument_checks_in_entry_order():
    from lsdradixsort_amd import errors as E

    L = _lib()
    n, r = 1000, 8
    fake = 1 << 20   # never dereferenced: every call below returns before a device is touched
    BIG = E.LSDSORT_MAX_KEYS

    def call(keys=fake, vals=fake, vb=64, w=fake, wb=None, n=n, r=r, kt=I64, desc=0):
        if wb is None:
            wb = L.lsdsort_wide_workspace_bytes(min(n, BIG), r if r in (4, 8) else 8, 64, vb if vb in (0, 32, 64) else 0)
        return L.lsdsort_keys64_device(keys, vals, vb, w, wb, n, r, kt, desc, None)

    # 1. key type and payload width, before everything else
    for kt in (U32, I32, F32, -1, 6):
        assert call(kt=kt, n=BIG + 1, r=7, keys=None, w=None) == E.LSDSORT_ERR_INVALID_ARG, kt
    for vb in (16, 8, -32, 128):
        assert call(vb=vb, n=BIG + 1, r=7, keys=None, w=None) == E.LSDSORT_ERR_INVALID_ARG, vb
    # 2. size, before the radix, the pointers and the workspace
    assert call(n=BIG + 1, r=7, keys=None, w=None) == E.LSDSORT_ERR_TOO_LARGE
    # 3. radix, before the empty call, the pointers and the workspace
    assert call(r=7, keys=None, w=None) == E.LSDSORT_ERR_INVALID_ARG
    assert call(r=7, n=0) == E.LSDSORT_ERR_INVALID_ARG
    # 4. nothing to do, before the pointers and the workspace
    for kt in (U64, I64, F64):
        for vb in (0, 32, 64):
            assert call(n=0, kt=kt, vb=vb, keys=None, vals=None, w=None, wb=0, desc=1) == E.LSDSORT_OK
    # 5. pointers, before the workspace
    assert call(keys=None, w=None) == E.LSDSORT_ERR_INVALID_ARG
    assert call(vals=None, vb=64, w=None) == E.LSDSORT_ERR_INVALID_ARG
    assert call(vals=None, vb=32, w=None) == E.LSDSORT_ERR_INVALID_ARG
    # 6. workspace: exactly lsdsort_wide_workspace_bytes(n, radix_bits, 64, val_bits) (keys only: no payload array is asked for)
    assert call(w=None) == E.LSDSORT_ERR_WORKSPACE
    assert call(vals=None, vb=0, w=None) == E.LSDSORT_ERR_WORKSPACE
    assert call(w=fake + 8) == E.LSDSORT_ERR_WORKSPACE                                  # misaligned
    for vb in (0, 32, 64):
        need = L.lsdsort_wide_workspace_bytes(n, r, 64, vb)
        assert need > 0 and call(vb=vb, wb=need - 1) == E.LSDSORT_ERR_WORKSPACE
    # 7. without a gfx950 device the last check answers; with one, this test does not get here on bogus pointers
    import torch

    if not torch.cuda.is_available():
        for kt in (U64, I64, F64):
            for desc in (0, 1):
                for vb in (0, 32, 64):
                    assert call(kt=kt, desc=desc, vb=vb, vals=fake if vb else None) == E.LSDSORT_ERR_NO_DEVICE
        assert call(r=4) == E.LSDSORT_ERR_NO_DEVICE


def test_existing_wide_entries_keep_their_answers():
    """lsdsort_u64_device and lsdsort_records_device are now calls of the typed path: same statuses as before."""
    from lsdradixsort_amd import errors as E

    L = _lib()
    fake = 1 << 20
    wb = L.lsdsort_wide_workspace_bytes(1000, 8, 64, 64)
    assert L.lsdsort_u64_device(None, None, 0, 0, 8, None) == E.LSDSORT_OK
    assert L.lsdsort_u64_device(None, fake, wb, 10, 8, None) == E.LSDSORT_ERR_INVALID_ARG
    assert L.lsdsort_u64_device(fake, None, 0, 10, 8, None) == E.LSDSORT_ERR_WORKSPACE
    assert L.lsdsort_u64_device(fake, fake, wb, E.LSDSORT_MAX_KEYS + 1, 8, None) == E.LSDSORT_ERR_TOO_LARGE
    assert L.lsdsort_records_device(fake, fake, 32, 32, fake, wb, 10, 8, None) == E.LSDSORT_ERR_INVALID_ARG
    assert L.lsdsort_records_device(fake, fake, 64, 0, fake, wb, 10, 8, None) == E.LSDSORT_ERR_INVALID_ARG
    assert L.lsdsort_records_device(fake, fake, 64, 64, fake, wb, 10, 5, None) == E.LSDSORT_ERR_INVALID_ARG
    assert L.lsdsort_records_device(fake, fake, 64, 64, fake, wb - 1, 1000, 8, None) == E.LSDSORT_ERR_WORKSPACE
    assert L.lsdsort_records_device(fake, fake, 32, 64, None, 0, 1000, 8, None) == E.LSDSORT_ERR_WORKSPACE


@pytest.mark.parametrize("kt", [U64, I64, F64])
def test_32_bit_entries_refuse_the_64_bit_key_types(kt):
    from lsdradixsort_amd import errors as E

    L = _lib()
    fake = 1 << 20
    n = 1000
    assert L.lsdsort_keys_device(fake, None, fake, L.lsdsort_workspace_bytes(n, 8, 0), n, 8, kt, 0, None) == E.LSDSORT_ERR_INVALID_ARG
    assert L.lsdsort_segmented_device(fake, None, fake, 4, n, kt, 0, fake, L.lsdsort_segmented_workspace_bytes(n, 4, 0),
                                      None) == E.LSDSORT_ERR_INVALID_ARG
    assert L.lsdsort_topk_device(fake, 4, 250, 5, kt, 1, fake, fake, fake, L.lsdsort_topk_workspace_bytes(4, 250, 5),
                                 None) == E.LSDSORT_ERR_INVALID_ARG


def test_wide_kernels_no_scratch_no_spill():
    if hipcc() is None:
        pytest.skip("no hipcc on this machine")
    res = kernel_resources("wide.hip")
    names = list(res)
    # the payload words' kernels are kept; the keys' kernels come with and without the map
    for must, count in (("split_u64_kernel", 1), ("merge_u64_kernel", 1), ("split_keys64_kernel", 2), ("merge_keys64_kernel", 2)):
        assert sum(must in name for name in names) == count, (must, names)
    for name, r in res.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r)
