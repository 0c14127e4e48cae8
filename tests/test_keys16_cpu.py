"""CPU suite: the 16-bit sort's C-ABI surface (lsdsort_keys16_device and its three companions), its argument checks without a
device, its workspace figure, the Python wrappers' own argument errors, and the resources of every kernel of keys16.hip from
hipcc's own remarks."""
import os
import re

import pytest

from _faces import FakeCuda, lib as _lib, no_library
from _kernel_resources import hipcc, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U16, I16, F16, BF16 = range(4)
ENTRIES = ("lsdsort_keys16_workspace_bytes", "lsdsort_keys16_device", "lsdsort_keys16_check_device", "lsdsort_set_keys16_route")


def test_header_ctypes_table_and_faces_have_the_entries():
    from lsdradixsort_amd import _lib as binding
    from lsdradixsort_amd import errors as E

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsdsort.h")).read(), flags=re.S)
    for name in ENTRIES:
        assert re.search(r"LSDSORT_API\s+[\w\s\*]+?\b" + name + r"\s*\(", text), name
        assert name in binding.SIGNATURES
        assert hasattr(_lib(), name)
    body = re.search(r"typedef\s+enum\s+lsdsort_key16_type\s*\{(.*?)\}\s*lsdsort_key16_type\s*;", text, flags=re.S).group(1)
    enum = {k: int(v) for k, v in re.findall(r"(LSDSORT_KEY16_\w+)\s*=\s*(\d+)", body)}
    assert enum == {"LSDSORT_KEY16_U16": 0, "LSDSORT_KEY16_I16": 1, "LSDSORT_KEY16_F16": 2, "LSDSORT_KEY16_BF16": 3}
    for name, value in enum.items():
        assert getattr(E, name) == value
    assert E.KEY_TYPES_16 == {"uint16": enum["LSDSORT_KEY16_U16"], "int16": enum["LSDSORT_KEY16_I16"],
                              "float16": enum["LSDSORT_KEY16_F16"], "bfloat16": enum["LSDSORT_KEY16_BF16"]}
    # the 32- and 64-bit enum keeps its six enumerators
    old = re.search(r"typedef\s+enum\s+lsdsort_key_type\s*\{(.*?)\}\s*lsdsort_key_type\s*;", text, flags=re.S).group(1)
    assert len(re.findall(r"LSDSORT_KEY_\w+\s*=", old)) == 6
    hpp = open(os.path.join(ROOT, "include", "lsdsort.hpp")).read()
    for ctype in ("uint16_t", "int16_t"):
        assert re.search(r"inline\s+void\s+sort16_device\s*\(\s*%s\s*\*" % ctype, hpp), ctype
    import lsdradixsort_amd as lsd

    for name in ("GPUSort16", "sort16", "keys16_workspace_bytes", "set_keys16_route"):
        assert callable(getattr(lsd, name)) and name in lsd.api.__all__, name


def test_argument_checks_in_entry_order():
    from lsdradixsort_amd import errors as E

    L = _lib()
    n = 1000
    fake = 1 << 20   # never dereferenced: every call below returns before a device is touched
    BIG = E.LSDSORT_MAX_KEYS

    def call(keys=fake, vals=None, w=fake, wb=None, n=n, kt=I16, desc=0):
        if wb is None:
            wb = L.lsdsort_keys16_workspace_bytes(min(n, BIG), 1 if vals else 0)
        return L.lsdsort_keys16_device(keys, vals, w, wb, n, kt, desc, None)

    # 1. key type, before everything else
    for kt in (-1, 4, 5, 100):
        assert call(kt=kt, n=BIG + 1, keys=None, w=None) == E.LSDSORT_ERR_INVALID_ARG, kt
        assert call(kt=kt, n=0) == E.LSDSORT_ERR_INVALID_ARG, kt
    # 2. size, before the empty call, the pointers and the workspace
    assert call(n=BIG + 1, keys=None, w=None) == E.LSDSORT_ERR_TOO_LARGE
    # 3. nothing to do, before the pointers and the workspace
    for kt in (U16, I16, F16, BF16):
        for desc in (0, 1):
            assert call(n=0, kt=kt, desc=desc, keys=None, w=None, wb=0) == E.LSDSORT_OK
    # 4. the keys, before the workspace
    assert call(keys=None, w=None) == E.LSDSORT_ERR_INVALID_ARG
    assert call(keys=None, vals=fake, w=None) == E.LSDSORT_ERR_INVALID_ARG
    assert call(keys=fake + 1, w=None) == E.LSDSORT_ERR_INVALID_ARG                      # 2-byte alignment is the least
    # 5. workspace: exactly lsdsort_keys16_workspace_bytes(n, pairs)
    assert call(w=None) == E.LSDSORT_ERR_WORKSPACE
    assert call(w=fake + 128) == E.LSDSORT_ERR_WORKSPACE                                # misaligned
    for vals in (None, fake):
        need = L.lsdsort_keys16_workspace_bytes(n, 1 if vals else 0)
        assert need > 0 and call(vals=vals, wb=need - 1) == E.LSDSORT_ERR_WORKSPACE
    assert call(vals=fake, wb=L.lsdsort_keys16_workspace_bytes(n, 0)) == E.LSDSORT_ERR_WORKSPACE   # a keys-only figure for pairs
    # 6. without a gfx950 device the last check answers; with one, this test does not get here on bogus pointers
    import torch

    if not torch.cuda.is_available():
        for kt in (U16, I16, F16, BF16):
            for desc in (0, 1):
                for vals in (None, fake):
                    assert call(kt=kt, desc=desc, vals=vals) == E.LSDSORT_ERR_NO_DEVICE
        assert call(keys=fake + 2) == E.LSDSORT_ERR_NO_DEVICE                           # 2-byte alignment is enough
    # the check entry: its own arguments first, an empty call is clean
    assert L.lsdsort_keys16_check_device(None, n, 0, None) == E.LSDSORT_ERR_WORKSPACE
    assert L.lsdsort_keys16_check_device(fake, n, 2, None) == E.LSDSORT_ERR_INVALID_ARG
    assert L.lsdsort_keys16_check_device(fake, 0, 1, None) == E.LSDSORT_OK


def test_workspace_figure():
    from lsdradixsort_amd import errors as E

    L = _lib()
    ladder = [0, 1, 7, 8, 9, 1000, 16384, 16385, 65535, 65536, 65537, (1 << 20) + 13, 1 << 24, 1 << 28, E.LSDSORT_MAX_KEYS]
    for pairs in (0, 1):
        prev = 0
        for n in ladder:
            b = L.lsdsort_keys16_workspace_bytes(n, pairs)
            assert b > 0 and b % 256 == 0 and b >= prev, (n, pairs, b, prev)
            # both routes: the table of 65536 counters, the widened keys and the sort inside
            assert b >= 4 * 65536 + 4 * n + L.lsdsort_workspace_bytes(n, 8, pairs), (n, pairs)
            prev = b
    for n in ladder:
        assert L.lsdsort_keys16_workspace_bytes(n, 1) >= L.lsdsort_keys16_workspace_bytes(n, 0)
    for pairs in (0, 1):
        assert L.lsdsort_keys16_workspace_bytes(E.LSDSORT_MAX_KEYS + 1, pairs) == 0
    for pairs in (2, -1, 3):
        assert L.lsdsort_keys16_workspace_bytes(1000, pairs) == 0


def test_route_setter():
    from lsdradixsort_amd import errors as E

    L = _lib()
    try:
        for route in (-1, 0, 1):
            assert L.lsdsort_set_keys16_route(route) == E.LSDSORT_OK
        for route in (2, -2, 100):
            assert L.lsdsort_set_keys16_route(route) == E.LSDSORT_ERR_INVALID_ARG
    finally:
        assert L.lsdsort_set_keys16_route(-1) == E.LSDSORT_OK


def test_wrappers_check_their_tensors_before_the_library(no_library):
    import torch

    lsd = no_library
    for dtype in (torch.int16, torch.float16, torch.bfloat16):
        t = torch.zeros(8, dtype=dtype)
        with pytest.raises(TypeError):
            lsd.GPUSort16(t, key_type=str(dtype).replace("torch.", ""))        # a CPU tensor
        with pytest.raises(TypeError):
            lsd.sort16(t)
    with pytest.raises(TypeError):
        lsd.GPUSort16([3, 1, 2])
    with pytest.raises(TypeError):
        lsd.sort16(torch.zeros(8, dtype=torch.int32))


def test_dtype_and_key_type_must_agree(no_library, monkeypatch):
    """A float tensor with an integer key_type, or the reverse, is a TypeError -- checked on tensors that pass for CUDA tensors, so
    that the test needs no device."""
    import torch

    lsd = no_library

    def fake(dtype):
        return torch.zeros(8, dtype=dtype).as_subclass(FakeCuda)

    bad = [(torch.float16, "int16"), (torch.float16, "uint16"), (torch.bfloat16, "int16"), (torch.bfloat16, "float16"),
           (torch.float16, "bfloat16"), (torch.int16, "float16"), (torch.int16, "bfloat16")]
    for dtype, key_type in bad:
        with pytest.raises(TypeError):
            lsd.GPUSort16(fake(dtype), key_type=key_type)
    with pytest.raises(ValueError):
        lsd.GPUSort16(fake(torch.int16), key_type="int32")                      # no key type of this entry at all
    with pytest.raises(TypeError):
        lsd.GPUSort16(fake(torch.int16).view(2, 4), key_type="int16")           # 1-D only


def test_keys16_kernels_no_scratch_no_spill():
    if hipcc() is None:
        pytest.skip("no hipcc on this machine")
    res = kernel_resources("keys16.hip")
    names = list(res)
    for must in ("keys16_count_kernel", "keys16_scan_kernel", "keys16_fill_kernel", "keys16_widen_kernel", "keys16_narrow_kernel"):
        assert sum(must in name for name in names) == 1, (must, names)
    for name, r in res.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r)
