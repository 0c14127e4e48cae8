"""CPU suite: the top-p filter for 16-bit rows (topp16.hip) -- its C-ABI surface (lsdsort_topp16_filter_device and its workspace
figure), its argument checks without a device, the Python face's own argument errors and host conversions (GPUTopP16Filter,
topp16_filter_rows), the float64 oracle and acceptance rule of tests/_topp16.py on hand-computed rows and on the sharp rows of the GPU
suite, and the resources of every kernel of the unit from hipcc's own remarks."""
import json
import math
import os
import re

import numpy as np
import pytest

import _topp16 as tp
from _faces import FakeCuda, lib as _lib, no_library
from _kernel_resources import hipcc, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "kernel_resources_topp16.json")
U16, I16, F16, BF16 = range(4)
ENTRIES = ("lsdsort_topp16_filter_workspace_bytes", "lsdsort_topp16_filter_device")
NAMES = ("GPUTopP16Filter", "topp16_filter_workspace_bytes", "topp16_filter_rows")


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
    flt = binding.SIGNATURES["lsdsort_topp16_filter_device"]
    assert flt[0] == binding.c_int and len(flt[1]) == 10 and flt[1][5] == ctypes.c_uint16
    assert binding.SIGNATURES[ENTRIES[0]] == (binding.c_size, [binding.c_size] * 2)
    doc = header[header.index("Top-p (nucleus) FILTER"):header.index("lsdsort_topp16_filter_workspace_bytes(size_t")]
    for word in ("graph", "DETERMINISTIC", "lsdsort_topk16_filter_device", "in place", "2^-12"):   # the contract's points
        assert word in doc, word
    for name in NAMES:
        assert callable(getattr(lsd, name)) and name in lsd.api.__all__, name
    makefile = open(os.path.join(ROOT, "lsdradixsort_amd", "csrc", "Makefile")).read()
    assert "topp16" in re.search(r"^NAMES\s*:=(.*)$", makefile, flags=re.M).group(1).split()
    assert "topp16" not in open(os.path.join(ROOT, "include", "lsdsort.hpp")).read()     # no wrapper in the C++ face


def test_argument_checks_in_entry_order():
    from lsdradixsort_amd import errors as E

    L = _lib()
    rows, cols = 10, 1000
    fake = 1 << 20   # never dereferenced: every call below returns before a device is touched
    BIG = E.LSDSORT_MAX_KEYS

    def call(keys=fake, p=fake, out=fake + (1 << 16), w=fake, wb=None, rows=rows, cols=cols, kt=BF16, fill=0xFF80):
        if wb is None:
            wb = L.lsdsort_topp16_filter_workspace_bytes(rows, cols)
        return L.lsdsort_topp16_filter_device(keys, rows, cols, p, kt, fill, out, w, wb, None)

    # 1. key type, before everything else: float16 and bfloat16 only
    for kt in (-1, U16, I16, 4, 5, 100):
        assert call(kt=kt, rows=BIG + 1, keys=None, p=None, out=None, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG, kt
        assert call(kt=kt, rows=0, wb=0) == E.LSDSORT_ERR_INVALID_ARG, kt
        assert call(kt=kt) == E.LSDSORT_ERR_INVALID_ARG, kt
    # 2. sizes, before the empty call, the pointers and the workspace
    assert call(rows=BIG + 1, cols=1, keys=None, p=None, out=None, w=None, wb=0) == E.LSDSORT_ERR_TOO_LARGE
    assert call(rows=1 << 15, cols=1 << 15, keys=None, p=fake + 1, out=None, w=None, wb=0) == E.LSDSORT_ERR_TOO_LARGE
    assert call(rows=2, cols=BIG // 2 + 1, keys=fake + 1, out=None, w=None, wb=0) == E.LSDSORT_ERR_TOO_LARGE
    # 3. nothing to do
    for kt in (F16, BF16):
        assert call(kt=kt, rows=0, keys=None, p=None, out=None, w=None, wb=0) == E.LSDSORT_OK
        assert call(kt=kt, cols=0, keys=fake + 1, p=fake + 2, out=fake + 1, w=None, wb=0) == E.LSDSORT_OK
    # 4. NULL or odd d_keys or d_out; then NULL or misaligned d_p
    assert call(keys=None, p=None, w=None) == E.LSDSORT_ERR_INVALID_ARG
    assert call(out=None, w=None) == E.LSDSORT_ERR_INVALID_ARG
    assert call(p=None, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG
    for off in (1, 3, 7, 15):
        assert call(keys=fake + off, w=None) == E.LSDSORT_ERR_INVALID_ARG, off
        assert call(out=fake + off, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG, off
    for off in (1, 2, 3, 6, 13):
        assert call(p=fake + off, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG, off
    # 5. workspace: exactly lsdsort_topp16_filter_workspace_bytes(rows, cols)
    assert call(w=None) == E.LSDSORT_ERR_WORKSPACE
    assert call(w=fake + 128) == E.LSDSORT_ERR_WORKSPACE
    need = L.lsdsort_topp16_filter_workspace_bytes(rows, cols)
    assert need > 0 and call(wb=need - 1) == E.LSDSORT_ERR_WORKSPACE
    assert call(out=fake, wb=need - 1) == E.LSDSORT_ERR_WORKSPACE                       # in place passes check 4
    for src in (2, 6, 14):
        for dst in (0, 4, 10):
            assert call(keys=fake + src, out=fake + (1 << 16) + dst, w=None) == E.LSDSORT_ERR_WORKSPACE, (src, dst)   # alignments may differ
    assert call(rows=3, cols=70001, wb=L.lsdsort_topp16_filter_workspace_bytes(3, 70001) - 1) == E.LSDSORT_ERR_WORKSPACE
    # 6. the device
    import torch

    if not torch.cuda.is_available():
        for kt in (F16, BF16):
            for fill in (0, 0x7E7E, 0xFFFF):
                assert call(kt=kt, fill=fill) == E.LSDSORT_ERR_NO_DEVICE
            assert call(kt=kt, rows=3, cols=70001) == E.LSDSORT_ERR_NO_DEVICE
        assert call(out=fake) == E.LSDSORT_ERR_NO_DEVICE                                # in place
        assert call(keys=fake + 14, out=fake + 6, p=fake + 12, cols=1001) == E.LSDSORT_ERR_NO_DEVICE


# (rows, cols) -> bytes: the top-k filter's figure (control block 256, 16 B per row, above 16384 keys per row 8 KiB of counters per
# row) and above 16384 keys per row 16 KiB of mass bins per row; every array rounded up to 256 bytes
PINNED = {(1, 1): 512, (10, 1000): 512, (17, 1000): 768, (3, 16384): 512, (3, 16385): 74240, (3, 70001): 74240, (128, 128256): 3148032,
          (1, (1 << 20) + 13): 25088, (4096, 131072): 100729088}


def test_workspace_figure():
    from lsdradixsort_amd import errors as E

    L = _lib()
    BIG = E.LSDSORT_MAX_KEYS
    f, flt = L.lsdsort_topp16_filter_workspace_bytes, L.lsdsort_topk16_filter_workspace_bytes
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
            if cols <= 16384:
                assert b == flt(rows, cols), (rows, cols, b)                              # the filter's figure
            else:
                assert b == flt(rows, cols) + rows * 16384, (rows, cols, b)               # 16 KiB of mass bins per row on top of it
                assert 2 * b <= 2 * rows * cols * 2, (rows, cols, b)                      # O(rows), never O(rows * cols)
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
    assert f(1, 16385) > f(1, 16384) and f(2, 1 << 24) > f(1, 1 << 24) and f(3, 70001) == f(3, 16385)
    assert f(0, 1000) % 256 == 0 and f(10, 0) % 256 == 0
    assert f(BIG + 1, 1) == 0 and f(1, BIG + 1) == 0 and f(BIG + 1, 0) == 0
    assert f(2, BIG // 2 + 1) == 0 and f(1 << 15, 1 << 15) == 0
    assert f(1, BIG) > 0 and f(BIG, 1) > 0
    for (rows, cols), want in PINNED.items():
        assert f(rows, cols) == want, (rows, cols, f(rows, cols), want)


def test_wrappers_check_their_arguments_before_the_library(no_library):
    import torch

    lsd = no_library

    def fake(dtype, shape=(2, 4)):
        return torch.zeros(shape, dtype=dtype).as_subclass(FakeCuda)

    p2 = fake(torch.float32, (2,))
    for dtype in (torch.float16, torch.bfloat16):
        ok = str(dtype).replace("torch.", "")
        with pytest.raises(TypeError):
            lsd.GPUTopP16Filter(torch.zeros((2, 4), dtype=dtype), p2, key_type=ok)       # a CPU tensor
        with pytest.raises(TypeError):
            lsd.topp16_filter_rows(torch.zeros((2, 4), dtype=dtype), 0.9)
        other = "float16" if ok == "bfloat16" else "bfloat16"
        with pytest.raises(TypeError):
            lsd.GPUTopP16Filter(fake(dtype), p2, key_type=other)                         # a key type that does not fit the dtype
        for key_type in ("int16", "uint16", "float32", "half", ""):
            with pytest.raises(ValueError):
                lsd.GPUTopP16Filter(fake(dtype), p2, key_type=key_type)                  # a key type this entry does not have
        with pytest.raises(TypeError):
            lsd.GPUTopP16Filter(fake(dtype, (2, 2, 2)), p2, key_type=ok)                 # 1-D or 2-D only
        with pytest.raises(TypeError):
            lsd.GPUTopP16Filter(fake(dtype, (4, 4)).t(), fake(torch.float32, (4,)), key_type=ok)   # contiguous only
        for bad in (torch.zeros(2, dtype=torch.float32), fake(torch.float64, (2,)), fake(torch.int32, (2,)), [0.5, 0.5], 0.5, None,
                    fake(torch.float32, (4,))[::2]):
            with pytest.raises(TypeError):
                lsd.GPUTopP16Filter(fake(dtype), bad, key_type=ok)                       # d_p: a contiguous float32 CUDA tensor
        for count in (0, 1, 3, 8):
            with pytest.raises(ValueError):
                lsd.GPUTopP16Filter(fake(dtype), fake(torch.float32, (count,)), key_type=ok)
        with pytest.raises(ValueError):
            lsd.GPUTopP16Filter(fake(dtype, (4,)), p2, key_type=ok)                      # 1-D input: one row
        for fill in (-1, 0x10000, 1.5, "0", True):
            with pytest.raises(ValueError):
                lsd.GPUTopP16Filter(fake(dtype), p2, key_type=ok, fill=fill)
        wrong = torch.float16 if dtype != torch.float16 else torch.bfloat16
        for out in (fake(dtype, (2, 5)), fake(dtype, (8,)), fake(wrong), torch.zeros((2, 4), dtype=dtype)):
            with pytest.raises((TypeError, ValueError)):
                lsd.GPUTopP16Filter(fake(dtype), p2, key_type=ok, out=out)
        x = fake(dtype, (3, 2, 4))
        for p in ("0.9", None, True, fake(torch.int32, (6,)), fake(torch.float16, (6,)), ["a"] * 6):
            with pytest.raises(TypeError):
                lsd.topp16_filter_rows(x, p)
        for p in ([0.5, 0.5], [0.5] * 7, fake(torch.float32, (5,)), fake(torch.float64, (2, 3, 4))):
            with pytest.raises(ValueError):
                lsd.topp16_filter_rows(x, p)
        with pytest.raises(TypeError):
            lsd.topp16_filter_rows(fake(dtype, ()), 0.9)                                 # at least one dimension
        with pytest.raises(TypeError):
            lsd.topp16_filter_rows(fake(dtype, (4, 4)).t(), 0.9, inplace=True)           # in place: contiguous only
        # empty shapes: nothing to do, the library is not reached
        for shape in ((0, 4), (3, 0), (2, 0, 5)):
            e = fake(dtype, shape)
            assert lsd.topp16_filter_rows(e, 0.9).shape == e.shape and lsd.topp16_filter_rows(e, 0.9, inplace=True) is e
    for dtype in (torch.int16, torch.float32, torch.int32):
        with pytest.raises(TypeError):
            lsd.topp16_filter_rows(fake(dtype), 0.9)
        with pytest.raises(TypeError):
            lsd.GPUTopP16Filter(fake(dtype), p2, key_type="bfloat16")


def test_host_conversions_of_p_and_fill(no_library):
    import torch

    api = no_library.api
    vec = api._p_per_row
    for p, want in ((0.9, [0.9] * 4), (1, [1.0] * 4), (0, [0.0] * 4), (-2.5, [-2.5] * 4), ([0.1, 0.5, 1.0, 2.0], [0.1, 0.5, 1.0, 2.0]),
                    ((0.25, 0.5, 0.75, 1), [0.25, 0.5, 0.75, 1.0]), (np.array([0.5, 0.25, 0.125, 0.0]), [0.5, 0.25, 0.125, 0.0]),
                    (torch.tensor([0.1, 0.2, 0.3, 0.4], dtype=torch.float64), [0.1, 0.2, 0.3, 0.4]),
                    (torch.tensor([[0.5, 0.25], [0.75, 1.5]]), [0.5, 0.25, 0.75, 1.5])):
        got = vec(p, 4, "cpu")
        assert got.dtype == torch.float32 and got.shape == (4,) and got.is_contiguous(), p
        assert got.tolist() == [float(np.float32(v)) for v in want], (p, got)
    assert math.isnan(vec(float("nan"), 2, "cpu")[1].item())
    own = torch.tensor([0.9, 0.8, 0.7, 0.6], dtype=torch.float32)
    assert vec(own, 4, "cpu").data_ptr() == own.data_ptr()                                 # used as it is
    for p in (torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.float16), "0.9", None, True):
        with pytest.raises(TypeError):
            vec(p, 4, "cpu")
    for p in ([0.1, 0.2, 0.3], torch.zeros(5), []):
        with pytest.raises(ValueError):
            vec(p, 4, "cpu")
    bits = api._fill_bits16
    assert bits(torch.bfloat16, None, True) == 0xFF80 and bits(torch.float16, None, True) == 0xFC00   # -inf
    assert bits(torch.bfloat16, -1.0, True) == 0xBF80 and bits(torch.float16, -1.0, True) == 0xBC00
    assert bits(torch.bfloat16, float("-inf"), True) == 0xFF80 and bits(torch.float16, 0.0, True) == 0


# ---- the oracle itself -----------------------------------------------------------------------------------------------------------
def _row(values, key_type="bfloat16"):
    return tp.bits_of_values(np.array(values, dtype=np.float32), key_type)


def _kept(row, p, key_type="bfloat16"):
    out = tp.filter_np(row[None, :], np.array([p], dtype=np.float32), key_type)[0]
    return (out != tp.FILL).tolist()


@pytest.mark.parametrize("key_type", tp.TYPES)
def test_the_oracle_on_hand_computed_rows(key_type):
    # [ln 4, ln 2, 0, 0] in exact arithmetic has weights 4 : 2 : 1 : 1 of 8, A = 0, 1/2, 3/4, 3/4.  The 16-bit roundings of ln 4 and
    # ln 2 move them by less than 1 %, so p is kept 5 % away from the steps
    row = _row([math.log(4), math.log(2), 0.0, 0.0], key_type)
    s, mass, A, Z = tp.groups(row, key_type)
    assert s.size == 3 and np.allclose(mass / Z, [0.5, 0.25, 0.25], atol=0.01) and np.allclose(A / Z, [0, 0.5, 0.75], atol=0.01)
    assert mass[0] == 1.0 and abs(Z - 2.0) < 0.02                                          # w = 1 at the maximum
    for p, want in ((0.0, [1, 0, 0, 0]), (-1.0, [1, 0, 0, 0]), (1e-30, [1, 0, 0, 0]), (0.3, [1, 0, 0, 0]), (0.45, [1, 0, 0, 0]),
                    (0.55, [1, 1, 0, 0]), (0.7, [1, 1, 0, 0]), (0.8, [1, 1, 1, 1]), (0.999, [1, 1, 1, 1])):
        assert _kept(row, p, key_type) == [bool(x) for x in want], p
    for p in (1.0, 1.5, float("nan")):
        assert tp.is_off(p) and np.array_equal(tp.filter_np(row[None, :], np.array([p], dtype=np.float32), key_type)[0], row)
    assert not tp.is_off(0.0) and not tp.is_off(-1.0) and not tp.is_off(1.0 - 2.0 ** -24)
    pinf, ninf = tp.POS_INF[key_type], tp.NEG_INF[key_type]
    # +inf: the two +inf carry all the mass (x == m), every number has none; a +NaN is the best value and weighs nothing
    row = np.array([pinf, _row([3.0], key_type)[0], pinf, ninf, 0x7FFF, 0xFFFF], dtype=np.uint16)
    s, mass, A, Z = tp.groups(row, key_type)
    assert Z == 2.0 and mass.tolist() == [0, 2, 0, 0, 0] and A.tolist() == [0, 0, 2, 2, 2]
    assert _kept(row, 0.5, key_type) == [True, False, True, False, True, False]
    assert _kept(row, 0.0, key_type) == [False, False, False, False, True, False]          # the best value alone: the +NaN
    # all -inf: every key is the maximum
    row = np.full(5, ninf, dtype=np.uint16)
    assert tp.groups(row, key_type)[3] == 5.0 and _kept(row, 0.1, key_type) == [True] * 5
    # all NaN: no mass at all, the best value is kept
    row = np.array([0xFFFF, 0x7FFF, ninf + 1, 0x7FFF], dtype=np.uint16)
    assert tp.groups(row, key_type)[3] == 0.0 and _kept(row, 0.9, key_type) == [False, True, False, True]
    # one key
    for p in (0.0, 0.5, -3.0):
        assert _kept(_row([-5.0], key_type), p, key_type) == [True]
    # -0.0 ranks below +0.0 and weighs the same
    row = np.array([0x8000, 0x0000], dtype=np.uint16)
    assert _kept(row, 0.4, key_type) == [False, True] and _kept(row, 0.6, key_type) == [True, True]
    # the acceptance rule: within the tolerance both neighbours pass, outside it one does
    row = _row([1.0, 0.0], key_type)
    s, mass, A, Z = tp.groups(row, key_type)
    step = np.float32(mass[0] / Z)
    assert len(tp.acceptable(row, step, key_type)) == 2 and len(tp.acceptable(row, step + np.float32(0.01), key_type)) == 1
    good = np.array([row[0], tp.FILL], dtype=np.uint16)
    assert tp.check_row(good, row, 0.5, key_type) is None and tp.check_row(row, row, 0.5, key_type) is not None
    assert tp.check_row(np.array([tp.FILL, row[1]], dtype=np.uint16), row, 0.5, key_type) is not None   # not a set of best keys
    assert tp.check_row(np.array([tp.FILL, tp.FILL], dtype=np.uint16), row, 0.5, key_type) is not None
    assert tp.check_row(row, row, 1.0, key_type) is None and tp.check_row(good, row, 1.0, key_type) is not None


@pytest.mark.parametrize("key_type", tp.TYPES)
@pytest.mark.parametrize("name", sorted(tp.SHARP_SETS))
def test_sharp_rows_have_exactly_one_acceptable_threshold(name, key_type):
    cases = 0
    for cols in (64, 257, 1024, 1025, 16384, 16385, 40000):
        keys, p = tp.sharp_rows(name, cols, key_type, seed=cols)
        assert keys.shape == (tp.SHARP_SETS[name].size, cols) and p.dtype == np.float32  # one row per level, every level present
        tp.assert_sharp(keys, p, key_type)
        s, mass, A, Z = tp.groups(keys[0], key_type)
        assert mass.min() / Z > 0.01 > 4 * tp.M                                            # every value carries mass far above M
        kept = (tp.filter_np(keys, p, key_type) != tp.FILL).sum(axis=1)
        assert (np.diff(kept) > 0).all() and kept[-1] == cols                              # value j in turn is the threshold
        cases += keys.shape[0]
    assert cases >= 21


# ---- kernel resources ------------------------------------------------------------------------------------------------------------
def test_kernels_no_scratch_no_spill_and_recorded_resources():
    if hipcc() is None:
        pytest.skip("no hipcc on this machine")
    res = kernel_resources("topp16.hip")
    names = list(res)
    once = ("topp16_clear_kernel", "topp16_best_kernel", "topp16_mass_kernel", "topp16_scan0_kernel", "topp16_count_kernel",
            "topp16_scan1_kernel", "topp16_apply_kernel")
    for must in once:
        assert sum(must in name for name in names) == 1, (must, names)
    assert sum("topp16_short_kernel" in name for name in names) == 2, names                # wavefront / workgroup
    assert len(names) == len(once) + 2, names
    for name, r in res.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r)
    want = json.load(open(GOLDEN))["topp16.hip"]
    assert sorted(res) == sorted(want), f"kernels gone: {sorted(set(want) - set(res))}, new: {sorted(set(res) - set(want))}"
    for name, w in want.items():
        assert res[name]["occupancy"] >= w["occupancy"], f"{name}: {res[name]['occupancy']} waves/SIMD, recorded {w['occupancy']}"
        assert res[name]["lds_bytes"] == w["lds_bytes"], f"{name}: {res[name]['lds_bytes']} B of static LDS, recorded {w['lds_bytes']}"


def test_the_unit_includes_the_shared_headers_only_and_has_no_inline_assembly():
    text = open(os.path.join(ROOT, "lsdradixsort_amd", "csrc", "topp16.hip")).read()
    assert set(re.findall(r'#include "([^"]+)"', text)) == {"../../include/lsdsort.h", "keys16_map.hpp", "lsd_device.hpp", "lsd_host.hpp",
                                                             "mass_rows16.hpp", "radix_select.hpp", "select_tiles16.hpp"}
    assert "asm" not in re.sub(r"//.*", "", text)
    # the launches the GPU suite runs past their grid caps
    launch = re.compile(r"(\w+_kernel(?:<[^<>]*>)?)[>,(\s]*dim3\(grid_for\(([^,()]+),\s*(\w+)\s*,\s*(\w+)\s*\)\)")
    found = {k: (items.strip(), a, b) for k, items, a, b in launch.findall(text)}
    assert found["topp16_short_kernel<1>"] == ("rows", "8", "16384") and found["topp16_short_kernel<16>"] == ("rows", "1", "4096")
