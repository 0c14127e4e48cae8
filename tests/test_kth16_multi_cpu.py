"""CPU suite: the multi-rank k-th value selection for 16-bit keys -- its C-ABI surface (lsdsort_kth16_multi_device and its workspace
figure), its argument checks without a device, the Python face's own argument errors (GPUKth16Multi, quantile16_rows), the resources
of every kernel of kth16_multi.hip from hipcc's own remarks, and the launch lines of its two capped row loops."""
import json
import os
import re

import pytest

import _row_rounds as rr
from _faces import FakeCuda, lib as _lib, no_library
from _kernel_resources import hipcc, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "kernel_resources_kth16_multi.json")
GOLDEN_32 = os.path.join(ROOT, "tests", "golden", "kernel_resources_kth_multi.json")
U16, I16, F16, BF16 = range(4)
ENTRIES = ("lsdsort_kth16_multi_workspace_bytes", "lsdsort_kth16_multi_device")
NAMES = ("GPUKth16Multi", "kth16_multi_workspace_bytes", "quantile16_rows")


def test_header_ctypes_table_and_package_have_the_entries():
    import lsdradixsort_amd as lsd
    from lsdradixsort_amd import _lib as binding

    header = open(os.path.join(ROOT, "include", "lsdsort.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"LSDSORT_API\s+[\w\s\*]+?\b" + name + r"\s*\(", text), name
        assert name in binding.SIGNATURES
        assert hasattr(_lib(), name)
    assert int(re.search(r"#define\s+LSDSORT_KTH_MAX_RANKS\s+(\d+)", header).group(1)) == 8 == lsd.errors.LSDSORT_KTH_MAX_RANKS
    # the single-rank 16-bit signature with (ranks, num_ranks) where it has the rank: the 32-bit multi-rank signature
    one, multi = binding.SIGNATURES["lsdsort_kth16_device"], binding.SIGNATURES["lsdsort_kth16_multi_device"]
    assert multi[0] == one[0] and multi[1][:3] == one[1][:3] and multi[1][5:] == one[1][4:]
    assert multi == binding.SIGNATURES["lsdsort_kth_multi_device"]
    assert binding.SIGNATURES["lsdsort_kth16_multi_workspace_bytes"][1] == [binding.c_size] * 3
    for name in NAMES:
        assert callable(getattr(lsd, name)) and name in lsd.api.__all__, name
    makefile = open(os.path.join(ROOT, "lsdradixsort_amd", "csrc", "Makefile")).read()
    assert "kth16_multi" in re.search(r"^NAMES\s*:=(.*)$", makefile, flags=re.M).group(1).split()


def ranks_array(ranks):
    import ctypes

    return None if ranks is None else (ctypes.c_size_t * max(len(ranks), 1))(*ranks)


def test_argument_checks_in_entry_order():
    from lsdradixsort_amd import errors as E

    L = _lib()
    rows, cols = 10, 1000
    fake = 1 << 20   # never dereferenced: every call below returns before a device is touched
    BIG = E.LSDSORT_MAX_KEYS
    OUT = (cols, cols + 5)   # ranks outside the row

    def call(keys=fake, out=fake, idx=fake, w=fake, wb=None, rows=rows, cols=cols, ranks=(7, 0, 999), m=None, kt=BF16, largest=0):
        m = (0 if ranks is None else len(ranks)) if m is None else m
        if wb is None:
            wb = L.lsdsort_kth16_multi_workspace_bytes(rows, cols, m)
        return L.lsdsort_kth16_multi_device(keys, rows, cols, ranks_array(ranks), m, kt, largest, out, idx, w, wb, None)

    # 1. key type, before everything else
    for kt in (-1, 4, 5, 100):
        assert call(kt=kt, rows=BIG + 1, ranks=None, m=9, keys=None, out=None, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG, kt
        assert call(kt=kt, rows=0, wb=0) == E.LSDSORT_ERR_INVALID_ARG, kt
    # 2. the number of ranks, before the sizes, the empty call, the ranks, the pointers and the workspace
    assert call(ranks=tuple(range(9)), wb=0) == E.LSDSORT_ERR_INVALID_ARG
    assert call(ranks=None, m=9, rows=BIG + 1, keys=None, out=None, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG
    assert call(ranks=None, m=9, rows=0, wb=0) == E.LSDSORT_ERR_INVALID_ARG
    assert call(ranks=None, m=BIG, cols=0, wb=0) == E.LSDSORT_ERR_INVALID_ARG
    # 3. size, before the empty call, the ranks, the pointers and the workspace
    assert call(rows=BIG + 1, cols=1, ranks=OUT, keys=None, out=None, w=None, wb=0) == E.LSDSORT_ERR_TOO_LARGE
    assert call(rows=1 << 15, cols=1 << 15, ranks=None, m=2, keys=None, out=None, w=None, wb=0) == E.LSDSORT_ERR_TOO_LARGE
    assert call(rows=2, cols=BIG // 2 + 1, ranks=OUT, keys=fake + 1, out=None, w=None, wb=0) == E.LSDSORT_ERR_TOO_LARGE
    assert call(rows=BIG // 8 + 1, cols=1, ranks=None, m=8, keys=None, out=None, w=None, wb=0) == E.LSDSORT_ERR_TOO_LARGE   # rows * ranks
    assert call(rows=BIG // 2 + 1, cols=0, ranks=None, m=2, keys=None, out=None, w=None, wb=0) == E.LSDSORT_ERR_TOO_LARGE
    # 4. nothing to do, before the ranks (an empty row has no valid rank), the pointers and the workspace
    for kt in (U16, I16, F16, BF16):
        for largest in (0, 1):
            assert call(kt=kt, largest=largest, rows=0, ranks=OUT, keys=None, out=None, idx=None, w=None, wb=0) == E.LSDSORT_OK
            assert call(kt=kt, largest=largest, rows=0, ranks=None, m=3, keys=fake + 1, out=None, w=None, wb=0) == E.LSDSORT_OK
            assert call(kt=kt, largest=largest, cols=0, ranks=(0, 9), keys=None, out=fake + 1, w=None, wb=0) == E.LSDSORT_OK
            assert call(kt=kt, largest=largest, ranks=(), keys=None, out=None, idx=None, w=None, wb=0) == E.LSDSORT_OK
            assert call(kt=kt, largest=largest, ranks=None, m=0, keys=fake + 3, out=None, w=None, wb=0) == E.LSDSORT_OK
    # 5. the ranks, before the pointers and the workspace: NULL, or any one of them outside the row
    assert call(ranks=None, m=3, keys=None, out=None, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG
    assert call(ranks=(0, cols, 5), keys=None, out=None, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG        # in the middle
    assert call(ranks=(cols,), keys=fake + 2, out=None, w=fake + 128, wb=0) == E.LSDSORT_ERR_INVALID_ARG
    assert call(ranks=(0, 1, 2, 3, 4, 5, 6, cols + 1), keys=None, out=None, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG
    assert call(ranks=(3, BIG), keys=None, out=None, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG
    assert call(rows=1, cols=1, ranks=(0, 1), keys=None, out=None, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG
    # 6. the keys and the values, before the workspace: NULL, or odd
    assert call(keys=None, w=None) == E.LSDSORT_ERR_INVALID_ARG
    assert call(out=None, w=None) == E.LSDSORT_ERR_INVALID_ARG
    for off in (1, 3, 7, 15):
        assert call(keys=fake + off, w=None) == E.LSDSORT_ERR_INVALID_ARG, off
        assert call(out=fake + off, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG, off
    assert call(keys=fake + 6, out=fake + 5, w=None) == E.LSDSORT_ERR_INVALID_ARG
    # 7. workspace: exactly lsdsort_kth16_multi_workspace_bytes(rows, cols, num_ranks)
    assert call(w=None) == E.LSDSORT_ERR_WORKSPACE
    assert call(w=fake + 128) == E.LSDSORT_ERR_WORKSPACE                                # misaligned
    need = L.lsdsort_kth16_multi_workspace_bytes(rows, cols, 3)
    assert need > 0 and call(wb=need - 1) == E.LSDSORT_ERR_WORKSPACE
    assert call(idx=None, wb=need - 1) == E.LSDSORT_ERR_WORKSPACE                       # one figure, with or without indices
    for off in (2, 4, 6, 14):
        assert call(keys=fake + off, out=fake + 16 - off, w=None) == E.LSDSORT_ERR_WORKSPACE, off   # 2-byte alignment passes check 6
    long_need = L.lsdsort_kth16_multi_workspace_bytes(3, 70001, 8)
    assert call(rows=3, cols=70001, ranks=(70000, 0, 1, 2, 3, 4, 5, 5), wb=long_need - 1) == E.LSDSORT_ERR_WORKSPACE
    assert call(rows=3, cols=70001, ranks=(5,) * 8, wb=L.lsdsort_kth16_multi_workspace_bytes(3, 70001, 7)) == E.LSDSORT_ERR_WORKSPACE
    # 8. without a gfx950 device the last check answers; with one, this test does not get here on bogus pointers
    import torch

    if not torch.cuda.is_available():
        for kt in (U16, I16, F16, BF16):
            for largest in (0, 1):
                for idx in (None, fake):
                    assert call(kt=kt, largest=largest, idx=idx) == E.LSDSORT_ERR_NO_DEVICE
        assert call(keys=fake + 2) == E.LSDSORT_ERR_NO_DEVICE                           # 2-byte, not 16-byte aligned
        assert call(keys=fake + 14, out=fake + 6, cols=1001, ranks=(1000, 1000)) == E.LSDSORT_ERR_NO_DEVICE
        assert call(ranks=(0,)) == E.LSDSORT_ERR_NO_DEVICE and call(ranks=tuple(range(992, 1000))) == E.LSDSORT_ERR_NO_DEVICE
        assert call(rows=3, cols=70001, ranks=(35000, 0, 70000)) == E.LSDSORT_ERR_NO_DEVICE   # the long tier
        assert call(rows=3, cols=70001, ranks=(35000, 0, 70000), idx=None) == E.LSDSORT_ERR_NO_DEVICE


def bound(rows, cols, m):
    """The issue's bounds.  Long rows: the control block, 8 KiB of level-0 counters per ROW, and per row and rank a state (16 B), 32
    level-1 counters (128 B) and 4 B per 16384 keys; four arrays rounded up to 256 bytes.  Short tiers: the control block and a
    state per row and rank, one array rounded up."""
    if cols > 16384:
        return 256 + rows * (8192 + m * (16 + 128 + 4 * -(-cols // 16384))) + 4 * 255
    return 256 + 16 * rows * m + 255


def test_workspace_figure():
    from lsdradixsort_amd import errors as E

    L = _lib()
    BIG = E.LSDSORT_MAX_KEYS
    f = L.lsdsort_kth16_multi_workspace_bytes
    ladder = [1, 2, 7, 8, 9, 1000, 1024, 1025, 16384, 16385, 65536, 131073, (1 << 20) + 13, 1 << 24, BIG]
    row_ladder = [1, 2, 3, 64, 65, 513, 4096, 4097, 1 << 15, 1 << 20, BIG]
    rank_ladder = [1, 2, 3, 8]

    def legal(rows, cols, m):
        return rows * cols <= BIG and rows * m <= BIG

    seen = 0
    for m in rank_ladder:
        for rows in row_ladder:
            prev = 0
            for cols in ladder:
                if not legal(rows, cols, m):
                    assert f(rows, cols, m) == 0, (rows, cols, m)
                    continue
                b = f(rows, cols, m)
                assert b > 0 and b % 256 == 0 and b >= prev, (rows, cols, m, b, prev)      # monotonic in cols
                assert b <= bound(rows, cols, m), (rows, cols, m, b)
                prev = b
                seen += 1
        for cols in ladder:                                                                # monotonic in rows
            prev = 0
            for rows in row_ladder:
                if legal(rows, cols, m):
                    b = f(rows, cols, m)
                    assert b >= prev, (rows, cols, m)
                    prev = b
    assert seen > 240
    for rows in row_ladder:                                                                # monotonic in the number of ranks
        for cols in ladder:
            prev = 0
            for m in range(0, 9):
                if legal(rows, cols, m):
                    b = f(rows, cols, m)
                    assert b % 256 == 0 and b >= prev, (rows, cols, m)
                    prev = b
    assert f(1, 16385, 2) > f(1, 16384, 2) and f(2, 1 << 24, 3) > f(1, 1 << 24, 3) and f(3, 70001, 3) > f(3, 70001, 2)
    # the level-0 counters are per row, not per (row, rank): eight single-rank workspaces are more than one of eight ranks
    for rows, cols in ((3, 70001), (128, 128256), (1, 1 << 24)):
        assert 8 * f(rows, cols, 1) > f(rows, cols, 8), (rows, cols)
        assert f(rows, cols, 8) < L.lsdsort_kth_multi_workspace_bytes(rows, cols, 8), (rows, cols)   # the 32-bit form's 8 KiB per slot
    assert f(0, 1000, 3) % 256 == 0 and f(10, 0, 3) % 256 == 0 and f(10, 1000, 0) % 256 == 0
    # above the limits, and more ranks than a call takes
    assert f(BIG + 1, 1, 1) == 0 and f(1, BIG + 1, 1) == 0 and f(BIG + 1, 0, 1) == 0
    assert f(2, BIG // 2 + 1, 2) == 0 and f(1 << 15, 1 << 15, 2) == 0 and f(BIG // 8 + 1, 1, 8) == 0
    assert f(1, BIG, 8) > 0 and f(BIG, 1, 1) > 0 and f(BIG // 8, 1, 8) > 0
    for rows, cols in ((1, 1), (10, 1000), (3, 70001), (0, 0)):
        assert f(rows, cols, 9) == 0 and f(rows, cols, 100) == 0, (rows, cols)


def test_wrappers_check_their_tensors_before_the_library(no_library):
    import torch

    lsd = no_library
    for dtype, key_type in ((torch.int16, "int16"), (torch.int16, "uint16"), (torch.float16, "float16"), (torch.bfloat16, "bfloat16")):
        with pytest.raises(TypeError):
            lsd.GPUKth16Multi(torch.zeros(8, dtype=dtype), [1, 2], key_type=key_type)   # a CPU tensor
    with pytest.raises(TypeError):
        lsd.quantile16_rows(torch.zeros(8, dtype=torch.bfloat16), 0.5)
    with pytest.raises(TypeError):
        lsd.GPUKth16Multi([3, 1, 2], [1])
    with pytest.raises(TypeError):
        lsd.quantile16_rows([3.0, 1.0, 2.0], 0.5)


def test_dtype_key_type_ranks_q_and_mode(no_library):
    """Wrong dtype, a key type that does not fit the dtype, a 3-D or non-contiguous input, 0 or 9 ranks, a rank outside
    0 .. cols - 1, quantile16_rows on an int16 tensor, a 0-D tensor and an empty last dimension, q outside [0, 1], an unknown
    interpolation -- checked on tensors that pass for CUDA tensors, so that the test needs no device."""
    import torch

    lsd = no_library

    def fake(dtype, shape=(2, 4)):
        return torch.zeros(shape, dtype=dtype).as_subclass(FakeCuda)

    for dtype in (torch.int32, torch.float32, torch.int64, torch.uint8, torch.float64):
        with pytest.raises(TypeError):
            lsd.GPUKth16Multi(fake(dtype), [1])
        with pytest.raises(TypeError):
            lsd.quantile16_rows(fake(dtype), 0.5)
    with pytest.raises(TypeError):
        lsd.quantile16_rows(fake(torch.int16), 0.5)                                # the float types only
    for dtype in (torch.float16, torch.bfloat16):
        with pytest.raises(TypeError):
            lsd.quantile16_rows(fake(dtype, ()), 0.5)                              # at least one dimension
    fits = {torch.int16: ("uint16", "int16"), torch.float16: ("float16",), torch.bfloat16: ("bfloat16",)}
    for dtype, mine in fits.items():
        for key_type in ("uint16", "int16", "float16", "bfloat16"):
            if key_type not in mine:
                with pytest.raises(TypeError):
                    lsd.GPUKth16Multi(fake(dtype), [1, 2], key_type=key_type)      # a key type that does not fit the dtype
        for key_type in ("uint32", "int32", "float32", "uint64", "float64", "half", ""):
            with pytest.raises(ValueError):
                lsd.GPUKth16Multi(fake(dtype), [1, 2], key_type=key_type)          # a key type this entry does not have
        ok = mine[0]
        with pytest.raises(TypeError):
            lsd.GPUKth16Multi(fake(dtype, (2, 2, 2)), [1], key_type=ok)            # 1-D or 2-D only
        with pytest.raises(TypeError):
            lsd.GPUKth16Multi(fake(dtype, (4, 4)).t(), [1], key_type=ok)           # contiguous only
        for ranks in ([], list(range(9)), [0] * 9, [-1], [0, 4], [1, 2, 100], [3, 2, 1, 0, -1], 3, None):
            with pytest.raises(ValueError):
                lsd.GPUKth16Multi(fake(dtype), ranks, key_type=ok)
        with pytest.raises(ValueError):
            lsd.GPUKth16Multi(fake(dtype, (4,)), [0, 4], key_type=ok, largest=True)
    with pytest.raises(TypeError):
        lsd.GPUKth16Multi(fake(torch.bfloat16), [1])                               # the default key type is int16
    x = fake(torch.bfloat16, (3, 2, 4))
    for q in (-0.1, 1.5, [0.5, 1.0001], [0.2, -1e-9], float("nan"), torch.tensor([0.5, 2.0]), torch.zeros((2, 2))):
        with pytest.raises(ValueError):
            lsd.quantile16_rows(x, q)
    for mode in ("cubic", "", "Linear", None):
        with pytest.raises(ValueError):
            lsd.quantile16_rows(x, 0.5, interpolation=mode)
    for dtype in (torch.float16, torch.bfloat16):
        for shape in ((3, 0), (0,), (2, 3, 0)):
            with pytest.raises(ValueError):
                lsd.quantile16_rows(fake(dtype, shape), 0.5)


def test_kernels_no_scratch_no_spill_and_recorded_resources():
    if hipcc() is None:
        pytest.skip("no hipcc on this machine")
    res = kernel_resources("kth16_multi.hip")
    names = list(res)
    once = ("kth16m_clear_kernel", "kth16m_hist0_kernel", "kth16m_hist1_kernel", "kth16m_scan1_kernel", "kth16m_count_kernel",
            "pick_slots_kernelINS0_10Kth16MultiE", "kth16m_locate_kernel", "kth16m_value_kernel")
    for must in once:
        assert sum(must in name for name in names) == 1, (must, names)
    assert sum("kth16m_short_kernel" in name for name in names) == 2, names               # one wavefront, one workgroup
    assert sum("kth16m_scan0_kernel" in name for name in names) == 2, names               # StopKth, and never-stop for values only
    assert len(names) == len(once) + 2 + 2, names
    assert all("kth16m_" in name or "_kernelINS0_10Kth16MultiE" in name for name in names), names   # every kernel names its unit
    for name, r in res.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r)
    want = json.load(open(GOLDEN))["kth16_multi.hip"]
    assert sorted(res) == sorted(want), f"kernels gone: {sorted(set(want) - set(res))}, new: {sorted(set(res) - set(want))}"
    for name, w in want.items():
        assert res[name]["occupancy"] >= w["occupancy"], f"{name}: {res[name]['occupancy']} waves/SIMD, recorded {w['occupancy']}"
        assert res[name]["lds_bytes"] == w["lds_bytes"], f"{name}: {res[name]['lds_bytes']} B of static LDS, recorded {w['lds_bytes']}"
    # level 1: 32 counters per leader -- eight slots are 1 KiB, and nothing else of size
    hist1 = next(r for name, r in res.items() if "kth16m_hist1_kernel" in name)
    assert 8 * 32 * 4 <= hist1["lds_bytes"] <= 8 * 32 * 4 + 256, hist1
    # the short kernels: the occupancy of kth_multi.hip's short kernels (7 and 6 waves per SIMD) with kth16.hip's static LDS
    multi32 = json.load(open(GOLDEN_32))["kth_multi.hip"]
    one16 = kernel_resources("kth16.hip")
    for waves, least in ((1, 7), (16, 6)):
        tag = "short_kernelILi%dEE" % waves
        recorded = next(r for name, r in multi32.items() if tag in name)
        single = next(r for name, r in one16.items() if tag in name)
        mine = next(r for name, r in res.items() if tag in name)
        assert recorded["occupancy"] == least
        assert mine["occupancy"] >= least and mine["lds_bytes"] == single["lds_bytes"], (waves, single, mine)


# <kernel><template arguments> , dim3(grid_for(<items>, <per>, <cap>)): the form tests/test_row_rounds_cpu.py reads
LAUNCH = re.compile(r"(\w+_kernel(?:<[^<>]*>)?)[>,(\s]*dim3\(grid_for\(([^,()]+),\s*(\w+)\s*,\s*(\w+)\s*\)\)")


@pytest.mark.parametrize("kernel,per,cap,shape", [("kth16m_short_kernel<1>", 8, 16384, "WAVE16"), ("kth16m_short_kernel<16>", 1, 4096, "GROUP")])
def test_short_kernels_launch_lines_and_second_round_shapes(kernel, per, cap, shape):
    text = open(os.path.join(ROOT, "lsdradixsort_amd", "csrc", "kth16_multi.hip")).read()
    found = {(items.strip(), a, b) for k, items, a, b in LAUNCH.findall(text) if k == kernel}
    assert found == {("rows", str(per), str(cap))}, f"{kernel} is launched with {sorted(found)}"
    assert re.search(r"cols <= \(size_t\)kWaveSegCap\b", text) and re.search(r"cols <= \(size_t\)kLocalSortCap\b", text)
    rows, cols = rr.SHAPES[shape]
    assert per * cap < rows, f"{shape}: one round of {kernel} covers {per * cap} >= {rows} rows"
    rest = rows % (per * cap)
    assert rest != 0 and (per == 1 or rest % per != 0), f"{shape}: the last round of {kernel} holds {rest} rows: no partly filled workgroup"
    assert per * cap == rr.stride_of(shape, "kth16"), f"{shape}: {kernel} strides by {per * cap}"
    assert (cols <= rr.TIERS["wave"]) == (per == 8) and cols <= rr.TIERS["group"]
