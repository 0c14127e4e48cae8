"""CPU suite: the multi-rank k-th value selection's C-ABI surface (lsdsort_kth_multi_device and its workspace figure), its argument
checks without a device, the Python face's own argument errors, quantile_rows' rank arithmetic against torch.quantile on the CPU,
the resources of every kernel of kth_multi.hip from hipcc's own remarks, and the launch lines of its two capped row loops."""
import json
import os
import re

import pytest

import _row_rounds as rr
from _faces import FakeCuda, lib as _lib, no_library
from _kernel_resources import hipcc, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "kernel_resources_kth_multi.json")
U32, I32, F32 = range(3)
ENTRIES = ("lsdsort_kth_multi_workspace_bytes", "lsdsort_kth_multi_device")
NAMES = ("GPUKthMulti", "kth_multi_workspace_bytes", "quantile_rows", "quantile_ranks")
MODES = ("linear", "lower", "higher", "midpoint", "nearest")


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
    # the single-rank signature with (ranks, num_ranks) where it has the rank
    one, multi = binding.SIGNATURES["lsdsort_kth_device"], binding.SIGNATURES["lsdsort_kth_multi_device"]
    assert multi[0] == one[0] and multi[1][:3] == one[1][:3] and multi[1][5:] == one[1][4:]
    assert binding.SIGNATURES["lsdsort_kth_multi_workspace_bytes"][1] == [binding.c_size] * 3
    for name in NAMES:
        assert callable(getattr(lsd, name)) and name in lsd.api.__all__, name


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

    def call(keys=fake, out=fake, idx=fake, w=fake, wb=None, rows=rows, cols=cols, ranks=(7, 0, 999), m=None, kt=F32, largest=0):
        m = (0 if ranks is None else len(ranks)) if m is None else m
        if wb is None:
            wb = L.lsdsort_kth_multi_workspace_bytes(rows, cols, m)
        return L.lsdsort_kth_multi_device(keys, rows, cols, ranks_array(ranks), m, kt, largest, out, idx, w, wb, None)

    # 1. key type, before everything else (the 64-bit key types are not this entry's either)
    for kt in (-1, 3, 4, 5, 100):
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
    for kt in (U32, I32, F32):
        for largest in (0, 1):
            assert call(kt=kt, largest=largest, rows=0, ranks=OUT, keys=None, out=None, idx=None, w=None, wb=0) == E.LSDSORT_OK
            assert call(kt=kt, largest=largest, rows=0, ranks=None, m=3, keys=fake + 1, out=None, w=None, wb=0) == E.LSDSORT_OK
            assert call(kt=kt, largest=largest, cols=0, ranks=(0, 9), keys=None, out=fake + 2, w=None, wb=0) == E.LSDSORT_OK
            assert call(kt=kt, largest=largest, ranks=(), keys=None, out=None, idx=None, w=None, wb=0) == E.LSDSORT_OK
            assert call(kt=kt, largest=largest, ranks=None, m=0, keys=fake + 3, out=None, w=None, wb=0) == E.LSDSORT_OK
    # 5. the ranks, before the pointers and the workspace: NULL, or any one of them outside the row
    assert call(ranks=None, m=3, keys=None, out=None, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG
    assert call(ranks=(0, cols, 5), keys=None, out=None, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG        # in the middle
    assert call(ranks=(cols,), keys=fake + 2, out=None, w=fake + 128, wb=0) == E.LSDSORT_ERR_INVALID_ARG
    assert call(ranks=(0, 1, 2, 3, 4, 5, 6, cols + 1), keys=None, out=None, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG
    assert call(ranks=(3, BIG), keys=None, out=None, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG
    assert call(rows=1, cols=1, ranks=(0, 1), keys=None, out=None, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG
    # 6. the keys and the values, before the workspace: NULL, or not 4-byte aligned
    assert call(keys=None, w=None) == E.LSDSORT_ERR_INVALID_ARG
    assert call(out=None, w=None) == E.LSDSORT_ERR_INVALID_ARG
    for off in (1, 2, 3):
        assert call(keys=fake + off, w=None) == E.LSDSORT_ERR_INVALID_ARG, off
        assert call(out=fake + off, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG, off
    assert call(keys=fake + 6, out=fake + 4, w=None) == E.LSDSORT_ERR_INVALID_ARG
    # 7. workspace: exactly lsdsort_kth_multi_workspace_bytes(rows, cols, num_ranks)
    assert call(w=None) == E.LSDSORT_ERR_WORKSPACE
    assert call(w=fake + 128) == E.LSDSORT_ERR_WORKSPACE                                # misaligned
    need = L.lsdsort_kth_multi_workspace_bytes(rows, cols, 3)
    assert need > 0 and call(wb=need - 1) == E.LSDSORT_ERR_WORKSPACE
    assert call(idx=None, wb=need - 1) == E.LSDSORT_ERR_WORKSPACE                       # one figure, with or without indices
    assert call(keys=fake + 4, out=fake + 12, w=None) == E.LSDSORT_ERR_WORKSPACE        # 4-byte alignment passes check 6
    long_need = L.lsdsort_kth_multi_workspace_bytes(3, 70001, 8)
    assert call(rows=3, cols=70001, ranks=(70000, 0, 1, 2, 3, 4, 5, 5), wb=long_need - 1) == E.LSDSORT_ERR_WORKSPACE
    assert call(rows=3, cols=70001, ranks=(5,) * 8, wb=L.lsdsort_kth_multi_workspace_bytes(3, 70001, 7)) == E.LSDSORT_ERR_WORKSPACE
    # 8. without a gfx950 device the last check answers; with one, this test does not get here on bogus pointers
    import torch

    if not torch.cuda.is_available():
        for kt in (U32, I32, F32):
            for largest in (0, 1):
                for idx in (None, fake):
                    assert call(kt=kt, largest=largest, idx=idx) == E.LSDSORT_ERR_NO_DEVICE
        assert call(keys=fake + 4) == E.LSDSORT_ERR_NO_DEVICE                           # 4-byte, not 16-byte aligned
        assert call(keys=fake + 12, out=fake + 8, cols=1001, ranks=(1000, 1000)) == E.LSDSORT_ERR_NO_DEVICE
        assert call(ranks=(0,)) == E.LSDSORT_ERR_NO_DEVICE and call(ranks=tuple(range(992, 1000))) == E.LSDSORT_ERR_NO_DEVICE
        assert call(rows=3, cols=70001, ranks=(35000, 0, 70000)) == E.LSDSORT_ERR_NO_DEVICE   # the long tier


def bound(rows, cols, m):
    """The issue's bound: control block, 16 B per row and rank, and above 16384 keys per row 2048 counters and 4 B per 16384 keys
    per row and rank; three arrays rounded up to 256 bytes."""
    is_long = cols > 16384
    return 256 + rows * m * (16 + ((8192 + 4 * -(-cols // 16384)) if is_long else 0)) + 3 * 255


def test_workspace_figure():
    from lsdradixsort_amd import errors as E

    L = _lib()
    BIG = E.LSDSORT_MAX_KEYS
    f = L.lsdsort_kth_multi_workspace_bytes
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
                if cols >= 16385:                                                          # O(rows * ranks), never O(rows * cols):
                    assert b <= 4 * rows * cols * m, (rows, cols, m, b)                    # per rank, the keys' bytes at the most
                    assert cols < 65536 or 4 * b <= 4 * rows * cols * m, (rows, cols, m, b)   # a quarter from 65536 keys per row on
                else:
                    assert b <= 256 + rows * m * 16 + 255, (rows, cols, m, b)              # the short tiers: a state per slot
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
    assert f(3, 70001, 1) == L.lsdsort_kth_workspace_bytes(3, 70001) and f(9, 1000, 1) == L.lsdsort_kth_workspace_bytes(9, 1000)
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
    for dtype, key_type in ((torch.int32, "int32"), (torch.int32, "uint32"), (torch.float32, "float32")):
        with pytest.raises(TypeError):
            lsd.GPUKthMulti(torch.zeros(8, dtype=dtype), [1, 2], key_type=key_type)   # a CPU tensor
    with pytest.raises(TypeError):
        lsd.quantile_rows(torch.zeros(8), 0.5)
    with pytest.raises(TypeError):
        lsd.GPUKthMulti([3, 1, 2], [1])
    with pytest.raises(TypeError):
        lsd.quantile_rows([3.0, 1.0, 2.0], 0.5)


def test_dtype_key_type_ranks_q_and_mode(no_library):
    """Wrong dtype, a key type this entry does not have, a 3-D or non-contiguous input, 0 or 9 ranks, a rank outside
    0 .. cols - 1, q outside [0, 1], an unknown interpolation, an empty last dimension -- checked on tensors that pass for CUDA
    tensors, so that the test needs no device."""
    import torch

    lsd = no_library

    def fake(dtype, shape=(2, 4)):
        return torch.zeros(shape, dtype=dtype).as_subclass(FakeCuda)

    for dtype in (torch.int16, torch.float16, torch.bfloat16, torch.int64, torch.float64, torch.uint8):
        with pytest.raises(TypeError):
            lsd.GPUKthMulti(fake(dtype), [1])
        with pytest.raises(TypeError):
            lsd.quantile_rows(fake(dtype), 0.5)
    with pytest.raises(TypeError):
        lsd.quantile_rows(fake(torch.int32), 0.5)                                # float32 only
    with pytest.raises(TypeError):
        lsd.quantile_rows(fake(torch.float32, ()), 0.5)                          # at least one dimension
    for dtype in (torch.int32, torch.float32):
        for key_type in ("int16", "float16", "bfloat16", "uint64", "int64", "float64", "double", ""):
            with pytest.raises(ValueError):
                lsd.GPUKthMulti(fake(dtype), [1, 2], key_type=key_type)
        with pytest.raises(TypeError):
            lsd.GPUKthMulti(fake(dtype, (2, 2, 2)), [1], key_type="float32")     # 1-D or 2-D only
        with pytest.raises(TypeError):
            lsd.GPUKthMulti(fake(dtype, (4, 4)).t(), [1], key_type="float32")    # contiguous only
        for ranks in ([], list(range(9)), [0] * 9, [-1], [0, 4], [1, 2, 100], [3, 2, 1, 0, -1], 3, None):
            with pytest.raises(ValueError):
                lsd.GPUKthMulti(fake(dtype), ranks, key_type="float32")
        with pytest.raises(ValueError):
            lsd.GPUKthMulti(fake(dtype, (4,)), [0, 4], key_type="float32", largest=True)
    for key_type in ("uint32", "int32"):
        with pytest.raises(TypeError):
            lsd.GPUKthMulti(fake(torch.float32), [1], key_type=key_type)         # a float32 tensor is float32 keys, nothing else
    with pytest.raises(TypeError):
        lsd.GPUKthMulti(fake(torch.float32), [1])                                # ... the default key type included
    x = fake(torch.float32, (3, 2, 4))
    for q in (-0.1, 1.5, [0.5, 1.0001], [0.2, -1e-9], float("nan"), torch.tensor([0.5, 2.0]), torch.zeros((2, 2))):
        with pytest.raises(ValueError):
            lsd.quantile_rows(x, q)
        with pytest.raises(ValueError):
            lsd.quantile_ranks(q, 4)
    for mode in ("cubic", "", "Linear", None):
        with pytest.raises(ValueError):
            lsd.quantile_rows(x, 0.5, interpolation=mode)
    for shape in ((3, 0), (0,), (2, 3, 0)):
        with pytest.raises(ValueError):
            lsd.quantile_rows(fake(torch.float32, shape), 0.5)


QS = [0.37, [0.5], [0.0, 0.25, 1.0], [0.999, 0.01, 0.5, 0.5, 0.75, 0.33333334]]


@pytest.mark.parametrize("cols", [1, 2, 3, 7, 1001, 70001])
def test_quantile_ranks_is_torch_quantile_on_sorted_rows(cols, no_library):
    """quantile_ranks applied to the sorted rows IS torch.quantile, value for value and in shape: every mode, q a float and lists
    of 1, 3 and 6, as tensors too."""
    import torch

    lsd = no_library
    g = torch.Generator().manual_seed(cols)
    x = torch.randn((2, 3, cols), generator=g)
    x[..., ::5] = 2.5   # ties
    ordered = x.sort(dim=-1).values
    for mode in MODES:
        for q in QS + [torch.tensor(0.62), torch.tensor(QS[2])]:
            below, above, weights, scalar = lsd.quantile_ranks(q, cols, mode)
            assert all(0 <= r < cols for r in below + (above or [])), (mode, q)
            assert (above is None) == (weights is None) == (mode in ("lower", "higher", "nearest"))
            got = ordered[..., below]
            if above is not None:
                assert all(b <= a <= b + 1 for b, a in zip(below, above)), "floor and ceiling of one rank"
                got = torch.lerp(got, ordered[..., above], weights)
            got = got.movedim(-1, 0)
            got = got[0] if scalar else got
            want = torch.quantile(x, q if isinstance(q, torch.Tensor) else torch.tensor(q), dim=-1, interpolation=mode)
            assert got.shape == want.shape and torch.equal(got, want), (mode, q, cols)
            if isinstance(q, float):
                assert torch.equal(got, torch.quantile(x, q, dim=-1, interpolation=mode)), (mode, q, cols)


def test_kernels_no_scratch_no_spill_and_recorded_resources():
    if hipcc() is None:
        pytest.skip("no hipcc on this machine")
    res = kernel_resources("kth_multi.hip")
    names = list(res)
    once = ("kthm_clear_kernel", "kthm_hist0_kernel", "kthm_count_kernel", "pick_slots_kernelINS0_8KthMultiE", "kthm_locate_kernel")
    for must in once:
        assert sum(must in name for name in names) == 1, (must, names)
    assert sum("kthm_short_kernel" in name for name in names) == 2, names                 # one wavefront, one workgroup
    assert sum("kthm_scan_kernel" in name for name in names) == 3, names                  # three digit levels
    hist = [name for name in names if "kthm_hist_kernel" in name]                         # levels 1 and 2, SLOTS 2, 4 and 8
    assert len(hist) == 6, names
    for slots in (2, 4, 8):
        mine = [name for name in hist if re.search(r"ILi[12]ELi%dEE" % slots, name)]
        assert len(mine) == 2 and all(res[name]["lds_bytes"] == slots * 2048 * 4 for name in mine), (slots, hist)
    assert len(names) == len(once) + 2 + 3 + 6, names
    assert all("kthm_" in name or "_kernelINS0_8KthMultiE" in name for name in names), names   # every kernel names its unit
    for name, r in res.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r)
    want = json.load(open(GOLDEN))["kth_multi.hip"]
    assert sorted(res) == sorted(want), f"kernels gone: {sorted(set(want) - set(res))}, new: {sorted(set(res) - set(want))}"
    for name, w in want.items():
        assert res[name]["occupancy"] >= w["occupancy"], f"{name}: {res[name]['occupancy']} waves/SIMD, recorded {w['occupancy']}"
        assert res[name]["lds_bytes"] == w["lds_bytes"], f"{name}: {res[name]['lds_bytes']} B of static LDS, recorded {w['lds_bytes']}"
    # the short kernels keep the single-rank kernels' occupancy: the slot loop costs no wave
    one = kernel_resources("kth.hip")
    for waves in (1, 16):
        tag = "short_kernelILi%dEE" % waves
        single = next(r for name, r in one.items() if tag in name)
        multi = next(r for name, r in res.items() if tag in name)
        assert multi["occupancy"] >= single["occupancy"] and multi["lds_bytes"] == single["lds_bytes"], (waves, single, multi)


# <kernel><template arguments> , dim3(grid_for(<items>, <per>, <cap>)): the form tests/test_row_rounds_cpu.py reads
LAUNCH = re.compile(r"(\w+_kernel(?:<[^<>]*>)?)[>,(\s]*dim3\(grid_for\(([^,()]+),\s*(\w+)\s*,\s*(\w+)\s*\)\)")


@pytest.mark.parametrize("kernel,per,cap,shape", [("kthm_short_kernel<1>", 8, 16384, "WAVE32"), ("kthm_short_kernel<16>", 1, 4096, "GROUP")])
def test_short_kernels_launch_lines_and_second_round_shapes(kernel, per, cap, shape):
    text = open(os.path.join(ROOT, "lsdradixsort_amd", "csrc", "kth_multi.hip")).read()
    found = {(items.strip(), a, b) for k, items, a, b in LAUNCH.findall(text) if k == kernel}
    assert found == {("rows", str(per), str(cap))}, f"{kernel} is launched with {sorted(found)}"
    assert re.search(r"cols <= \(size_t\)kWaveSegCap\b", text) and re.search(r"cols <= \(size_t\)kLocalSortCap\b", text)
    rows, cols = rr.SHAPES[shape]
    assert per * cap < rows, f"{shape}: one round of {kernel} covers {per * cap} >= {rows} rows"
    rest = rows % (per * cap)
    assert rest != 0 and (per == 1 or rest % per != 0), f"{shape}: the last round of {kernel} holds {rest} rows: no partly filled workgroup"
    assert per * cap == rr.stride_of(shape, "kth"), f"{shape}: {kernel} strides by {per * cap}"
    assert (cols <= rr.TIERS["wave"]) == (per == 8) and cols <= rr.TIERS["group"]
