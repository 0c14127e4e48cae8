"""CPU suite: the draw for 16-bit logit rows (sample16.hip) -- its C-ABI surface (lsdsort_sample16_device and its workspace figure),
its argument checks without a device, the Python face's own argument errors and host conversions (GPUSample16, sample16_rows), the
float64 oracle and acceptance rule of tests/_sample16.py on hand-computed rows and on every sharp row the GPU suite uses, and the
resources of every kernel of the unit from hipcc's own remarks."""
import json
import math
import os
import re

import numpy as np
import pytest

import _sample16 as sm
import _topp16 as tp
from _faces import FakeCuda, lib as _lib, no_library
from _kernel_resources import hipcc, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "kernel_resources_sample16.json")
U16, I16, F16, BF16 = range(4)
ENTRIES = ("lsdsort_sample16_workspace_bytes", "lsdsort_sample16_device")
NAMES = ("GPUSample16", "sample16_workspace_bytes", "sample16_rows")
SHARP_COLS = (64, 257, 1024, 1025, 16384, 16385, 32769, 40000)   # test_gpu_sample16.py's


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
    draw = binding.SIGNATURES["lsdsort_sample16_device"]
    assert draw[0] == binding.c_int and len(draw[1]) == 10 and draw[1][4] == binding.c_int and draw[1][8] == binding.c_size
    assert all(draw[1][i] == ctypes.c_void_p for i in (0, 3, 5, 6, 7, 9))
    assert binding.SIGNATURES[ENTRIES[0]] == (binding.c_size, [binding.c_size] * 2)
    doc = header[header.index("The DRAW of a sampling step"):header.index("lsdsort_sample16_workspace_bytes(size_t")]
    for word in ("graph", "DETERMINISTIC", "in any batch", "lsdsort_topp16_filter_device", "lsdsort_topk16_filter_device", "2^-12", "2^-11",
                 "POSITION order", "index -1", "READ ONLY", "bit 1024"):   # the contract's points
        assert word in doc, word
    for name in NAMES:
        assert callable(getattr(lsd, name)) and name in lsd.api.__all__, name
    init = open(os.path.join(ROOT, "lsdradixsort_amd", "__init__.py")).read()
    assert "GPUSample16, sample16_workspace_bytes, sample16_rows," in init
    makefile = open(os.path.join(ROOT, "lsdradixsort_amd", "csrc", "Makefile")).read()
    assert "sample16" in re.search(r"^NAMES\s*:=(.*)$", makefile, flags=re.M).group(1).split()
    assert "sample16" not in open(os.path.join(ROOT, "include", "lsdsort.hpp")).read()     # no wrapper in the C++ face


def test_argument_checks_in_entry_order():
    from lsdradixsort_amd import errors as E

    L = _lib()
    rows, cols = 10, 1000
    fake = 1 << 20   # never dereferenced: every call below returns before a device is touched
    BIG = E.LSDSORT_MAX_KEYS

    def call(keys=fake, u=fake + (1 << 12), idx=fake + (1 << 16), lp=fake + (1 << 17), w=fake, wb=None, rows=rows, cols=cols, kt=BF16):
        if wb is None:
            wb = L.lsdsort_sample16_workspace_bytes(rows, cols)
        return L.lsdsort_sample16_device(keys, rows, cols, u, kt, idx, lp, w, wb, None)

    # 1. key type, before everything else: float16 and bfloat16 only
    for kt in (-1, U16, I16, 4, 5, 100):
        assert call(kt=kt, rows=BIG + 1, keys=None, u=None, idx=None, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG, kt
        assert call(kt=kt, rows=0, wb=0) == E.LSDSORT_ERR_INVALID_ARG, kt
        assert call(kt=kt) == E.LSDSORT_ERR_INVALID_ARG, kt
    # 2. sizes, before the empty call, the pointers and the workspace
    assert call(rows=BIG + 1, cols=1, keys=None, u=None, idx=None, w=None, wb=0) == E.LSDSORT_ERR_TOO_LARGE
    assert call(rows=1 << 15, cols=1 << 15, keys=None, u=fake + 1, idx=None, w=None, wb=0) == E.LSDSORT_ERR_TOO_LARGE
    assert call(rows=2, cols=BIG // 2 + 1, keys=fake + 1, idx=None, lp=fake + 1, w=None, wb=0) == E.LSDSORT_ERR_TOO_LARGE
    # 3. nothing to do
    for kt in (F16, BF16):
        assert call(kt=kt, rows=0, keys=None, u=None, idx=None, lp=None, w=None, wb=0) == E.LSDSORT_OK
        assert call(kt=kt, cols=0, keys=fake + 1, u=fake + 2, idx=fake + 1, lp=fake + 3, w=None, wb=0) == E.LSDSORT_OK
    # 4. NULL or odd d_keys, before d_u and d_index
    assert call(keys=None, u=None, idx=None, w=None) == E.LSDSORT_ERR_INVALID_ARG
    for off in (1, 3, 7, 15):
        assert call(keys=fake + off, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG, off
    # 5. NULL or misaligned d_u or d_index
    assert call(u=None, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG
    assert call(idx=None, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG
    for off in (1, 2, 3, 6, 13):
        assert call(u=fake + off, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG, off
        assert call(idx=fake + off, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG, off
    # 6. a d_logprob that is given and misaligned; NULL is "no logprob" and passes on to the workspace check
    for off in (1, 2, 3, 6, 13):
        assert call(lp=fake + off, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG, off
    assert call(lp=None, w=None) == E.LSDSORT_ERR_WORKSPACE
    # 7. workspace: exactly lsdsort_sample16_workspace_bytes(rows, cols)
    assert call(w=None) == E.LSDSORT_ERR_WORKSPACE
    assert call(w=fake + 128) == E.LSDSORT_ERR_WORKSPACE
    need = L.lsdsort_sample16_workspace_bytes(rows, cols)
    assert need > 0 and call(wb=need - 1) == E.LSDSORT_ERR_WORKSPACE
    for src in (2, 6, 14):
        assert call(keys=fake + src, w=None) == E.LSDSORT_ERR_WORKSPACE, src               # any 2-byte alignment of the keys
    assert call(rows=3, cols=70001, wb=L.lsdsort_sample16_workspace_bytes(3, 70001) - 1) == E.LSDSORT_ERR_WORKSPACE
    # 8. the device
    import torch

    if not torch.cuda.is_available():
        for kt in (F16, BF16):
            assert call(kt=kt) == E.LSDSORT_ERR_NO_DEVICE
            assert call(kt=kt, lp=None) == E.LSDSORT_ERR_NO_DEVICE
            assert call(kt=kt, rows=3, cols=70001) == E.LSDSORT_ERR_NO_DEVICE
        assert call(keys=fake + 14, u=fake + 12, idx=fake + 4, cols=1001) == E.LSDSORT_ERR_NO_DEVICE


def figure(rows, cols):
    """the control block, 16 B per row, and for rows above 16384 keys 8 B per chunk of the chunk cap min(2048, ceil(cols / 16384));
    every array rounded up to 256 bytes"""
    up = lambda x: -(-x // 256) * 256
    sums = rows * min(2048, -(-cols // 16384)) * 8 if cols > 16384 else 0
    return up(up(256 + rows * 16) + sums)


PINNED = {(1, 1): 512, (10, 1000): 512, (17, 1000): 768, (3, 16384): 512, (3, 16385): 768, (3, 70001): 768, (128, 128256): 10496,
          (1, (1 << 20) + 13): 1280, (4096, 131072): 327936}


def test_workspace_figure():
    from lsdradixsort_amd import errors as E

    L = _lib()
    BIG = E.LSDSORT_MAX_KEYS
    f = L.lsdsort_sample16_workspace_bytes
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
            assert b == figure(rows, cols), (rows, cols, b, figure(rows, cols))
            assert b <= 1024 + 32 * rows + rows * cols // 1024, (rows, cols, b)           # O(rows), never O(rows * cols)
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
    assert f(3, 70001) > f(3, 16384) and f(2, 1 << 24) > f(1, 1 << 24)
    assert f(0, 1000) % 256 == 0 and f(10, 0) % 256 == 0
    assert f(BIG + 1, 1) == 0 and f(1, BIG + 1) == 0 and f(BIG + 1, 0) == 0
    assert f(2, BIG // 2 + 1) == 0 and f(1 << 15, 1 << 15) == 0
    assert f(1, BIG) > 0 and f(BIG, 1) > 0
    for (rows, cols), want in PINNED.items():
        assert f(rows, cols) == want == figure(rows, cols), (rows, cols, f(rows, cols), want)


def test_wrappers_check_their_arguments_before_the_library(no_library):
    import torch

    lsd = no_library

    def fake(dtype, shape=(2, 4)):
        return torch.zeros(shape, dtype=dtype).as_subclass(FakeCuda)

    u2 = fake(torch.float32, (2,))
    for dtype in (torch.float16, torch.bfloat16):
        ok = str(dtype).replace("torch.", "")
        with pytest.raises(TypeError):
            lsd.GPUSample16(torch.zeros((2, 4), dtype=dtype), u2, key_type=ok)           # a CPU tensor
        with pytest.raises(TypeError):
            lsd.sample16_rows(torch.zeros((2, 4), dtype=dtype), 0.5)
        other = "float16" if ok == "bfloat16" else "bfloat16"
        with pytest.raises(TypeError):
            lsd.GPUSample16(fake(dtype), u2, key_type=other)                             # a key type that does not fit the dtype
        for key_type in ("int16", "uint16", "float32", "half", ""):
            with pytest.raises(ValueError):
                lsd.GPUSample16(fake(dtype), u2, key_type=key_type)                      # a key type this entry does not have
        with pytest.raises(TypeError):
            lsd.GPUSample16(fake(dtype, (2, 2, 2)), u2, key_type=ok)                     # 1-D or 2-D only
        with pytest.raises(TypeError):
            lsd.GPUSample16(fake(dtype, (4, 4)).t(), fake(torch.float32, (4,)), key_type=ok)   # contiguous only
        for bad in (torch.zeros(2, dtype=torch.float32), fake(torch.float64, (2,)), fake(torch.int32, (2,)), [0.5, 0.5], 0.5, None,
                    fake(torch.float32, (4,))[::2]):
            with pytest.raises(TypeError):
                lsd.GPUSample16(fake(dtype), bad, key_type=ok)                           # d_u: a contiguous float32 CUDA tensor
        for count in (0, 1, 3, 8):
            with pytest.raises(ValueError):
                lsd.GPUSample16(fake(dtype), fake(torch.float32, (count,)), key_type=ok)
        with pytest.raises(ValueError):
            lsd.GPUSample16(fake(dtype, (4,)), u2, key_type=ok)                          # 1-D input: one row
        for out in (fake(torch.int32, (3,)), fake(torch.int64, (2,)), fake(torch.int32, (2, 1)), torch.zeros(2, dtype=torch.int32)):
            with pytest.raises((TypeError, ValueError)):
                lsd.GPUSample16(fake(dtype), u2, key_type=ok, out=out)
        for logprobs in (fake(torch.float32, (3,)), fake(torch.float64, (2,)), torch.zeros(2, dtype=torch.float32), 1, "yes", None):
            with pytest.raises((TypeError, ValueError)):
                lsd.GPUSample16(fake(dtype), u2, key_type=ok, logprobs=logprobs)
        x = fake(dtype, (3, 2, 4))
        for u in ("0.9", True, fake(torch.int32, (6,)), fake(torch.float16, (6,)), ["a"] * 6):
            with pytest.raises(TypeError, match="^u: "):
                lsd.sample16_rows(x, u)
        for u in ([0.5, 0.5], [0.5] * 7, fake(torch.float32, (5,)), fake(torch.float64, (2, 3, 4))):
            with pytest.raises(ValueError, match="^u: "):
                lsd.sample16_rows(x, u)
        with pytest.raises(TypeError, match="^top_p: "):
            lsd.sample16_rows(x, 0.5, top_p="0.9")
        with pytest.raises(ValueError, match="^top_p: "):
            lsd.sample16_rows(x, 0.5, top_p=[0.9] * 5)
        with pytest.raises(TypeError, match="^k: "):
            lsd.sample16_rows(x, 0.5, top_k="5")
        with pytest.raises(TypeError):
            lsd.sample16_rows(fake(dtype, ()), 0.5)                                      # at least one dimension
        # empty shapes: nothing to do, the library is not reached
        for shape in ((0, 4), (3, 0), (2, 0, 5)):
            got = lsd.sample16_rows(fake(dtype, shape), 0.5)
            assert got.shape == shape[:-1] and got.dtype == torch.int64 and (got == -1).all()
            got, lp = lsd.sample16_rows(fake(dtype, shape), 0.5, return_logprobs=True)
            assert got.shape == lp.shape == shape[:-1] and lp.dtype == torch.float32 and torch.isnan(lp).all()
    for dtype in (torch.int16, torch.float32, torch.int32):
        with pytest.raises(TypeError):
            lsd.sample16_rows(fake(dtype), 0.5)
        with pytest.raises(TypeError):
            lsd.GPUSample16(fake(dtype), u2, key_type="bfloat16")


def test_host_conversions_of_u(no_library):
    import torch

    vec = no_library.api._p_per_row
    for u, want in ((0.5, [0.5] * 4), (1, [1.0] * 4), (0, [0.0] * 4), (-2.5, [-2.5] * 4), ([0.1, 0.5, 1.0, 2.0], [0.1, 0.5, 1.0, 2.0]),
                    (np.array([0.5, 0.25, 0.125, 0.0]), [0.5, 0.25, 0.125, 0.0]),
                    (torch.tensor([[0.5, 0.25], [0.75, 1.5]], dtype=torch.float64), [0.5, 0.25, 0.75, 1.5])):
        got = vec(u, 4, "cpu", "u")
        assert got.dtype == torch.float32 and got.shape == (4,) and got.is_contiguous(), u
        assert got.tolist() == [float(np.float32(v)) for v in want], (u, got)
    own = torch.tensor([0.9, 0.8, 0.7, 0.6], dtype=torch.float32)
    assert vec(own, 4, "cpu", "u").data_ptr() == own.data_ptr()                            # used as it is
    with pytest.raises(TypeError, match="^u: a float"):
        vec(None, 4, "cpu", "u")
    with pytest.raises(ValueError, match=r"^u: one entry per row \(4\), got 3"):
        vec([0.1, 0.2, 0.3], 4, "cpu", "u")
    with pytest.raises(TypeError, match="^p: a float"):                                     # the filter's name stays the default
        vec(None, 4, "cpu")
    with pytest.raises(ValueError, match=r"^p: one entry per row"):
        vec(torch.zeros(5), 4, "cpu")


# ---- the oracle itself -----------------------------------------------------------------------------------------------------------
def _row(values, key_type="bfloat16"):
    return tp.bits_of_values(np.array(values, dtype=np.float32), key_type)


@pytest.mark.parametrize("key_type", sm.TYPES)
def test_the_oracle_on_hand_computed_rows(key_type):
    # [0, -ln 2, -ln 4] has the masses 1, 1/2, 1/4 of 7/4 in exact arithmetic: the boundaries lie at 4/7 and 6/7.  The 16-bit
    # roundings of ln 2 and ln 4 move them by less than 1 %, so u is kept 3 % away from them, and AT a boundary both neighbours pass
    for values, bounds in (([0.0, -math.log(2), -math.log(4)], (4 / 7, 6 / 7)), ([-math.log(4), -math.log(2), 0.0], (1 / 7, 3 / 7))):
        row = _row(values, key_type)
        w, C, Z = sm.cdf(row, key_type)
        assert np.allclose(w, np.exp(np.array(values)), atol=0.01) and abs(Z - 1.75) < 0.02 and C[0] == 0.0 and w.max() == 1.0
        for u, want in ((0.0, 0), (-0.0, 0), (-1.0, 0), (float("nan"), 0), (2.0 ** -149, 0), (bounds[0] - 0.03, 0), (bounds[0] + 0.03, 1),
                        (bounds[1] - 0.03, 1), (bounds[1] + 0.03, 2), (1.0 - 2.0 ** -24, 2), (1.0, 2), (1.5, 2)):
            assert sm.exact_index(row, u, key_type) == want, (values, u)
            assert sm.acceptable(row, u, key_type) == [want], (values, u)
        exact = [float(C[1] / Z), float(C[2] / Z)]
        assert sm.acceptable(row, np.float32(exact[0]), key_type) == [0, 1] and sm.acceptable(row, np.float32(exact[1]), key_type) == [1, 2]
        assert abs(sm.logprob64(row, int(np.argmax(w)), key_type) + math.log(1.75)) < 0.02
        assert abs(sm.logprob64(row, int(np.argmin(w)), key_type) + math.log(7)) < 0.02
    pinf, ninf = tp.POS_INF[key_type], tp.NEG_INF[key_type]
    # a key without mass is never drawn: NaNs, and -inf under a finite maximum; u = 0 draws the first key that has mass, u >= 1 the last
    row = np.array([0x7FFF, ninf, _row([1.0], key_type)[0], 0xFFFF, ninf, _row([1.0], key_type)[0], ninf, pinf + 1], dtype=np.uint16)
    for u, want in ((0.0, 2), (0.49, 2), (0.51, 5), (1.0, 5), (7.0, 5), (float("nan"), 2)):
        assert sm.exact_index(row, u, key_type) == want and sm.acceptable(row, u, key_type) == [want], u
    assert sm.acceptable(row, 0.5, key_type) == [2, 5]
    assert sm.logprob64(row, 2, key_type) == -math.log(2)
    # several +inf carry all the mass (x == m)
    row = np.array([_row([3.0], key_type)[0], pinf, 0x7FFF, pinf, ninf], dtype=np.uint16)
    assert [sm.exact_index(row, u, key_type) for u in (0.0, 0.4, 0.6, 1.0)] == [1, 1, 3, 3] and sm.logprob64(row, 3, key_type) == -math.log(2)
    # a row of -inf alone draws uniformly from its keys
    row = np.full(5, ninf, dtype=np.uint16)
    assert sm.cdf(row, key_type)[2] == 5.0
    assert [sm.exact_index(row, u, key_type) for u in (0.0, 0.19, 0.21, 0.5, 0.79, 0.81, 1.0)] == [0, 0, 1, 2, 3, 4, 4]
    assert sm.logprob64(row, 4, key_type) == -math.log(5)
    # a row of NaNs: no number, index -1, logprob NaN, whatever u
    row = np.array([0xFFFF, 0x7FFF, ninf + 1, pinf + 1], dtype=np.uint16)
    for u in sm.U_CYCLE:
        assert sm.exact_index(row, u, key_type) == -1 and sm.acceptable(row, u, key_type) == [-1]
    assert math.isnan(sm.logprob64(row, -1, key_type))
    # one key
    for u in sm.U_CYCLE:
        assert sm.acceptable(_row([-5.0], key_type), u, key_type) == [0]
    # check_rows: the accepted index passes, its neighbour and a key without mass do not; a logprob off by more than 2^-11 does not
    row = _row([1.0, 0.0, float("-inf")], key_type)[None, :]
    u = np.array([0.5], dtype=np.float32)
    lp = sm.logprob64(row[0], 0, key_type)
    sm.check_rows(np.array([0]), row, u, key_type, np.array([lp + 0.9 * sm.LOGPROB_TOL]))
    for index, logprob in (([1], None), ([2], None), ([-1], None), ([0], [lp + 1.1 * sm.LOGPROB_TOL]), ([0], [float("nan")])):
        with pytest.raises(AssertionError):
            sm.check_rows(np.array(index), row, u, key_type, None if logprob is None else np.array(logprob))


def test_u_cycle_and_placement_positions():
    assert sm.U_CYCLE.dtype == np.float32 and sm.U_CYCLE.size == 12 and np.isnan(sm.U_CYCLE[-1]) and np.signbit(sm.U_CYCLE[1])
    assert sm.U_CYCLE[2] > 0 and sm.U_CYCLE[2].view(np.uint32) == 1                        # the smallest denormal
    assert (sm.cycle_u(8, 0).view(np.uint32) != sm.cycle_u(8, 1).view(np.uint32)).all()
    assert sm.chunk_len(48, 40000) == 16384 and sm.chunk_len(4096, 131072) == 262144 and sm.chunk_len(128, 128256) == 16384
    at = sm.placement_positions(40000, 16384)
    assert len(at) <= sm.HEAVY and at[0] == 0 and at[-1] == 39999
    for head in range(8):                                                                  # whatever the row's head
        for p in (head - 1, head, head + 7, head + 8, head + 511, head + 512, head + 1023, head + 1024, head + 16383, head + 16384):
            assert p < 0 or p in at, (head, p)
    assert sm.placement_positions(64, 16384) == list(range(16)) + [63]


@pytest.mark.parametrize("key_type", sm.TYPES)
@pytest.mark.parametrize("name", sorted(sm.SHARP_SETS))
@pytest.mark.parametrize("placement", [False, True], ids=["random", "placement"])
def test_sharp_rows_have_exactly_one_acceptable_index(placement, name, key_type):
    """every sharp row of test_gpu_sample16.py: acceptance there is equality with the oracle"""
    for cols in SHARP_COLS:
        keys, u, at = sm.sharp_rows(name, cols, key_type, seed=cols, placement=placement)
        n = min(sm.HEAVY, cols)
        assert keys.shape == (n, cols) and u.dtype == np.float32 and at.shape == (n,) and (np.diff(at) > 0).all()
        assert not (keys == tp.FILL).any()
        sm.assert_sharp(keys, u, key_type)
        assert np.array_equal(sm.exact_rows(keys, u, key_type), at)                        # row j draws heavy key j
        w, C, Z = sm.cdf(keys[0], key_type)
        assert (w[at] / Z >= 0.005).all() and 0.005 > 8 * sm.M                             # every heavy key far above the window
        if placement:
            assert set(sm.placement_positions(cols, sm.chunk_len(n, cols))) <= set(at.tolist())


# ---- kernel resources ------------------------------------------------------------------------------------------------------------
def test_kernels_no_scratch_no_spill_and_recorded_resources():
    if hipcc() is None:
        pytest.skip("no hipcc on this machine")
    res = kernel_resources("sample16.hip")
    names = list(res)
    once = ("sample16_clear_kernel", "sample16_best_kernel", "sample16_sum_kernel", "sample16_pick_kernel", "sample16_locate_kernel")
    for must in once:
        assert sum(must in name for name in names) == 1, (must, names)
    assert sum("sample16_short_kernel" in name for name in names) == 2, names              # wavefront / workgroup
    assert len(names) == len(once) + 2, names
    for name, r in res.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r)
    want = json.load(open(GOLDEN))["sample16.hip"]
    assert sorted(res) == sorted(want), f"kernels gone: {sorted(set(want) - set(res))}, new: {sorted(set(res) - set(want))}"
    for name, w in want.items():
        assert res[name]["occupancy"] >= w["occupancy"], f"{name}: {res[name]['occupancy']} waves/SIMD, recorded {w['occupancy']}"
        assert res[name]["lds_bytes"] == w["lds_bytes"], f"{name}: {res[name]['lds_bytes']} B of static LDS, recorded {w['lds_bytes']}"


def test_the_unit_includes_the_shared_headers_only_and_has_no_inline_assembly():
    csrc = os.path.join(ROOT, "lsdradixsort_amd", "csrc")
    text = open(os.path.join(csrc, "sample16.hip")).read()
    assert set(re.findall(r'#include "([^"]+)"', text)) == {"../../include/lsdsort.h", "keys16_map.hpp", "lsd_device.hpp", "lsd_host.hpp",
                                                             "mass_rows16.hpp", "radix_select.hpp"}
    code = re.sub(r"//.*", "", text)
    assert "asm" not in code
    for name in ("load_tile", "load_head", "locate_tile", "store_tile", "store_head", "same_phase"):   # select_tiles16.hpp's, not this unit's
        assert not re.search(r"\b" + name + r"\b", code), name
    # the mass functions live once, in keys16_map.hpp, for the filter and the draw
    shared = open(os.path.join(csrc, "keys16_map.hpp")).read()
    for name in ("kMassShift", "struct Values16", "bool is_number(", "float value_of(", "uint64_t mass_of(", "uint64_t mass_of_key("):
        assert shared.count(name) >= 1, name
        for unit in ("topp16.hip", "sample16.hip"):
            assert re.sub(r"//.*", "", open(os.path.join(csrc, unit)).read()).count(name if "(" in name or " " in name else name + " =") == 0, (unit, name)
    # the launches the GPU suite runs past their grid caps
    launch = re.compile(r"(\w+_kernel(?:<[^<>]*>)?)[>,(\s]*dim3\(grid_for\(([^,()]+),\s*(\w+)\s*,\s*(\w+)\s*\)\)")
    found = {k: (items.strip(), a, b) for k, items, a, b in launch.findall(text)}
    assert found["sample16_short_kernel<1>"] == ("rows", "8", "16384") and found["sample16_short_kernel<16>"] == ("rows", "1", "4096")
