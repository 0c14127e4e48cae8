"""CPU suite: per-row temperature and min-p of the 16-bit sampling chain -- the C-ABI surface of lsdsort_topp16_filter_ex_device and
lsdsort_sample16_ex_device, their argument checks without a device, the Python face's optional arguments, and the float64 oracle of
tests/_temper16.py: hand-computed rows, equality with _topp16 / _sample16 at T = 1, and the two conditions the GPU suite leans on --
its sharp inputs admit exactly one answer, and over its random families at most 1 % of the rows have a key within 4 B of theta."""
import math
import os
import re

import numpy as np
import pytest

import _sample16 as sm
import _temper16 as tm
import _topp16 as tp
from _faces import FakeCuda, lib as _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U16, I16, F16, BF16 = range(4)
ENTRIES = ("lsdsort_topp16_filter_ex_device", "lsdsort_sample16_ex_device")


def test_header_ctypes_table_and_units_have_the_entries():
    import ctypes

    from lsdradixsort_amd import _lib as binding

    header = open(os.path.join(ROOT, "include", "lsdsort.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"LSDSORT_API\s+int\s+" + name + r"\s*\(", text), name
        assert name in binding.SIGNATURES and hasattr(_lib(), name)
    flt, drw = (binding.SIGNATURES[name] for name in ENTRIES)
    assert flt[0] == binding.c_int and len(flt[1]) == 12 and flt[1][7] == ctypes.c_uint16 and flt[1][3:6] == [ctypes.c_void_p] * 3
    assert drw[0] == binding.c_int and len(drw[1]) == 11 and drw[1][3:5] == [ctypes.c_void_p] * 2
    doc = header[header.index("TEMPERATURE and a MIN-P"):header.index("lsdsort_topp16_filter_ex_device(const void*")]
    for word in ("NULL", "GREEDY", "2^64", "SAME BITS", "theta", "2^-22", "STRICTER", "replay", "Checks, in order"):
        assert word in doc, word
    doc = header[header.index("The draw with a TEMPERATURE"):header.index("lsdsort_sample16_ex_device(const void*")]
    for word in ("NULL", "greedy", "SAME BITS", "TEMPERED", "2^-22", "replay"):
        assert word in doc, word
    units = {u: open(os.path.join(ROOT, "lsdradixsort_amd", "csrc", u)).read() for u in ("topp16.hip", "sample16.hip", "keys16_map.hpp")}
    for name in ("scale_of(float", "minp_threshold(uint32_t", "minp_theta(float", "mass_of(float x, float best, float c)"):
        assert name in units["keys16_map.hpp"] and name not in units["topp16.hip"] and name not in units["sample16.hip"], name
    assert "1.44269504" not in units["topp16.hip"] + units["sample16.hip"]                # the literal lives in the header alone


def test_filter_argument_checks_in_entry_order():
    from lsdradixsort_amd import errors as E

    L = _lib()
    rows, cols = 10, 1000
    fake = 1 << 20   # never dereferenced: every call below returns before a device is touched
    BIG = E.LSDSORT_MAX_KEYS

    def call(keys=fake, p=fake, mp=fake + 64, t=fake + 128, out=fake + (1 << 16), w=fake, wb=None, rows=rows, cols=cols, kt=BF16, fill=0xFF80):
        if wb is None:
            wb = L.lsdsort_topp16_filter_workspace_bytes(rows, cols)
        return L.lsdsort_topp16_filter_ex_device(keys, rows, cols, p, mp, t, kt, fill, out, w, wb, None)

    for kt in (-1, U16, I16, 4, 100):                                                     # 1. key type
        assert call(kt=kt, rows=BIG + 1, keys=None, out=None, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG, kt
        assert call(kt=kt, rows=0, wb=0) == E.LSDSORT_ERR_INVALID_ARG, kt
    assert call(rows=BIG + 1, cols=1, keys=None, p=fake + 1, out=None, w=None, wb=0) == E.LSDSORT_ERR_TOO_LARGE   # 2. sizes
    assert call(rows=2, cols=BIG // 2 + 1, keys=fake + 1, mp=fake + 2, w=None, wb=0) == E.LSDSORT_ERR_TOO_LARGE
    for kt in (F16, BF16):                                                                # 3. nothing to do
        assert call(kt=kt, rows=0, keys=None, p=None, mp=None, t=None, out=None, w=None, wb=0) == E.LSDSORT_OK
        assert call(kt=kt, cols=0, keys=fake + 1, p=fake + 2, mp=fake + 1, t=fake + 3, out=fake + 1, w=None, wb=0) == E.LSDSORT_OK
    assert call(keys=None, w=None) == E.LSDSORT_ERR_INVALID_ARG                            # 4. keys and out, then the three arrays
    assert call(out=None, w=None) == E.LSDSORT_ERR_INVALID_ARG
    for off in (1, 3, 7):
        assert call(keys=fake + off, w=None) == E.LSDSORT_ERR_INVALID_ARG, off
        assert call(out=fake + off, w=None) == E.LSDSORT_ERR_INVALID_ARG, off
    for off in (1, 2, 3, 6, 13):
        for which in ("p", "mp", "t"):
            assert call(**{which: fake + off}, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG, (which, off)
    assert call(w=None) == E.LSDSORT_ERR_WORKSPACE                                        # 5. the workspace, the old figure
    assert call(w=fake + 128) == E.LSDSORT_ERR_WORKSPACE
    need = L.lsdsort_topp16_filter_workspace_bytes(rows, cols)
    assert call(wb=need - 1) == E.LSDSORT_ERR_WORKSPACE and call(out=fake, wb=need - 1) == E.LSDSORT_ERR_WORKSPACE
    assert call(rows=3, cols=70001, wb=L.lsdsort_topp16_filter_workspace_bytes(3, 70001) - 1) == E.LSDSORT_ERR_WORKSPACE
    for p in (None, fake):                                                                # every NULL combination is accepted
        for mp in (None, fake + 64):
            for t in (None, fake + 128):
                assert call(p=p, mp=mp, t=t, w=None) == E.LSDSORT_ERR_WORKSPACE, (p, mp, t)
    import torch

    if not torch.cuda.is_available():                                                     # 6. the device
        for shape in ((rows, cols), (3, 4099), (3, 70001)):
            for p in (None, fake):
                for mp in (None, fake + 64):
                    for t in (None, fake + 128):
                        assert call(p=p, mp=mp, t=t, rows=shape[0], cols=shape[1]) == E.LSDSORT_ERR_NO_DEVICE, (shape, p, mp, t)
        assert call(out=fake, kt=F16) == E.LSDSORT_ERR_NO_DEVICE
    # the old entry still refuses a NULL d_p
    assert L.lsdsort_topp16_filter_device(fake, rows, cols, None, BF16, 0, fake, None, 0, None) == E.LSDSORT_ERR_INVALID_ARG


def test_draw_argument_checks_in_entry_order():
    from lsdradixsort_amd import errors as E

    L = _lib()
    rows, cols = 10, 1000
    fake = 1 << 20
    BIG = E.LSDSORT_MAX_KEYS

    def call(keys=fake, u=fake + 64, t=fake + 128, index=fake + 256, logprob=fake + 512, w=fake, wb=None, rows=rows, cols=cols, kt=BF16):
        if wb is None:
            wb = L.lsdsort_sample16_workspace_bytes(rows, cols)
        return L.lsdsort_sample16_ex_device(keys, rows, cols, u, t, kt, index, logprob, w, wb, None)

    for kt in (-1, U16, I16, 4, 100):
        assert call(kt=kt, rows=BIG + 1, keys=None, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG, kt
    assert call(rows=BIG + 1, cols=1, keys=None, t=fake + 1, w=None, wb=0) == E.LSDSORT_ERR_TOO_LARGE
    for kt in (F16, BF16):
        assert call(kt=kt, rows=0, keys=None, u=None, t=None, index=None, w=None, wb=0) == E.LSDSORT_OK
        assert call(kt=kt, cols=0, keys=fake + 1, t=fake + 3, w=None, wb=0) == E.LSDSORT_OK
    assert call(keys=None, w=None) == E.LSDSORT_ERR_INVALID_ARG and call(keys=fake + 1, w=None) == E.LSDSORT_ERR_INVALID_ARG
    assert call(u=None, w=None) == E.LSDSORT_ERR_INVALID_ARG and call(index=None, w=None) == E.LSDSORT_ERR_INVALID_ARG
    for off in (1, 2, 3, 6, 13):
        for which in ("u", "t", "index", "logprob"):
            assert call(**{which: fake + off}, w=None, wb=0) == E.LSDSORT_ERR_INVALID_ARG, (which, off)
    assert call(w=None) == E.LSDSORT_ERR_WORKSPACE and call(w=fake + 128) == E.LSDSORT_ERR_WORKSPACE
    assert call(wb=L.lsdsort_sample16_workspace_bytes(rows, cols) - 1) == E.LSDSORT_ERR_WORKSPACE
    for t in (None, fake + 128):
        for logprob in (None, fake + 512):
            assert call(t=t, logprob=logprob, w=None) == E.LSDSORT_ERR_WORKSPACE, (t, logprob)
    import torch

    if not torch.cuda.is_available():
        for shape in ((rows, cols), (3, 4099), (3, 70001)):
            for t in (None, fake + 128):
                for logprob in (None, fake + 512):
                    assert call(t=t, logprob=logprob, rows=shape[0], cols=shape[1]) == E.LSDSORT_ERR_NO_DEVICE, (shape, t, logprob)


# ---- the Python face -------------------------------------------------------------------------------------------------------------------
class _Recorder:
    """stands in for the library: records which entry was called with what, answers OK"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 1 << 12 if name.endswith("workspace_bytes") else 0
        return entry


@pytest.fixture
def face(monkeypatch):
    import torch

    import lsdradixsort_amd as lsd

    rec = _Recorder()
    monkeypatch.setattr(lsd.api, "lib", lambda: rec)
    monkeypatch.setattr(lsd.api, "_temp_workspace", lambda nbytes, device, stream: torch.zeros(nbytes, dtype=torch.uint8))
    monkeypatch.setattr(lsd.api, "_stream", lambda stream: None)

    def fake(dtype, shape):
        return torch.zeros(shape, dtype=dtype).as_subclass(FakeCuda)

    return lsd, rec, fake


def test_the_old_symbols_are_called_when_no_new_argument_is_given(face):
    import torch

    lsd, rec, fake = face
    x, f2 = fake(torch.bfloat16, (2, 4)), lambda: fake(torch.float32, (2,))
    out = fake(torch.bfloat16, (2, 4))
    lsd.GPUTopP16Filter(x, f2(), key_type="bfloat16", out=out)
    lsd.GPUSample16(x, f2(), key_type="bfloat16", out=fake(torch.int32, (2,)))
    names = [n for n, a in rec.calls if n.endswith("_device")]
    assert names == ["lsdsort_topp16_filter_device", "lsdsort_sample16_device"], names
    assert len(rec.calls[1][1]) == 10 and len(rec.calls[-1][1]) == 10                       # exactly the old argument lists
    rec.calls.clear()
    p, mp, t = f2(), f2(), f2()
    lsd.GPUTopP16Filter(x, p, key_type="bfloat16", out=out, d_min_p=mp, d_temperature=t)
    lsd.GPUTopP16Filter(x, None, key_type="bfloat16", out=out, d_min_p=mp)
    lsd.GPUTopP16Filter(x, p, key_type="bfloat16", out=out, d_temperature=t)
    lsd.GPUSample16(x, p, key_type="bfloat16", out=fake(torch.int32, (2,)), d_temperature=t)
    got = [(n, a) for n, a in rec.calls if n.endswith("_device")]
    assert [n for n, a in got] == ["lsdsort_topp16_filter_ex_device"] * 3 + ["lsdsort_sample16_ex_device"]
    assert got[0][1][3:6] == (p.data_ptr(), mp.data_ptr(), t.data_ptr())
    assert got[1][1][3:6] == (None, mp.data_ptr(), None) and got[2][1][3:6] == (p.data_ptr(), None, t.data_ptr())
    assert got[3][1][3:5] == (p.data_ptr(), t.data_ptr())


def test_the_new_arguments_are_checked(face):
    import torch

    lsd, rec, fake = face
    x, p2 = fake(torch.bfloat16, (2, 4)), fake(torch.float32, (2,))
    for name in ("d_min_p", "d_temperature"):
        for bad in (torch.zeros(2), fake(torch.float64, (2,)), [0.5, 0.5], 0.5, fake(torch.float32, (4,))[::2]):
            with pytest.raises(TypeError):
                lsd.GPUTopP16Filter(x, p2, key_type="bfloat16", **{name: bad})
        for count in (1, 3):
            with pytest.raises(ValueError):
                lsd.GPUTopP16Filter(x, p2, key_type="bfloat16", **{name: fake(torch.float32, (count,))})
    with pytest.raises(TypeError):
        lsd.GPUTopP16Filter(x, None, key_type="bfloat16")                                  # d_p may be None with d_min_p only
    with pytest.raises(TypeError):
        lsd.GPUTopP16Filter(x, None, key_type="bfloat16", d_temperature=p2)
    for bad in (torch.zeros(2), 0.7, fake(torch.float64, (2,))):
        with pytest.raises(TypeError):
            lsd.GPUSample16(x, p2, key_type="bfloat16", d_temperature=bad)
    with pytest.raises(ValueError):
        lsd.GPUSample16(x, p2, key_type="bfloat16", d_temperature=fake(torch.float32, (3,)))
    assert not [n for n, a in rec.calls if n.endswith("_device")], "the library was reached"
    for kw in ({"min_p": "0.1"}, {"temperature": None, "min_p": True}, {"temperature": fake(torch.int32, (2,))}):
        with pytest.raises(TypeError):
            lsd.topp16_filter_rows(x, 0.9, **kw)
    for kw in ({"min_p": [0.1] * 3}, {"temperature": fake(torch.float32, (5,))}):
        with pytest.raises(ValueError):
            lsd.topp16_filter_rows(x, 0.9, **kw)
        with pytest.raises(ValueError):
            lsd.sample16_rows(x, 0.5, **kw)
    with pytest.raises(TypeError):
        lsd.topp16_filter_rows(x, None)                                                    # p may be None with min_p only
    e = fake(torch.bfloat16, (0, 4))
    assert lsd.topp16_filter_rows(e, None, min_p=0.1, temperature=0.7).shape == e.shape


# ---- the oracle on hand-computed rows ------------------------------------------------------------------------------------------------------
def _row(values, key_type="bfloat16"):
    return tp.bits_of_values(np.array(values, dtype=np.float32), key_type)


def _kept(row, p, mp, T, key_type):
    return (tm.filter_row(row, p, mp, T, key_type) != tm.FILL).tolist()


@pytest.mark.parametrize("key_type", tm.TYPES)
def test_the_oracle_on_hand_computed_rows(key_type):
    # [ln 4, ln 2, 0] at T = 0.5 weighs 16 : 4 : 1 of 21, at T = 2 it weighs 2 : sqrt 2 : 1 of 4.414 (16-bit roundings below 1 %)
    row = _row([math.log(4), math.log(2), 0.0], key_type)
    for T, want in ((0.5, [16 / 21, 4 / 21, 1 / 21]), (2.0, [2 / 4.4142, 1.4142 / 4.4142, 1 / 4.4142]), (1.0, [4 / 7, 2 / 7, 1 / 7])):
        s, mass, A, Z = tm.groups(row, key_type, T)
        assert np.allclose(mass / Z, want, atol=0.01) and mass[0] == 1.0, (T, mass / Z)
    assert _kept(row, 0.8, None, 0.5, key_type) == [True, True, False] and _kept(row, 0.8, None, 2.0, key_type) == [True, True, True]
    assert _kept(row, 0.7, None, 0.5, key_type) == [True, False, False] and _kept(row, 0.7, None, 2.0, key_type) == [True, True, False]
    # min-p: probability ratios to the best are 1/4 and 1/16 at T = 0.5, 0.707 and 0.5 at T = 2
    assert _kept(row, None, 0.2, 0.5, key_type) == [True, True, False] and _kept(row, None, 0.3, 0.5, key_type) == [True, False, False]
    assert _kept(row, None, 0.6, 2.0, key_type) == [True, True, False] and _kept(row, None, 0.4, 2.0, key_type) == [True, True, True]
    assert _kept(row, 0.7, 0.01, 0.5, key_type) == [True, False, False] and _kept(row, 0.99, 0.3, 0.5, key_type) == [True, False, False]   # the stricter
    for mp in (None, 0.0, -1.0, float("nan")):                                             # min-p off
        assert _kept(row, None, mp, 0.5, key_type) == [True] * 3 and _kept(row, 0.7, mp, 0.5, key_type) == [True, False, False]
    # greedy with ties: the maximum's duplicates alone have mass; top-p on keeps the best value alone; the draw is the j-th tie
    row = _row([1.0, 3.0, 2.0, 3.0, 3.0, -1.0], key_type)
    for T in (0.0, -1.0, float("nan"), 2.0 ** -149, 1e-39):
        assert tm.is_greedy(T), T
        w, C, Z = tm.cdf(row, key_type, T)
        assert w.tolist() == [0, 1, 0, 1, 1, 0] and Z == 3.0
        assert _kept(row, 0.9, None, T, key_type) == [False, True, False, True, True, False]
        assert _kept(row, None, 1e-9, T, key_type) == [False, True, False, True, True, False]   # theta = value(m)
        assert [tm.exact_index(row, u, key_type, T) for u in (0.0, 0.3, 0.4, 0.7, 1.0)] == [1, 1, 3, 4, 4]
        assert tm.logprob64(row, 3, key_type, T) == -math.log(3.0)
    assert not tm.is_greedy(2.0 ** -126) and not tm.is_greedy(float("inf")) and tm.scale32(1.0) == float(np.float32(1.44269504088896341))
    assert tm.scale32(float("inf")) == tm.scale32(2.0 ** 65) == float(np.float32(tm.LOG2E / 2.0 ** 64)) > 0
    # mp = 1 and above: the best value alone, every duplicate, the +NaN above them
    row = np.concatenate([_row([2.0, 1.0, 2.0], key_type), np.array([0x7FFF], dtype=np.uint16)])
    for mp in (1.0, 2.0, float("inf")):
        assert _kept(row, None, mp, 0.7, key_type) == [True, False, True, True], mp
    # theta == 0 with both zeros: -0.0 is kept, the number below is not
    row = np.array([0x0000, 0x8000, _row([-0.5], key_type)[0]], dtype=np.uint16)
    assert _kept(row, None, 1.0, 1.0, key_type) == [True, True, False] and _kept(row, None, 0.7, 1.0, key_type) == [True, True, False]
    row = np.array([0x8000, _row([-0.5], key_type)[0], 0x8000], dtype=np.uint16)
    assert _kept(row, None, 1.0, 1.0, key_type) == [True, False, True]
    # -inf under T = +inf: no mass, and min-p drops it although every finite key stays
    ninf, pinf = tp.NEG_INF[key_type], tp.POS_INF[key_type]
    row = np.array([_row([5.0], key_type)[0], ninf, _row([-60.0], key_type)[0]], dtype=np.uint16)
    w, C, Z = tm.cdf(row, key_type, float("inf"))
    assert w[1] == 0.0 and w[0] == 1.0 and abs(w[2] - 1.0) < 1e-15
    assert _kept(row, None, 1e-9, float("inf"), key_type) == [True, False, True]
    # a maximum of +inf: it alone has mass and theta = +inf
    row = np.array([pinf, _row([3.0], key_type)[0], pinf, ninf], dtype=np.uint16)
    for T in (0.5, 2.0, float("inf")):
        assert tm.cdf(row, key_type, T)[0].tolist() == [1, 0, 1, 0]
        assert _kept(row, None, 1e-9, T, key_type) == [True, False, True, False] and _kept(row, 0.9, 0.5, T, key_type) == [True, False, True, False]
    # a row without a number keeps its best key value alone
    row = np.array([0xFFFF, 0x7FFF, ninf + 1, 0x7FFF], dtype=np.uint16)
    assert _kept(row, None, 0.5, 1.0, key_type) == [False, True, False, True]
    # the acceptance rule: in the band both answers pass, outside it one does
    row = _row([1.0, 0.0], key_type)
    inside = np.float32(math.exp(-1.0))
    assert tm.check_row(row, row, None, inside, 1.0, key_type) is None
    assert tm.check_row(np.array([row[0], tm.FILL], dtype=np.uint16), row, None, inside, 1.0, key_type) is None
    assert tm.check_row(row, row, None, 0.5, 1.0, key_type) is not None and tm.check_row(row, row, None, 0.3, 1.0, key_type) is None
    assert tm.check_row(np.array([tm.FILL, row[1]], dtype=np.uint16), row, None, 0.3, 1.0, key_type) is not None
    assert tm.logprob_tol(row, 1, key_type, 2.0 ** -10) == sm.LOGPROB_TOL + 2.0 ** -22 * 1024


@pytest.mark.parametrize("key_type", tm.TYPES)
def test_at_T_1_the_oracle_is_the_siblings_oracle(key_type):
    for cols in (9, 1000, 20001):
        for name, keys in tp.families(3, cols, key_type, seed=cols).items():
            p, u = tp.cycle_p(3, cols), sm.cycle_u(3, cols)
            for r in range(3):
                for mine, theirs in zip(tm.groups(keys[r], key_type), tp.groups(keys[r], key_type)):
                    assert np.array_equal(mine, theirs), name
                for mine, theirs in zip(tm.cdf(keys[r], key_type), sm.cdf(keys[r], key_type)):
                    assert np.array_equal(mine, theirs), name
                if not tp.is_off(p[r]):
                    assert tm.exact_threshold(keys[r], p[r], key_type) == tp.exact_threshold(keys[r], p[r], key_type)
                    assert tm.acceptable(keys[r], p[r], key_type) == tp.acceptable(keys[r], p[r], key_type)
                assert tm.acceptable_index(keys[r], u[r], key_type) == sm.acceptable(keys[r], u[r], key_type)
                i = tm.exact_index(keys[r], u[r], key_type)
                assert i == sm.exact_index(keys[r], u[r], key_type) and tm.logprob64(keys[r], i, key_type) == sm.logprob64(keys[r], i, key_type)
            assert np.array_equal(tm.filter_np(keys, p, None, None, key_type), tp.filter_np(keys, p, key_type)), name
        keys = tp.special_rows(cols, key_type, seed=cols)
        p = tp.cycle_p(keys.shape[0], 3)
        assert np.array_equal(tm.filter_np(keys, p, None, np.ones(keys.shape[0], dtype=np.float32), key_type), tp.filter_np(keys, p, key_type))


# ---- the conditions the GPU suite leans on ---------------------------------------------------------------------------------------------------
SHARP_COLS = (64, 257, 1024, 1025, 16384, 16385, 40000)


@pytest.mark.parametrize("key_type", tm.TYPES)
@pytest.mark.parametrize("name", sorted(tp.SHARP_SETS))
def test_sharp_inputs_admit_exactly_one_answer(name, key_type):
    filters = draws = 0
    for cols in SHARP_COLS:
        keys, mp, T = tm.sharp_minp_rows(name, cols, key_type, seed=cols)
        assert keys.shape[0] >= 2 and keys.shape[0] == mp.size == T.size
        tm.assert_sharp_minp(keys, mp, T, key_type)
        kept = (tm.filter_np(keys, None, mp, T, key_type) != tm.FILL).sum(axis=1)
        assert (np.diff(kept) > 0).all() and 0 < kept[0] and kept[-1] < cols, kept        # pair j in turn is the threshold
        filters += keys.shape[0]
        for T1 in (0.5, 2.0):
            keys, p = tm.sharp_topp_rows(name, cols, key_type, T1, seed=cols)
            assert keys.shape[0] >= 2
            tm.assert_sharp_topp(keys, p, np.full(p.size, T1), key_type)
            filters += keys.shape[0]
            for placement in (False, True):
                keys, u, at = tm.sharp_draw_rows(name, cols, key_type, T1, seed=cols, placement=placement)
                assert keys.shape[0] >= 8
                tm.assert_sharp_draw(keys, u, np.full(u.size, T1), key_type)
                assert [tm.exact_index(keys[r], u[r], key_type, T1) for r in range(u.size)] == at.tolist()
                draws += keys.shape[0]
    assert filters >= 40 and draws >= 200


@pytest.mark.parametrize("key_type", tm.TYPES)
def test_the_band_is_met_by_at_most_one_row_in_a_hundred(key_type):
    """over every random-family input of test_gpu_temper16.py (the same generator), the rows with a key within 4 B of theta"""
    rows = hit = 0
    for cols in tm.COLS:
        for name, keys, p, mp, T in tm.family_cases(cols, key_type):
            rows += keys.shape[0]
            hit += tm.rows_in_band(keys, mp, T, key_type)
    assert rows > 2000 and hit <= rows // 100, (hit, rows)
