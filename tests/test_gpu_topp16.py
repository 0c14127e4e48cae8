"""GPU suite: the top-p filter for float16 / bfloat16 rows -- lsdsort_topp16_filter_device (GPUTopP16Filter, topp16_filter_rows) --
against the float64 oracle and the acceptance rule of tests/_topp16.py: a returned row is every key at least as good as its worst
kept value T and the fill word elsewhere, bit for bit, and T is consistent with p +- 2^-12 of the row's mass.  On sharp rows, on rows
whose masses are 0 or 1 and against torch that is equality with the oracle.  The fill word 0x7E7E occurs nowhere in the inputs; the
fault word is read after every call (check_fault=True).

Boundaries of the implementation (lsdradixsort_amd/csrc/topp16.hip): rows of up to 1024 keys take one wavefront (eight rows per
workgroup, so the p's cycle from row to row), up to 16384 one workgroup, longer ones many workgroups per row in chunks of 16384 keys;
every row is read from its own first 16-byte line on; stores are 16-byte groups where source and destination rows share their 16-byte
phase and key by key otherwise."""
import numpy as np
import pytest
import torch

import lsdradixsort_amd as lsd
import _rowk16 as rk
import _topp16 as tp
from _device_arrays import DTYPES, bits, captured, fault_word, stream_ptr, to_dev
from _guarded import assert_intact, guarded, guarded_workspace
from _guarded16 import assert_intact16, bits_of, guarded16
from _key_oracle import KEY_TYPES16 as KEY_TYPES

pytestmark = pytest.mark.gpu

COLS = (1, 2, 63, 64, 65, 1023, 1024, 1025, 4097, 16383, 16384, 16385, 20481, 40000, 70001)
ROWS = (1, 3, 8, 9, 17)
SHARP_COLS = (64, 257, 1024, 1025, 16384, 16385, 40000)
TIER_SHAPES = [(17, 1000), (3, 4099), (3, 70001)]   # one per tier, all with odd or unaligned rows


def dev_f32(values):
    return torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32).copy()).cuda()


def run_both(keys, p, key_type, what, offset=0):
    """out of place and in place; the two agree bit for bit, the inputs are left alone.  Returns the result's bits."""
    dk, d_p = to_dev(keys, key_type, offset), dev_f32(p)
    out = lsd.GPUTopP16Filter(dk, d_p, key_type=key_type, fill=tp.FILL, check_fault=True)
    assert out.shape == dk.shape and out.dtype == dk.dtype and out.data_ptr() != dk.data_ptr(), what
    got = bits(out)
    assert np.array_equal(bits(dk), keys), f"{what}: input changed"
    own = dk.clone()
    same = lsd.GPUTopP16Filter(own, d_p, key_type=key_type, fill=tp.FILL, out=own, check_fault=True)
    assert same is own and np.array_equal(bits(own), got), f"{what}: in place differs"
    assert np.array_equal(d_p.cpu().numpy().view(np.uint32), np.asarray(p, dtype=np.float32).view(np.uint32)), f"{what}: the p's were changed"
    return got


# ---- shapes at the tier and tile boundaries ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("key_type", tp.TYPES)
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("cols", COLS)
def test_shapes_with_cycling_p(cols, rows, key_type):
    for name, keys in tp.families(rows, cols, key_type, seed=1000 * rows + cols).items():
        for shift in range(0, tp.P_CYCLE.size, rows):
            p = tp.cycle_p(rows, shift)
            got = run_both(keys, p, key_type, f"{name} {rows}x{cols} {key_type}")
            tp.check_rows(got, keys, p, key_type)
            if name == "all equal":
                assert np.array_equal(got, keys), "a row of equal keys is never filled"
            lowest = np.flatnonzero(p <= 0)
            best = rk.sortable16_np(keys, key_type, True).min(axis=1, keepdims=True)
            only_best = np.where(rk.sortable16_np(keys, key_type, True) == best, keys, np.uint16(tp.FILL))
            assert np.array_equal(got[lowest], only_best[lowest]), f"{name}: p <= 0 keeps the best value and its duplicates alone"


@pytest.mark.parametrize("key_type", tp.TYPES)
@pytest.mark.parametrize("name", sorted(tp.SHARP_SETS))
@pytest.mark.parametrize("cols", SHARP_COLS)
def test_sharp_rows_equal_the_float64_oracle(cols, name, key_type):
    keys, p = tp.sharp_rows(name, cols, key_type, seed=cols)
    tp.assert_sharp(keys, p, key_type)                                  # exactly one acceptable T per row, no row left out
    got = run_both(keys, p, key_type, f"sharp {name} x{cols} {key_type}", offset=3)
    want = tp.filter_np(keys, p, key_type)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"{bad.size} rows differ from the oracle, first row {bad[0]} (value {bad[0]} of the level set, p = {p[bad[0]]!r})"


@pytest.mark.parametrize("key_type", tp.TYPES)
@pytest.mark.parametrize("cols", (65, 4097, 20481))
def test_float_specials_equal_the_float64_oracle(cols, key_type):
    """several +inf, all -inf, NaNs of both signs, all NaN: the masses are 0 or 1, so the oracle is exact"""
    keys = tp.special_rows(cols, key_type, seed=cols)
    for shift in range(tp.P_CYCLE.size):
        p = tp.cycle_p(keys.shape[0], shift)
        got = run_both(keys, p, key_type, f"specials x{cols} {key_type}")
        want = tp.filter_np(keys, p, key_type)
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"p = {p}: {bad.shape[0]} words differ, first at {bad[0]}"


# ---- the raw entry inside guard zones ----------------------------------------------------------------------------------------------
def raw_filter(keys, p, key_type, src_skip, dst_skip, in_place=False, short_by=0):
    rows, cols = keys.shape
    L = lsd.lib()
    kw, kv = guarded16(keys, src_skip, DTYPES[key_type])
    ow, ov = (kw, kv) if in_place else guarded16(np.full(rows * cols, 0x5A5A, dtype=np.uint16), dst_skip)
    pw, pv = guarded(np.ascontiguousarray(p, dtype=np.float32).view(np.uint32), 8)
    need = L.lsdsort_topp16_filter_workspace_bytes(rows, cols)
    assert need > 0 and need % 256 == 0
    ww, wv = guarded_workspace(need)
    torch.cuda.synchronize()
    st = L.lsdsort_topp16_filter_device(kv.data_ptr(), rows, cols, pv.data_ptr(), KEY_TYPES[key_type], tp.FILL, ov.data_ptr(), wv.data_ptr(),
                                        need - short_by, stream_ptr())
    return st, (kw, kv), (ow, ov), (pw, pv), (ww, wv)


@pytest.mark.parametrize("shape", [(9, 999), (3, 4099), (3, 70001)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_source_and_destination_at_different_offsets(shape):
    """odd cols; the source at every even byte offset 0 .. 14 against the destination at every one, and in place at every one"""
    rows, cols = shape
    keys = tp.normal_rows(rows, cols, "bfloat16", 4, seed=cols)
    p = tp.cycle_p(rows, 2)     # 0.1, 0.5, 0.9, ..
    first = None
    for src in range(0, 16, 2):
        for dst in list(range(0, 16, 2)) + [None]:
            st, (kw, kv), (ow, ov), (pw, pv), (ww, wv) = raw_filter(keys, p, "bfloat16", src, dst or 0, in_place=dst is None)
            assert st == 0, (st, src, dst)
            assert lsd.lib().lsdsort_check_device(wv.data_ptr(), None) == 0
            got = bits_of(ov).reshape(rows, cols)
            if first is None:
                first = got
                tp.check_rows(first, keys, p, "bfloat16")
            assert np.array_equal(got, first), f"source at +{src}, destination at +{dst}: differs from the first result"
            assert_intact16(keys=kw, out=ow)
            assert_intact(p=pw, workspace=ww)
            assert dst is None or np.array_equal(bits_of(kv), keys.reshape(-1)), "a read-only input was changed"


@pytest.mark.parametrize("skip_bytes", [0, 2, 6, 14])
@pytest.mark.parametrize("shape", TIER_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_guard_bands_and_exact_workspace(shape, skip_bytes):
    rows, cols = shape
    keys = tp.normal_rows(rows, cols, "float16", 4, seed=cols + skip_bytes)
    p = tp.cycle_p(rows, skip_bytes // 2)
    st, *_ = raw_filter(keys, p, "float16", skip_bytes, skip_bytes, short_by=1)
    assert st == lsd.errors.LSDSORT_ERR_WORKSPACE, "one byte less than the figure is refused"
    for in_place in (False, True):
        st, (kw, kv), (ow, ov), (pw, pv), (ww, wv) = raw_filter(keys, p, "float16", skip_bytes, (skip_bytes + 6) % 16, in_place)
        assert st == 0, st
        assert lsd.lib().lsdsort_check_device(wv.data_ptr(), None) == 0
        assert fault_word(wv) == 0, "fault word"
        tp.check_rows(bits_of(ov).reshape(rows, cols), keys, p, "float16")
        assert_intact16(keys=kw, out=ow)
        assert_intact(p=pw, workspace=ww)
        assert np.array_equal(pv.cpu().numpy().view(np.uint32), p.view(np.uint32)), "the p's were changed"


# ---- determinism -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key_type", tp.TYPES)
@pytest.mark.parametrize("shape", [(17, 1000), (5, 4099), (5, 70001)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_same_bits_on_every_call_and_row_by_row(shape, key_type):
    rows, cols = shape
    keys = tp.normal_rows(rows, cols, key_type, 4, seed=cols + 7)
    p = np.random.default_rng(cols).choice(np.array([0.5, 0.8, 0.9, 0.95, 0.99], dtype=np.float32), rows)
    dk, d_p = to_dev(keys, key_type), dev_f32(p)
    first = bits(lsd.GPUTopP16Filter(dk, d_p, key_type=key_type, fill=tp.FILL, check_fault=True))
    tp.check_rows(first, keys, p, key_type)
    again = bits(lsd.GPUTopP16Filter(dk, d_p, key_type=key_type, fill=tp.FILL, check_fault=True))
    assert np.array_equal(first, again), "the same call twice"
    for r in range(rows):
        alone = bits(lsd.GPUTopP16Filter(dk[r:r + 1], d_p[r:r + 1], key_type=key_type, fill=tp.FILL, check_fault=True))
        assert np.array_equal(alone[0], first[r]), f"row {r} filtered alone differs from the row in its batch"
    lsd.set_rank_method(0)
    try:
        assert np.array_equal(bits(lsd.GPUTopP16Filter(dk, d_p, key_type=key_type, fill=tp.FILL, check_fault=True)), first)
    finally:
        lsd.set_rank_method(-1)


# ---- graph replay ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_place", [False, True], ids=["copy", "in place"])
@pytest.mark.parametrize("shape", TIER_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_graph_replay_follows_p_and_keys(shape, in_place):
    rows, cols = shape
    L = lsd.lib()
    assert L.lsdsort_prepare_device() == 0
    dk = torch.zeros((rows, cols), dtype=torch.int16, device="cuda")
    d_p = torch.full((rows,), 0.5, dtype=torch.float32, device="cuda")
    out = dk if in_place else torch.zeros((rows, cols), dtype=torch.int16, device="cuda")
    ws = torch.empty(L.lsdsort_topp16_filter_workspace_bytes(rows, cols), dtype=torch.uint8, device="cuda")

    def call():
        st = L.lsdsort_topp16_filter_device(dk.data_ptr(), rows, cols, d_p.data_ptr(), KEY_TYPES["bfloat16"], tp.FILL, out.data_ptr(),
                                            ws.data_ptr(), ws.numel(), stream_ptr())
        assert st == 0, st

    kinds = tp.families(rows, cols, "bfloat16", seed=cols + 4)
    dk.copy_(torch.from_numpy(kinds["normal sigma 1"].view(np.int16)))
    g = captured(call)
    for step, name in enumerate(("normal sigma 4", "shared top 11 bits", "normal sigma 4", "normal sigma 4")):   # the keys change, then only p
        keys = kinds[name]
        p = tp.cycle_p(rows, step + 1)
        d_p.copy_(dev_f32(p))
        seen = []
        for replay in range(2):
            dk.copy_(torch.from_numpy(keys.view(np.int16)))   # in place the first replay has filtered them
            if not in_place:
                out.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert fault_word(ws) == 0, f"replay on {name}: fault word {fault_word(ws):#x}"
            tp.check_rows(bits(out), keys, p, "bfloat16")
            seen.append(bits(out).copy())
        assert np.array_equal(seen[0], seen[1]), "two replays differ"
    assert L.lsdsort_check_device(ws.data_ptr(), None) == 0


# ---- composition: top-k, then top-p over the renormalised survivors ----------------------------------------------------------------
@pytest.mark.parametrize("key_type", tp.TYPES)
@pytest.mark.parametrize("shape", TIER_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_topk_filter_then_topp_filter_in_place(shape, key_type):
    rows, cols = shape
    keys = tp.normal_rows(rows, cols, key_type, 4, seed=cols + 9)
    k = rk.cycle([50, 1, cols // 2, 0, 7], rows)
    p = tp.cycle_p(rows, 2)
    ninf = tp.NEG_INF[key_type]
    after_k = rk.filter_np(keys, k, key_type, True, fill=ninf)
    d_k, d_p = torch.from_numpy(k.view(np.int32).copy()).cuda(), dev_f32(p)
    x = to_dev(keys, key_type)
    lsd.GPUTopK16Filter(x, d_k, key_type=key_type, largest=True, fill=ninf, out=x, check_fault=True)
    assert np.array_equal(bits(x), after_k)
    y = x.clone()
    lsd.GPUTopP16Filter(y, d_p, key_type=key_type, fill=tp.FILL, out=y, check_fault=True)
    tp.check_rows(bits(y), after_k, p, key_type)                        # the oracle on the top-k-filtered row: w(-inf) = 0
    lsd.GPUTopP16Filter(x, d_p, key_type=key_type, out=x, check_fault=True)   # as a caller composes them: both fill with -inf
    assert np.array_equal(bits(x), np.where(bits(y) == tp.FILL, np.uint16(ninf), bits(y)))


# ---- past the grid caps of the short kernels -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(131072 + 9, 9), (4096 + 3, 1025)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_row_loops_go_round_again(shape):
    """one round of the wave tier covers 8 * 16384 rows, one of the workgroup tier 4096: a second, partly filled round whose rows
    carry other p's than the first round's.  A row's result does not depend on the batch, so the rows of each round filtered in a
    call of their own (one round each) give the expected bits; the first and last rows of every round also go through the oracle."""
    rows, cols = shape
    stride = 8 * 16384 if cols <= 1024 else 4096
    assert stride < rows < 2 * stride
    keys = tp.normal_rows(rows, cols, "bfloat16", 4, seed=rows)
    r = np.arange(rows)
    p = tp.P_CYCLE[(r + r // stride) % tp.P_CYCLE.size]
    assert (p[:-stride].view(np.uint32) != p[stride:].view(np.uint32)).all()
    dk, d_p = to_dev(keys, "bfloat16", 1), dev_f32(p)
    got = bits(lsd.GPUTopP16Filter(dk, d_p, key_type="bfloat16", fill=tp.FILL, check_fault=True))
    parts = [bits(lsd.GPUTopP16Filter(dk[a:b], d_p[a:b], key_type="bfloat16", fill=tp.FILL, check_fault=True)) for a, b in ((0, stride), (stride, rows))]
    bad = np.flatnonzero((got != np.concatenate(parts)).any(axis=1))
    assert bad.size == 0, f"{bad.size} rows differ, first row {bad[0]} = round {bad[0] // stride}, row {bad[0] % stride} of it"
    for a in (0, stride - 40, stride, rows - 40):
        tp.check_rows(got[a:a + 40], keys[a:a + 40], p[a:a + 40], "bfloat16")
    own = dk.clone()
    lsd.GPUTopP16Filter(own, d_p, key_type="bfloat16", fill=tp.FILL, out=own, check_fault=True)
    assert np.array_equal(bits(own), got), "in place"


# ---- the torch-shaped face ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bfloat16", "float16"])
@pytest.mark.parametrize("name", ["near two", "three"])
def test_topp16_filter_rows_against_torch(name, dtype):
    """rows of pairwise distinct values -- permutations of a sharp level set, so torch's sort has no ties to break -- with p at the
    midpoint of each value's mass: sort descending, softmax in float64, cumsum - probs >= p masked, scattered back"""
    key_type = str(dtype).replace("torch.", "")
    levels = tp.SHARP_SETS[name]
    n = levels.size
    rng = np.random.default_rng(n)
    keys = np.stack([levels[rng.permutation(n)] for _ in range(2 * n)])
    p = np.empty(2 * n, dtype=np.float32)
    for r in range(2 * n):
        s, mass, A, Z = tp.groups(keys[r], key_type)
        p[r] = ((2 * A + mass) / (2 * Z))[r % n]
    tp.assert_sharp(keys, p, key_type)
    x = to_dev(keys, key_type).view(2, n, n)
    d_p = dev_f32(p)
    ordered, idx = torch.sort(x.double(), dim=-1, descending=True)
    probs = torch.softmax(ordered, dim=-1)
    mask = torch.cumsum(probs, dim=-1) - probs >= d_p.double().view(2, n, 1)
    want = torch.empty_like(ordered).scatter_(-1, idx, ordered.masked_fill(mask, float("-inf"))).to(dtype)
    for form in (p.tolist(), torch.from_numpy(p.astype(np.float64)), d_p.view(2, n), d_p):
        got = lsd.topp16_filter_rows(x, form)
        assert got.shape == x.shape and got.dtype == x.dtype and got.data_ptr() != x.data_ptr()
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), type(form)
    kept = (want.view(-1, n) != float("-inf")).sum(dim=1).cpu().numpy()
    assert np.array_equal(kept, np.arange(2 * n) % n + 1), "value j of a row keeps j + 1 keys"
    # one p for every row; a fill of the caller's; off rows; in place
    got = lsd.topp16_filter_rows(x, float(p[0]))
    one = torch.empty_like(ordered).scatter_(-1, idx, ordered.masked_fill(torch.cumsum(probs, dim=-1) - probs >= float(p[0]), -7.0)).to(dtype)
    assert torch.equal(lsd.topp16_filter_rows(x, float(p[0]), fill=-7.0).view(torch.int16), one.view(torch.int16))
    assert torch.equal(got.view(torch.int16), torch.where(one == -7.0, torch.tensor(float("-inf"), dtype=dtype, device="cuda"), one).view(torch.int16))
    for off in (1.0, 1.5, float("nan"), 2):
        assert torch.equal(lsd.topp16_filter_rows(x, off).view(torch.int16), x.view(torch.int16)), off
    own = x.clone()
    assert lsd.topp16_filter_rows(own, d_p, inplace=True) is own and torch.equal(own.view(torch.int16), want.view(torch.int16))
