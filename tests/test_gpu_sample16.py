"""GPU suite: the draw for float16 / bfloat16 rows -- lsdsort_sample16_device (GPUSample16, sample16_rows) -- against the float64
oracle and the acceptance rule of tests/_sample16.py: a returned index has mass and is consistent with u +- 2^-12 of the row's mass; the
returned logprob is within 2^-11 of float64.  On sharp rows, on rows whose masses are 0 or 1 and against torch that is equality.  The
fault word is read after every call (check_fault=True); the keys and the u's are compared bit for bit after the call.

Boundaries of the implementation (lsdradixsort_amd/csrc/sample16.hip): rows of up to 1024 keys take one wavefront (eight rows per
workgroup, so the u's cycle from row to row), up to 16384 one workgroup of 16 wavefronts, longer ones many workgroups per row in chunks
of 16384 keys; every row is read from its own first 16-byte line on, in 16-byte loads of eight keys per lane, 512 keys per lane round
and 1024 per wave tile."""
import numpy as np
import pytest
import torch

import lsdradixsort_amd as lsd
import _rowk16 as rk
import _sample16 as sm
import _topp16 as tp
from _device_arrays import DTYPES, bits, captured, fault_word, stream_ptr, to_dev
from _guarded import assert_intact, guarded, guarded_workspace
from _guarded16 import assert_intact16, bits_of, guarded16
from _key_oracle import KEY_TYPES16 as KEY_TYPES

pytestmark = pytest.mark.gpu

COLS = (1, 2, 7, 8, 9, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 4097, 16383, 16384, 16385, 20481, 32769, 40000, 70001)
ROWS = (1, 3, 8, 9, 17)
SHARP_COLS = (64, 257, 1024, 1025, 16384, 16385, 32769, 40000)
TIER_SHAPES = [(17, 1000), (3, 4099), (3, 70001)]   # one per tier, all with odd or unaligned rows
SENT_INDEX, SENT_LOGPROB = 0x5A5A5A5A, 0x5B5B5B5B


def dev_f32(values):
    return torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32).copy()).cuda()


def draw(keys, u, key_type, what, offset=0):
    """(index, logprob) on the host; the keys and the u's are left alone"""
    dk, d_u = to_dev(keys, key_type, offset), dev_f32(u)
    index, logprob = lsd.GPUSample16(dk, d_u, key_type=key_type, logprobs=True, check_fault=True)
    assert index.shape == logprob.shape == (keys.shape[0],) and index.dtype == torch.int32 and logprob.dtype == torch.float32, what
    assert np.array_equal(bits(dk), keys), f"{what}: the keys were changed"
    assert np.array_equal(d_u.cpu().numpy().view(np.uint32), np.asarray(u, dtype=np.float32).view(np.uint32)), f"{what}: the u's were changed"
    return index.cpu().numpy(), logprob.cpu().numpy()


# ---- shapes at the tier, tile and load boundaries ------------------------------------------------------------------------------------
@pytest.mark.parametrize("key_type", sm.TYPES)
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("cols", COLS)
def test_shapes_with_cycling_u(cols, rows, key_type):
    for name, keys in tp.families(rows, cols, key_type, seed=1000 * rows + cols).items():
        for shift in range(0, sm.U_CYCLE.size, rows):
            u = sm.cycle_u(rows, shift)
            index, logprob = draw(keys, u, key_type, f"{name} {rows}x{cols} {key_type}")
            sm.check_rows(index, keys, u, key_type, logprob)
            if name == "all equal":   # q = 2^32 for every key: u n 2^32 is exact in a double
                want = [min(cols - 1, int(np.floor(sm.clip_u(v) * cols))) for v in u]
                assert index.tolist() == want, f"{rows}x{cols} {key_type}: rows of equal keys"


@pytest.mark.parametrize("key_type", sm.TYPES)
@pytest.mark.parametrize("name", sorted(sm.SHARP_SETS))
@pytest.mark.parametrize("placement", [False, True], ids=["random", "placement"])
@pytest.mark.parametrize("cols", SHARP_COLS)
def test_sharp_rows_equal_the_float64_oracle(cols, placement, name, key_type):
    """one row per heavy key, u at the midpoint of its interval: exactly one index is acceptable (asserted for these very rows by
    test_sample16_cpu.py); `placement` puts heavy keys on both sides of every load, lane-round, wave-tile and chunk boundary"""
    keys, u, at = sm.sharp_rows(name, cols, key_type, seed=cols, placement=placement)
    index, logprob = draw(keys, u, key_type, f"sharp {name} x{cols} {key_type}", offset=3)
    bad = np.flatnonzero(index != at)
    assert bad.size == 0, f"{bad.size} rows differ from the oracle, first row {bad[0]}: index {index[bad[0]]}, oracle {at[bad[0]]}, u = {u[bad[0]]!r}"
    sm.check_rows(index, keys, u, key_type, logprob)


@pytest.mark.parametrize("key_type", sm.TYPES)
@pytest.mark.parametrize("cols", (65, 4097, 20481))
def test_float_specials_equal_the_float64_oracle(cols, key_type):
    """several +inf, all -inf, NaNs of both signs, all NaN: the masses are 0 or 1, so float64 is exact and so is u n 2^32 in a
    double: the floor(u_c n)-th key of the maximum in position order; -1 and a NaN logprob for a row of NaNs"""
    keys = tp.special_rows(cols, key_type, seed=cols)
    v = tp.values64(keys, key_type)
    for shift in range(sm.U_CYCLE.size):
        u = sm.cycle_u(keys.shape[0], shift)
        index, logprob = draw(keys, u, key_type, f"specials x{cols} {key_type}")
        for r in range(keys.shape[0]):
            number = ~np.isnan(v[r])
            if not number.any():
                assert index[r] == -1 and np.isnan(logprob[r]), (r, index[r], logprob[r])
                continue
            at = np.flatnonzero(number & (v[r] == v[r][number].max()))
            want = at[min(at.size - 1, int(np.floor(sm.clip_u(u[r]) * at.size)))]
            assert index[r] == want, f"row {r}, u = {u[r]!r}: index {index[r]}, want {want} of {at.size} maxima"
            assert abs(float(logprob[r]) + np.log(at.size)) <= sm.LOGPROB_TOL, (r, logprob[r], at.size)


# ---- the raw entry inside guard zones ----------------------------------------------------------------------------------------------
def raw_draw(keys, u, key_type, skip, with_logprob=True, short_by=0):
    rows, cols = keys.shape
    L = lsd.lib()
    kw, kv = guarded16(keys, skip, DTYPES[key_type])
    uw, uv = guarded(np.ascontiguousarray(u, dtype=np.float32).view(np.uint32), 8)
    iw, iv = guarded(np.full(rows, SENT_INDEX, dtype=np.uint32), 4)
    lw, lv = guarded(np.full(rows, SENT_LOGPROB, dtype=np.uint32), 12)
    need = L.lsdsort_sample16_workspace_bytes(rows, cols)
    assert need > 0 and need % 256 == 0
    ww, wv = guarded_workspace(need)
    torch.cuda.synchronize()
    st = L.lsdsort_sample16_device(kv.data_ptr(), rows, cols, uv.data_ptr(), KEY_TYPES[key_type], iv.data_ptr(),
                                   lv.data_ptr() if with_logprob else None, wv.data_ptr(), need - short_by, stream_ptr())
    return st, (kw, kv), (uw, uv), (iw, iv), (lw, lv), (ww, wv)


@pytest.mark.parametrize("shape", [(17, 1000), (17, 1001), (3, 4099), (3, 4100), (3, 70001), (3, 70000)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_phase_of_the_key_buffer_in_guard_bands(shape):
    """odd and even cols, the keys at every even byte offset 0 .. 14; d_index, d_logprob, d_u and the workspace (at its exact
    figure) in guard bands; without d_logprob the index is the same bits and nothing else is written"""
    rows, cols = shape
    keys = tp.normal_rows(rows, cols, "bfloat16", 4, seed=cols)
    u = sm.cycle_u(rows, 4)     # 0.1, 0.5, 0.9, ..
    st, *_ = raw_draw(keys, u, "bfloat16", 2, short_by=1)
    assert st == lsd.errors.LSDSORT_ERR_WORKSPACE, "one byte less than the figure is refused"
    first = None
    for skip in range(0, 16, 2):
        for with_logprob in (True, False):
            st, (kw, kv), (uw, uv), (iw, iv), (lw, lv), (ww, wv) = raw_draw(keys, u, "bfloat16", skip, with_logprob)
            assert st == 0, (st, skip)
            assert lsd.lib().lsdsort_check_device(wv.data_ptr(), None) == 0 and fault_word(wv) == 0, "fault word"
            index, logprob = iv.cpu().numpy(), lv.cpu().numpy().view(np.float32)
            if first is None:
                first = index
                sm.check_rows(first, keys, u, "bfloat16", logprob)
            assert np.array_equal(index, first), f"keys at +{skip}, logprob {with_logprob}: differs from the first result"
            if with_logprob:
                sm.check_rows(index, keys, u, "bfloat16", logprob)
            else:
                assert (lv.cpu().numpy().view(np.uint32) == SENT_LOGPROB).all(), "d_logprob was not passed and was written"
            assert_intact16(keys=kw)
            assert_intact(u=uw, index=iw, logprob=lw, workspace=ww)
            assert np.array_equal(bits_of(kv), keys.reshape(-1)), "the keys were changed"
            assert np.array_equal(uv.cpu().numpy().view(np.uint32), u.view(np.uint32)), "the u's were changed"


# ---- determinism -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key_type", sm.TYPES)
@pytest.mark.parametrize("shape", [(17, 1000), (5, 4099), (5, 70001)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_same_bits_on_every_call_in_any_batch_and_row_slot(shape, key_type):
    rows, cols = shape
    keys = tp.normal_rows(rows, cols, key_type, 4, seed=cols + 7)
    u = np.random.default_rng(cols).random(rows).astype(np.float32)
    dk, d_u = to_dev(keys, key_type), dev_f32(u)

    def both(k, v):
        index, logprob = lsd.GPUSample16(k, v, key_type=key_type, logprobs=True, check_fault=True)
        return index.cpu().numpy(), logprob.cpu().numpy().view(np.uint32)

    first = both(dk, d_u)
    sm.check_rows(first[0], keys, u, key_type, first[1].view(np.float32))
    for call in range(9):
        again = both(dk, d_u)
        assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1]), f"call {call + 2} differs from the first"
    for r in range(rows):
        alone = both(dk[r:r + 1], d_u[r:r + 1])
        assert alone[0][0] == first[0][r] and alone[1][0] == first[1][r], f"row {r} drawn alone differs from the row in its batch"
    # the same (row, u) at other `rows` and in other row slots: reversed, and every row repeated among copies of row 0
    back = both(to_dev(keys[::-1].copy(), key_type, 1), dev_f32(u[::-1]))
    assert np.array_equal(back[0][::-1], first[0]) and np.array_equal(back[1][::-1], first[1]), "the rows in reverse order"
    order = np.array([0, 0, 0] + [r for r in range(rows) for _ in range(2)] + [0] * 4)
    wide = both(to_dev(keys[order], key_type, 5), dev_f32(u[order]))
    assert np.array_equal(wide[0], first[0][order]) and np.array_equal(wide[1], first[1][order]), f"{order.size} rows instead of {rows}"


# ---- graph replay ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", TIER_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_graph_replay_follows_u_and_keys(shape):
    rows, cols = shape
    L = lsd.lib()
    assert L.lsdsort_prepare_device() == 0
    dk = torch.zeros((rows, cols), dtype=torch.int16, device="cuda")
    d_u = torch.full((rows,), 0.5, dtype=torch.float32, device="cuda")
    index = torch.zeros((rows,), dtype=torch.int32, device="cuda")
    logprob = torch.zeros((rows,), dtype=torch.float32, device="cuda")
    ws = torch.empty(L.lsdsort_sample16_workspace_bytes(rows, cols), dtype=torch.uint8, device="cuda")

    def call():
        st = L.lsdsort_sample16_device(dk.data_ptr(), rows, cols, d_u.data_ptr(), KEY_TYPES["bfloat16"], index.data_ptr(), logprob.data_ptr(),
                                       ws.data_ptr(), ws.numel(), stream_ptr())
        assert st == 0, st

    kinds = tp.families(rows, cols, "bfloat16", seed=cols + 4)
    dk.copy_(torch.from_numpy(kinds["normal sigma 1"].view(np.int16)))
    g = captured(call)
    seen = []
    for step, name in enumerate(("normal sigma 4", "lone maximum", "normal sigma 4", "normal sigma 4")):   # the keys change, then only u
        keys = kinds[name]
        u = sm.cycle_u(rows, step + 3)
        dk.copy_(torch.from_numpy(keys.view(np.int16)))
        d_u.copy_(dev_f32(u))
        for replay in range(2):
            index.fill_(-7)
            logprob.fill_(7.0)
            g.replay()
            torch.cuda.synchronize()
            assert fault_word(ws) == 0, f"replay on {name}: fault word {fault_word(ws):#x}"
            sm.check_rows(index.cpu().numpy(), keys, u, "bfloat16", logprob.cpu().numpy())
            seen.append(index.cpu().numpy())
        assert np.array_equal(seen[-1], seen[-2]), "two replays differ"
    assert L.lsdsort_check_device(ws.data_ptr(), None) == 0


# ---- composition: top-k, top-p, sample over the renormalised survivors -------------------------------------------------------------
@pytest.mark.parametrize("key_type", sm.TYPES)
@pytest.mark.parametrize("shape", TIER_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_topk_filter_then_topp_filter_then_draw_on_one_buffer(shape, key_type):
    rows, cols = shape
    keys = tp.normal_rows(rows, cols, key_type, 4, seed=cols + 9)
    k = rk.cycle([50, 1, cols // 2, 0, 7], rows)
    p = tp.cycle_p(rows, 2)
    u = np.random.default_rng(cols + 1).random(rows).astype(np.float32)
    ninf = tp.NEG_INF[key_type]
    d_k, d_p, d_u = torch.from_numpy(k.view(np.int32).copy()).cuda(), dev_f32(p), dev_f32(u)
    x = to_dev(keys, key_type)
    lsd.GPUTopK16Filter(x, d_k, key_type=key_type, largest=True, out=x, check_fault=True)
    lsd.GPUTopP16Filter(x, d_p, key_type=key_type, out=x, check_fault=True)
    index, logprob = lsd.GPUSample16(x, d_u, key_type=key_type, logprobs=True, check_fault=True)
    filtered = bits(x)
    index, logprob = index.cpu().numpy(), logprob.cpu().numpy()
    assert (filtered == ninf).sum() > 0 and (index >= 0).all()
    assert (filtered[np.arange(rows), index] != ninf).all(), "a filled key was drawn"
    assert np.array_equal(filtered[np.arange(rows), index], keys[np.arange(rows), index])
    sm.check_rows(index, filtered, u, key_type, logprob)                # the oracle on the filtered buffer: w(-inf) = 0
    x0 = to_dev(keys, key_type)
    got, lp = lsd.sample16_rows(x0, d_u, top_k=torch.from_numpy(k.view(np.int32).copy()).cuda(), top_p=d_p, return_logprobs=True)
    assert got.dtype == torch.int64 and got.shape == (rows,) and np.array_equal(got.cpu().numpy(), index)
    assert np.array_equal(lp.cpu().numpy().view(np.uint32), logprob.view(np.uint32))
    assert np.array_equal(bits(x0), keys), "sample16_rows filters a copy"
    assert np.array_equal(lsd.sample16_rows(x0, u.tolist(), top_k=k.view(np.int32).tolist(), top_p=p.tolist()).cpu().numpy(), index)


# ---- past the grid caps of the short kernels -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(131072 + 9, 40), (4097 + 3, 1025)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_row_loops_go_round_again(shape):
    """one round of the wave tier covers 8 * 16384 rows, one of the workgroup tier 4096: a second, partly filled round.  Every row is
    the same row with a u of its own -- the sums are computed once and the acceptance rule is applied to all rows at a time --
    except two rows of the second round, which hold other keys and go through the oracle on their own."""
    rows, cols = shape
    stride = 8 * 16384 if cols <= 1024 else 4096
    assert stride < rows < 2 * stride
    row = tp.normal_rows(1, cols, "bfloat16", 4, seed=rows)
    keys = np.tile(row, (rows, 1))
    late = [stride + 1, rows - 1]
    keys[late] = tp.normal_rows(2, cols, "bfloat16", 1, seed=rows + 1)
    u = np.random.default_rng(rows).random(rows).astype(np.float32)
    u[:sm.U_CYCLE.size] = sm.U_CYCLE
    u[stride:] = np.roll(sm.U_CYCLE, 5)[:rows - stride]                  # the rows of the second round
    index, logprob = draw(keys, u, "bfloat16", f"{rows}x{cols}", offset=1)
    w, C, Z = sm.cdf(row[0], "bfloat16")
    uc = np.nan_to_num(u.astype(np.float64), nan=0.0).clip(0.0, 1.0)
    same = np.setdiff1d(np.arange(rows), late)
    i = index[same]
    assert ((i >= 0) & (i < cols)).all()
    ok = (w[i] > 0) & (C[i] <= (uc[same] + sm.M) * Z) & (C[i] + w[i] >= (uc[same] - sm.M) * Z)
    assert ok.all(), f"{(~ok).sum()} rows are not accepted, first row {same[np.flatnonzero(~ok)[0]]}"
    v = tp.values64(row[0], "bfloat16")
    assert np.abs(logprob[same] - ((v[i] - v.max()) - np.log(Z))).max() <= sm.LOGPROB_TOL
    sm.check_rows(index[late], keys[late], u[late], "bfloat16", logprob[late])
    for a in (0, stride - 20, stride, rows - 20):
        sm.check_rows(index[a:a + 20], keys[a:a + 20], u[a:a + 20], "bfloat16", logprob[a:a + 20])


# ---- against torch -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bfloat16", "float16"])
@pytest.mark.parametrize("cols", (257, 4099, 20481))
def test_sharp_rows_against_torch_cumsum_and_searchsorted(cols, dtype):
    """searchsorted(cumsum(softmax(x.float())), u, right=True) on sharp rows without NaNs: float32's cumsum is off by far less than
    the quarter per cent between u and the ends of the drawn key's interval"""
    key_type = str(dtype).replace("torch.", "")
    keys, u, at = sm.sharp_rows("near two", cols, key_type, seed=cols + 1, placement=True, nans=False)
    x, d_u = to_dev(keys, key_type), dev_f32(u)
    want = torch.searchsorted(torch.cumsum(torch.softmax(x.float(), -1), -1), d_u[:, None], right=True).view(-1)
    assert np.array_equal(want.cpu().numpy(), at)
    for form in (u.tolist(), torch.from_numpy(u.astype(np.float64)), d_u):
        got = lsd.sample16_rows(x, form)
        assert got.dtype == torch.int64 and got.shape == (keys.shape[0],) and torch.equal(got, want), type(form)
    got, lp = lsd.sample16_rows(x.view(2, -1, cols), d_u.view(2, -1), return_logprobs=True)
    assert got.shape == lp.shape == (2, keys.shape[0] // 2) and torch.equal(got.view(-1), want)
    ref = torch.log_softmax(x.double(), -1).gather(1, want[:, None]).view(-1)
    assert (lp.view(-1).double() - ref).abs().max().item() <= sm.LOGPROB_TOL
    wide = torch.stack([x, x], dim=2)[:, :, 0]                          # not contiguous: sample16_rows draws from a copy
    assert not wide.is_contiguous() and torch.equal(lsd.sample16_rows(wide, d_u), want)


@pytest.mark.parametrize("key_type", sm.TYPES)
def test_frequencies_of_a_sharp_row(key_type):
    """one sharp row of 48 keys 4096 times with u_r = (r + 1/2) / 4096: every key is drawn 4096 w_i / Z times, to within the
    acceptance window at both ends of its interval (2 M 4096 = 2 draws) and the rounding of the count"""
    keys, _, at = sm.sharp_rows("near two", sm.HEAVY, key_type, seed=48)
    assert keys.shape == (sm.HEAVY, sm.HEAVY) and np.array_equal(at, np.arange(sm.HEAVY))
    n = 4096
    u = ((np.arange(n) + 0.5) / n).astype(np.float32)
    index, logprob = draw(np.tile(keys[0], (n, 1)), u, key_type, "frequencies")
    assert (np.diff(index) >= 0).all(), "the index grows with u"
    w, C, Z = sm.cdf(keys[0], key_type)
    count = np.bincount(index, minlength=sm.HEAVY)
    assert count.sum() == n and np.abs(count - n * w / Z).max() <= 2 * sm.M * n + 1, (count, n * w / Z)


def test_sample16_rows_draws_its_own_u_from_a_generator():
    x = to_dev(tp.normal_rows(64, 5000, "bfloat16", 4, seed=3), "bfloat16").view(4, 16, 5000)
    gen = torch.Generator(device="cuda")
    runs = []
    for seed in (11, 11, 12):
        gen.manual_seed(seed)
        got, lp = lsd.sample16_rows(x, generator=gen, top_k=50, top_p=0.9, return_logprobs=True)
        assert got.shape == lp.shape == (4, 16) and got.dtype == torch.int64 and lp.dtype == torch.float32
        assert ((got >= 0) & (got < 5000)).all() and (lp <= 0).all()
        runs.append(got.cpu().numpy())
    assert np.array_equal(runs[0], runs[1]) and not np.array_equal(runs[0], runs[2])
    gen.manual_seed(11)
    want = torch.rand((64,), dtype=torch.float32, device="cuda", generator=gen)
    assert np.array_equal(lsd.sample16_rows(x, want, top_k=50, top_p=0.9).cpu().numpy(), runs[0])
    assert lsd.sample16_rows(x).shape == (4, 16)                         # the default generator
