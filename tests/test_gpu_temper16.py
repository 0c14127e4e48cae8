"""GPU suite: per-row temperature and min-p of the 16-bit sampling chain -- lsdsort_topp16_filter_ex_device and
lsdsort_sample16_ex_device (GPUTopP16Filter, GPUSample16, topp16_filter_rows and sample16_rows with min_p / temperature) -- against the
float64 oracle and the acceptance rules of tests/_temper16.py.  With T NULL or 1 and min-p NULL or 0 the ex entries give the bits of
the entries without them.  On sharp rows and on rows whose masses are 0 or 1 acceptance is equality with the oracle
(test_temper16_cpu.py asserts the sharpness of these very inputs).  The fault word is read after every call.

Boundaries of the implementation (topp16.hip, sample16.hip): rows of up to 1024 keys take one wavefront (eight rows per workgroup, so
p, mp, T and u cycle from row to row with coprime periods), up to 16384 one workgroup, longer ones many workgroups per row; in the
long tier a row whose select is off and whose min-p is on runs the best-key kernel and scan 1 only."""
import numpy as np
import pytest
import torch

import lsdradixsort_amd as lsd
import _rowk16 as rk
import _sample16 as sm
import _temper16 as tm
import _topp16 as tp
from _device_arrays import DTYPES, bits, captured, fault_word, stream_ptr, to_dev
from _guarded import assert_intact, guarded, guarded_workspace
from _guarded16 import assert_intact16, bits_of, guarded16
from _key_oracle import KEY_TYPES16 as KEY_TYPES

pytestmark = pytest.mark.gpu

SHARP_COLS = (64, 257, 1024, 1025, 16384, 16385, 40000)
TIER_SHAPES = [(17, 1000), (3, 4099), (3, 70001)]   # one per tier, all with odd or unaligned rows
SENT_INDEX, SENT_LOGPROB = 0x5A5A5A5A, 0x5B5B5B5B


def dev_f32(values):
    return None if values is None else torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32).copy()).cuda()


def ptr(t):
    return None if t is None else t.data_ptr()


def ex_filter(dk, d_p, d_mp, d_t, key_type, out=None):
    """the raw ex entry on device tensors, any of the three arrays None (NULL); returns the result's bits"""
    rows, cols = dk.shape
    L = lsd.lib()
    res = torch.empty_like(dk) if out is None else out
    ws = torch.empty(L.lsdsort_topp16_filter_workspace_bytes(rows, cols), dtype=torch.uint8, device="cuda")
    st = L.lsdsort_topp16_filter_ex_device(dk.data_ptr(), rows, cols, ptr(d_p), ptr(d_mp), ptr(d_t), KEY_TYPES[key_type], tp.FILL,
                                           res.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr())
    assert st == 0, st
    torch.cuda.synchronize()
    assert fault_word(ws) == 0, f"fault word {fault_word(ws):#x}"
    return bits(res)


def filter_both(keys, p, mp, T, key_type, what, offset=0):
    """the ex entry out of place and in place: the two agree bit for bit, the inputs are left alone.  Returns the result's bits."""
    dk, d_p, d_mp, d_t = to_dev(keys, key_type, offset), dev_f32(p), dev_f32(mp), dev_f32(T)
    got = ex_filter(dk, d_p, d_mp, d_t, key_type)
    assert np.array_equal(bits(dk), keys), f"{what}: input changed"
    own = dk.clone()
    assert np.array_equal(ex_filter(own, d_p, d_mp, d_t, key_type, out=own), got), f"{what}: in place differs"
    for name, dev, host in (("p", d_p, p), ("mp", d_mp, mp), ("T", d_t, T)):
        if host is not None:
            assert np.array_equal(dev.cpu().numpy().view(np.uint32), np.asarray(host, dtype=np.float32).view(np.uint32)), f"{what}: {name} was changed"
    return got


def ex_draw(dk, d_u, d_t, key_type, with_logprob=True):
    """the raw ex draw: (index, logprob bits as uint32) on the host"""
    rows, cols = dk.shape
    L = lsd.lib()
    index = torch.full((rows,), -7, dtype=torch.int32, device="cuda")
    logprob = torch.full((rows,), -7.0, dtype=torch.float32, device="cuda") if with_logprob else None
    ws = torch.empty(L.lsdsort_sample16_workspace_bytes(rows, cols), dtype=torch.uint8, device="cuda")
    st = L.lsdsort_sample16_ex_device(dk.data_ptr(), rows, cols, d_u.data_ptr(), ptr(d_t), KEY_TYPES[key_type], index.data_ptr(), ptr(logprob),
                                      ws.data_ptr(), ws.numel(), stream_ptr())
    assert st == 0, st
    torch.cuda.synchronize()
    assert fault_word(ws) == 0, f"fault word {fault_word(ws):#x}"
    return index.cpu().numpy(), (logprob.cpu().numpy() if with_logprob else None)


def draw(keys, u, T, key_type, what, offset=0):
    dk, d_u, d_t = to_dev(keys, key_type, offset), dev_f32(u), dev_f32(T)
    index, logprob = ex_draw(dk, d_u, d_t, key_type)
    assert np.array_equal(bits(dk), keys), f"{what}: the keys were changed"
    return index, logprob


# ---- identity: T NULL or 1, min-p NULL or 0 give the bits of the entries without them ----------------------------------------------
@pytest.mark.parametrize("key_type", tm.TYPES)
@pytest.mark.parametrize("shape", [(17, 1000), (9, 1024), (3, 4099), (5, 16384), (3, 16385), (3, 70001)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_without_temperature_and_min_p_the_bits_are_the_old_entries(shape, key_type):
    rows, cols = shape
    keys = tp.normal_rows(rows, cols, key_type, 4, seed=cols + 1)
    p, u = tp.cycle_p(rows, 2), sm.cycle_u(rows, 3)
    dk, d_p, d_u = to_dev(keys, key_type, 1), dev_f32(p), dev_f32(u)
    ones, zeros = dev_f32(np.ones(rows)), dev_f32(np.zeros(rows))
    old = bits(lsd.GPUTopP16Filter(dk, d_p, key_type=key_type, fill=tp.FILL, check_fault=True))
    for d_mp in (None, zeros):
        for d_t in (None, ones):
            assert np.array_equal(ex_filter(dk, d_p, d_mp, d_t, key_type), old), (d_mp is None, d_t is None)
            own = dk.clone()
            assert np.array_equal(ex_filter(own, d_p, d_mp, d_t, key_type, out=own), old), ("in place", d_mp is None, d_t is None)
    index, logprob = lsd.GPUSample16(dk, d_u, key_type=key_type, logprobs=True, check_fault=True)
    index, logprob = index.cpu().numpy(), logprob.cpu().numpy()
    for d_t in (None, ones):
        got_i, got_l = ex_draw(dk, d_u, d_t, key_type)
        assert np.array_equal(got_i, index) and np.array_equal(got_l.view(np.uint32), logprob.view(np.uint32)), d_t is None
    # the Python face with arrays of ones and zeros reaches the ex entries
    assert np.array_equal(bits(lsd.GPUTopP16Filter(dk, d_p, key_type=key_type, fill=tp.FILL, d_min_p=zeros, d_temperature=ones, check_fault=True)), old)
    assert np.array_equal(lsd.GPUSample16(dk, d_u, key_type=key_type, d_temperature=ones, check_fault=True).cpu().numpy(), index)


# ---- the random families under the cycles ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key_type", tm.TYPES)
@pytest.mark.parametrize("cols", tm.COLS)
def test_families_with_cycling_p_min_p_temperature_and_u(cols, key_type):
    """every family at a row count of its own; from family to family all three arrays, no d_p (min-p alone), no d_min_p (top-p under
    T alone).  Rows with the select off and min-p on lie next to rows with both off and rows with both on: the cycles hold off values."""
    for f, (name, keys, p, mp, T) in enumerate(tm.family_cases(cols, key_type)):
        p, mp = (None if f % 3 == 1 else p), (None if f % 3 == 2 else mp)
        what = f"{name} {keys.shape[0]}x{cols} {key_type}"
        got = filter_both(keys, p, mp, T, key_type, what, offset=f % 8)
        tm.check_rows(got, keys, p, mp, T, key_type)
        if name == "all equal":
            assert np.array_equal(got, keys), "a row of equal keys is never filled"
        u = sm.cycle_u(keys.shape[0], f + cols)
        index, logprob = draw(keys, u, T, key_type, what, offset=f % 8)
        tm.check_draws(index, keys, u, T, key_type, logprob)


@pytest.mark.parametrize("key_type", tm.TYPES)
@pytest.mark.parametrize("cols", (65, 4097, 20481))
def test_float_specials_equal_the_float64_oracle(cols, key_type):
    """several +inf, all -inf, NaNs of both signs, all NaN: the masses are 0 or 1 at every temperature and theta is an infinity, a NaN
    or far from every key, so the oracle is exact"""
    keys = tp.special_rows(cols, key_type, seed=cols)
    rows = keys.shape[0]
    v = tp.values64(keys, key_type)
    for shift in range(0, 14 * 13, 17):
        p, mp, T, u = tp.cycle_p(rows, shift), tm.cycle_mp(rows, shift // 2), tm.cycle_t(rows, shift // 3), sm.cycle_u(rows, shift)
        got = filter_both(keys, p, mp, T, key_type, f"specials x{cols} {key_type}")
        want = tm.filter_np(keys, p, mp, T, key_type)
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"p = {p}, mp = {mp}, T = {T}: {bad.shape[0]} words differ, first at {bad[0]}"
        index, logprob = draw(keys, u, T, key_type, "specials")
        for r in range(rows):
            number = ~np.isnan(v[r])
            if not number.any():
                assert index[r] == -1 and np.isnan(logprob[r]), (r, index[r], logprob[r])
                continue
            at = np.flatnonzero(number & (v[r] == v[r][number].max()))
            want_i = at[min(at.size - 1, int(np.floor(sm.clip_u(u[r]) * at.size)))]
            assert index[r] == want_i and abs(float(logprob[r]) + np.log(at.size)) <= sm.LOGPROB_TOL, (r, T[r], index[r], want_i, logprob[r])


# ---- sharp rows: equality with the oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key_type", tm.TYPES)
@pytest.mark.parametrize("name", sorted(tp.SHARP_SETS))
@pytest.mark.parametrize("cols", SHARP_COLS)
def test_sharp_rows_equal_the_float64_oracle(cols, name, key_type):
    keys, mp, T = tm.sharp_minp_rows(name, cols, key_type, seed=cols)                    # min-p alone: one row per pair of values
    got = filter_both(keys, None, mp, T, key_type, f"sharp min-p {name} x{cols} {key_type}", offset=3)
    want = tm.filter_np(keys, None, mp, T, key_type)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"min-p: {bad.size} rows differ, first row {bad[0]} (mp = {mp[bad[0]]!r}, T = {T[bad[0]]!r})"
    off = np.full(mp.size, 1.0, dtype=np.float32)                                        # the same with a d_p that says "off"
    assert np.array_equal(filter_both(keys, off, mp, T, key_type, "sharp min-p, p off"), want)
    for T1 in (0.5, 2.0):
        keys, p = tm.sharp_topp_rows(name, cols, key_type, T1, seed=cols)                # top-p under T
        Tv = np.full(p.size, T1, dtype=np.float32)
        got = filter_both(keys, p, None, Tv, key_type, f"sharp top-p {name} x{cols} {key_type} T = {T1}", offset=5)
        want = tm.filter_np(keys, p, None, Tv, key_type)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, f"top-p at T = {T1}: {bad.size} rows differ, first row {bad[0]} (p = {p[bad[0]]!r})"
        # both: each row's sharp p with a sharp mp of the same row -- the stricter one wins, exactly
        keys2, mp2, T2 = tm.sharp_minp_rows(name, cols, key_type, seed=cols)
        n = min(p.size, mp2.size)
        mp_T1 = np.float32(np.exp(np.log(mp2[:n].astype(np.float64)) * T2[:n] / T1))     # the same theta under T1
        keys3 = keys[:n]
        tm.assert_sharp_minp(keys3, mp_T1, Tv[:n], key_type)
        got = filter_both(keys3, p[:n][::-1].copy(), mp_T1, Tv[:n], key_type, "sharp both")
        assert np.array_equal(got, tm.filter_np(keys3, p[:n][::-1], mp_T1, Tv[:n], key_type)), f"both at T = {T1}"


@pytest.mark.parametrize("key_type", tm.TYPES)
@pytest.mark.parametrize("name", sorted(tp.SHARP_SETS))
@pytest.mark.parametrize("placement", [False, True], ids=["random", "placement"])
@pytest.mark.parametrize("cols", SHARP_COLS)
def test_sharp_draws_equal_the_float64_oracle(cols, placement, name, key_type):
    for T1 in (0.5, 2.0):
        keys, u, at = tm.sharp_draw_rows(name, cols, key_type, T1, seed=cols, placement=placement)
        Tv = np.full(u.size, T1, dtype=np.float32)
        index, logprob = draw(keys, u, Tv, key_type, f"sharp {name} x{cols} {key_type} T = {T1}", offset=3)
        bad = np.flatnonzero(index != at)
        assert bad.size == 0, f"T = {T1}: {bad.size} rows differ, first row {bad[0]}: index {index[bad[0]]}, oracle {at[bad[0]]}, u = {u[bad[0]]!r}"
        tm.check_draws(index, keys, u, Tv, key_type, logprob)


@pytest.mark.parametrize("key_type", tm.TYPES)
@pytest.mark.parametrize("ties", [1, 2, 37])
@pytest.mark.parametrize("cols", (63, 1025, 4097, 20001))
def test_greedy_rows_draw_the_jth_tie(cols, ties, key_type):
    """every greedy T of the cycle: the j-th duplicate of the maximum in position order, j = floor(u * ties), exact; logprob -ln ties"""
    row, at = tm.greedy_rows(cols, key_type, ties, seed=cols + ties)
    greedy = np.array([t for t in tm.T_CYCLE if tm.is_greedy(t)], dtype=np.float32)
    assert greedy.size == 4
    us = np.array([0.0, 0.26, 0.49, 0.51, 0.76, 1.0 - 2.0 ** -24, 1.0, np.nan], dtype=np.float32)
    u, T = np.repeat(us, greedy.size), np.tile(greedy, us.size)
    keys = np.tile(row, (u.size, 1))
    index, logprob = draw(keys, u, T, key_type, f"greedy x{cols}")
    want = [int(at[min(at.size - 1, int(np.floor(sm.clip_u(v) * at.size)))]) for v in u]
    assert index.tolist() == want
    assert np.abs(logprob + np.log(at.size)).max() <= sm.LOGPROB_TOL
    # a top-p filter that is on keeps the best value alone; min-p likewise
    only = np.where(np.isin(np.arange(cols), at), row, np.uint16(tp.FILL))
    for p, mp in ((np.full(u.size, 0.9), None), (None, np.full(u.size, 1e-9)), (np.full(u.size, 0.5), np.full(u.size, 0.5))):
        got = filter_both(keys, p, mp, T, key_type, "greedy filter")
        assert (got == only[None, :]).all()


def test_frequencies_over_equidistant_u_under_T_2():
    """one sharp row, 4096 equidistant u: every heavy key is drawn 4096 w / Z times, within one for the grid and two for 2 M at the
    interval's two ends"""
    keys, _, at = tm.sharp_draw_rows("near two", 1025, "bfloat16", 2.0, seed=5)
    row = keys[0]
    n = 4096
    u = ((np.arange(n) + 0.5) / n).astype(np.float32)
    Tv = np.full(n, 2.0, dtype=np.float32)
    index, _ = draw(np.tile(row, (n, 1)), u, Tv, "bfloat16", "frequencies")
    w, C, Z = tm.cdf(row, "bfloat16", 2.0)
    count = np.bincount(index, minlength=row.size)
    assert count[w == 0].sum() == 0
    heavy = np.flatnonzero(w / Z >= 0.005)
    assert np.abs(count[heavy] - n * w[heavy] / Z).max() <= 1 + 2 * n * tm.M, np.abs(count[heavy] - n * w[heavy] / Z).max()


# ---- composition on one buffer -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key_type", tm.TYPES)
@pytest.mark.parametrize("shape", TIER_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_topk_filter_then_ex_filter_then_ex_draw_in_place(shape, key_type):
    rows, cols = shape
    keys = tp.normal_rows(rows, cols, key_type, 4, seed=cols + 9)
    k = rk.cycle([50, 1, cols // 2, 0, 7], rows)
    p, mp, T, u = tp.cycle_p(rows, 2), tm.cycle_mp(rows, 4), tm.cycle_t(rows, 5), sm.cycle_u(rows, 4)
    ninf = tp.NEG_INF[key_type]
    after_k = rk.filter_np(keys, k, key_type, True, fill=ninf)
    x = to_dev(keys, key_type)
    lsd.GPUTopK16Filter(x, torch.from_numpy(k.view(np.int32).copy()).cuda(), key_type=key_type, largest=True, fill=ninf, out=x, check_fault=True)
    assert np.array_equal(bits(x), after_k)
    d_p, d_mp, d_t, d_u = dev_f32(p), dev_f32(mp), dev_f32(T), dev_f32(u)
    y = x.clone()
    lsd.GPUTopP16Filter(y, d_p, key_type=key_type, fill=tp.FILL, out=y, d_min_p=d_mp, d_temperature=d_t, check_fault=True)
    tm.check_rows(bits(y), after_k, p, mp, T, key_type)                  # the oracle on the top-k-filtered row: w(-inf) = 0 at any T
    lsd.GPUTopP16Filter(x, d_p, key_type=key_type, out=x, d_min_p=d_mp, d_temperature=d_t, check_fault=True)   # as a caller composes them
    final = np.where(bits(y) == tp.FILL, np.uint16(ninf), bits(y))
    assert np.array_equal(bits(x), final)
    index, logprob = lsd.GPUSample16(x, d_u, key_type=key_type, logprobs=True, d_temperature=d_t, check_fault=True)
    index, logprob = index.cpu().numpy(), logprob.cpu().numpy()
    tm.check_draws(index, final, u, T, key_type, logprob)
    for r in range(rows):                                                # the drawn key survived both filters
        assert bits(y)[r, index[r]] == keys[r, index[r]] != tp.FILL and after_k[r, index[r]] == keys[r, index[r]], r


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bfloat16", "float16"])
def test_sample16_rows_against_a_float32_torch_restatement(dtype):
    """rows of pairwise distinct values (permutations of a sharp level set: no ties for torch to break) under T; top_k = 9 of 12, top_p
    at the midpoint of a value's mass among the nine, min_p at the midpoint between two values, u at the midpoint of a survivor"""
    key_type = str(dtype).replace("torch.", "")
    levels = tp.SHARP_SETS["near two"]
    n, k = levels.size, 9
    rng = np.random.default_rng(n)
    rows = 4 * n
    keys = np.stack([levels[rng.permutation(n)] for _ in range(rows)])
    T = tm.SHARP_T[np.arange(rows) % tm.SHARP_T.size]
    after_k = rk.filter_np(keys, np.full(rows, k, dtype=np.uint32), key_type, True, fill=tp.NEG_INF[key_type])
    p, mp, u, want = (np.empty(rows, dtype=np.float32) for _ in range(4))
    for r in range(rows):
        s, mass, A, Z = tm.groups(after_k[r], key_type, T[r])
        p[r] = ((2 * A + mass) / (2 * Z))[2 + r % (k - 2)]              # keeps 3 .. 9 values
        v = np.sort(tp.values64(after_k[r], key_type))[::-1]
        j = 1 + (r // 3) % (k - 2)                                      # keeps 2 .. 8 values
        mp[r] = np.exp(((v[j] + v[j + 1]) / 2 - v[0]) / float(T[r]))
    tm.assert_sharp_topp(after_k, p, T, key_type)
    tm.assert_sharp_minp(after_k, mp, T, key_type)
    final = tm.filter_np(after_k, p, mp, T, key_type, fill=tp.NEG_INF[key_type])
    for r in range(rows):
        w, C, Z = tm.cdf(final[r], key_type, T[r])
        live = np.flatnonzero(w > 0)
        i = live[r % live.size]
        u[r], want[r] = (2 * C[i] + w[i]) / (2 * Z), i
    tm.assert_sharp_draw(final, u, T, key_type)
    x = to_dev(keys, key_type)
    got, logprob = lsd.sample16_rows(x, dev_f32(u), top_k=k, top_p=dev_f32(p), min_p=dev_f32(mp), temperature=dev_f32(T), return_logprobs=True)
    assert got.dtype == torch.int64 and got.cpu().numpy().tolist() == want.astype(np.int64).tolist()
    assert np.array_equal(bits(x), keys), "x was changed"
    # the restatement: float32 torch, the three filters one after the other, then the inverse CDF
    logits = x.float() / dev_f32(T)[:, None]
    kth = torch.topk(logits, k, dim=-1).values[:, -1:]
    logits = logits.masked_fill(logits < kth, float("-inf"))
    ordered, idx = torch.sort(logits, dim=-1, descending=True)
    probs = torch.softmax(ordered, dim=-1)
    mask = torch.cumsum(probs, dim=-1) - probs >= dev_f32(p)[:, None]
    logits = torch.empty_like(ordered).scatter_(-1, idx, ordered.masked_fill(mask, float("-inf")))
    probs = torch.softmax(logits, dim=-1)
    logits = logits.masked_fill(probs < dev_f32(mp)[:, None] * probs.max(dim=-1, keepdim=True).values, float("-inf"))
    probs = torch.softmax(logits, dim=-1)
    ref = torch.searchsorted(torch.cumsum(probs, dim=-1), dev_f32(u)[:, None], right=True).view(-1)
    assert ref.cpu().numpy().tolist() == want.astype(np.int64).tolist(), "the restatement disagrees with the oracle"
    ref_logprob = torch.log(probs.gather(-1, ref[:, None])).view(-1)
    assert (logprob - ref_logprob).abs().max().item() <= 2 * sm.LOGPROB_TOL
    # topp16_filter_rows with the same arguments gives the filtered rows
    kept = lsd.topp16_filter_rows(to_dev(after_k, key_type), dev_f32(p), min_p=dev_f32(mp), temperature=dev_f32(T))
    assert np.array_equal(bits(kept), final)
    assert np.array_equal(bits(lsd.topp16_filter_rows(to_dev(after_k, key_type), None, min_p=mp.tolist(), temperature=T.tolist())),
                          tm.filter_np(after_k, None, mp, T, key_type, fill=tp.NEG_INF[key_type]))


# ---- the raw entries inside guard zones ---------------------------------------------------------------------------------------------------
def raw_filter(keys, p, mp, T, key_type, src_skip, dst_skip, in_place=False, short_by=0):
    rows, cols = keys.shape
    L = lsd.lib()
    kw, kv = guarded16(keys, src_skip, DTYPES[key_type])
    ow, ov = (kw, kv) if in_place else guarded16(np.full(rows * cols, 0x5A5A, dtype=np.uint16), dst_skip)
    arrays = [None if a is None else guarded(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32), skip) for a, skip in ((p, 8), (mp, 4), (T, 12))]
    need = L.lsdsort_topp16_filter_workspace_bytes(rows, cols)
    ww, wv = guarded_workspace(need)
    torch.cuda.synchronize()
    st = L.lsdsort_topp16_filter_ex_device(kv.data_ptr(), rows, cols, *[None if a is None else a[1].data_ptr() for a in arrays], KEY_TYPES[key_type],
                                           tp.FILL, ov.data_ptr(), wv.data_ptr(), need - short_by, stream_ptr())
    return st, (kw, kv), (ow, ov), arrays, (ww, wv)


@pytest.mark.parametrize("shape", [(9, 999), (9, 1000), (3, 4099), (3, 4100), (3, 70001), (3, 70000)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_filter_in_guard_bands_with_each_array_present_and_null(shape):
    """odd and even cols; the keys at every even byte offset 0 .. 14, out of place and in place, at the exact workspace figure; every
    combination of the three arrays present and NULL"""
    rows, cols = shape
    keys = tp.normal_rows(rows, cols, "bfloat16", 4, seed=cols)
    full = (tp.cycle_p(rows, 2), tm.cycle_mp(rows, 5), tm.cycle_t(rows, 6))
    st, *_ = raw_filter(keys, *full, "bfloat16", 2, 4, short_by=1)
    assert st == lsd.errors.LSDSORT_ERR_WORKSPACE, "one byte less than the figure is refused"
    for combo in range(8):
        p, mp, T = (a if combo >> i & 1 else None for i, a in enumerate(full))
        first = None
        for src in range(0, 16, 2):
            for in_place in (False, True):
                st, (kw, kv), (ow, ov), arrays, (ww, wv) = raw_filter(keys, p, mp, T, "bfloat16", src, (src + 6) % 16, in_place)
                assert st == 0, (st, combo, src)
                assert lsd.lib().lsdsort_check_device(wv.data_ptr(), None) == 0 and fault_word(wv) == 0
                got = bits_of(ov).reshape(rows, cols)
                if first is None:
                    first = got
                    tm.check_rows(first, keys, p, mp, T, "bfloat16")
                assert np.array_equal(got, first), f"arrays {combo:03b}, keys at +{src}, in place {in_place}: differs from the first result"
                assert_intact16(keys=kw, out=ow)
                assert_intact(workspace=ww, **{f"array{i}": a[0] for i, a in enumerate(arrays) if a is not None})
                assert in_place or np.array_equal(bits_of(kv), keys.reshape(-1)), "a read-only input was changed"
                for a, host in zip(arrays, (p, mp, T)):
                    assert a is None or np.array_equal(a[1].cpu().numpy().view(np.uint32), host.view(np.uint32)), "an array was changed"


@pytest.mark.parametrize("shape", [(17, 1000), (17, 1001), (3, 4099), (3, 4100), (3, 70001), (3, 70000)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_draw_in_guard_bands_with_and_without_temperature(shape):
    rows, cols = shape
    L = lsd.lib()
    keys = tp.normal_rows(rows, cols, "bfloat16", 4, seed=cols)
    u, T = sm.cycle_u(rows, 4), tm.cycle_t(rows, 4)
    need = L.lsdsort_sample16_workspace_bytes(rows, cols)
    for t_host in (T, None):
        first = None
        for skip in range(0, 16, 2):
            kw, kv = guarded16(keys, skip, torch.bfloat16)
            uw, uv = guarded(u.view(np.uint32), 8)
            tw, tv = guarded(T.view(np.uint32), 12) if t_host is not None else (None, None)
            iw, iv = guarded(np.full(rows, SENT_INDEX, dtype=np.uint32), 4)
            lw, lv = guarded(np.full(rows, SENT_LOGPROB, dtype=np.uint32), 12)
            ww, wv = guarded_workspace(need)
            torch.cuda.synchronize()
            call = lambda wb: L.lsdsort_sample16_ex_device(kv.data_ptr(), rows, cols, uv.data_ptr(), ptr(tv), KEY_TYPES["bfloat16"], iv.data_ptr(),
                                                           lv.data_ptr(), wv.data_ptr(), wb, stream_ptr())
            assert call(need - 1) == lsd.errors.LSDSORT_ERR_WORKSPACE
            assert call(need) == 0
            assert L.lsdsort_check_device(wv.data_ptr(), None) == 0 and fault_word(wv) == 0
            index, logprob = iv.cpu().numpy().view(np.int32), lv.cpu().numpy().view(np.float32)
            if first is None:
                first = (index.copy(), logprob.copy())
                tm.check_draws(index, keys, u, t_host, "bfloat16", logprob)
            assert np.array_equal(index, first[0]) and np.array_equal(logprob.view(np.uint32), first[1].view(np.uint32)), f"keys at +{skip}"
            assert_intact16(keys=kw)
            assert_intact(u=uw, index=iw, logprob=lw, workspace=ww, **({"T": tw} if tw is not None else {}))
            assert np.array_equal(bits_of(kv), keys.reshape(-1)), "the keys were changed"


# ---- determinism ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key_type", tm.TYPES)
@pytest.mark.parametrize("shape", [(17, 1000), (5, 4099), (5, 70001)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_same_bits_on_ten_calls_and_row_by_row(shape, key_type):
    rows, cols = shape
    keys = tp.normal_rows(rows, cols, key_type, 4, seed=cols + 7)
    rng = np.random.default_rng(cols)
    p = rng.choice(np.array([0.5, 0.9, 0.99, 1.0], dtype=np.float32), rows)
    mp = rng.choice(np.array([0.0, 0.01, 0.1], dtype=np.float32), rows)
    T = rng.choice(np.array([0.0, 0.5, 0.7, 1.3, 4.0], dtype=np.float32), rows)
    u = rng.random(rows).astype(np.float32)
    dk, d_p, d_mp, d_t, d_u = to_dev(keys, key_type), dev_f32(p), dev_f32(mp), dev_f32(T), dev_f32(u)
    first = ex_filter(dk, d_p, d_mp, d_t, key_type)
    tm.check_rows(first, keys, p, mp, T, key_type)
    index, logprob = ex_draw(dk, d_u, d_t, key_type)
    tm.check_draws(index, keys, u, T, key_type, logprob)
    for again in range(9):
        assert np.array_equal(ex_filter(dk, d_p, d_mp, d_t, key_type), first), "the same filter call again"
        i2, l2 = ex_draw(dk, d_u, d_t, key_type)
        assert np.array_equal(i2, index) and np.array_equal(l2.view(np.uint32), logprob.view(np.uint32)), "the same draw again"
    for r in range(rows):
        alone = ex_filter(dk[r:r + 1], d_p[r:r + 1], d_mp[r:r + 1], d_t[r:r + 1], key_type)
        assert np.array_equal(alone[0], first[r]), f"row {r} filtered alone differs from the row in its batch"
        i1, l1 = ex_draw(dk[r:r + 1], d_u[r:r + 1], d_t[r:r + 1], key_type)
        assert i1[0] == index[r] and l1.view(np.uint32)[0] == logprob.view(np.uint32)[r], f"row {r} drawn alone"


# ---- graph replay --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", TIER_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_graph_replay_follows_every_array_and_the_keys(shape):
    """the ex filter in place and the ex draw on its result, captured once; T, mp, p, u and the keys change between replays and every
    replay equals a fresh call"""
    rows, cols = shape
    L = lsd.lib()
    assert L.lsdsort_prepare_device() == 0
    src = torch.zeros((rows, cols), dtype=torch.int16, device="cuda")
    buf = torch.zeros((rows, cols), dtype=torch.int16, device="cuda")
    d_p, d_mp, d_t, d_u = (torch.full((rows,), 0.5, dtype=torch.float32, device="cuda") for _ in range(4))
    index = torch.zeros(rows, dtype=torch.int32, device="cuda")
    logprob = torch.zeros(rows, dtype=torch.float32, device="cuda")
    ws_f = torch.empty(L.lsdsort_topp16_filter_workspace_bytes(rows, cols), dtype=torch.uint8, device="cuda")
    ws_d = torch.empty(L.lsdsort_sample16_workspace_bytes(rows, cols), dtype=torch.uint8, device="cuda")
    code = KEY_TYPES["bfloat16"]

    def call():
        buf.copy_(src)
        st = L.lsdsort_topp16_filter_ex_device(buf.data_ptr(), rows, cols, d_p.data_ptr(), d_mp.data_ptr(), d_t.data_ptr(), code, tp.NEG_INF["bfloat16"],
                                               buf.data_ptr(), ws_f.data_ptr(), ws_f.numel(), stream_ptr())
        assert st == 0, st
        st = L.lsdsort_sample16_ex_device(buf.data_ptr(), rows, cols, d_u.data_ptr(), d_t.data_ptr(), code, index.data_ptr(), logprob.data_ptr(),
                                          ws_d.data_ptr(), ws_d.numel(), stream_ptr())
        assert st == 0, st

    kinds = tp.families(rows, cols, "bfloat16", seed=cols + 4)
    src.copy_(torch.from_numpy(kinds["normal sigma 1"].view(np.int16)))
    g = captured(call)
    for step, name in enumerate(("normal sigma 4", "shared top 11 bits", "normal sigma 4", "normal sigma 4", "lone maximum")):
        keys = kinds[name]
        p, mp, T, u = tp.cycle_p(rows, step + 1), tm.cycle_mp(rows, 2 * step + 3), tm.cycle_t(rows, 3 * step + 5), sm.cycle_u(rows, step + 3)
        src.copy_(torch.from_numpy(keys.view(np.int16)))
        for dev, host in ((d_p, p), (d_mp, mp), (d_t, T), (d_u, u)):
            dev.copy_(dev_f32(host))
        g.replay()
        torch.cuda.synchronize()
        assert fault_word(ws_f) == 0 and fault_word(ws_d) == 0, name
        got, got_i, got_l = bits(buf).copy(), index.cpu().numpy().copy(), logprob.cpu().numpy().copy()
        fresh = to_dev(keys, "bfloat16")
        lsd.GPUTopP16Filter(fresh, d_p, key_type="bfloat16", out=fresh, d_min_p=d_mp, d_temperature=d_t, check_fault=True)
        fi, fl = lsd.GPUSample16(fresh, d_u, key_type="bfloat16", logprobs=True, d_temperature=d_t, check_fault=True)
        assert np.array_equal(got, bits(fresh)), f"replay {step} on {name}: the filter differs from a fresh call"
        assert np.array_equal(got_i, fi.cpu().numpy()) and np.array_equal(got_l.view(np.uint32), fl.cpu().numpy().view(np.uint32)), f"replay {step}: the draw"
        assert not (keys == tp.NEG_INF["bfloat16"]).any()                 # so -inf can stand for the fill word in the oracle's check
        tm.check_rows(got, keys, p, mp, T, "bfloat16", fill=tp.NEG_INF["bfloat16"])
        tm.check_draws(got_i, got, u, T, "bfloat16", got_l)
    assert L.lsdsort_check_device(ws_f.data_ptr(), None) == 0 and L.lsdsort_check_device(ws_d.data_ptr(), None) == 0


# ---- past the grid caps of the short kernels ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(131073, 8), (4097, 1025)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_row_loops_go_round_again(shape):
    """one round of the wave tier covers 8 * 16384 rows, one of the workgroup tier 4096: a second round of one row.  Off rows,
    select-off rows with min-p on and rows with both on are interleaved by the cycles.  A row's result does not depend on the batch,
    so each round in a call of its own gives the expected bits; the rows around the round boundary also go through the oracle."""
    rows, cols = shape
    stride = 8 * 16384 if cols <= 1024 else 4096
    assert stride < rows < 2 * stride
    keys = tp.normal_rows(rows, cols, "bfloat16", 4, seed=rows)
    r = np.arange(rows)
    p, mp, T = tp.P_CYCLE[(r + r // stride) % tp.P_CYCLE.size], tm.MP_CYCLE[(r + 2 * (r // stride)) % tm.MP_CYCLE.size], tm.T_CYCLE[(r + 3 * (r // stride)) % tm.T_CYCLE.size]
    u = sm.U_CYCLE[(r + r // stride) % sm.U_CYCLE.size]
    dk, d_p, d_mp, d_t, d_u = to_dev(keys, "bfloat16", 1), dev_f32(p), dev_f32(mp), dev_f32(T), dev_f32(u)
    got = ex_filter(dk, d_p, d_mp, d_t, "bfloat16")
    index, logprob = ex_draw(dk, d_u, d_t, "bfloat16")
    for a, b in ((0, stride), (stride, rows)):
        part = ex_filter(dk[a:b], d_p[a:b], d_mp[a:b], d_t[a:b], "bfloat16")
        bad = np.flatnonzero((got[a:b] != part).any(axis=1))
        assert bad.size == 0, f"{bad.size} rows differ, first row {a + bad[0]}"
        pi, pl = ex_draw(dk[a:b], d_u[a:b], d_t[a:b], "bfloat16")
        assert np.array_equal(index[a:b], pi) and np.array_equal(logprob[a:b].view(np.uint32), pl.view(np.uint32))
    for a in (0, stride - 40, rows - 41):
        tm.check_rows(got[a:a + 41], keys[a:a + 41], p[a:a + 41], mp[a:a + 41], T[a:a + 41], "bfloat16")
        tm.check_draws(index[a:a + 41], keys[a:a + 41], u[a:a + 41], T[a:a + 41], "bfloat16", logprob[a:a + 41])
    own = dk.clone()
    assert np.array_equal(ex_filter(own, d_p, d_mp, d_t, "bfloat16", out=own), got), "in place"
    assert np.array_equal(ex_filter(dk, None, d_mp, d_t, "bfloat16")[stride - 8:], ex_filter(dk[stride - 8:], None, d_mp[stride - 8:], d_t[stride - 8:], "bfloat16")), "no d_p"
