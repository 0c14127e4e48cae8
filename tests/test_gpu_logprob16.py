"""GPU suite: log-probabilities, ranks and the log-sum-exp of given tokens of float16 / bfloat16 rows -- lsdsort_logprob16_device
(GPULogprob16, logprobs16_rows, top_logprobs16_rows) -- against the float64 oracle of tests/_logprob16.py: a logprob within
2^-11 + 2^-22 |(x - m) / T| (NaN and infinities exactly), a rank exactly, the lse within 2^-11 + 2^-22 |m / T|.  On the index the draw
returned the logprob is the draw's, bit for bit.  The control block is read after every call: this entry raises no fault.

Boundaries of the implementation (lsdradixsort_amd/csrc/logprob16.hip): rows of up to 1024 keys take one wavefront (eight rows per
workgroup, so ids and T cycle from row to row), up to 16384 one workgroup of 16 wavefronts, longer ones one workgroup per chunk of
16384 keys; every row is read from its own first 16-byte line on, in 16-byte loads of eight keys per lane, 512 keys per lane round and
1024 per wave tile."""
import numpy as np
import pytest
import torch

import lsdradixsort_amd as lsd
import _logprob16 as lg
import _sample16 as sm
import _temper16 as tm
import _topp16 as tp
from _device_arrays import bits, captured, stream_ptr, to_dev
from _guarded import assert_intact, guarded, guarded_workspace
from _guarded16 import assert_intact16, bits_of, guarded16
from _key_oracle import KEY_TYPES16 as KEY_TYPES

pytestmark = pytest.mark.gpu

TIER_SHAPES = [(17, 1000), (3, 4099), (3, 70001)]   # one per tier, all with odd or unaligned rows
SENT_LOGPROB, SENT_RANK, SENT_LSE = 0x5B5B5B5B, 0x5A5A5A5A, 0x5C5C5C5C


def dev_f32(values):
    return None if values is None else torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32).copy()).cuda()


def dev_i32(values):
    return torch.from_numpy(np.ascontiguousarray(values, dtype=np.int32).copy()).cuda()


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def ptr(t):
    return None if t is None else t.data_ptr()


def raw(dk, d_ids, d_t, key_type, ranks=True, lse=True, ws=None):
    """the raw entry on device tensors: (logprob, rank or None, lse or None) on the host.  The outputs start as sentinels, so a word
    that was not written shows; the control block is read back and lsdsort_check_device asked."""
    rows, cols = dk.shape
    slots = d_ids.shape[1]
    L = lsd.lib()
    logprob = torch.full((rows, slots), 7.0, dtype=torch.float32, device="cuda")
    rank = torch.full((rows, slots), -7, dtype=torch.int32, device="cuda") if ranks else None
    total = torch.full((rows,), 7.0, dtype=torch.float32, device="cuda") if lse else None
    if ws is None:
        ws = torch.full((L.lsdsort_logprob16_workspace_bytes(rows, cols, slots),), 0x7E, dtype=torch.uint8, device="cuda")
    st = L.lsdsort_logprob16_device(dk.data_ptr(), rows, cols, d_ids.data_ptr(), slots, ptr(d_t), KEY_TYPES[key_type], logprob.data_ptr(), ptr(rank),
                                    ptr(total), ws.data_ptr(), ws.numel(), stream_ptr())
    assert st == 0, st
    assert L.lsdsort_check_device(ws.data_ptr(), None) == 0 and int(ws[:256].view(torch.int32).abs().sum().item()) == 0, "the control block"
    return logprob.cpu().numpy(), (rank.cpu().numpy() if ranks else None), (total.cpu().numpy() if lse else None)


def run(keys, ids, T, key_type, what, offset=0, ranks=True, lse=True):
    """the raw entry on host arrays; the keys, the ids and T are left alone"""
    dk, d_ids, d_t = to_dev(keys, key_type, offset), dev_i32(ids), dev_f32(T)
    got = raw(dk, d_ids, d_t, key_type, ranks, lse)
    assert np.array_equal(bits(dk), keys), f"{what}: the keys were changed"
    assert np.array_equal(d_ids.cpu().numpy(), ids), f"{what}: the ids were changed"
    assert T is None or np.array_equal(u32(d_t.cpu().numpy()), u32(np.asarray(T, dtype=np.float32))), f"{what}: T was changed"
    return got


# ---- the families at the tier, tile and load boundaries -------------------------------------------------------------------------------
@pytest.mark.parametrize("key_type", lg.TYPES)
@pytest.mark.parametrize("cols", lg.COLS)
def test_families_and_specials_with_cycling_slots_temperature_and_ids(cols, key_type):
    """_temper16's reduction: every family at a row count of its own, cycling through ROWS; the slot count cycles through 1, 2, 21 and
    32 from family to family, T through T_CYCLE by row; the ids mix random positions, 0, cols - 1, the argmax, a NaN's and a -inf's
    position and padding of every kind"""
    cases = [(name, keys, T) for name, keys, p, mp, T in tm.family_cases(cols, key_type)]
    special = tp.special_rows(cols, key_type, seed=cols)
    cases.append(("specials", special, lg.cycle_t(special.shape[0], cols)))
    cases.append(("specials, no T", special, None))
    at = lg.COLS.index(cols)
    for f, (name, keys, T) in enumerate(cases):
        slots = lg.SLOTS[(at + f) % len(lg.SLOTS)]
        ids = lg.mixed_ids(keys, slots, key_type, seed=cols + f)
        what = f"{name} {keys.shape[0]}x{cols} {key_type} slots {slots}"
        logprob, rank, lse = run(keys, ids, T, key_type, what, offset=f % 8)
        lg.check_rows(logprob, rank, lse, keys, ids, T, key_type)
        if name == "all equal":
            inside = (ids >= 0) & (ids < cols)
            assert (rank[inside] == 0).all() and np.abs(logprob[inside] + np.log(cols)).max() <= sm.LOGPROB_TOL, what


@pytest.mark.parametrize("key_type", lg.TYPES)
@pytest.mark.parametrize("ties", [1, 3, 37])
@pytest.mark.parametrize("cols", (63, 1025, 20001))
def test_greedy_rows_give_minus_ln_ties_and_minus_infinity(cols, ties, key_type):
    row, at = tm.greedy_rows(cols, key_type, ties, seed=cols + ties)
    greedy = np.array([t for t in tm.T_CYCLE if tm.is_greedy(t)], dtype=np.float32)
    assert greedy.size == 4
    keys = np.tile(row, (greedy.size, 1))
    others = np.setdiff1d(np.arange(cols), at)[:5]
    ids = np.tile(np.concatenate([at[:3], at[-1:], others, [-1]]).astype(np.int32), (greedy.size, 1))
    logprob, rank, lse = run(keys, ids, greedy, key_type, f"greedy x{cols}")
    n = min(3, at.size) + 1
    assert np.abs(logprob[:, :n] + np.log(at.size)).max() <= sm.LOGPROB_TOL and (rank[:, :n] == 0).all()
    assert (logprob[:, n:-1] == -np.inf).all() and (rank[:, n:-1] >= at.size).all()
    assert np.isnan(logprob[:, -1]).all() and (rank[:, -1] == -1).all() and np.isnan(lse).all()
    lg.check_rows(logprob, rank, lse, keys, ids, greedy, key_type)


# ---- the bits of the draw ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key_type", lg.TYPES)
@pytest.mark.parametrize("cols", (513, 16383, 70001))
def test_on_the_drawn_index_the_logprob_is_the_draws_bit_for_bit(cols, key_type):
    rows = 28
    L = lsd.lib()
    keys = tp.normal_rows(rows, cols, key_type, 4, seed=cols + 3)
    keys[3] = tp.special_rows(cols, key_type, seed=1)[1]                 # a row of -inf
    keys[5] = tp.special_rows(cols, key_type, seed=1)[3]                 # a row of NaNs: index -1, a padding id here
    keys[7] = tp.special_rows(cols, key_type, seed=1)[0]                 # +inf among numbers and NaNs
    u = sm.cycle_u(rows, 4)
    dk, d_u = to_dev(keys, key_type, 1), dev_f32(u)
    for T in (None, np.ones(rows, dtype=np.float32), lg.cycle_t(rows, 0)):
        d_t = dev_f32(T)
        index = torch.full((rows,), -7, dtype=torch.int32, device="cuda")
        drawn = torch.full((rows,), 7.0, dtype=torch.float32, device="cuda")
        ws = torch.empty(L.lsdsort_sample16_workspace_bytes(rows, cols), dtype=torch.uint8, device="cuda")
        st = L.lsdsort_sample16_ex_device(dk.data_ptr(), rows, cols, d_u.data_ptr(), ptr(d_t), KEY_TYPES[key_type], index.data_ptr(), drawn.data_ptr(),
                                          ws.data_ptr(), ws.numel(), stream_ptr())
        assert st == 0 and L.lsdsort_check_device(ws.data_ptr(), None) == 0
        logprob, _, _ = raw(dk, index.view(rows, 1), d_t, key_type, ranks=False, lse=False)
        want, got = drawn.cpu().numpy(), logprob[:, 0]
        same = (u32(want) == u32(got)) | (np.isnan(want) & np.isnan(got) & (index.cpu().numpy() < 0))
        assert same.all(), f"T {'NULL' if T is None else T[:3]}: rows {np.flatnonzero(~same)[:4]} differ: draw {want[~same][:4]}, this entry {got[~same][:4]}"
        assert int(index[5]) == -1 and np.isnan(got[5])
        with_ranks, _, _ = raw(dk, index.view(rows, 1), d_t, key_type, ranks=True, lse=True)      # the other outputs change no bit
        assert np.array_equal(u32(with_ranks), u32(logprob))


# ---- against torch ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bfloat16", "float16"])
@pytest.mark.parametrize("slots", [1, 21])
@pytest.mark.parametrize("cols", (1000, 4099, 40001))
def test_against_torch_log_softmax_gather_and_a_count(cols, slots, dtype):
    """normal logits: at sigma 4 a bfloat16 row of this length holds every value many times over, so the ranks are ranks among ties"""
    key_type = str(dtype).replace("torch.", "")
    rows = 12
    keys = tp.normal_rows(rows, cols, key_type, 4, seed=cols + slots)
    assert cols < 40000 or key_type == "float16" or np.unique(keys[0]).size < cols // 4                  # value ties for free
    T = np.array([0.5, 0.7, 1.0, 1.3, 4.0, 1.0], dtype=np.float32)[np.arange(rows) % 6]
    ids = np.random.default_rng(cols).integers(0, cols, (rows, slots)).astype(np.int32)
    x, d_ids, d_t = to_dev(keys, key_type), dev_i32(ids), dev_f32(T)
    logprob, rank, lse = raw(x, d_ids, d_t, key_type)
    scaled = x.float() / d_t[:, None]
    ref = torch.log_softmax(scaled, -1).gather(-1, d_ids.long()).cpu().numpy()
    v = x.gather(-1, d_ids.long())
    ref_rank = torch.stack([(x > v[:, s:s + 1]).sum(-1) for s in range(slots)], dim=1).cpu().numpy()
    m = x.float().max(-1, keepdim=True).values
    gap = ((x.float().gather(-1, d_ids.long()) - m) / d_t[:, None]).abs().cpu().numpy()
    # float32 torch carries its own rounding of x / T and of the sum: twice the entry's bound
    assert (np.abs(logprob - ref) <= 2 * (sm.LOGPROB_TOL + 2.0 ** -22 * gap)).all(), np.abs(logprob - ref).max()
    assert np.array_equal(rank, ref_rank)
    ref_lse = torch.logsumexp(scaled.double(), -1).cpu().numpy()
    assert (np.abs(lse - ref_lse) <= lg.LSE_TOL + 2.0 ** -22 * np.abs((m[:, 0] / d_t).cpu().numpy())).all()
    lg.check_rows(logprob, rank, lse, keys, ids, T, key_type)


# ---- placement ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key_type", lg.TYPES)
@pytest.mark.parametrize("cols", (64, 1024, 1025, 16384, 16385, 40000))
def test_queried_positions_on_both_sides_of_every_boundary_for_every_head(cols, key_type):
    """eight rows of an odd-length array start at eight different phases of a 16-byte line; every row asks for both sides of the head /
    body line, the 8-key load, the 512-key lane round, the 1024-key wave tile and the chunk boundary.  Then the key AT a boundary is
    made the row's lone maximum: a key missed or counted twice there shows in the rank of every other slot and in Z."""
    odd = cols if cols % 2 else cols - 1                                 # rows of an odd length: eight phases within eight rows
    rows = 8
    at = [p for p in sm.placement_positions(odd, sm.chunk_len(rows, odd)) if p < odd]
    keys = tp.normal_rows(rows, odd, key_type, 4, seed=cols)
    T = lg.cycle_t(rows, 4)
    phases = {((2 * r * odd) % 16) // 2 for r in range(rows)}
    assert len(phases) == 8
    for a in range(0, len(at), lg.MAX_SLOTS):
        part = at[a:a + lg.MAX_SLOTS]
        ids = np.tile(np.array(part, dtype=np.int32), (rows, 1))
        logprob, rank, lse = run(keys, ids, T, key_type, f"placement x{odd} {key_type}")
        lg.check_rows(logprob, rank, lse, keys, ids, T, key_type)
    # the key AT each boundary made the row's lone maximum: rank 0 for it, and every other slot's rank counts it
    for p in at[::3]:
        spiked = keys.copy()
        spiked[:, p] = tp.bits_of_values(np.array([60.0]), key_type)[0]
        ids = np.tile(np.array([p, (p + 1) % odd, (p + odd - 1) % odd], dtype=np.int32), (rows, 1))
        logprob, rank, lse = run(spiked, ids, T, key_type, f"spike at {p}")
        assert (rank[:, 0] == 0).all() and (rank[:, 1:] >= 1).all(), p
        lg.check_rows(logprob, rank, lse, spiked, ids, T, key_type)


# ---- the raw entry inside guard zones ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(17, 1000), (17, 1001), (3, 4099), (3, 4100), (3, 70001), (3, 70000)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_phase_of_the_key_buffer_in_guard_bands_with_each_optional_array_present_and_null(shape):
    """odd and even cols, the keys at every even byte offset 0 .. 14; the ids, T, the three outputs and the workspace (at its exact
    figure) in guard bands; every combination of d_rank, d_lse and d_temperature present and NULL: the logprob does not depend on the
    outputs asked for, and an output that was not passed is not written"""
    rows, cols = shape
    slots = 21
    L = lsd.lib()
    keys = tp.normal_rows(rows, cols, "bfloat16", 4, seed=cols)
    ids = lg.mixed_ids(keys, slots, "bfloat16", seed=cols)
    T = lg.cycle_t(rows, 4)
    need = L.lsdsort_logprob16_workspace_bytes(rows, cols, slots)
    assert need > 0 and need % 256 == 0
    first = {}
    for combo in range(8):
        with_rank, with_lse, with_t = (bool(combo >> i & 1) for i in range(3))
        for skip in range(0, 16, 2):
            kw, kv = guarded16(keys, skip, torch.bfloat16)
            iw, iv = guarded(ids.view(np.uint32), 4)
            tw, tv = guarded(T.view(np.uint32), 12) if with_t else (None, None)
            lw, lv = guarded(np.full(rows * slots, SENT_LOGPROB, dtype=np.uint32), 8)
            rw, rv = guarded(np.full(rows * slots, SENT_RANK, dtype=np.uint32), 12)
            sw, sv = guarded(np.full(rows, SENT_LSE, dtype=np.uint32), 4)
            ww, wv = guarded_workspace(need)
            torch.cuda.synchronize()
            call = lambda wb: L.lsdsort_logprob16_device(kv.data_ptr(), rows, cols, iv.data_ptr(), slots, ptr(tv), KEY_TYPES["bfloat16"], lv.data_ptr(),
                                                         rv.data_ptr() if with_rank else None, sv.data_ptr() if with_lse else None, wv.data_ptr(), wb,
                                                         stream_ptr())
            assert call(need - 1) == lsd.errors.LSDSORT_ERR_WORKSPACE, "one byte less than the figure is refused"
            assert call(need) == 0
            assert L.lsdsort_check_device(wv.data_ptr(), None) == 0 and int(wv[:4].view(torch.int32).item()) == 0
            logprob = lv.cpu().numpy().view(np.float32).reshape(rows, slots)
            rank = rv.cpu().numpy().view(np.int32).reshape(rows, slots)
            lse = sv.cpu().numpy().view(np.float32)
            if with_t not in first:
                first[with_t] = logprob.copy()
                lg.check_rows(logprob, None, None, keys, ids, T if with_t else None, "bfloat16")
            assert np.array_equal(u32(logprob), u32(first[with_t])), f"outputs {combo:03b}, keys at +{skip}: the logprob differs from the first result"
            if with_rank or with_lse:
                lg.check_rows(logprob, rank if with_rank else None, lse if with_lse else None, keys, ids, T if with_t else None, "bfloat16")
            assert with_rank or (u32(rank) == SENT_RANK).all(), "d_rank was not passed and was written"
            assert with_lse or (u32(lse) == SENT_LSE).all(), "d_lse was not passed and was written"
            assert_intact16(keys=kw)
            assert_intact(ids=iw, logprob=lw, rank=rw, lse=sw, workspace=ww, **({"T": tw} if with_t else {}))
            assert np.array_equal(bits_of(kv), keys.reshape(-1)), "the keys were changed"
            assert np.array_equal(iv.cpu().numpy().view(np.uint32), ids.view(np.uint32).reshape(-1)), "the ids were changed"


# ---- workspace reuse -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key_type", lg.TYPES)
def test_a_workspace_last_used_by_a_larger_call_shows_nothing_stale(key_type):
    """one workspace: 5 rows of 131073 keys (nine chunks each) with 32 slots, then 3 rows of 20001 keys (two chunks) with 2 slots, then a
    short-tier call, each equal to a call on a fresh workspace"""
    L = lsd.lib()
    ws = torch.full((L.lsdsort_logprob16_workspace_bytes(5, 131073, 32),), 0x7E, dtype=torch.uint8, device="cuda")
    for rows, cols, slots in ((5, 131073, 32), (3, 20001, 2), (5, 131073, 21), (3, 20001, 32), (4, 900, 7), (2, 70001, 1)):
        assert L.lsdsort_logprob16_workspace_bytes(rows, cols, slots) <= ws.numel()
        keys = tp.normal_rows(rows, cols, key_type, 4, seed=cols + slots)
        ids = lg.mixed_ids(keys, slots, key_type, seed=slots)
        T = lg.cycle_t(rows, slots)
        dk, d_ids, d_t = to_dev(keys, key_type), dev_i32(ids), dev_f32(T)
        used = raw(dk, d_ids, d_t, key_type, ws=ws)
        fresh = raw(dk, d_ids, d_t, key_type)
        for a, b, what in zip(used, fresh, ("logprob", "rank", "lse")):
            assert np.array_equal(u32(a), u32(b)), f"{rows}x{cols} slots {slots}: {what} on the used workspace differs"
        lg.check_rows(*used, keys, ids, T, key_type)
        without = raw(dk, d_ids, d_t, key_type, ranks=False, lse=False, ws=ws)               # a call without ranks leaves the counts alone
        assert np.array_equal(u32(without[0]), u32(used[0]))


# ---- determinism -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key_type", lg.TYPES)
@pytest.mark.parametrize("shape", TIER_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_same_bits_on_every_call_in_any_batch_and_row_slot(shape, key_type):
    rows, cols = shape
    slots = 21
    keys = tp.normal_rows(rows, cols, key_type, 4, seed=cols + 7)
    ids = lg.mixed_ids(keys, slots, key_type, seed=cols)
    T = lg.cycle_t(rows, 3)
    dk, d_ids, d_t = to_dev(keys, key_type), dev_i32(ids), dev_f32(T)

    def same(a, b):
        return all(np.array_equal(u32(x), u32(y)) for x, y in zip(a, b))

    first = raw(dk, d_ids, d_t, key_type)
    lg.check_rows(*first, keys, ids, T, key_type)
    for call in range(9):
        assert same(raw(dk, d_ids, d_t, key_type), first), f"call {call + 2} differs from the first"
    for r in range(rows):
        alone = raw(dk[r:r + 1], d_ids[r:r + 1], d_t[r:r + 1], key_type)
        assert same(alone, [x[r:r + 1] for x in first]), f"row {r} alone differs from the row in its batch"
    # the same (row, ids, T) at other `rows` and in other row slots: reversed, and every row repeated among copies of row 0
    back = raw(to_dev(keys[::-1].copy(), key_type, 1), dev_i32(ids[::-1]), dev_f32(T[::-1]), key_type)
    assert same([x[::-1] for x in back], first), "the rows in reverse order"
    order = np.array([0, 0, 0] + [r for r in range(rows) for _ in range(2)] + [0] * 4)
    wide = raw(to_dev(keys[order], key_type, 5), dev_i32(ids[order]), dev_f32(T[order]), key_type)
    assert same(wide, [x[order] for x in first]), f"{order.size} rows instead of {rows}"
    # a slot's answer does not depend on the other slots of its row: every slot alone, and the slots in reverse
    for s in (0, 7, slots - 1):
        one = raw(dk, d_ids[:, s:s + 1].contiguous(), d_t, key_type)
        assert np.array_equal(u32(one[0][:, 0]), u32(first[0][:, s])) and np.array_equal(one[1][:, 0], first[1][:, s]) and np.array_equal(u32(one[2]), u32(first[2]))
    flipped = raw(dk, d_ids.flip(1).contiguous(), d_t, key_type)
    assert np.array_equal(u32(flipped[0][:, ::-1]), u32(first[0])) and np.array_equal(flipped[1][:, ::-1], first[1])


@pytest.mark.parametrize("key_type", lg.TYPES)
def test_the_same_row_gives_the_same_bits_in_every_size_class(key_type):
    """a row of 900 numbers followed by -inf and NaNs up to 1000, 5000 and 40000 keys: the mass and the numbers above a key are the same
    in all three, and so are the bits of the logprob, the ranks and the lse"""
    head = tp.normal_rows(6, 900, key_type, 4, seed=9)
    ids = np.random.default_rng(3).integers(0, 900, (6, 32)).astype(np.int32)
    T = lg.cycle_t(6, 4)
    seen = []
    for cols in (1000, 5000, 40000):
        rest = np.where(np.arange(cols - 900) % 2 == 0, np.uint16(tp.NEG_INF[key_type]), np.uint16(0x7FFF))
        keys = np.concatenate([head, np.tile(rest, (6, 1))], axis=1)
        seen.append(run(keys, ids, T, key_type, f"x{cols}"))
        lg.check_rows(*seen[-1], keys, ids, T, key_type)
    for other in seen[1:]:
        for a, b in zip(seen[0], other):
            assert np.array_equal(u32(a), u32(b))


def test_rows_above_2_to_the_25_keys_take_wider_chunks_and_give_the_same_bits():
    """up to 2^25 keys a long row is cut into chunks of 16384 keys; beyond, into 2048 chunks of whole tiles: at 2^25 + 4099 keys chunks
    of five tiles, 1639 of them, the last one partial.  The 900 numbers of a short row are spread over such a row among -inf and NaNs --
    row 0 evenly, row 1 on both sides of 450 chunk boundaries -- so the integer Z, the counts and with them every bit are those of the
    short row, which goes through the oracle."""
    key_type, n, cols = "bfloat16", 900, (1 << 25) + 4099
    chunk = 5 * 4096
    assert -(-cols // 2048) > 16384 and -(-(-(-cols // 2048)) // 4096) * 4096 == chunk
    small = tp.normal_rows(2, n, key_type, 4, seed=5)
    fill = lambda m: np.where(np.arange(m) % 2 == 0, np.uint16(tp.NEG_INF[key_type]), np.uint16(0x7FFF))
    compact = np.concatenate([small, np.tile(fill(100), (2, 1))], axis=1)
    at = np.stack([np.linspace(0, cols - 1, n).astype(np.int64),
                   np.sort(np.concatenate([np.arange(1, 451) * chunk - 1, np.arange(1, 451) * chunk + 7]))])
    wide = np.tile(fill(cols), (2, 1))
    for r in range(2):
        wide[r, at[r]] = small[r]
    ids = np.random.default_rng(7).integers(0, n, (2, 32)).astype(np.int32)
    T = np.array([0.7, 1.3], dtype=np.float32)
    want = run(compact, ids, T, key_type, "compact")
    lg.check_rows(*want, compact, ids, T, key_type)
    got = run(wide, np.take_along_axis(at, ids.astype(np.int64), axis=1).astype(np.int32), T, key_type, "wide", offset=3)
    for a, b, what in zip(got, want, ("logprob", "rank", "lse")):
        assert np.array_equal(u32(a), u32(b)), what


# ---- graph replay ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", TIER_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_graph_replay_follows_the_ids_the_temperature_and_the_keys(shape):
    rows, cols = shape
    slots = 21
    L = lsd.lib()
    assert L.lsdsort_prepare_device() == 0
    dk = torch.zeros((rows, cols), dtype=torch.int16, device="cuda")
    d_ids = torch.zeros((rows, slots), dtype=torch.int32, device="cuda")
    d_t = torch.full((rows,), 0.5, dtype=torch.float32, device="cuda")
    logprob = torch.zeros((rows, slots), dtype=torch.float32, device="cuda")
    rank = torch.zeros((rows, slots), dtype=torch.int32, device="cuda")
    total = torch.zeros((rows,), dtype=torch.float32, device="cuda")
    ws = torch.empty(L.lsdsort_logprob16_workspace_bytes(rows, cols, slots), dtype=torch.uint8, device="cuda")

    def call():
        st = L.lsdsort_logprob16_device(dk.data_ptr(), rows, cols, d_ids.data_ptr(), slots, d_t.data_ptr(), KEY_TYPES["bfloat16"], logprob.data_ptr(),
                                        rank.data_ptr(), total.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr())
        assert st == 0, st

    kinds = tp.families(rows, cols, "bfloat16", seed=cols + 4)
    dk.copy_(torch.from_numpy(kinds["normal sigma 1"].view(np.int16)))
    g = captured(call)
    for step, name in enumerate(("normal sigma 4", "lone maximum", "lone maximum", "lone maximum", "shared top 11 bits")):
        keys = kinds[name]                                                # the keys change, then only the ids, then only T
        ids = lg.mixed_ids(keys, slots, "bfloat16", seed=min(step, 2))
        T = lg.cycle_t(rows, min(step, 3))
        dk.copy_(torch.from_numpy(keys.view(np.int16)))
        d_ids.copy_(dev_i32(ids))
        d_t.copy_(dev_f32(T))
        seen = []
        for replay in range(2):
            logprob.fill_(7.0)
            rank.fill_(-7)
            total.fill_(7.0)
            g.replay()
            torch.cuda.synchronize()
            seen.append((logprob.cpu().numpy(), rank.cpu().numpy(), total.cpu().numpy()))
        fresh = raw(to_dev(keys, "bfloat16"), dev_i32(ids), dev_f32(T), "bfloat16")
        for a, b, c in zip(seen[0], seen[1], fresh):
            assert np.array_equal(u32(a), u32(b)) and np.array_equal(u32(a), u32(c)), f"replay {step} on {name} differs from a fresh call"
        lg.check_rows(*seen[0], keys, ids, T, "bfloat16")
    assert L.lsdsort_check_device(ws.data_ptr(), None) == 0


# ---- past the grid caps of the short kernels -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(131072 + 9, 8), (4096 + 3, 1025)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_row_loops_go_round_again(shape):
    """one round of the wave tier covers 8 * 16384 rows, one of the workgroup tier 4096: a second, partly filled round.  A row's result
    does not depend on the batch, so each round in a call of its own gives the expected bits; the rows around the round boundary and
    the last ones also go through the oracle."""
    rows, cols = shape
    slots = 5
    stride = 8 * 16384 if cols <= 1024 else 4096
    assert stride < rows < 2 * stride
    keys = tp.normal_rows(rows, cols, "bfloat16", 4, seed=rows)
    rng = np.random.default_rng(rows)
    ids = rng.integers(-1, cols + 1, (rows, slots)).astype(np.int32)
    r = np.arange(rows)
    T = tm.T_CYCLE[(r + 3 * (r // stride)) % tm.T_CYCLE.size]
    dk, d_ids, d_t = to_dev(keys, "bfloat16", 1), dev_i32(ids), dev_f32(T)
    got = raw(dk, d_ids, d_t, "bfloat16")
    for a, b in ((0, stride), (stride, rows)):
        part = raw(dk[a:b], d_ids[a:b], d_t[a:b], "bfloat16")
        for x, y, what in zip(got, part, ("logprob", "rank", "lse")):
            bad = np.flatnonzero((u32(x[a:b]) != u32(y)).reshape(b - a, -1).any(axis=1))
            assert bad.size == 0, f"{what}: {bad.size} rows differ, first row {a + bad[0]}"
    for a in (0, stride - 20, rows - 20):
        lg.check_rows(got[0][a:a + 20], got[1][a:a + 20], got[2][a:a + 20], keys[a:a + 20], ids[a:a + 20], T[a:a + 20], "bfloat16")


# ---- the Python conveniences -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bfloat16", "float16"])
def test_logprobs16_rows_with_forty_ids_per_row_and_any_dimensionality(dtype):
    key_type = str(dtype).replace("torch.", "")
    rows, cols, n = 12, 5000, 40
    keys = tp.normal_rows(rows, cols, key_type, 4, seed=n)
    ids = np.random.default_rng(n).integers(0, cols, (rows, n))
    ids[:, 7] = -1                                                        # padding
    ids[:, 35] = cols
    T = np.array([0.5, 1.0, 1.3], dtype=np.float32)[np.arange(rows) % 3]
    x = to_dev(keys, key_type)
    for form in (torch.from_numpy(ids).cuda(), torch.from_numpy(ids.astype(np.int32)).cuda()):
        logprob, rank, lse = lsd.logprobs16_rows(x, form, temperature=dev_f32(T), return_ranks=True, return_lse=True)
        assert logprob.shape == rank.shape == (rows, n) and lse.shape == (rows,) and logprob.dtype == lse.dtype == torch.float32 and rank.dtype == torch.int64
        lg.check_rows(logprob.cpu().numpy(), rank.cpu().numpy(), lse.cpu().numpy(), keys, ids, T, key_type)
    assert np.array_equal(bits(x), keys), "x was changed"
    inside = torch.from_numpy(np.where((ids < 0) | (ids >= cols), 0, ids)).cuda()
    ref = torch.log_softmax(x.float() / dev_f32(T)[:, None], -1).gather(-1, inside)
    keep = torch.from_numpy((ids >= 0) & (ids < cols)).cuda()
    assert ((logprob - ref).abs()[keep] <= 4 * sm.LOGPROB_TOL).all() and torch.isnan(logprob[~keep]).all() and (rank[~keep] == -1).all()
    # N-dimensional x; ids of x.shape[:-1] and of x.shape[:-1] + (n,); T as a float, a list and a float64 tensor
    x3 = x.view(2, 3, 2, cols)
    one = torch.from_numpy(ids[:, 0].copy()).cuda().view(2, 3, 2)
    got = lsd.logprobs16_rows(x3, one)
    assert got.shape == (2, 3, 2)
    lg.check_rows(got.cpu().numpy().reshape(rows, 1), None, None, keys, ids[:, :1], None, key_type)
    got, lse3 = lsd.logprobs16_rows(x3, torch.from_numpy(ids).cuda().view(2, 3, 2, n), temperature=0.7, return_lse=True)
    assert got.shape == (2, 3, 2, n) and lse3.shape == (2, 3, 2)
    lg.check_rows(got.cpu().numpy().reshape(rows, n), None, lse3.cpu().numpy().reshape(rows), keys, ids, np.full(rows, 0.7, dtype=np.float32), key_type)
    for form in (T.tolist(), torch.from_numpy(T.astype(np.float64))):
        again = lsd.logprobs16_rows(x, torch.from_numpy(ids).cuda(), temperature=form)
        assert np.array_equal(u32(again.cpu().numpy()), u32(logprob.cpu().numpy()))
    wide = torch.stack([x, x], dim=2)[:, :, 0]                            # not contiguous: a copy is scored
    assert not wide.is_contiguous() and torch.equal(lsd.logprobs16_rows(wide, one.view(rows)), lsd.logprobs16_rows(x, one.view(rows)))
    # GPULogprob16 with ids [rows] and outputs of the caller's
    out = torch.empty(rows, dtype=torch.float32, device="cuda")
    own_rank = torch.empty(rows, dtype=torch.int32, device="cuda")
    ret = lsd.GPULogprob16(x, one.view(rows).to(torch.int32), key_type=key_type, ranks=own_rank, out=out, check_fault=True)
    assert ret[0].data_ptr() == out.data_ptr() and ret[1].data_ptr() == own_rank.data_ptr() and len(ret) == 2
    lg.check_rows(out.cpu().numpy().reshape(rows, 1), own_rank.cpu().numpy().reshape(rows, 1), None, keys, ids[:, :1], None, key_type)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bfloat16", "float16"])
@pytest.mark.parametrize("n", [5, 40])
def test_top_logprobs16_rows_against_a_float32_torch_restatement(n, dtype):
    """rows of pairwise distinct values, so that torch.topk has no ties to break its own way"""
    key_type = str(dtype).replace("torch.", "")
    rows, cols = 6, 3000
    rng = np.random.default_rng(n)
    every = np.arange(1 << 16, dtype=np.uint16)
    size = np.abs(tp.values64(every, key_type))
    usable = every[(size >= 2.0 ** -7) & (size <= 64)]                   # bfloat16 has 3330 of them
    keys = np.stack([rng.permutation(usable)[:cols] for _ in range(rows)])
    assert all(np.unique(keys[r]).size == cols for r in range(rows))
    T = np.array([0.5, 1.0, 2.0], dtype=np.float32)[np.arange(rows) % 3]
    x = to_dev(keys, key_type).view(2, 3, cols)
    logprob, index = lsd.top_logprobs16_rows(x, n, temperature=dev_f32(T))
    assert logprob.shape == index.shape == (2, 3, n) and logprob.dtype == torch.float32 and index.dtype == torch.int64
    ref_all = torch.log_softmax(x.float() / dev_f32(T).view(2, 3, 1), -1)
    ref, ref_index = torch.topk(ref_all, n, dim=-1)
    assert torch.equal(index, ref_index)
    assert ((logprob - ref).abs() <= 2 * (sm.LOGPROB_TOL + 2.0 ** -22 * ref.abs())).all()
    lg.check_rows(logprob.cpu().numpy().reshape(rows, n), None, None, keys, index.cpu().numpy().reshape(rows, n), T, key_type)
    assert torch.equal(lsd.top_logprobs16_rows(x, n)[1], index)
