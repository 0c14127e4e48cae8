"""GPU suite: the three units that work on softmax masses -- the top-p / min-p filter (lsdsort_topp16_filter_device and _ex), the draw
(lsdsort_sample16_device and _ex) and lsdsort_logprob16_device -- bit for bit across their size classes and across every shift of a
row inside the lane, wave-tile and chunk layout.  tests/_tier_bits.py has the construction; test_tier_bits_cpu.py shows that the
inputs are what they claim and that the engine catches one size class being off by 2^-22 of one key's mass.

Part A  one base row of 509 keys embedded at every offset of every width among padding of zero mass: the index minus the offset, the
        logprob's bits, the filter's window, the logprob16 words, ranks and lse all equal the reference configuration's (W = 509,
        L = 0), with u and p on the ladders around the exact float32 values where the reference configuration's answer flips, found by
        bisection on the device.  The reference configuration's own results pass the float64 acceptance rules (the Reference does that).
Part B  the filter's threshold, a token's logprob and rank and the row's lse are functions of the MULTISET: three permutations.
Part C  integer logits under the temperature whose scale is exactly 1: IF v_exp_f32 is exact at integers the masses are powers of two
        and Python integers give the index and the kept set exactly, in every size class -- an anchor on what all classes share.

Every test prints the number of (row, configuration, point) comparisons it made."""
import numpy as np
import pytest
import torch

import lsdradixsort_amd as lsd
import _long_plan as lp
import _sample16 as sm
import _temper16 as tm
import _tier_bits as tb
import _topp16 as tp
from _device_arrays import DTYPES

pytestmark = pytest.mark.gpu


class DeviceOps:
    """the engine's `ops` on the library: the plain entries where there is neither T nor min-p, else the _ex entries; the fault word
    is read after every call"""
    device = "cuda"

    def draw(self, keys, u, T, key_type):
        return lsd.GPUSample16(keys.view(DTYPES[key_type]), u, key_type=key_type, logprobs=True, check_fault=True, d_temperature=T)

    def filter(self, keys, p, mp, T, key_type, out):
        got = lsd.GPUTopP16Filter(keys.view(DTYPES[key_type]), p, key_type=key_type, fill=tp.FILL, out=None if out is None else out.view(DTYPES[key_type]),
                                  check_fault=True, d_min_p=mp, d_temperature=T)
        return got.view(torch.int16)

    def logprob(self, keys, ids, T, key_type):
        return lsd.GPULogprob16(keys.view(DTYPES[key_type]), ids, key_type=key_type, ranks=True, lse=True, d_temperature=T, check_fault=True)


OPS = DeviceOps()
REFERENCES = {}
ROWS = range(12)


def reference(key_type, k):
    """the reference configuration's flip points, ladders and results of a base row: found on the device once, shared by every test"""
    if (key_type, k) not in REFERENCES:
        ref = tb.Reference(OPS, tb.base_rows(key_type)[k])
        # the ladders that run are the ladders that were planned: nothing is skipped
        assert ref.ladder_count() == (len(tb.draw_pairs(ref.base)), len(tb.filter_pairs(ref.base))) and ref.ladder_count()[0] >= tb.PAIRS
        assert ref.u.size == tb.LADDER * ref.ladder_count()[0] + sm.U_CYCLE.size and ref.p.size == tb.LADDER * ref.ladder_count()[1] + tp.P_CYCLE.size
        REFERENCES[key_type, k] = ref
    return REFERENCES[key_type, k]


def pads_of(W):
    return ("-inf",) if W == tb.B else tuple(tb.PADS)      # W = B has no padding


# ---- part A --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key_type", tb.TYPES)
@pytest.mark.parametrize("W", tb.WIDTHS)
def test_draw_has_the_reference_bits_in_every_tier_at_every_shift(W, key_type):
    made = sum(tb.check_draw_embedded(OPS, reference(key_type, k), W, pad) for k in ROWS for pad in pads_of(W))
    ladders = sum(reference(key_type, k).ladder_count()[0] for k in ROWS)
    assert ladders >= 12 * tb.PAIRS
    print(f"draw W={W} {key_type}: {made} comparisons, {ladders} ladders, {len(tb.offsets(W))} offsets")


@pytest.mark.parametrize("key_type", tb.TYPES)
@pytest.mark.parametrize("W", tb.WIDTHS)
def test_filter_has_the_reference_bits_in_every_tier_at_every_shift(W, key_type):
    made = sum(tb.check_filter_embedded(OPS, reference(key_type, k), W, pad) for k in ROWS for pad in pads_of(W))
    ladders = sum(reference(key_type, k).ladder_count()[1] for k in ROWS)
    assert ladders == sum(len(tb.filter_pairs(b)) for b in tb.base_rows(key_type)) and ladders >= 6 * tb.PAIRS
    print(f"filter W={W} {key_type}: {made} comparisons, {ladders} ladders, {len(tb.offsets(W))} offsets")


@pytest.mark.parametrize("key_type", tb.TYPES)
@pytest.mark.parametrize("W", tb.WIDTHS)
def test_logprob16_has_the_reference_bits_in_every_tier_at_every_shift(W, key_type):
    made = sum(tb.check_logprob_embedded(OPS, reference(key_type, k), W, pad) for k in ROWS for pad in pads_of(W))
    print(f"logprob16 W={W} {key_type}: {made} comparisons")


@pytest.mark.parametrize("key_type", tb.TYPES)
def test_a_row_without_a_number_stays_without_one(key_type):
    """NaNs of both signs alone, among NaN padding: -1 and a NaN logprob from the draw, NaN, -1 and a NaN lse from logprob16, at
    every width and offset and for every u"""
    rng = np.random.default_rng(3)
    pinf, ninf, pad = tp.POS_INF[key_type], tp.NEG_INF[key_type], tb.NEG_NAN[key_type]
    base = np.array([pinf + 1, ninf + 1, 0x7FFF, 0xFFFF, pad], dtype=np.uint16)[rng.integers(0, 5, tb.B)]
    for W in tb.WIDTHS:
        Ls = tb.offsets(W)
        rows_bits = np.stack([tb.embed(base, W, L, pad) for L in Ls])
        for T in (None, np.float32(0.7)):
            index, logprob = tb.run_draw(OPS, key_type, rows_bits, sm.U_CYCLE, T)
            assert (index == -1).all() and np.isnan(logprob.view(np.float32)).all(), f"W = {W}, T = {T}"
            ids = np.stack([np.arange(L, L + 32) for L in Ls])
            lp16, rank, lse = tb.run_logprob(OPS, key_type, rows_bits, ids, T)
            assert np.isnan(lp16.view(np.float32)).all() and (rank == -1).all() and np.isnan(lse.view(np.float32)).all(), f"W = {W}, T = {T}"


@pytest.mark.parametrize("entry", ["draw", "filter"])
def test_above_2_to_the_25_keys_the_wider_chunks_give_the_reference_bits(entry):
    """_long_plan's FIVE_TILES, [2 x 2^24 + 4099] bfloat16 in chunks of 20480 keys: the base row across the first chunk boundary of
    row 0 and at the end of row 1, three base rows, one padding kind each"""
    rows, cols = lp.SHAPES["FIVE_TILES"]
    chunk, per_row = lp.chunks_for(rows, cols)
    assert (chunk, per_row) == lp.PLAN["FIVE_TILES"][:2] and chunk > lp.MIN_CHUNK
    Ls = [lp.head_of(0, cols, 2) + chunk - tb.B // 2, cols - tb.B]
    made = 0
    for k, pad in ((0, "-inf"), (5, "-nan"), (9, "-inf")):
        check = tb.check_draw_embedded if entry == "draw" else tb.check_filter_embedded
        made += check(OPS, reference(lp.KEY_TYPE, k), cols, pad, Ls)
    print(f"{entry} FIVE_TILES: {made} comparisons")


# ---- part B --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key_type", tb.TYPES)
@pytest.mark.parametrize("tier", list(tb.TIER_WIDTH))
def test_order_of_the_keys_does_not_matter_where_the_design_says_so(tier, key_type):
    W = tb.TIER_WIDTH[tier]
    L = [(W - tb.B) // 2]
    made = 0
    for k in ROWS:
        ref = reference(key_type, k)
        for n, (name, perm) in enumerate(tb.permutations().items()):
            pad = list(tb.PADS)[(k + n) % 2]
            bits = ref.base.bits[perm]
            made += tb.check_filter_embedded(OPS, ref, W, pad, L, bits, ref.out[:, perm])
            made += tb.check_logprob_embedded(OPS, ref, W, pad, L, bits, np.argsort(perm))
    print(f"order {tier} {key_type}: {made} comparisons")


# ---- part C --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key_type", tb.TYPES)
@pytest.mark.parametrize("tier", list(tb.TIER_WIDTH))
def test_power_of_two_masses_give_the_integer_model_exactly(tier, key_type):
    """the premise -- v_exp_f32(d) == 2^d exactly for the integers d = -31 .. 0 -- and the shared arithmetic, G = min(Z - 1, floor(u Z))
    and ceil(p Z), in one: the model's index and kept set at every rung of the model's own ladders"""
    W = tb.TIER_WIDTH[tier]
    L = (W - tb.B) // 2
    made = 0
    for base, d in tb.model_rows(key_type):
        u, p = tb.model_ladders(base, d)
        rows_bits = tb.embed(base.bits, W, L, tb.PADS["-inf"][key_type])[None, :]
        index, logprob = tb.run_draw(OPS, key_type, rows_bits, u, base.T)
        want = np.array([tb.model_index(d, x) for x in u]) + L
        bad = np.flatnonzero(index[:, 0] != want)
        assert bad.size == 0, (f"{base}, {tier} tier: {bad.size} of {u.size} indices differ from the model, first at u = {u[bad[0]]!r} (bits "
                               f"{u[bad[:1]].view(np.uint32)[0]:#x}): index - L = {index[bad[0], 0] - L}, model {want[bad[0]] - L}")
        for k, x in enumerate(u):
            assert abs(float(logprob.view(np.float32)[k, 0]) - tm.logprob64(base.bits, int(want[k]) - L, key_type, base.T)) <= sm.LOGPROB_TOL
        out = tb.run_filter(OPS, key_type, rows_bits, p, base.T, None)[:, 0, :]
        for k, x in enumerate(p):
            kept = tb.model_kept(d, x)
            row = rows_bits[0].copy()
            if kept is not None:
                row[:] = tp.FILL
                row[L:L + tb.B] = np.where(kept, base.bits, np.uint16(tp.FILL))
            differ = np.flatnonzero(out[k] != row)
            assert differ.size == 0, (f"{base}, {tier} tier, p = {x!r} (bits {p[k:k + 1].view(np.uint32)[0]:#x}): {differ.size} words differ from the "
                                      f"model's kept set, first at {differ[0] - L}; kept {(out[k] != tp.FILL).sum()}, model {int(kept.sum())}")
        made += u.size + p.size
    print(f"model {tier} {key_type}: {made} comparisons")
