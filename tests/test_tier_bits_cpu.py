"""The inputs of test_gpu_tier_bits.py are what they claim to be, and its engine catches what it is for (no GPU needed).

test_gpu_tier_bits.py is worth what tests/_tier_bits.py builds: the widths must reach every size class and the offsets every boundary,
the padding must have zero mass, the ladders must not go empty and must stand among light keys, and the model of part C must be
consistent with the float64 oracle.  The constants are read from lsdradixsort_amd/csrc, so that a moved tier or tile fails this file
instead of emptying the GPU tests.  The engine itself runs here against a float64 restatement of the three units in numpy
(_tier_bits.NumpyOps): clean it passes, and with 1024 -- 2^-22 of a key's mass -- added to one key in one size class it fails."""
import re

import numpy as np
import pytest

import _long_plan as lp
import _sample16 as sm
import _temper16 as tm
import _tier_bits as tb
import _topp16 as tp
from test_row_rounds_cpu import constant, source

UPDATE = "update tests/_tier_bits.py (and DESIGN.md sections 6.13, 6.15 and 6.17) so that every size class and boundary is still reached"
UNITS = ("topp16", "sample16", "logprob16")
SOURCES = ("radix_select.hpp", "lsd_kernels.hpp", "keys16_map.hpp", "lsd_device.hpp")
ALL_ROWS = [(key_type, k) for key_type in tb.TYPES for k in range(12)]


def test_tier_and_tile_constants_of_the_sources():
    assert (constant("kWaveSegCap", *SOURCES), constant("kLocalSortCap", *SOURCES)) == (tb.WAVE_CAP, tb.GROUP_CAP) == (1024, 16384), UPDATE
    assert (constant("kMinChunk", *SOURCES), constant("kLongTile", *SOURCES)) == (lp.MIN_CHUNK, lp.LONG_TILE) == (16384, 4096), UPDATE
    assert constant("kGroupKeys", *SOURCES) == tb.LOAD_GROUP == 8 and constant("kRegs", *SOURCES) == 16, UPDATE
    assert constant("kWaveTile", *SOURCES) == tb.WAVE_TILE == 2 * tb.LANE_ROUND and tb.LANE_ROUND == 64 * tb.LOAD_GROUP, UPDATE
    for unit in UNITS:   # the units choose their size class by these two constants
        text = source(unit + ".hip")
        assert re.search(r"cols <= \(size_t\)kWaveSegCap\b", text) and re.search(r"cols <= \(size_t\)kLocalSortCap\b", text), f"{unit}.hip: {UPDATE}"
    text = source("mass_rows16.hpp")   # the lane layout the offsets aim at: register 8 j + e is body position q0 + 8 (64 j + lane) + e
    assert "q0 + ((uint32_t)j * 64u + lane) * kGroupKeys" in text, UPDATE   # read_body, the draw's and the log-probabilities' row read
    for unit in ("sample16", "logprob16"):
        assert '#include "mass_rows16.hpp"' in source(unit + ".hip") and "read_body(" in source(unit + ".hip"), UPDATE


def test_widths_reach_every_size_class_and_offsets_every_boundary():
    assert [tb.tier_of(W) for W in tb.WIDTHS] == ["wave", "wave", "group", "group", "group", "long", "long"]
    assert tb.WIDTHS[0] == tb.B and tb.WAVE_CAP in tb.WIDTHS and tb.WAVE_CAP + 1 in tb.WIDTHS and tb.GROUP_CAP in tb.WIDTHS and tb.GROUP_CAP + 1 in tb.WIDTHS
    assert lp.chunks_for(40, 16385) == (16384, 2) and lp.chunks_for(40, 70001) == (16384, 5), "the long widths: kMinChunk chunks at any batch used here"
    assert {tb.tier_of(W) for W in tb.TIER_WIDTH.values()} == {"wave", "group", "long"} and set(tb.TIER_WIDTH.values()) <= set(tb.WIDTHS)
    for W in tb.WIDTHS:
        Ls = tb.offsets(W)
        assert Ls[0] == 0 and Ls[-1] == W - tb.B and all(0 <= L <= W - tb.B for L in Ls) and len(Ls) <= 40
        if W > tb.B + 9:
            assert set(range(10)) <= set(Ls), "every phase of the 8-key load group, and one group on"
        for b in tb.boundaries(W):   # the boundary lies at row position b + head, head = 0 .. 7: all three hold for every head
            before = [L for L in Ls if L + tb.B <= b]
            across = [L for L in Ls if L < b and b + 7 < L + tb.B]
            after = [L for L in Ls if L >= b + 7]
            # a row that ends within 7 keys of the boundary has it across only for some heads: there the row's end, L = W - B, is the case
            assert before and (across or W <= b + 7) and (after or b + 7 + tb.B > W), f"W = {W}, boundary {b}: {Ls}"
    assert tb.boundaries(70001) == [512, 1024, 4096, 16384, 65536] and tb.boundaries(1024) == [512]
    # the batch of a width lies 3 elements behind a 16-byte line and W is odd or even: the rows of odd widths have every head
    assert {(-(tb.SKIP + r * 70001) * 2 % 16) // 2 for r in range(len(tb.offsets(70001)))} == set(range(8))
    rows, cols = lp.SHAPES["FIVE_TILES"]
    assert lp.chunks_for(rows, cols)[0] == 5 * lp.LONG_TILE and lp.SKIP[2] == 2 * tb.SKIP, "the wider-chunk plan, the same buffer phase"


def test_embed_is_padding_base_padding():
    base = tb.base_rows("bfloat16")[0].bits
    for W, L in ((tb.B, 0), (1024, 0), (1024, 515), (4099, 1777)):
        pad = tb.PADS["-nan"]["bfloat16"]
        want = np.array([pad] * L + base.tolist() + [pad] * (W - L - tb.B), dtype=np.uint16)
        assert np.array_equal(tb.embed(base, W, L, pad), want)


@pytest.mark.parametrize("key_type", tb.TYPES)
def test_base_rows_have_their_families_parameters_and_an_anchor(key_type):
    rows = tb.base_rows(key_type)
    assert len(rows) == 12 and {b.name for b in rows} == set(tb.FAMILIES)
    assert {None if b.T is None else b.T.tobytes() for b in rows} == {None if T is None else T.tobytes() for T in tb.TEMPERATURES}
    assert {b.mp for b in rows} == {None, tb.MIN_P} and tb.T_LOG2E.view(np.uint32) == 0x3FB8AA3B
    ninf, pinf = tp.NEG_INF[key_type], tp.POS_INF[key_type]
    for b in rows:
        v = tp.values64(b.bits, key_type)
        assert tb.has_anchor(b.bits, key_type), f"{b}: no finite number and no +inf -- the padding would carry mass"
        assert not (b.bits == tp.FILL).any() and np.nanmax(np.abs(v[np.isfinite(v)]), initial=0) <= 64
        if b.name == "nans":
            assert (b.bits == ninf).any() and not (b.bits == pinf).any() and (np.isnan(v) & (b.bits < 0x8000)).any() and (np.isnan(v) & (b.bits >= 0x8000)).any()
        if b.name == "+inf maximum":
            assert (b.bits == pinf).sum() >= tb.PAIRS + 1
        if b.name == "four values":
            assert np.unique(b.bits).size == 4
        if b.name == "lone maximum":
            gap = v.max() - v
            assert (gap == 0).sum() == 1 and ((gap >= 7.9) & (gap <= 14.1)).sum() >= 290
    for name, pads in tb.PADS.items():   # the padding kinds: zero mass under any finite or +inf maximum, never above a number in a rank
        value = tp.values64(np.array([pads[key_type]], dtype=np.uint16), key_type)[0]
        assert np.isneginf(value) if name == "-inf" else (np.isnan(value) and pads[key_type] >= 0x8000)
        assert pads[key_type] != tp.FILL
        for b in rows[:2]:
            w, C, Z = tm.cdf(tb.embed(b.bits, 1024, 100, pads[key_type]), key_type, b.t())
            w0, C0, Z0 = tm.cdf(b.bits, key_type, b.t())
            assert Z == Z0 and np.array_equal(w[100:100 + tb.B], w0) and w[:100].sum() == 0 and w[100 + tb.B:].sum() == 0


@pytest.mark.parametrize("key_type,k", ALL_ROWS)
def test_pairs_are_enough_light_and_inside(key_type, k):
    """At least 12 neighbouring pairs per row for the draw, every boundary C_j / Z in (2^-20, 1 - 2^-10), at least 4 of them light
    crossings: both keys below 2^-10 of the row and w * 2^32 >= 16.  The rows whose maximum is +inf are exempt from the light
    crossings alone: their masses are 0 or 1, and 509 keys cannot make 1 / (count of +inf) fall below 2^-10.  The filter's pairs are
    neighbouring distinct VALUES inside the min-p set: a row of four values has at most three, a +inf row none (one value has mass);
    every other row has 12 unless min-p cuts them short."""
    b = tb.base_rows(key_type)[k]
    pairs = tb.draw_pairs(b)
    w, C, Z = tm.cdf(b.bits, key_type, b.t())
    assert len(pairs) >= tb.PAIRS and len({j for i, j, at, light in pairs}) == len(pairs)
    for i, j, at, light in pairs:
        assert i < j and w[i] * 2.0 ** 32 >= 16 and w[j] * 2.0 ** 32 >= 16 and (w[i + 1:j] * 2.0 ** 32 < 16).all(), "neighbours among the keys that carry mass"
        assert 2.0 ** -20 < at < 1 - 2.0 ** -10 and at == C[j] / Z
        assert light == (w[i] / Z < 2.0 ** -10 and w[j] / Z < 2.0 ** -10)
    if b.name != "+inf maximum":
        assert sum(light for i, j, at, light in pairs) >= tb.LIGHT_PAIRS, f"{b}: light crossings"
    fpairs = tb.filter_pairs(b)
    assert all(2.0 ** -20 < at < 1 - 2.0 ** -10 and 0 < count <= tb.B for count, at, light in fpairs)
    assert len({count for count, at, light in fpairs}) == len(fpairs)
    if b.name == "+inf maximum":
        assert fpairs == []
    elif b.name == "four values":
        assert 2 <= len(fpairs) <= 3
    elif b.mp is None:
        assert len(fpairs) == tb.PAIRS and sum(light for count, at, light in fpairs) >= tb.LIGHT_PAIRS
    else:
        assert len(fpairs) >= 4, f"{b}: pairs inside the min-p set"


def test_ladders_and_bisection():
    flips = tb.bisect_flips(lambda bits: (bits >= np.array([100, 0x3F000000, 0x3F7FFFF0])).astype(np.int64), [1, 1, 1])
    assert flips.tolist() == [100, 0x3F000000, 0x3F7FFFF0]
    rungs = tb.ladders(flips[1:2])
    assert rungs.dtype == np.float32 and rungs.view(np.uint32).tolist() == list(range(0x3F000000 - 4, 0x3F000000 + 4))
    with pytest.raises(AssertionError):
        tb.bisect_flips(lambda bits: (bits >= 2).astype(np.int64), [1])          # a flip point at the end of the range


def test_ids_of_logprob16():
    for key_type in tb.TYPES:
        for b in tb.base_rows(key_type):
            ids, kind = tb.base_ids(b)
            v = tp.values64(b.bits, key_type)
            at = ids[kind == 0]
            assert ids.size == 32 and (kind == 0).sum() == 26 and ((0 <= at) & (at < tb.B)).all() and np.unique(at).size == at.size
            assert int(np.nanargmax(np.where(np.isnan(v), -np.inf, v))) in at and 0 in at and tb.B - 1 in at
            assert np.isnan(v).any() == np.isnan(v[at]).any(), "a NaN key where the row holds one"
            assert np.unique(v[at][~np.isnan(v[at])]).size < (~np.isnan(v[at])).sum() or np.unique(v[~np.isnan(v)]).size == (~np.isnan(v)).sum(), "a tie"
            placed = tb.ids_at(ids, kind, 4099, 77)
            assert np.array_equal(placed[kind == 0], at + 77) and sorted(placed[kind != 0].tolist()) == sorted([-1, -7, -2 ** 31, 4099, 4104, 2 ** 31 - 1])
            perm = tb.permutations()["shuffled"]
            where = np.argsort(perm)
            assert np.array_equal(b.bits[perm][tb.ids_at(ids, kind, tb.B, 0, where)[kind == 0]], b.bits[at])


def test_the_model_temperature_has_scale_one():
    assert tb.T_LOG2E == np.float32(tm.LOG2E) and tm.scale32(tb.T_LOG2E) == 1.0, "c = float32(log2 e / float64(T)) is exactly 1"
    assert np.float32(tm.LOG2E / float(tb.T_LOG2E)) == np.float32(1.0) and not tm.is_greedy(tb.T_LOG2E)


@pytest.mark.parametrize("key_type", tb.TYPES)
def test_the_model_is_consistent_with_the_float64_rules(key_type):
    """part C: on every ladder point the model's index is acceptable and its kept set passes the filter's rule; the model's flips
    are flips; the rows have graded d, ties and light keys in front"""
    rows = tb.model_rows(key_type)
    assert len(rows) == 4
    for base, d in rows:
        assert d.min() >= -31 and d.max() == 0 and (d == 0).sum() >= 1 and np.unique(d).size >= 12 and np.unique(d).size < tb.B // 4
        assert (d[:tb.B // 3] <= -12).all(), "the light keys in front"
        assert np.abs(tp.values64(base.bits, key_type)).max() <= 64 and base.T.tobytes() == tb.T_LOG2E.tobytes()
        q, Z = tb.model_masses(d)
        assert q.min() >= 2 and Z == sum(1 << (32 + int(x)) for x in d)
        u, p = tb.model_ladders(base, d)
        pairs, fpairs = tb.draw_pairs(base), tb.filter_pairs(base)
        assert len(pairs) >= tb.PAIRS and len(fpairs) >= 4 and u.size == 8 * len(pairs) + sm.U_CYCLE.size and p.size == 8 * len(fpairs) + tp.P_CYCLE.size
        for k, (i, j, at, light) in enumerate(pairs):
            got = [tb.model_index(d, x) for x in u[8 * k:8 * k + 8]]
            assert max(got[:4]) < j <= min(got[4:]), "four rungs on each side of the model's flip"
        for k, (count, at, light) in enumerate(fpairs):
            got = [int(tb.model_kept(d, x).sum()) for x in p[8 * k:8 * k + 8]]
            assert max(got[:4]) < count <= min(got[4:])
        for x in u:
            assert tb.model_index(d, x) in tm.acceptable_index(base.bits, x, key_type, tb.T_LOG2E), (base, x)
        for x in p:
            kept = tb.model_kept(d, x)
            got = base.bits if kept is None else np.where(kept, base.bits, np.uint16(tp.FILL))
            assert tm.check_row(got, base.bits, x, None, tb.T_LOG2E, key_type) is None, (base, x)


# ---- the engine against a float64 restatement ------------------------------------------------------------------------------------------------
ENGINE_ROWS = [("bfloat16", 0), ("float16", 5), ("bfloat16", 9)]    # no parameters; a temperature; NaNs, the model temperature and min-p
ENGINE_LS = {1024: [0, 3, 258, 515], 1025: [0, 5, 507, 516]}


@pytest.fixture(scope="module")
def references():
    ops = tb.NumpyOps()
    return {(key_type, k): tb.Reference(ops, tb.base_rows(key_type)[k]) for key_type, k in ENGINE_ROWS}


@pytest.mark.parametrize("key_type,k", ENGINE_ROWS)
def test_engine_passes_on_an_exact_function_of_the_row(references, key_type, k):
    ref, ops = references[key_type, k], tb.NumpyOps()
    assert ref.ladder_count() == (len(tb.draw_pairs(ref.base)), len(tb.filter_pairs(ref.base)))
    for W, pad in ((1024, "-inf"), (1025, "-nan")):
        Ls = ENGINE_LS[W]
        assert tb.check_draw_embedded(ops, ref, W, pad, Ls) == len(tb.draw_variants(ref.base)) * ref.u.size * len(Ls)
        assert tb.check_filter_embedded(ops, ref, W, pad, Ls) == 2 * len(tb.filter_variants(ref.base)) * ref.p.size * len(Ls)
        assert tb.check_logprob_embedded(ops, ref, W, pad, Ls) == len(tb.draw_variants(ref.base)) * 32 * len(Ls)
    perm = tb.permutations()["shuffled"]
    assert tb.check_filter_embedded(ops, ref, 1025, "-inf", [258], ref.base.bits[perm], ref.out[:, perm]) > 0
    assert tb.check_logprob_embedded(ops, ref, 1025, "-inf", [258], ref.base.bits[perm], np.argsort(perm)) > 0


@pytest.mark.parametrize("key_type,k", ENGINE_ROWS)
def test_engine_fails_on_one_size_class_off_by_1024_in_one_mass(references, key_type, k):
    """1024 is 2^-22 of the heaviest key's mass and below 2^-30 of these rows': every existing tolerance passes it by a factor of
    2^10 and more.  The wave class stays clean and passes; the workgroup class, which carries the defect, fails draw and filter."""
    ref, ops = references[key_type, k], tb.NumpyOps(defect=("group", 1024))
    tb.check_draw_embedded(ops, ref, 1024, "-inf", ENGINE_LS[1024])
    tb.check_filter_embedded(ops, ref, 1024, "-inf", ENGINE_LS[1024])
    with pytest.raises(AssertionError, match="reference configuration"):
        tb.check_draw_embedded(ops, ref, 1025, "-inf", ENGINE_LS[1025])
    with pytest.raises(AssertionError, match="reference configuration"):
        tb.check_filter_embedded(ops, ref, 1025, "-inf", ENGINE_LS[1025])
