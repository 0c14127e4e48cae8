"""The shapes of tests/_long_plan.py still reach the regimes of the long rows' chunk plan, every long-tier unit is on the list of
test_gpu_long_plan.py, and that module's inputs and oracles are what they claim to be (no GPU needed).

test_gpu_long_plan.py is worth what its shapes are worth.  Here kMinChunk, kMaxChunks, kLongTile and kLocalSortCap are read from
lsdradixsort_amd/csrc the way test_row_rounds_cpu.py reads the launch lines, the plan restated in Python is held against the table
of the shapes, and every shape against the property that defines each of its regimes: a retuned constant or a shrunk shape fails
this file instead of silently moving the GPU tests back into the regime every other test runs."""
import glob
import os
import re

import numpy as np
import pytest
import torch

import _long_plan as lp
import _sample16 as sm
import _topp16 as tp
import test_gpu_long_plan as gpu_tests
from test_row_rounds_cpu import CSRC, constant, source

UPDATE = "update the shapes of tests/_long_plan.py (and DESIGN.md section 6) so that every regime of the chunk plan is still reached"
SOURCES = ("radix_select.hpp", "lsd_kernels.hpp", "lsd_device.hpp")


def constants():
    return (constant("kMinChunk", *SOURCES), constant("kMaxChunks", *SOURCES), constant("kLongThreads", *SOURCES) * constant("kRegs", *SOURCES),
            constant("kLocalSortCap", *SOURCES))


def test_the_restated_plan_has_the_constants_of_the_sources():
    assert constants() == (lp.MIN_CHUNK, lp.MAX_CHUNKS, lp.LONG_TILE, lp.LOCAL_SORT_CAP) == (16384, 2048, 4096, 16384), \
        f"kMinChunk, kMaxChunks, kLongTile, kLocalSortCap are now {constants()}: {UPDATE}"
    assert constant("kLongTile", *SOURCES) == lp.LONG_TILE
    text = re.sub(r"\s+", " ", source("radix_select.hpp"))     # the three lines the restatement restates
    assert "size_t chunk = max_sz(kMinChunk, (n + kMaxChunks - 1) / kMaxChunks);" in text, UPDATE
    assert "chunk = (chunk + kLongTile - 1) / kLongTile * kLongTile;" in text and "(uint32_t)((cols + chunk - 1) / chunk)" in text, UPDATE
    assert "chunk_cap_for(size_t cols) { return min_sz(kMaxChunks, (cols + kMinChunk - 1) / kMinChunk); }" in text, UPDATE


@pytest.mark.parametrize("name", list(lp.SHAPES))
def test_plan_of_the_shape(name):
    rows, cols = lp.SHAPES[name]
    assert lp.chunks_for(rows, cols) + (lp.chunk_cap_for(cols),) == lp.PLAN[name], f"{name}: {UPDATE}"
    assert cols % 2 == 1 and rows * cols < (1 << 30), f"{name}: odd rows, and a call the library accepts"
    chunk, per_row = lp.chunks_for(rows, cols)
    assert per_row <= lp.chunk_cap_for(cols), "the plan never has more chunks than the stride of `counts`"
    assert lp.chunks_for(3, 70001) == (16384, 5) and lp.chunk_cap_for(70001) == 5, "below 2^25 keys: kMinChunk, per_row == cap"
    assert sm.chunk_len(rows, cols) == chunk and sm.chunk_len(3, 70001) == 16384, "_sample16.chunk_len is this plan"


def test_last_chunk_of_five_tiles():
    rows, cols = lp.SHAPES["FIVE_TILES"]
    chunk, per_row = lp.chunks_for(rows, cols)
    assert cols - (per_row - 1) * chunk == 8195, UPDATE


def regime_holds(regime, rows, cols):
    min_chunk, max_chunks, tile, local_cap = constants()
    chunk, per_row = lp.chunks_for(rows, cols)
    cap = lp.chunk_cap_for(cols)
    return {
        "odd tiles": chunk > min_chunk and (chunk // tile) % 2 == 1,
        "per_row below cap": per_row < cap and rows >= 2,
        "above 512 chunks": per_row > 512,
        "whole row": per_row == 1 and cols > local_cap,
        "at cap": per_row == max_chunks == cap and chunk == min_chunk,
        "partial last chunk": 0 < cols - (per_row - 1) * chunk < chunk and per_row > 1,
    }[regime]


@pytest.mark.parametrize("name,regime", [(n, g) for n, regimes in lp.REGIMES.items() for g in regimes], ids=lambda v: v.replace(" ", "_"))
def test_shape_reaches_its_regime(name, regime):
    rows, cols = lp.SHAPES[name]
    assert regime_holds(regime, rows, cols), f"{name} {rows}x{cols}: plan {lp.chunks_for(rows, cols)}, cap {lp.chunk_cap_for(cols)} is not '{regime}': {UPDATE}"


def test_every_regime_is_reached_and_the_old_shapes_reach_none():
    assert {g for regimes in lp.REGIMES.values() for g in regimes} == {"odd tiles", "per_row below cap", "above 512 chunks", "whole row", "at cap",
                                                                       "partial last chunk"}
    for rows, cols in ((3, 70001), (5, 131073), (3, 300007), (1, (1 << 20) + 13)):   # the largest long shapes of the other modules
        assert not any(regime_holds(g, rows, cols) for g in ("odd tiles", "per_row below cap", "above 512 chunks", "whole row", "at cap"))
    # sample16's pick gives a lane ceil(chunks / 64) consecutive chunks: 13 at FIVE_TILES, one below 65 chunks
    assert -(-lp.PLAN["FIVE_TILES"][1] // 64) == 13 and -(-5 // 64) == 1
    # the smallest that reach their regime: one row less, or the row a tile shorter, and the regime is gone
    assert not regime_holds("whole row", 2047, 16385) and not regime_holds("at cap", 1, (1 << 25) - 3 - 16384)
    assert not regime_holds("odd tiles", 2, 1 << 24)


def test_every_long_tier_unit_is_on_the_gpu_tests_list():
    units = sorted(os.path.basename(path)[:-4] for path in glob.glob(os.path.join(CSRC, "*.hip"))
                   if re.search(r"\b(chunks_for|select_long)\s*\(", open(path).read()))
    assert len(units) >= 9, units
    for unit in units:
        if unit in lp.UNITS_TESTED_ELSEWHERE:
            continue
        assert unit in lp.UNIT_ENTRIES, f"{unit}.hip cuts long rows by chunks_for: add its entries to tests/_long_plan.py and test_gpu_long_plan.py"
        for entry in lp.UNIT_ENTRIES[unit]:
            assert entry in gpu_tests.RUN, f"{unit}.hip: entry {entry} is not run by test_gpu_long_plan.py"
            assert re.search(r"\blsdsort_" + entry + r"_device\b", source(unit + ".hip")), f"{unit}.hip does not define lsdsort_{entry}_device"
            for name in gpu_tests.BIG:
                assert (name, entry) in gpu_tests.CASES, f"{entry} is not run at {name}"
    assert set(lp.UNIT_ENTRIES) | set(lp.UNITS_TESTED_ELSEWHERE) == set(units), "a unit on the list no longer cuts long rows by chunks_for"
    assert set(gpu_tests.BIG) == {"FIVE_TILES", "WHOLE_ROW", "AT_CAP"} and len(gpu_tests.RUN) == 9


# ---- where the ranks, k and u send the pick ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["FIVE_TILES", "AT_CAP", "MANY_TILES"])
@pytest.mark.parametrize("size", [2, 4])
def test_ranks_lie_on_both_sides_of_the_chunk_boundaries(name, size):
    rows, cols = lp.SHAPES[name]
    chunk, per_row = lp.chunks_for(rows, cols)
    ranks = set(lp.ranks_of(name, size))
    for head in lp.heads(name, size):
        assert 0 < head < 16 // size
        for c in (1, 511, 512, per_row - 1):
            assert {c * chunk + head - 1, c * chunk + head} <= ranks
            assert (lp.chunk_at(c * chunk + head - 1, head, chunk), lp.chunk_at(c * chunk + head, head, chunk)) == (c - 1, c)
        assert {head - 1, head} <= ranks and lp.chunk_at(head - 1, head, chunk) == 0     # chunk 0 carries the head
        if name != "AT_CAP":
            fifth = [p for p in ranks if lp.chunk_at(p, head, chunk) == 512 and (p - head) % chunk // lp.LONG_TILE == 4]
            assert fifth, "a rank in the fifth tile of a chunk"
    assert lp.chunk_at(cols - 1, lp.heads(name, size)[0], chunk) == per_row - 1, "the last chunk is not empty"
    assert lp.head_of(0, cols, 2) == 5 and lp.head_of(0, cols, 4) == 1, "the first row lies 3 elements behind a 16-byte line"
    if rows == 2:
        assert len(lp.heads(name, size)) == 2, "the two rows start at different 16-byte phases"


def test_per_row_calls_send_the_rows_of_a_call_far_apart():
    rows, cols = lp.SHAPES["FIVE_TILES"]
    chunk, per_row = lp.chunks_for(rows, cols)
    ranks = lp.ranks_of("FIVE_TILES", 2)
    apart = [abs(ranks[lp.spread(ranks, shift, 0, rows)] - ranks[lp.spread(ranks, shift, 1, rows)]) // chunk for shift in range(len(ranks))]
    assert max(apart) > 512 and sum(a > 100 for a in apart) > len(apart) // 2, apart
    kinds = [lp.row_kind(r) for r in range(lp.SHAPES["WHOLE_ROW"][0])]
    assert all(a != b for a, b in zip(kinds, kinds[1:])) and set(kinds) == set(lp.FAMILIES)


@pytest.mark.parametrize("name", ["FIVE_TILES", "AT_CAP", "MANY_TILES"])
def test_equal_draws_aim_at_the_boundaries(name):
    rows, cols = lp.SHAPES[name]
    chunk, per_row = lp.chunks_for(rows, cols)
    for head in lp.heads(name, 2):
        u, index = lp.equal_draws(name, head)
        assert {0, 1, 511, 512, per_row - 1} <= {lp.chunk_at(int(i), head, chunk) for i in index}
        assert index[-4] == cols - 1 and index[-3] == cols - 1 and index[-2] == 0 and index[-1] == 0 and index.max() < cols
        for x, i in zip(u[:-5], index[:-5]):
            assert float(x) * cols == float(np.float64(x) * np.float64(cols)) and i == min(cols - 1, int(float(x) * cols))
            assert (int(x.view(np.uint32)) & 0x7FFFFF).bit_length() + cols.bit_length() <= 53, "u_c * cols is exact in a double"


# ---- the select oracles --------------------------------------------------------------------------------------------------------------
def test_torch_sort_agrees_with_numpy_at_a_small_shape():
    rows, cols = 3, 4099
    rng = np.random.default_rng(7)
    keys = np.stack([lp._row_bits(kind, r, cols, 4, rng) for r, kind in enumerate(("uniform bits", "four values", "uniform bits"))])
    ranks = [0, 1, 5, cols // 2, cols - 2, cols - 1]
    for largest in (False, True):
        ev, ei, _, _ = lp.stable_at_ranks_np(keys, 4, largest, ranks)
        tv, ti = lp.stable_at_ranks_torch(torch.from_numpy(keys.view(np.int32)), largest, ranks)
        assert np.array_equal(ev, tv) and np.array_equal(ei, ti), largest
    assert (keys[0] >> 23 == 0x1FF).any() and (keys[0] == 0x80000000).any(), "NaNs of the negative sign and -0.0 are among the keys"


def test_equal_oracle_is_the_stable_sort_of_equal_keys():
    for size in (2, 4):
        keys = np.full((2, 77), lp.EQUAL[size], dtype={2: np.uint16, 4: np.uint32}[size])
        for largest in (False, True):
            ev, ei, fv, fi = lp.stable_at_ranks_np(keys, size, largest, [0, 5, 76], first=9)
            assert (ev == lp.EQUAL[size]).all() and np.array_equal(ei, np.tile(np.array([0, 5, 76], dtype=np.uint32), (2, 1)))
            assert np.array_equal(fi, np.tile(np.arange(9, dtype=np.uint32), (2, 1)))
    ev, ei, fv, fi = lp.equal_oracle("AT_CAP", 2, 5)
    assert np.array_equal(ei[0], np.array(lp.ranks_of("AT_CAP", 2), dtype=np.uint32)) and np.array_equal(fi[0], np.arange(5))


def test_the_two_rows_of_a_family_differ():
    keys = lp.select_keys("WHOLE_ROW", 2)["cycle"]
    assert not (keys == 0x7E7E).any(), "none is the fill word of the filter tests"
    for r in range(6):
        distinct = np.unique(keys[r]).size
        assert {"uniform bits": distinct > 8000, "four values": distinct == 4, "all equal": distinct == 1}[lp.row_kind(r)]
    rng = np.random.default_rng(3)
    a, b = (np.bincount(np.searchsorted(lp.FOUR[2], lp._row_bits("four values", r, 100000, 2, rng)), minlength=4) for r in (0, 1))
    assert a.argmax() != b.argmax() and abs(a[0] - b[0]) > 5000, "the two rows draw the four values in other proportions"


# ---- the sharp rows: checked here, on the very rows the GPU tests use ----------------------------------------------------------------
def test_cached_oracles_are_those_of_the_helpers_at_a_small_shape():
    keys, u, at = sm.sharp_rows("near two", 70001, "bfloat16", seed=5, placement=True, rows=3)
    draw = lp.Draw(keys[0], "bfloat16")
    for r in range(0, u.size, 5):
        for x in (u[r], np.float32(0), np.float32(1), np.float32(np.nan), np.float32(0.37)):
            assert draw.exact(x) == sm.exact_index(keys[0], x, "bfloat16") and draw.acceptable(x) == sm.acceptable(keys[0], x, "bfloat16")
        assert draw.logprob(int(at[r])) == sm.logprob64(keys[0], int(at[r]), "bfloat16")
    none = lp.Draw(np.full(9, 0x7FFF, dtype=np.uint16), "bfloat16")
    assert none.exact(np.float32(0.5)) == -1 and none.acceptable(np.float32(0.5)) == [-1]
    rows, p = tp.sharp_rows("around zero", 4099, "bfloat16", seed=6)
    nucleus = lp.Nucleus(rows[0], "bfloat16")
    assert all(np.array_equal(a, b) for a, b in zip((nucleus.s, nucleus.mass, nucleus.A, nucleus.Z), tp.groups(rows[0], "bfloat16")))
    assert np.array_equal(nucleus.midpoints(), p)
    for x in list(p) + [np.float32(0), np.float32(0.5), np.float32(1.0 - 2.0 ** -24)]:
        assert nucleus.threshold(x) == tp.exact_threshold(rows[0], x, "bfloat16") and nucleus.acceptable(x) == tp.acceptable(rows[0], x, "bfloat16")
        assert np.array_equal(nucleus.filtered(x), tp.filter_np(rows[:1], np.array([x]), "bfloat16")[0])


@pytest.mark.parametrize("name", ["FIVE_TILES", "AT_CAP"])
def test_long_sharp_rows_are_sharp(name):
    rows, cols = lp.SHAPES[name]
    chunk, per_row = lp.chunks_for(rows, cols)
    keys, u, at = lp.sharp_inputs(name)
    light = {tp.NEG_INF["bfloat16"], int(tp.bits_of_values(np.array([-60.0]), "bfloat16")[0]), tp.POS_INF["bfloat16"] + 1, tp.NEG_INF["bfloat16"] + 1,
             0x7FFF, 0xFFFF}
    draws, ps = lp.draw_cases(name), lp.nucleus_cases(name)
    assert all(case.shape == (rows,) and case.dtype == np.float32 for case in draws + ps)
    for r in range(rows):
        head = lp.head_of(r, cols, 2)
        forced = set(lp.sharp_positions(rows, cols, head))
        assert forced <= set(at[r].tolist()) and len(at[r]) == sm.HEAVY
        for c in (1, 511, 512, per_row - 1):      # placement_positions' chunk-boundary pair of this head, at these boundaries
            assert {c * chunk + head - 1, c * chunk + head} <= forced & set(sm.placement_positions(cols, c * chunk))
        assert {0, cols - 1, head - 1, head} <= forced
        seen = np.bincount(keys[r], minlength=1 << 16)
        seen[keys[r][at[r]]] -= np.bincount(keys[r][at[r]], minlength=1 << 16)[keys[r][at[r]]]
        assert set(np.flatnonzero(seen).tolist()) <= light, "every other key is -inf, a NaN or the filler"
        draw = lp.draws(name)[r]
        others = ~np.isin(draw.mass, at[r])
        assert others.sum() > cols // 64, "the filler has mass in float64"
        assert np.floor(draw.w[others].max() * 2.0 ** 32) == 0, "and none in the device's fixed point"
        us = sorted({float(case[r]) for case in draws})
        assert len(us) >= len(forced) - 1
        for x in us:
            assert draw.acceptable(np.float32(x)) == [draw.exact(np.float32(x))], (name, r, x)     # _sample16.assert_sharp's rule
        assert {0, 1, 511, 512, per_row - 1} <= {lp.chunk_at(draw.exact(np.float32(x)), head, chunk) for x in us}
        nucleus = lp.nuclei(name)[r]
        for x in sorted({float(case[r]) for case in ps}):
            assert nucleus.acceptable(np.float32(x)) == [nucleus.threshold(np.float32(x))], (name, r, x)   # _topp16.assert_sharp's rule
    if rows == 2:
        assert not np.array_equal(keys[0], keys[1]) and set(at[0].tolist()) != set(at[1].tolist())
        far = [abs(lp.draws(name)[0].exact(case[0]) - lp.draws(name)[1].exact(case[1])) // chunk for case in draws[:1] + draws[-1:]]
        assert min(far) > 512, f"the two rows of a call want chunks {far} apart"


def test_whole_row_sharp_rows_are_sharp():
    rows, cols = lp.SHAPES["WHOLE_ROW"]
    keys, u, at = lp.sharp_inputs("WHOLE_ROW")
    ps = lp.sharp_p("WHOLE_ROW")
    for j in range(3):                                         # the three rows the 2049 cycle through, each with all its pairs
        assert len(u[j]) == sm.HEAVY and np.array_equal(keys[j], keys[j + 3]) and not np.array_equal(keys[j], keys[j + 1])
        sm.assert_sharp(np.broadcast_to(keys[j], (len(u[j]), cols)), u[j], "bfloat16")
        tp.assert_sharp(np.broadcast_to(keys[j], (len(ps[j]), cols)), ps[j], "bfloat16")
    (case_u,), (case_p,) = lp.draw_cases("WHOLE_ROW"), lp.nucleus_cases("WHOLE_ROW")
    assert case_u.shape == case_p.shape == (rows,)
    for r in (0, 1, 2, 3, 500, 2048):
        assert case_u[r] == u[r % 3][(r // 3) % sm.HEAVY] and case_p[r] == ps[r % 3][(r // 3) % len(ps[r % 3])]
    assert all(len({float(case_u[r]) for r in range(j, rows, 3)}) == sm.HEAVY for j in range(3)), "every pair of every row is drawn"
