"""The shapes of tests/_seg_plan.py still lie past the table and grid caps of the segmented sort's large tier (no GPU needed).

test_gpu_segmented_plan.py is worth what its shapes are worth.  Here the constants and the grid_for(items, per, cap) arguments of
the capped launches are read from lsdradixsort_amd/csrc/segmented.hip and held against _seg_plan's restatement; every shape is held
to the regime it is there for; plan()'s table sizes are held against lsdsort_segmented_workspace_bytes (the library loads without a
GPU); and the worst-case argument behind those sizes is tried on random and adversarial segmentations.  So raising a cap, a tile or
a tier boundary fails this file instead of silently turning the GPU tests into first-round tests."""
import os
import re

import numpy as np
import pytest

import _seg_plan as sp

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lsdradixsort_amd", "csrc")
UPDATE = ("update the constants and SHAPES of tests/_seg_plan.py (ITEMS, ITEMS_TIGHT, ITEMS_FALLBACK, FALLBACK_TIGHT, TILES, MIXED) "
          "and DESIGN.md section 6.3 so that every capped loop of the large tier still goes round again")
FILES = ("segmented.hip", "lsd_kernels.hpp", "lsd_host.hpp")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def constant(name, *files):
    """the value of an integer constant `name = <expression of literals, other constants, + - * />` from the named sources (as in
    test_row_rounds_cpu.py)"""
    texts = [source(f) for f in files]

    def value(word):
        if re.fullmatch(r"\d+u?", word):
            return int(word.rstrip("u"))
        for text in texts:
            m = re.search(r"constexpr[^;]*\b" + word + r"\s*=\s*([^,;]+)[,;]", text)
            if m:
                expr = re.sub(r"\(\w+_t\)|\(int\)", "", m.group(1))
                assert re.fullmatch(r"[\w\s+\-*/()]+", expr), f"{word} = {expr!r}: not an integer expression this test can read"
                return int(eval(re.sub(r"[A-Za-z_]\w*|\d+u", lambda t: str(value(t.group(0))), expr).replace("/", "//")))
        raise AssertionError(f"constant {word} not found in {files}: {UPDATE}")

    return value(name)


def grid_args(anchor):
    """(per, cap) of the first grid_for(items, per, cap) at or after `anchor` in segmented.hip"""
    text = source("segmented.hip")
    at = text.find(anchor)
    assert at >= 0, f"segmented.hip: {anchor!r} not found any more: {UPDATE}"
    m = re.compile(r"grid_for\((.+?),\s*(\w+)\s*,\s*(\w+)\s*\)\)?[,;]").search(text, at)
    assert m, f"segmented.hip: no grid_for(items, per, cap) after {anchor!r}: {UPDATE}"
    return constant(m.group(2), *FILES), constant(m.group(3), *FILES)


# the launch (or the named grid) each entry of _seg_plan.GRIDS restates
ANCHORS = {"plan": "hipLaunchKernelGGL(seg_plan_kernel", "wave": "wave_grid =", "group": "launch_segment_sort(sp,",
           "items": "hipLaunchKernelGGL(seg_tiles_kernel", "tiles": "tile_grid ="}


def test_constants_and_caps_are_the_sources():
    got = {"SEG_TILE": constant("kSegTile", *FILES), "SCAN_BLOCK": constant("kScanBlock", *FILES),
           "WAVE_CAP": constant("kWaveSegCap", *FILES), "GROUP_CAP": constant("kLocalSortCap", *FILES),
           "CTL_BYTES": constant("kCtlBytes", *FILES), "ALIGN": constant("kAlign", *FILES)}
    for name, value in got.items():
        assert getattr(sp, name) == value, f"{name}: the sources say {value}, _seg_plan {getattr(sp, name)}: {UPDATE}"
    for name, anchor in ANCHORS.items():
        assert grid_args(anchor) == sp.GRIDS[name], \
            f"{name}: launched with (per, cap) = {grid_args(anchor)}, _seg_plan.GRIDS says {sp.GRIDS[name]}: {UPDATE}"
    text = source("segmented.hip")
    m = re.search(r"__launch_bounds__\((\d+)\) seg_scan_sums_kernel", text)
    assert m and int(m.group(1)) == sp.SUMS_ROUND and f"c0 += {sp.SUMS_ROUND}u" in text, \
        f"seg_scan_sums_kernel no longer carries every {sp.SUMS_ROUND} block sums: {UPDATE}"
    enum = re.search(r"kCntWave = (\d), kCntGroup = (\d), kCntItems = (\d), kCntTiles = (\d), kCntHistTiles = (\d)", text)
    assert enum and [int(x) for x in enum.groups()] == [1, 2, 3, 4, 5], f"the control block's counters moved: {UPDATE}"


def past(count, cap, what, name):
    assert count > cap, f"{name}: {count} {what} fit one round of {cap}: {UPDATE}"
    assert count % cap != 0, f"{name}: {count} {what} end on a full round of {cap}: {UPDATE}"


@pytest.mark.parametrize("name", ["ITEMS", "ITEMS_TIGHT", "ITEMS_FALLBACK", "FALLBACK_TIGHT", "MIXED"])
def test_item_shapes_take_a_second_round_of_the_tile_table_kernel(name):
    sizes, local, _, _ = sp.SHAPES[name]
    p = sp.plan_of(name)
    assert p["items_grid"] == sp.GRIDS["items"][1], f"{name}: seg_tiles_kernel's grid {p['items_grid']} is not at its cap: {UPDATE}"
    past(p["items"], p["items_grid"], "items", name)
    assert p["items"] == sp.ITEM_SEGS and p["hist_tiles"] == p["tiles"], f"{name}: every large segment is an item of several tiles"
    assert p["items"] <= p["max_items"] and p["tiles"] <= p["max_tiles"] and p["hist_tiles"] <= p["max_hist_tiles"]
    large = sizes[sizes > (sp.GROUP_CAP if local else 1)]
    assert (large > sp.SEG_TILE).all() and (large % sp.SEG_TILE != 0).all(), f"{name}: every large segment ends on a short tile"
    if "TIGHT" in name:
        assert (large % sp.SEG_TILE == 1).all(), f"{name}: every segment one key past whole tiles"
        assert p["max_tiles"] - p["tiles"] == 1 and p["max_hist_tiles"] - p["hist_tiles"] == 1 and p["max_items"] - p["items"] == 1, \
            f"{name}: tables not one entry from full: {p}: {UPDATE}"
    else:
        assert len(set(large.tolist())) > large.size // 2, f"{name}: ragged segments"
    if name == "MIXED":
        assert (p["wave"], p["group"]) == (3000, 600) and int((sizes == 0).sum()) == (3600 + sp.ITEM_SEGS) // 10
        assert {2, sp.WAVE_CAP, sp.WAVE_CAP + 1, sp.GROUP_CAP} <= set(sizes.tolist()), "the tiers' extreme sizes"
    elif local:
        assert (p["wave"], p["group"]) == (0, 0)


def test_the_issue_table():
    """the figures the shapes were chosen by"""
    want = {"ITEMS": (17140981, 1027, 5135), "ITEMS_TIGHT": (16827395, 1027, 5135), "ITEMS_FALLBACK": (4521205, 1027, 2054),
            "FALLBACK_TIGHT": (4207619, 1027, 2054), "TILES": (70397549, 67, 17252)}
    for name, (n, items, tiles) in want.items():
        p = sp.plan_of(name)
        assert (sp.offsets_of(name)[1], p["items"], p["tiles"]) == (n, items, tiles), f"{name}: {UPDATE}"
    assert (sp.plan_of("ITEMS_TIGHT")["max_tiles"], sp.plan_of("ITEMS_TIGHT")["max_hist_tiles"]) == (5136, 5136)
    assert (sp.plan_of("FALLBACK_TIGHT")["max_tiles"], sp.plan_of("FALLBACK_TIGHT")["max_hist_tiles"]) == (2055, 2055)
    assert sp.plan_of("TILES")["block_sums"] == 1079
    assert 23_000_000 < sp.offsets_of("MIXED")[1] < 25_000_000


def test_tiles_shape_takes_a_second_round_of_hist_scatter_and_the_carry():
    sizes, local, _, _ = sp.SHAPES["TILES"]
    p = sp.plan_of("TILES")
    assert p["tile_grid"] == sp.GRIDS["tiles"][1], f"TILES: the tile grid {p['tile_grid']} is not at its cap: {UPDATE}"
    past(p["tiles"], p["tile_grid"], "tiles", "TILES")
    past(p["block_sums"], sp.SUMS_ROUND, "scan block sums", "TILES")
    assert (sizes % sp.SEG_TILE != 0).all() and len(set(sizes.tolist())) == sizes.size, "TILES: every segment ragged, none alike"
    nt = -(-sizes // sp.SEG_TILE)
    assert (nt > 256).all(), f"TILES: seg_tiles_kernel's inner loop (256 threads) comes round for every item: {UPDATE}"
    # a segment's block of counts is 256 * nt entries, in whatever order the planner's atomics place the blocks: blocks of different
    # lengths, and no run of c of them ends where the carry's first round does (entry SUMS_ROUND * SCAN_BLOCK), so one straddles it
    edge_tiles = sp.SUMS_ROUND * sp.SCAN_BLOCK // 256
    assert len(set(nt.tolist())) > 1 and not any(c * nt.min() <= edge_tiles <= c * nt.max() for c in range(1, sizes.size + 1)), \
        f"TILES: a block of counts can end on the carry's round boundary, hist tile {edge_tiles}: {UPDATE}"
    # the other shapes stay inside the first round of both: what they reach is the item round alone
    for name in ("ITEMS", "ITEMS_TIGHT", "ITEMS_FALLBACK", "FALLBACK_TIGHT"):
        q = sp.plan_of(name)
        assert q["tiles"] < sp.GRIDS["tiles"][1] and q["block_sums"] < sp.SUMS_ROUND


def test_short_offsets_of_the_graph_case_leave_the_large_tier_empty():
    n = sp.offsets_of("ITEMS")[1]
    p = sp.plan(np.full(sp.ITEM_SEGS, sp.SHORT_SIZE), True, n)
    assert (p["wave"], p["group"], p["items"], p["tiles"], p["hist_tiles"]) == (sp.ITEM_SEGS, 0, 0, 0, 0)
    assert sp.ITEM_SEGS * sp.SHORT_SIZE < n // 100
    q = sp.plan_of("ITEMS")
    assert all(p[k] == q[k] for k in p if k.endswith("grid") or k.startswith("max_")), "the same launches and tables: (n, segs) alone"


@pytest.mark.parametrize("pairs", [0, 1])
@pytest.mark.parametrize("name", list(sp.SHAPES))
def test_table_sizes_against_the_library(name, pairs):
    import lsdradixsort_amd as lsd
    sizes, local, _, _ = sp.SHAPES[name]
    n = sp.offsets_of(name)[1]
    want = int(lsd.lib().lsdsort_segmented_workspace_bytes(n, sizes.size, pairs))
    got = sp.workspace_bytes(sp.plan_of(name), n, pairs)
    assert got == want, f"{name} pairs={pairs}: the layout rebuilt from plan()'s caps takes {got} bytes, the library says {want}: {UPDATE}"


def random_sizes(rng, case):
    """a well-formed segmentation of a small array: (sizes, n)"""
    n = int(rng.integers(1, 300000))
    style = case % 4
    if style == 0:     # random cuts
        segs = int(rng.integers(1, 200))
        cuts = np.sort(rng.integers(0, n + 1, segs + 1))
        return np.diff(cuts), n
    if style == 1:     # adversarial: as many segments of k tiles + 1 keys as fit, the rest short
        k = int(rng.integers(1, 6))
        sizes = [k * sp.SEG_TILE + 1] * (n // (k * sp.SEG_TILE + 1))
    elif style == 2:   # mixed multiples, one past and one short of whole tiles
        sizes = []
        while sum(sizes) + 6 * sp.SEG_TILE < n:
            sizes.append(int(rng.integers(1, 6)) * sp.SEG_TILE + int(rng.choice([1, 1, 1, -1, 0, 2])))
    else:              # the tier boundaries and the smallest listed segment
        pool = [0, 1, 2, 3, sp.WAVE_CAP, sp.WAVE_CAP + 1, sp.SEG_TILE, sp.SEG_TILE + 1, sp.GROUP_CAP, sp.GROUP_CAP + 1]
        sizes = []
        while sum(sizes) + sp.GROUP_CAP + 1 < n:
            sizes.append(int(rng.choice(pool)))
    rest = n - sum(sizes)
    sizes += [2] * int(rng.integers(0, rest // 2 + 1))   # the smallest listed segments fill (some of) what is left
    sizes = np.array(sizes, dtype=np.int64)
    return sizes[rng.permutation(sizes.size)], n


def test_no_well_formed_segmentation_overfills_a_table():
    rng = np.random.default_rng(63)
    tightest = {}
    for case in range(4000):
        sizes, n = random_sizes(rng, case)
        assert sizes.sum() <= n
        for local in (True, False):
            p = sp.plan(sizes, local, n)
            what = f"n={n}, {sizes.size} segments (style {case % 4}), local={local}: {p}"
            assert p["wave"] <= p["listed"] and p["group"] <= p["group_cap"], what
            assert p["items"] <= p["max_items"] and p["tiles"] <= p["max_tiles"] and p["hist_tiles"] <= p["max_hist_tiles"], what
            assert p["block_sums"] <= p["max_hist_tiles"] * 256 // sp.SCAN_BLOCK + 1 and p["block_sums"] <= p["scan_grid"], what
            for k in ("items", "tiles", "hist_tiles"):
                tightest[k] = min(tightest.get(k, 1 << 30), p["max_" + k] - p[k])
    assert max(tightest.values()) <= 1, f"the adversarial cases come within one entry of every table: {tightest}"


def test_inputs_rotate_their_kind_with_the_segment():
    off = np.concatenate([[0], np.cumsum([300] * 13)]) + 5
    n = int(off[-1]) + 3
    for key_type, kinds in (("uint32", 5), ("float32", 6)):
        kind = sp.segment_kinds(13, key_type)
        assert (kind[1:] != kind[:-1]).all() and set(kind.tolist()) == set(range(kinds))
        keys = sp.make_keys(off, n, key_type, seed=1, device="cpu").numpy().view(np.uint32)
        assert keys.size == n and np.array_equal(keys, sp.make_keys(off, n, key_type, 1, "cpu").numpy().view(np.uint32))
        for s in range(13):
            seg = keys[off[s]:off[s + 1]]
            distinct = np.unique(seg).size
            if kind[s] == 0:
                assert distinct > 290
            elif kind[s] == 1:
                assert 100 < int((seg == 0).sum()) < 200
            elif kind[s] == 2:
                assert ((seg & 0xFF00FFFF) == 0x5A00C3E1).all() and distinct > 100
            elif kind[s] == 3:
                assert distinct == 4
            elif kind[s] == 4:
                assert distinct == 1
            else:
                assert np.isin(seg, np.array(sp.SPECIALS, dtype=np.uint32)).sum() > 50 and distinct > 150
