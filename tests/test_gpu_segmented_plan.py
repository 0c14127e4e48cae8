"""GPU suite: the segmented sort's large tier past its table and grid caps, bit-exact, with the planner's counters read back.

The shapes of tests/_seg_plan.py (held to their regimes by test_seg_plan_cpu.py) send seg_tiles_kernel, seg_hist_kernel,
seg_scatter_kernel and the carry of seg_scan_sums_kernel round their capped loops a second time, with ragged segments, short last
tiles, payloads, typed keys and digits that are far from uniform, and fill the tile tables to within one entry of seg_layout's
worst-case sizes.  Every call runs in a workspace of exactly lsdsort_segmented_workspace_bytes inside guard bands, with the keys
and payloads in guard bands too; after it the fault word and every band are checked, keys and payloads are compared bit for bit
with torch's stable sort of (segment id << 32 | sortable key) (_seg_plan.expected_dev), and the five counters the planner left in
the control block are compared with _seg_plan.plan(): a case that stops reaching its regime fails instead of passing for another
reason.  Run with -s to see the counters."""
import numpy as np
import pytest
import torch

import lsdradixsort_amd as lsd
import _seg_plan as sp
from _device_arrays import stream_ptr
from _guarded import GUARD, SENT32, assert_intact, guarded_workspace
from _key_oracle import KEY_TYPES32 as KEY_TYPES

pytestmark = pytest.mark.gpu

_inputs, _wanted = {}, {}   # made once per module and left unchanged


def offsets_dev(off):
    return torch.from_numpy(off.astype(np.uint32).view(np.int32)).cuda()


def shape_inputs(name, key_type, seed):
    """(offsets, n, keys' bits as int32 on the device) of a shape"""
    key = (name, key_type, seed)
    if key not in _inputs:
        off, n = sp.offsets_of(name)
        _inputs[key] = (off, n, sp.make_keys(off, n, key_type, seed))
    return _inputs[key]


def wanted(name, key_type, seed, descending):
    """(sorted keys, payloads of an arange) of the reference"""
    key = (name, key_type, seed, descending)
    if key not in _wanted:
        off, n, keys = shape_inputs(name, key_type, seed)
        want, idx = sp.expected_dev(keys, off, key_type, descending)
        vals = torch.arange(n, dtype=torch.int64, device="cuda")
        vals[int(off[0]):int(off[-1])] = idx
        _wanted[key] = (want, vals.to(torch.int32))
    return _wanted[key]


def guarded_dev(values):
    """_guarded.guarded for an int32 tensor that is on the device already: (whole, view)"""
    n = values.numel()
    whole = torch.full((GUARD + n + GUARD,), SENT32, dtype=torch.int32, device="cuda")
    view = whole[GUARD:GUARD + n]
    view.copy_(values)
    return whole, view


def assert_same(got, want, what):
    if not torch.equal(got, want):
        bad = (got != want).nonzero().reshape(-1)
        at = int(bad[0])
        raise AssertionError(f"{what}: {bad.numel()} words differ, first at {at}: got {int(got[at]) & 0xFFFFFFFF:#x} "
                             f"want {int(want[at]) & 0xFFFFFFFF:#x}")


def assert_counters(ws, plan, what):
    got = sp.read_counters(ws)
    print(f"{what}: counters {got}; caps items {plan['max_items']} tiles {plan['max_tiles']} hist tiles {plan['max_hist_tiles']}; "
          f"grids items {plan['items_grid']} tiles {plan['tile_grid']}; block sums {plan['block_sums']}")
    assert got == {k: plan[k] for k in sp.COUNTERS}, f"{what}: the planner counted {got}, _seg_plan.plan() {plan}"
    return got


class Call:
    """one raw call of the C entry: keys, payloads and an exactly sized workspace inside sentinel zones"""

    def __init__(self, keys, off, pairs, key_type="uint32", descending=False, ws=None):
        self.n, self.segs = keys.numel(), off.size - 1
        self.keys_whole, self.keys = guarded_dev(keys)
        self.vals_whole, self.vals = guarded_dev(torch.arange(self.n, dtype=torch.int32, device="cuda")) if pairs else (None, None)
        self.off = offsets_dev(off)
        self.ws_whole, self.ws = ws or guarded_workspace(lsd.lib().lsdsort_segmented_workspace_bytes(self.n, self.segs, int(pairs)))
        self.code, self.descending = KEY_TYPES[key_type], int(descending)

    def launch(self):
        st = lsd.lib().lsdsort_segmented_device(self.keys.data_ptr(), self.vals.data_ptr() if self.vals is not None else None,
                                                self.off.data_ptr(), self.segs, self.n, self.code, self.descending,
                                                self.ws.data_ptr(), self.ws.numel(), stream_ptr())
        assert st == 0, st
        return self

    def check(self, want_keys, want_vals, plan, what):
        """fault word, guard zones, every word of the outputs, the counters"""
        assert lsd.lib().lsdsort_check_device(self.ws.data_ptr(), stream_ptr()) == 0, f"{what}: fault word set"
        torch.cuda.synchronize()
        fault = int(self.ws[:4].view(torch.int32).item())
        assert fault == 0, f"{what}: fault word {fault:#x}"
        assert_intact(keys=self.keys_whole, payloads=self.vals_whole, workspace=self.ws_whole)
        counters = assert_counters(self.ws, plan, what)
        assert_same(self.keys, want_keys, f"{what}: keys")
        if self.vals is not None:
            assert_same(self.vals, want_vals, f"{what}: payloads")
        return counters


def run_shape(name, key_type="uint32", descending=False, pairs=True, seed=1):
    off, n, keys = shape_inputs(name, key_type, seed)
    want_keys, want_vals = wanted(name, key_type, seed, descending)
    call = Call(keys, off, pairs, key_type, descending).launch()
    call.check(want_keys, want_vals, sp.plan_of(name), f"{name} {key_type} descending={descending} pairs={pairs}")
    return call


@pytest.mark.parametrize("key_type,descending,pairs", [("uint32", False, False), ("uint32", False, True), ("int32", True, True),
                                                       ("float32", False, True)],
                         ids=["uint32 keys", "uint32 pairs", "int32 descending pairs", "float32 specials pairs"])
def test_items_second_round_of_the_tile_table_kernel(key_type, descending, pairs):
    run_shape("ITEMS", key_type, descending, pairs)


def test_items_tight_tables_one_entry_from_full():
    run_shape("ITEMS_TIGHT")


@pytest.mark.parametrize("name", ["ITEMS_FALLBACK", "FALLBACK_TIGHT"])
def test_fallback_form_past_the_item_cap(name):
    """the ballot rank form: every segment of two or more keys goes to the large tier"""
    lsd.set_rank_method(0)
    try:
        run_shape(name)
        if name == "ITEMS_FALLBACK":
            fallback = run_shape(name, "float32", True)
    finally:
        lsd.set_rank_method(-1)
    if name == "ITEMS_FALLBACK":
        # the default form on the same input: wave and workgroup tiers, no item at all
        off, n, keys = shape_inputs(name, "float32", 1)
        sizes = sp.SHAPES[name][0]
        default = Call(keys, off, True, "float32", True).launch()
        default.check(*wanted(name, "float32", 1, True), sp.plan(sizes, True, n), f"{name} float32 descending, default form")
        assert_same(fallback.keys, default.keys, "the two forms' keys")
        assert_same(fallback.vals, default.vals, "the two forms' payloads")


@pytest.mark.parametrize("key_type,descending,pairs", [("uint32", False, False), ("float32", True, True)],
                         ids=["uint32 keys", "float32 descending pairs"])
def test_tiles_second_round_of_hist_scatter_and_the_scan_carry(key_type, descending, pairs):
    run_shape("TILES", key_type, descending, pairs)
    _inputs.clear()   # 70 M keys and their reference: not kept for the rest of the module
    _wanted.clear()


def test_mixed_all_three_tiers_and_the_item_round():
    name = "MIXED"
    call = run_shape(name)
    off, n, keys = shape_inputs(name, "uint32", 1)
    head, tail = sp.SHAPES[name][2:]
    assert int(off[0]) == head and n - int(off[-1]) == tail and head and tail
    assert_same(call.keys[:head], keys[:head], "untouched head")
    assert_same(call.keys[n - tail:], keys[n - tail:], "untouched tail")
    assert_same(call.vals[:head], torch.arange(head, dtype=torch.int32, device="cuda"), "untouched head payloads")
    assert_same(call.vals[n - tail:], torch.arange(n - tail, n, dtype=torch.int32, device="cuda"), "untouched tail payloads")


def test_same_bits_twice():
    """the planner fills its lists by atomics, so the tile table's order differs from call to call: the result must not"""
    name = "ITEMS"
    off, n, keys = shape_inputs(name, "uint32", 1)
    want = wanted(name, "uint32", 1, False)
    ws = guarded_workspace(lsd.lib().lsdsort_segmented_workspace_bytes(n, off.size - 1, 1))
    first = Call(keys, off, True, ws=ws).launch()
    c1 = first.check(*want, sp.plan_of(name), f"{name} first call")
    second = Call(keys, off, True, ws=ws).launch()
    c2 = second.check(*want, sp.plan_of(name), f"{name} second call")
    assert c1 == c2
    assert_same(first.keys, second.keys, "keys of the two calls")
    assert_same(first.vals, second.vals, "payloads of the two calls")


def test_graph_replay_across_the_regime():
    """captured with offsets that leave the large tier's tables empty (every workgroup of its launches leaves), replayed with those,
    with ITEMS' offsets and fresh keys, and with the short ones again"""
    name = "ITEMS"
    off_large, n, _ = shape_inputs(name, "uint32", 1)
    segs = off_large.size - 1
    short_sizes = np.full(segs, sp.SHORT_SIZE, dtype=np.int64)
    off_short = np.concatenate([[0], np.cumsum(short_sizes)])
    assert off_short[-1] < n // 100
    call = Call(torch.zeros(n, dtype=torch.int32, device="cuda"), off_short, True)
    plans = {"short": sp.plan(short_sizes, True, n), "large": sp.plan_of(name)}

    def fill(off, seed):
        keys = sp.make_keys(off, n, "uint32", seed)
        call.keys.copy_(keys)
        call.vals.copy_(torch.arange(n, dtype=torch.int32, device="cuda"))
        call.off.copy_(offsets_dev(off))
        return keys

    fill(off_short, 10)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call.launch()   # warm-up: device set-up stays out of the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    fill(off_short, 11)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call.launch()
    for replay, (which, off, seed) in enumerate((("short", off_short, 12), ("large", off_large, 13), ("short", off_short, 14))):
        keys = fill(off, seed)
        want, idx = sp.expected_dev(keys, off)
        vals = torch.arange(n, dtype=torch.int64, device="cuda")
        vals[int(off[0]):int(off[-1])] = idx
        g.replay()
        call.check(want, vals.to(torch.int32), plans[which], f"replay {replay} ({which} offsets)")
