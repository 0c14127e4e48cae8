"""GPU suite: the per-row kernels past their grid caps -- the second and later rounds of every row loop, bit-exact.

The short-row kernels of topk.hip, topk16.hip, kth.hip, kth16.hip and rows16.hip run under a capped grid and walk the rows in a
grid-stride loop that carries LDS state (digit counters, the found bin, per-wave counts, the staged row) from one row to the next.
The shapes of tests/_row_rounds.py are the smallest that send each of those loops round again and end on a partly filled round
(test_row_rounds_cpu.py holds them against the launch lines); the other files of the suite stay inside the first round.

Inputs: every row is of one kind -- uniform bits, four values, all equal, all but the lowest digit shared, float specials -- and row
r + stride, which the same wave or workgroup takes next, is of another kind than row r: consecutive rounds stop the select at
different depths and leave different counters behind.

Calls: the C entries on caller-owned arrays inside sentinel zones (_guarded.py, _guarded16.py), the workspace exactly as large as
the library says.  The OUTPUTS are prefilled with the sentinel and the inputs hold it nowhere, so a row that a later round failed
to write shows as such; torch's caching allocator could hand a wrapper the previous call's correct answer instead.  After every
call: status, fault word, both zones of every buffer, the input unchanged.

Expected: the order-preserving map restated in numpy, then np.argsort(axis=1, kind="stable") -- expected_np of _key_oracle.py.  A
mismatch is reported by row, round (row // stride) and slot within the round (row % stride)."""
import functools
import zlib

import numpy as np
import pytest
import torch

import _row_rounds as rr
import lsdradixsort_amd as lsd
from _device_arrays import DTYPES, stream_ptr
from _guarded import SENT32, assert_intact, assert_unchanged, guarded, guarded_workspace, without_sentinel
from _guarded16 import SENT16, assert_intact16, bits_of, guarded16
from _key_oracle import KEY_TYPES16, KEY_TYPES32, SPECIALS16, SPECIALS32, expected_np

pytestmark = pytest.mark.gpu

TYPES32 = ["int32", "float32"]
TYPES16 = ["int16", "bfloat16"]
ORDERS = (False, True)


def params(shapes, types, group_types=()):
    """(shape name, key type): `types` on every shape, `group_types` on GROUP as well"""
    return [pytest.param(s, t, id=f"{s}-{t}") for s in shapes for t in list(types) + (list(group_types) if s == "GROUP" else [])]


# ---- inputs and what to expect of them: made once, shared, never written ------------------------------------------------------
@functools.lru_cache(maxsize=3)
def case(shape_name, stride, key_type, shift=0):
    """(keys [rows, cols] as bits, {largest: (sorted keys, positions)}): rows of mixed kinds, the kind changing from round to round"""
    rows, cols = rr.SHAPES[shape_name]
    wide = key_type in KEY_TYPES32
    specials = SPECIALS32 if key_type == "float32" else SPECIALS16.get(key_type)
    seed = zlib.crc32(f"{shape_name} {key_type} {shift}".encode())
    keys = rr.mixed_rows(rows, cols, stride, 32 if wide else 16, specials, seed, shift)
    if wide:
        without_sentinel(keys)
    else:
        keys[keys == SENT16] ^= np.uint16(1)
    expected = {largest: expected_np(keys, key_type, largest) for largest in ORDERS}
    for a in (keys,) + expected[False] + expected[True]:
        a.setflags(write=False)
    return keys, expected


def assert_rows(got, want, stride, sentinel, what):
    """bit for bit over all rows; a failure names the first bad row, its round of the row loop and its slot within the round"""
    got = np.asarray(got).reshape(want.shape)
    if np.array_equal(got, want):
        return
    differ = got != want
    bad = np.flatnonzero(differ.reshape(want.shape[0], -1).any(axis=1))
    row = int(bad[0])
    untouched = int((differ & (got == sentinel)).sum())

    def words(a):
        a = np.atleast_1d(a)
        return " ".join(f"{int(x):#x}" for x in a[:8]) + (" .." if a.size > 8 else "")

    raise AssertionError(f"{what}: {bad.size} of {want.shape[0]} rows differ, in round(s) {np.unique(bad // stride).tolist()} of the row loop "
                         f"(a round is {stride} rows); first bad row {row} = round {row // stride}, slot {row % stride}; "
                         f"{untouched} of the {int(differ.sum())} differing words still hold the sentinel {sentinel:#x}; "
                         f"got {words(got[row])} want {words(want[row])}")


class Input:
    """the keys on the device inside guard zones; check(): zones intact and the keys as they were"""

    def __init__(self, keys, key_type):
        self.keys, self.wide = keys, key_type in KEY_TYPES32
        self.code = (KEY_TYPES32 if self.wide else KEY_TYPES16)[key_type]
        self.whole, self.view = guarded(keys) if self.wide else guarded16(keys, 0, DTYPES[key_type])

    def check(self):
        if self.wide:
            assert_intact(keys=self.whole)
            assert_unchanged(self.view, self.keys)
        else:
            assert_intact16(keys=self.whole)
            assert np.array_equal(bits_of(self.view), self.keys.reshape(-1)), "a read-only input was changed"


class Outputs:
    """values (32- or 16-bit), positions and a workspace of exactly `need` bytes, the first two full of the sentinel"""

    def __init__(self, words, wide, need, values=None):
        assert need > 0 and need % 256 == 0
        self.wide, self.words = wide, words
        if values is not None:
            self.vals_whole, self.vals = values           # in place: the keys' own buffer
        elif wide:
            self.vals_whole, self.vals = guarded(np.full(words, SENT32, dtype=np.uint32))
        else:
            self.vals_whole, self.vals = guarded16(np.full(words, SENT16, dtype=np.uint16))
        self.idx_whole, self.idx = guarded(np.full(words, SENT32, dtype=np.uint32))
        self.ws_whole, self.ws = guarded_workspace(need)
        torch.cuda.synchronize()

    def settle(self, status, with_idx=True):
        """after the call: status, fault word, every zone; returns (values, positions) as bits on the host"""
        assert status == 0, status
        assert lsd.lib().lsdsort_check_device(self.ws.data_ptr(), None) == 0, "fault word"
        torch.cuda.synchronize()
        fault = int(self.ws[:4].view(torch.int32).item())
        assert fault == 0, f"fault word {fault:#x}"
        if self.wide:
            assert_intact(values=self.vals_whole)
        else:
            assert_intact16(values=self.vals_whole)
        assert_intact(positions=self.idx_whole, workspace=self.ws_whole)
        idx = self.idx.cpu().numpy().view(np.uint32)
        if not with_idx:
            assert (idx == SENT32).all(), "no index buffer was given: nothing may be written"
        return (self.vals.cpu().numpy().view(np.uint32) if self.wide else bits_of(self.vals)), idx


def sent(inp):
    return SENT32 if inp.wide else SENT16


# ---- k-th value ---------------------------------------------------------------------------------------------------------------
def call_kth(inp, rows, cols, rank, largest, with_idx=True):
    L = lsd.lib()
    entry, size = (L.lsdsort_kth_device, L.lsdsort_kth_workspace_bytes) if inp.wide else (L.lsdsort_kth16_device, L.lsdsort_kth16_workspace_bytes)
    out = Outputs(rows, inp.wide, size(rows, cols))
    st = entry(inp.view.data_ptr(), rows, cols, rank, inp.code, int(largest), out.vals.data_ptr(), out.idx.data_ptr() if with_idx else None,
               out.ws.data_ptr(), out.ws.numel(), stream_ptr())
    got = out.settle(st, with_idx)
    inp.check()
    return got


def check_kth(shape_name, key_type, unit):
    rows, cols = rr.SHAPES[shape_name]
    stride = rr.stride_of(shape_name, unit)
    keys, expected = case(shape_name, stride, key_type)
    inp = Input(keys, key_type)
    for largest in ORDERS:
        ek, ei = expected[largest]
        for rank in (0, cols // 2, cols - 1):
            values, positions = call_kth(inp, rows, cols, rank, largest)
            what = f"{unit} {shape_name} {rows}x{cols} {key_type} largest={largest} rank={rank}"
            assert_rows(values, ek[:, rank], stride, sent(inp), f"{what}: values")
            assert_rows(positions, ei[:, rank], stride, SENT32, f"{what}: positions")
    rank = cols // 2
    values, _ = call_kth(inp, rows, cols, rank, True, with_idx=False)
    assert_rows(values, expected[True][0][:, rank], stride, sent(inp), f"{unit} {shape_name} {key_type} rank={rank}, no index buffer: values")


@pytest.mark.parametrize("shape_name,key_type", params(["WAVE32", "GROUP"], TYPES32))
def test_kth(shape_name, key_type):
    check_kth(shape_name, key_type, "kth")


@pytest.mark.parametrize("shape_name,key_type", params(["WAVE16", "GROUP"], TYPES16, ["float16"]))
def test_kth16(shape_name, key_type):
    check_kth(shape_name, key_type, "kth16")


# ---- top-k --------------------------------------------------------------------------------------------------------------------
def k_values(shape_name, cols):
    """1, a mid k and the largest k of the select route, cols for the sort route; OFFS: one k per route"""
    return [2, cols] if shape_name == "OFFS" else [1, cols // 3, 3 * cols // 4, cols]


def call_topk(inp, rows, cols, k, largest):
    L = lsd.lib()
    entry, size = (L.lsdsort_topk_device, L.lsdsort_topk_workspace_bytes) if inp.wide else (L.lsdsort_topk16_device, L.lsdsort_topk16_workspace_bytes)
    out = Outputs(rows * k, inp.wide, size(rows, cols, k))
    st = entry(inp.view.data_ptr(), rows, cols, k, inp.code, int(largest), out.vals.data_ptr(), out.idx.data_ptr(), out.ws.data_ptr(),
               out.ws.numel(), stream_ptr())
    got = out.settle(st)
    inp.check()
    return got


def check_topk(shape_name, key_type, unit):
    rows, cols = rr.SHAPES[shape_name]
    stride = rr.stride_of(shape_name, unit)
    keys, expected = case(shape_name, stride, key_type)
    inp = Input(keys, key_type)
    for largest in ORDERS:
        ek, ei = expected[largest]
        for k in k_values(shape_name, cols):
            assert (4 * k > 3 * cols) == (k == cols), "only k = cols takes the sort route"
            values, positions = call_topk(inp, rows, cols, k, largest)
            what = f"{unit} {shape_name} {rows}x{cols} {key_type} largest={largest} k={k}"
            assert_rows(values, ek[:, :k], stride, sent(inp), f"{what}: values")
            assert_rows(positions, ei[:, :k], stride, SENT32, f"{what}: positions")


@pytest.mark.parametrize("shape_name,key_type", params(["WAVE32", "OFFS", "GROUP"], TYPES32))
def test_topk(shape_name, key_type):
    check_topk(shape_name, key_type, "topk")


@pytest.mark.parametrize("shape_name,key_type", params(["WAVE16", "OFFS", "GROUP"], TYPES16, ["float16"]))
def test_topk16(shape_name, key_type):
    check_topk(shape_name, key_type, "topk16")


# ---- rows16 -------------------------------------------------------------------------------------------------------------------
def call_rows16(inp, rows, cols, descending, in_place=False):
    L = lsd.lib()
    out = Outputs(rows * cols, False, L.lsdsort_rows16_workspace_bytes(rows, cols), values=(inp.whole, inp.view) if in_place else None)
    st = L.lsdsort_rows16_device(inp.view.data_ptr(), rows, cols, inp.code, int(descending), out.vals.data_ptr(), out.idx.data_ptr(),
                                 out.ws.data_ptr(), out.ws.numel(), stream_ptr())
    got = out.settle(st)
    if not in_place:
        inp.check()
    return got


def check_rows16(shape_name, key_type, what, orders=ORDERS, in_place=False):
    rows, cols = rr.SHAPES[shape_name]
    stride = rr.stride_of(shape_name, "rows16")
    keys, expected = case(shape_name, stride, key_type)
    inp = None
    for descending in orders:
        if inp is None or in_place:
            inp = Input(keys, key_type)
        ek, ei = expected[descending]
        values, positions = call_rows16(inp, rows, cols, descending, in_place)
        tag = f"rows16 {what} {shape_name} {rows}x{cols} {key_type} descending={descending}"
        assert_rows(values, ek, stride, SENT16, f"{tag}: values")
        assert_rows(positions, ei, stride, SENT32, f"{tag}: positions")


@pytest.mark.parametrize("shape_name,key_type", params(["ROWS16_WAVE", "GROUP"], TYPES16, ["float16"]))
def test_rows16(shape_name, key_type):
    check_rows16(shape_name, key_type, "default route")


@pytest.mark.parametrize("key_type", TYPES16)
def test_rows16_widen_route(key_type):
    lsd.set_rows16_route(0)
    try:
        check_rows16("ROWS16_WAVE", key_type, "widen route")
    finally:
        lsd.set_rows16_route(-1)


def test_rows16_in_place():
    """d_out_keys == d_keys: every row is staged whole before it is stored, in the second round as in the first"""
    check_rows16("GROUP", "bfloat16", "in place", orders=(True,), in_place=True)


# ---- graph replay -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unit", ["topk", "topk16", "kth", "kth16", "rows16"])
def test_graph_replay_on_shifted_kinds(unit):
    """captured once on one input, replayed on a second one whose row kinds are shifted by one (every row changes its kind), then on
    the first again; the outputs hold the sentinel before every replay"""
    wide = not unit.endswith("16")
    shape_name, key_type = ("WAVE32", "int32") if wide else ("WAVE16", "int16")
    rows, cols = rr.SHAPES[shape_name]
    stride = rr.stride_of(shape_name, unit)
    arg = {"topk": 3 * cols // 4, "topk16": 3 * cols // 4, "kth": cols // 2, "kth16": cols // 2}.get(unit)   # k or rank
    width = {"topk": arg, "topk16": arg, "rows16": cols}.get(unit, 1)                                        # output words per row
    code = (KEY_TYPES32 if wide else KEY_TYPES16)[key_type]
    L = lsd.lib()
    assert L.lsdsort_prepare_device() == 0
    entry, size = getattr(L, f"lsdsort_{unit}_device"), getattr(L, f"lsdsort_{unit}_workspace_bytes")
    dk = torch.zeros(rows * cols, dtype=torch.int32 if wide else torch.int16, device="cuda")
    out_k = torch.zeros(rows * width, dtype=dk.dtype, device="cuda")
    out_i = torch.zeros(rows * width, dtype=torch.int32, device="cuda")
    ws = torch.empty(size(rows, cols, arg) if unit.startswith("topk") else size(rows, cols), dtype=torch.uint8, device="cuda")

    def call():
        args = (dk.data_ptr(), rows, cols) + (() if arg is None else (arg,)) + (code, 1, out_k.data_ptr(), out_i.data_ptr(), ws.data_ptr(),
                                                                                ws.numel(), stream_ptr())
        st = entry(*args)
        assert st == 0, st

    def put(keys):
        dk.copy_(torch.from_numpy(keys.reshape(-1).view(np.int32 if wide else np.int16).copy()))

    first, second = case(shape_name, stride, key_type), case(shape_name, stride, key_type, 1)
    put(first[0])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()   # warm-up: device set-up stays out of the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for name, (keys, expected) in (("shifted kinds", second), ("the first input again", first)):
        put(keys)
        out_k.fill_(SENT32 if wide else SENT16)
        out_i.fill_(SENT32)
        g.replay()
        torch.cuda.synchronize()
        fault = int(ws[:4].view(torch.int32).item())
        assert fault == 0, f"replay on {name}: fault word {fault:#x}"
        ek, ei = expected[True]
        if unit.startswith("kth"):
            ek, ei = ek[:, arg], ei[:, arg]
        elif unit.startswith("topk"):
            ek, ei = ek[:, :arg], ei[:, :arg]
        got_k = out_k.cpu().numpy().view(np.uint32 if wide else np.uint16)
        assert_rows(got_k, ek, stride, SENT32 if wide else SENT16, f"{unit} replay on {name}: values")
        assert_rows(out_i.cpu().numpy().view(np.uint32), ei, stride, SENT32, f"{unit} replay on {name}: positions")
        assert np.array_equal(dk.cpu().numpy().view(keys.dtype), keys.reshape(-1)), f"{unit} replay on {name}: input changed"
    assert L.lsdsort_check_device(ws.data_ptr(), None) == 0
