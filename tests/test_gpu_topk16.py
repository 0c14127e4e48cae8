"""GPU suite: lsdsort_topk16_device (GPUTopK16, topk16_rows), bit-exact over every output word, indices included.

Contract: row r's result is the first k items of the stable sort of the row in the requested order, with their positions.
Expected result: numpy, per row np.lexsort((positions, sortable16))[:k] with a numpy restatement of the key map -- never the code
under test.  torch.topk's values are a second witness where its order is the library's (int16, NaN-free and -0-free floats).

Boundaries of the implementation (lsdradixsort_amd/csrc/topk16.hip): rows of up to 1024 keys take one wavefront, up to 16384 one
workgroup, longer ones many workgroups per row (chunks of 16384 keys or more, 11 bits then 5); k above 3/4 of cols takes the sort
route; the winners are sorted by the segmented sort, whose own size classes change at k = 1024 and k = 16384.  Every row is split
by ITS address into the keys in front of its first 16-byte line, 16-byte groups, and the rest: odd cols and the byte offsets
0, 2, 6, 14 of the array put rows at every even offset within a line.  Every raw call here runs on outputs and a workspace
inside sentinel zones, with the workspace exactly as large as the library says."""
import numpy as np
import pytest
import torch

import lsdradixsort_amd as lsd
from _device_arrays import DTYPES, assert_equal, stream_ptr
from _guarded import assert_intact, guarded, guarded_workspace
from _guarded16 import assert_intact16, bits_of, guarded16
from _key_oracle import ALL_TYPES16 as ALL_TYPES, KEY_TYPES16 as KEY_TYPES, expected_np, make_keys16 as make_keys, sortable16_np

pytestmark = pytest.mark.gpu

OFFSETS = (0, 2, 6, 14)
FILL16, FILL32 = 0xA5A5, 0x3C3C3C3C   # what the outputs hold before a call


def k_values(cols):
    """1, 2, 63, 64, 65, either side of the winners' sort's size classes and of the sort route's threshold, cols - 1, cols"""
    thr = 3 * cols // 4   # the largest k of the select route
    ks = {1, 2, 63, 64, 65, 1023, 1024, 1025, 16383, 16384, 16385, thr - 1, thr, thr + 1, cols - 1, cols}
    return sorted(k for k in ks if 1 <= k <= cols)


class Call:
    """one raw call of the C entry: outputs and workspace inside sentinel zones, the values at byte offset `skip`"""

    def __init__(self, view, rows, cols, k, key_type, largest, skip=0, with_idx=True, stream=None, launch=True):
        L = lsd.lib()
        self.rows, self.k, self.with_idx, self.stream = rows, k, with_idx, stream
        self.vals_whole, self.vals = guarded16(np.full(rows * k, FILL16, dtype=np.uint16), skip)
        self.idx_whole, self.idx = guarded(np.full(rows * k, FILL32, dtype=np.uint32))
        self.ws_whole, self.ws = guarded_workspace(L.lsdsort_topk16_workspace_bytes(rows, cols, k))
        self.args = (view.data_ptr(), rows, cols, k, KEY_TYPES[key_type], int(largest), self.vals.data_ptr(),
                     self.idx.data_ptr() if with_idx else None, self.ws.data_ptr(), self.ws.numel(), stream_ptr(stream))
        torch.cuda.synchronize()
        if launch:
            self.launch()

    def launch(self):
        st = lsd.lib().lsdsort_topk16_device(*self.args)
        assert st == 0, st
        return self

    def result(self):
        """(values, indices) as [rows, k] uint16 / uint32 bits, after the fault word and every guard zone have been checked"""
        assert lsd.lib().lsdsort_check_device(self.ws.data_ptr(), stream_ptr(self.stream)) == 0
        torch.cuda.synchronize()
        fault = int(self.ws[:4].view(torch.int32).item())
        assert fault == 0, f"fault word {fault:#x}"
        assert_intact16(values=self.vals_whole)
        assert_intact(indices=self.idx_whole, workspace=self.ws_whole)
        idx = self.idx.cpu().numpy().view(np.uint32).reshape(self.rows, self.k)
        if not self.with_idx:
            assert (idx == FILL32).all(), "no index buffer was given: nothing may be written"
        return bits_of(self.vals).reshape(self.rows, self.k), idx


def check_case(view, shape, key_type, largest, k, ek, ei, what, skip=0, with_idx=True):
    rows, cols = shape
    values, indices = Call(view, rows, cols, k, key_type, largest, skip, with_idx).result()
    assert_equal(values, ek[:, :k], f"{what} k={k} values")
    if with_idx:
        assert_equal(indices, ei[:, :k], f"{what} k={k} indices")


# ---- every bit pattern ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("repeat", [1, 2], ids=["no ties", "every value twice"])
@pytest.mark.parametrize("key_type", ALL_TYPES)
def test_every_bit_pattern(key_type, repeat):
    """one long row of all 65536 values in a seeded order (once: no ties; twice: every value ties): the map, NaNs by sign at the
    two ends, -0 below +0"""
    perm = np.random.default_rng(16).permutation(1 << 16).astype(np.uint16)
    keys = np.tile(perm, repeat).reshape(1, -1)
    cols = keys.shape[1]
    whole, view = guarded16(keys, 0, DTYPES[key_type])
    for largest in (True, False):
        ek, ei = expected_np(keys, key_type, largest)
        for k in (1, 2, 255, 256, 257, 32767, 32768, 3 * cols // 4, 3 * cols // 4 + 1, cols):
            check_case(view, (1, cols), key_type, largest, k, ek, ei, f"all values x{repeat} {key_type} largest={largest}")
    assert_equal(bits_of(view), keys.reshape(-1), "input unchanged")
    assert_intact16(keys=whole)


# ---- size classes and row alignment ---------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (7, 1000), (513, 1023), (513, 1024), (513, 1025), (64, 16383), (64, 16384), (64, 16385), (5, 131073), (3, 300007)]


@pytest.mark.parametrize("key_type", ALL_TYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_size_classes_and_alignment_against_numpy(shape, key_type):
    rows, cols = shape
    keys = make_keys(rows, cols, key_type, seed=cols)
    expected = {largest: expected_np(keys, key_type, largest) for largest in (True, False)}
    for skip in OFFSETS:
        whole, view = guarded16(keys, skip, DTYPES[key_type])
        for largest in (True, False):
            ek, ei = expected[largest]
            for k in k_values(cols):
                check_case(view, shape, key_type, largest, k, ek, ei, f"{rows}x{cols} {key_type} largest={largest} offset {skip}", skip)
        assert_equal(bits_of(view), keys.reshape(-1), f"input unchanged (offset {skip})")
        assert_intact16(keys=whole)


# ---- ties -----------------------------------------------------------------------------------------------------------------------
def tie_inputs(rows, cols, key_type, seed):
    """name -> ([rows, cols] uint16, k values that fall inside the runs)"""
    rng = np.random.default_rng(seed)
    out = {}
    out["all equal"] = (np.full((rows, cols), 0x9E37, dtype=np.uint16), [1, cols // 3, cols - 1])
    four = np.array([5, 0x0100, 0x7FFF, 0xFFF0], dtype=np.uint16)
    out["four values"] = (four[rng.integers(0, 4, (rows, cols))], [1, cols // 5, cols // 2, 3 * cols // 4])
    shared = (np.uint16(0xAB00) | rng.integers(0, 256, (rows, cols)).astype(np.uint16))
    out["shared top byte"] = (shared, [1, 77 % cols + 1, cols // 2])
    run = min(100000, cols // 2)
    dup = rng.integers(0, 1 << 16, (rows, cols), dtype=np.uint32).astype(np.uint16)
    value = np.uint16(0x4000)
    for r in range(rows):
        dup[r, rng.permutation(cols)[:run]] = value
    s = sortable16_np(dup[0], key_type, False)
    sv = sortable16_np(np.array([value]), key_type, False)[0]
    below, above = int((s < sv).sum()), int((s > sv).sum())
    # row 0's k-th value is `value` either way round, with k inside its run of duplicates
    out["k-th value duplicated"] = (dup, [min(below, above) + run // 2, max(below, above) + run // 3])
    rnd = rng.integers(0, 1 << 16, (rows, cols), dtype=np.uint32).astype(np.uint16)
    asc = np.take_along_axis(rnd, np.argsort(sortable16_np(rnd, key_type, False), axis=1, kind="stable"), axis=1)
    out["sorted ascending"] = (asc, [1, cols // 7 + 1, cols // 2])
    out["sorted descending"] = (np.ascontiguousarray(asc[:, ::-1]), [1, cols // 7 + 1, cols // 2])
    return out


@pytest.mark.parametrize("key_type", ["uint16", "bfloat16"])
@pytest.mark.parametrize("shape", [(9, 700), (5, 9000), (3, 300007)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_ties_and_shared_prefixes_by_position(shape, key_type):
    rows, cols = shape
    for name, (keys, ks) in tie_inputs(rows, cols, key_type, seed=cols).items():
        whole, view = guarded16(keys, 2, DTYPES[key_type])
        for largest in (True, False):
            ek, ei = expected_np(keys, key_type, largest)
            for k in sorted(set(min(max(k, 1), cols) for k in ks)):
                check_case(view, shape, key_type, largest, k, ek, ei, f"{name} {rows}x{cols} {key_type} largest={largest}", 2)
        assert_equal(bits_of(view), keys.reshape(-1), f"{name}: input unchanged")
        assert_intact16(keys=whole)


# ---- the sort route at the segmented sort's item cap ----------------------------------------------------------------------------
@pytest.mark.parametrize("largest", [True, False])
def test_sort_route_past_the_segmented_sorts_item_cap(largest):
    """1027 rows of 16387 keys with k above 3/4 of cols: the sort route hands the segmented sort 1027 large segments with
    positions as payloads, three more than one round of its tile-table kernel takes (tests/_seg_plan.py, ITEMS).  int16 (ties in
    every row: 16387 keys of 65536 values), where torch's stable sort is the library's order."""
    rows, cols = 1027, 16387
    assert rows > 1024 and cols > 16384
    keys = make_keys(rows, cols, "int16", seed=1027)
    whole, view = guarded16(keys, 2, torch.int16)
    tk, ti = torch.sort(view.view(rows, cols), dim=-1, descending=largest, stable=True)
    ek, ei = bits_of(tk.contiguous()).reshape(rows, cols), ti.to(torch.int32).cpu().numpy().view(np.uint32)
    for k in (cols, 3 * cols // 4 + 1):
        check_case(view, (rows, cols), "int16", largest, k, ek, ei, f"{rows}x{cols} int16 largest={largest}")
    assert_equal(bits_of(view), keys.reshape(-1), "input unchanged")
    assert_intact16(keys=whole)


# ---- guards ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,k", [((9, 700), 33), ((9, 700), 1), ((5, 9000), 1500), ((3, 300007), 1000), ((3, 300007), 1),
                                     ((3, 300007), 299000)], ids=lambda v: str(v))
def test_guards_null_indices_and_fault_word(shape, k):
    """Call.result checks the sentinel zones around values, indices and workspace and the fault word; without an index buffer the
    one that was not passed stays as it was"""
    rows, cols = shape
    keys = make_keys(rows, cols, "float16", seed=k)
    ek, ei = expected_np(keys, "float16", True)
    whole, view = guarded16(keys, 6, torch.float16)
    for with_idx in (True, False):
        check_case(view, shape, "float16", True, k, ek, ei, f"{rows}x{cols} indices={with_idx}", 14, with_idx)
    assert_equal(bits_of(view), keys.reshape(-1), "input unchanged")
    assert_intact16(keys=whole)


# ---- other paths ----------------------------------------------------------------------------------------------------------------
THREE = [((9, 700), 33), ((5, 9000), 1500), ((3, 300007), 1000)]   # one short, one workgroup, one long


@pytest.mark.parametrize("shape,k", THREE, ids=lambda v: str(v))
def test_same_result_without_the_returning_add_rank_form(shape, k):
    rows, cols = shape
    keys = make_keys(rows, cols, "int16", seed=k + 1)
    ek, ei = expected_np(keys, "int16", False)
    whole, view = guarded16(keys, 0, torch.int16)
    lsd.set_rank_method(0)
    try:
        check_case(view, shape, "int16", False, k, ek, ei, f"rank method 0 {rows}x{cols}")
    finally:
        lsd.set_rank_method(-1)


@pytest.mark.parametrize("shape,k", THREE, ids=lambda v: str(v))
def test_two_streams_two_workspaces(shape, k):
    rows, cols = shape
    a = make_keys(rows, cols, "bfloat16", seed=1)
    b = make_keys(rows, cols, "bfloat16", seed=2)
    (_, da), (_, db) = guarded16(a, 2, torch.bfloat16), guarded16(b, 6, torch.bfloat16)
    serial_a = Call(da, rows, cols, k, "bfloat16", True).result()
    serial_b = Call(db, rows, cols, k, "bfloat16", False).result()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    s1.wait_stream(torch.cuda.current_stream())
    s2.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s1):
        par_a = Call(da, rows, cols, k, "bfloat16", True, stream=s1, launch=False)
    with torch.cuda.stream(s2):
        par_b = Call(db, rows, cols, k, "bfloat16", False, stream=s2, launch=False)
    torch.cuda.synchronize()
    par_a.launch()   # both are queued before either is waited for
    par_b.launch()
    torch.cuda.synchronize()
    for serial, par, keys, largest in ((serial_a, par_a, a, True), (serial_b, par_b, b, False)):
        values, indices = par.result()
        ek, ei = expected_np(keys, "bfloat16", largest)
        assert_equal(values, ek[:, :k], "values")
        assert_equal(indices, ei[:, :k], "indices")
        assert_equal(values, serial[0], "streams against the serial result: values")
        assert_equal(indices, serial[1], "streams against the serial result: indices")


@pytest.mark.parametrize("shape,k", [((40, 900), 17), ((6, 12000), 300), ((2, 500009), 2000)], ids=lambda v: str(v))
def test_graph_replay_on_fresh_inputs(shape, k):
    rows, cols = shape
    L = lsd.lib()
    assert L.lsdsort_prepare_device() == 0
    dk = torch.zeros((rows, cols), dtype=torch.int16, device="cuda")
    out_k = torch.zeros((rows, k), dtype=torch.int16, device="cuda")
    out_i = torch.zeros((rows, k), dtype=torch.int32, device="cuda")
    ws = torch.empty(L.lsdsort_topk16_workspace_bytes(rows, cols, k), dtype=torch.uint8, device="cuda")

    def call():
        st = L.lsdsort_topk16_device(dk.data_ptr(), rows, cols, k, KEY_TYPES["int16"], 1, out_k.data_ptr(), out_i.data_ptr(),
                                     ws.data_ptr(), ws.numel(), stream_ptr())
        assert st == 0, st

    dk.copy_(torch.from_numpy(make_keys(rows, cols, "int16", 1).view(np.int16)))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()   # warm-up: device set-up stays out of the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for seed in (2, 3, 4):
        keys = make_keys(rows, cols, "int16", seed)
        if seed == 3:
            keys = np.full((rows, cols), 0xFF85, dtype=np.uint16)   # all equal
        dk.copy_(torch.from_numpy(keys.view(np.int16)))
        out_k.zero_()
        out_i.zero_()
        g.replay()
        torch.cuda.synchronize()
        fault = int(ws[:4].view(torch.int32).item())
        assert fault == 0, f"replay {seed}: fault word {fault:#x}"
        ek, ei = expected_np(keys, "int16", True)
        assert_equal(bits_of(out_k).reshape(rows, k), ek[:, :k], f"replay {seed} values")
        assert_equal(out_i.cpu().numpy().view(np.uint32), ei[:, :k], f"replay {seed} indices")
    assert L.lsdsort_check_device(ws.data_ptr(), None) == 0


# ---- the torch-shaped face ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.int16, torch.float16, torch.bfloat16], ids=lambda d: str(d).replace("torch.", ""))
def test_topk16_rows_is_torch_topk(dtype):
    g = torch.Generator(device="cuda").manual_seed(5)
    if dtype == torch.int16:
        x = torch.randint(-(1 << 15), 1 << 15, (3, 5, 4000), generator=g, device="cuda", dtype=torch.int32).to(torch.int16)
    else:
        x = torch.randn((3, 5, 4000), generator=g, device="cuda").to(dtype)   # NaN-free
        x[x == 0] = 1.0                                                         # and free of zeros of either sign
    for largest in (True, False):
        v, i = lsd.topk16_rows(x, 10, largest=largest)
        tv, _ = torch.topk(x, 10, dim=-1, largest=largest, sorted=True)
        assert v.shape == tv.shape and v.dtype == dtype and i.dtype == torch.int64
        assert torch.equal(v, tv)
        assert torch.equal(torch.gather(x, -1, i), v)
    key_type = str(dtype).replace("torch.", "")
    v1, i1 = lsd.GPUTopK16(x[0, 0].contiguous(), 7, key_type=key_type, check_fault=True)
    assert v1.shape == (7,) and i1.shape == (7,) and i1.dtype == torch.int32 and v1.dtype == dtype
    assert torch.equal(v1, torch.topk(x[0, 0], 7).values)
    v2, i2 = lsd.GPUTopK16(x[0], 7, key_type=key_type, return_indices=False)
    assert i2 is None and v2.shape == (5, 7) and torch.equal(v2[0], v1)
