"""GPU suite: lsdsort_topk_device (GPUTopK, topk_rows), bit-exact over every output word, indices included.

Contract: row r's result is the first k items of the stable sort of the row in the requested order, with their positions.
Expected result: for small shapes numpy, per row np.lexsort((positions, sortable key))[:k]; for large shapes the library's own
sort_rows(x, descending=largest, return_indices=True) cut to k columns (pinned to numpy and torch.sort by test_gpu_segmented.py);
torch.topk's values are a third witness where its order is the library's (int32, NaN-free float32).  Every case runs once.

Boundaries of the implementation (lsdradixsort_amd/csrc/topk.hip): rows of up to 1024 keys take one wavefront, up to 16384 one
workgroup, longer ones many workgroups per row (chunks of 16384 keys or more); k above 3/4 of cols takes the sort route; the k
winners are sorted by the segmented sort, whose own size classes change at k = 1024 and k = 16384."""
import numpy as np
import pytest
import torch

import lsdradixsort_amd as lsd
from _device_arrays import assert_equal, bits, to_dev
from _key_oracle import KEY_TYPES32 as KEY_TYPES, expected_np, make_keys32 as make_keys

pytestmark = pytest.mark.gpu


def k_values(cols):
    """1, 2, 63, 64, 65, either side of the winners' sort's size classes and of the sort route's threshold, cols - 1, cols"""
    thr = 3 * cols // 4   # the largest k of the select route
    ks = {1, 2, 63, 64, 65, 1023, 1024, 1025, 16383, 16384, 16385, thr - 1, thr, thr + 1, cols - 1, cols}
    return sorted(k for k in ks if 1 <= k <= cols)


def check_case(dk, key_type, largest, k, ek, ei, what):
    """one call, every word of both outputs against the expected full order cut to k"""
    values, indices = lsd.GPUTopK(dk, k, key_type=key_type, largest=largest, check_fault=True)
    torch.cuda.synchronize()
    assert_equal(bits(values), ek[:, :k], f"{what} k={k} values")
    assert_equal(bits(indices), ei[:, :k], f"{what} k={k} indices")


SMALL_SHAPES = [(1, 1), (7, 1000), (513, 1023), (513, 1024), (513, 1025), (64, 16383), (64, 16384), (64, 16385)]


@pytest.mark.parametrize("key_type", ["uint32", "int32", "float32"])
@pytest.mark.parametrize("shape", SMALL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_short_rows_against_numpy(shape, key_type):
    rows, cols = shape
    keys = make_keys(rows, cols, key_type, seed=cols)
    dk = to_dev(keys, key_type)
    for largest in (True, False):
        ek, ei = expected_np(keys, key_type, largest)
        for k in k_values(cols):
            check_case(dk, key_type, largest, k, ek, ei, f"{rows}x{cols} {key_type} largest={largest}")
    assert_equal(bits(dk), keys, "input unchanged")


def expected_sort_rows(dk, largest):
    ek, ei = lsd.sort_rows(dk, descending=largest, return_indices=True)
    torch.cuda.synchronize()
    return ek, ei


def check_case_dev(dk, key_type, largest, k, ek, ei, what, witness=False):
    values, indices = lsd.GPUTopK(dk, k, key_type=key_type, largest=largest, check_fault=True)
    torch.cuda.synchronize()
    assert torch.equal(values.view(torch.int32), ek[:, :k].contiguous().view(torch.int32)), f"{what} k={k}: values differ"
    assert torch.equal(indices.to(torch.int64), ei[:, :k]), f"{what} k={k}: indices differ"
    if witness:   # torch does not promise which tie it returns: values only
        tv = torch.topk(dk, k, dim=-1, largest=largest, sorted=True).values
        assert torch.equal(values.view(torch.int32), tv.view(torch.int32)), f"{what} k={k}: values differ from torch.topk"


LONG_SHAPES = [(32, 131072), (4, (1 << 22) + 3), (1, (1 << 20) + 7)]


@pytest.mark.parametrize("key_type", ["int32", "float32"])
@pytest.mark.parametrize("shape", LONG_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_long_rows_against_sort_rows(shape, key_type):
    rows, cols = shape
    keys = make_keys(rows, cols, key_type, seed=cols + 1)
    dk = to_dev(keys, key_type)
    for largest in (True, False):
        ek, ei = expected_sort_rows(dk, largest)
        for k in k_values(cols):
            check_case_dev(dk, key_type, largest, k, ek, ei, f"{rows}x{cols} {key_type} largest={largest}")
    assert_equal(bits(dk), keys, "input unchanged")


@pytest.mark.parametrize("key_type", ["uint32", "int32", "float32"])
def test_long_row_against_numpy(key_type):
    rows, cols = 3, (1 << 20) + 7
    keys = make_keys(rows, cols, key_type, seed=11)
    dk = to_dev(keys, key_type)
    for largest in (True, False):
        ek, ei = expected_np(keys, key_type, largest)
        for k in (1, 65, 1024, 16385, 3 * cols // 4, 3 * cols // 4 + 1, cols):
            check_case(dk, key_type, largest, k, ek, ei, f"{rows}x{cols} {key_type} largest={largest}")


@pytest.mark.parametrize("key_type", ["int32", "float32"])
@pytest.mark.parametrize("shape", [(4096, 256), (32, 131072), (1, (1 << 22) + 5)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_values_against_torch_topk(shape, key_type):
    """third witness: NaN-free float32 (no -0.0 either: torch calls the zeros equal) and int32, where torch's order is ours"""
    rows, cols = shape
    rng = np.random.default_rng(cols + 5)
    if key_type == "float32":
        x = rng.standard_normal((rows, cols)).astype(np.float32)
        x[x == 0] = 1.0
        x[:, ::97] = np.float32(np.inf)
        x[:, 1::89] = -np.float32(np.inf)
        x[:, 2::83] = np.float32(1e-42)   # denormal
        dk = torch.from_numpy(x).cuda()
    else:
        dk = torch.from_numpy(rng.integers(-1 << 31, 1 << 31, (rows, cols), dtype=np.int64).astype(np.int32)).cuda()
    for largest in (True, False):
        ek, ei = expected_sort_rows(dk, largest)
        for k in (1, 8, 50, min(cols, 1024)):
            check_case_dev(dk, key_type, largest, k, ek, ei, f"{rows}x{cols} {key_type} largest={largest}", witness=True)


@pytest.mark.parametrize("largest", [True, False])
def test_sort_route_past_the_segmented_sorts_item_cap(largest):
    """1027 rows of 16387 keys with k above 3/4 of cols: the sort route hands the segmented sort 1027 large segments with
    positions as payloads, three more than one round of its tile-table kernel takes (tests/_seg_plan.py, ITEMS).  int32 with
    ties, where torch's stable sort is the library's order."""
    rows, cols = 1027, 16387
    assert rows > 1024 and cols > 16384
    g = torch.Generator(device="cuda").manual_seed(1027)
    dk = torch.randint(-(1 << 31), 1 << 31, (rows, cols), generator=g, device="cuda", dtype=torch.int64).to(torch.int32)
    dk[:, ::5] >>= 20   # ties within every row
    before = dk.clone()
    ek, ei = torch.sort(dk, dim=-1, descending=largest, stable=True)
    for k in (cols, 3 * cols // 4 + 1):
        check_case_dev(dk, "int32", largest, k, ek, ei, f"{rows}x{cols} int32 largest={largest}")
    assert torch.equal(dk, before), "input unchanged"


def test_one_row_of_2_26():
    cols = 1 << 26
    g = torch.Generator(device="cuda").manual_seed(26)
    dk = torch.rand(cols, generator=g, device="cuda", dtype=torch.float32).view(1, cols)
    before = dk.clone()
    ek, ei = expected_sort_rows(dk, True)
    for k in (1, 1024, 16385, 3 * cols // 4 + 1):
        check_case_dev(dk, "float32", True, k, ek, ei, f"1x2^26 float32 largest", witness=(k == 1024))
    assert torch.equal(dk, before), "input unchanged"


def test_2_28_keys():
    rows, cols = 64, 1 << 22
    g = torch.Generator(device="cuda").manual_seed(28)
    dk = torch.randint(-(1 << 31), 1 << 31, (rows, cols), generator=g, device="cuda", dtype=torch.int64).to(torch.int32)
    ek, ei = expected_sort_rows(dk, False)
    for k in (2, 100, 1025):
        check_case_dev(dk, "int32", False, k, ek, ei, "64x2^22 int32 smallest", witness=(k == 100))


def tie_inputs(rows, cols, seed):
    """name -> [rows, cols] uint32: inputs whose top bits agree, and the k values that fall inside their runs"""
    rng = np.random.default_rng(seed)
    out = {}
    out["all equal"] = (np.full((rows, cols), 0x9E3779B9, dtype=np.uint32), [1, cols // 3, cols - 1])
    four = np.array([5, 0x00010000, 0x7FFFFFFF, 0xFFFFFFF0], dtype=np.uint32)
    out["four values"] = (four[rng.integers(0, 4, (rows, cols))], [1, cols // 5, cols // 2, 3 * cols // 4])
    shared = (np.uint32(0xABCDEF00) | rng.integers(0, 256, (rows, cols)).astype(np.uint32))
    out["shared top 24 bits"] = (shared, [1, 77 % cols + 1, cols // 2])
    run = min(100000, cols // 2)
    dup = rng.integers(0, 1 << 32, (rows, cols), dtype=np.uint64).astype(np.uint32)
    value = np.uint32(0x40000000)
    for r in range(rows):
        dup[r, rng.permutation(cols)[:run]] = value
    below = int((dup[0] < value).sum())
    above = int((dup[0] > value).sum())
    # row 0's k-th value is `value` either way round, with k inside its run of duplicates
    out["k-th value duplicated"] = (dup, [min(below, above) + run // 2, max(below, above) + run // 3])
    asc = np.sort(rng.integers(0, 1 << 32, (rows, cols), dtype=np.uint64).astype(np.uint32), axis=1)
    out["sorted ascending"] = (asc, [1, cols // 7 + 1, cols // 2])
    out["sorted descending"] = (np.ascontiguousarray(asc[:, ::-1]), [1, cols // 7 + 1, cols // 2])
    return out


@pytest.mark.parametrize("key_type", ["uint32", "float32"])
@pytest.mark.parametrize("shape", [(9, 700), (5, 9000), (3, 300007)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_ties_and_shared_prefixes_by_position(shape, key_type):
    rows, cols = shape
    for name, (keys, ks) in tie_inputs(rows, cols, seed=cols).items():
        dk = to_dev(keys, key_type)
        for largest in (True, False):
            ek, ei = expected_np(keys, key_type, largest)
            for k in sorted(set(min(max(k, 1), cols) for k in ks)):
                check_case(dk, key_type, largest, k, ek, ei, f"{name} {rows}x{cols} {key_type} largest={largest}")
        assert_equal(bits(dk), keys, f"{name}: input unchanged")


def raw_call(dk, k, key_type, largest, with_idx=True, stream=None, guard=64):
    """the C entry on output buffers with guard words on both sides; returns (values, indices or None, workspace)"""
    rows, cols = dk.shape
    L = lsd.lib()
    out_k = torch.full((rows * k + 2 * guard,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    out_i = torch.full((rows * k + 2 * guard,), 0x3C3C3C3C, dtype=torch.int32, device="cuda")
    ws = torch.empty(L.lsdsort_topk_workspace_bytes(rows, cols, k), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    st = L.lsdsort_topk_device(dk.data_ptr(), rows, cols, k, KEY_TYPES[key_type], int(largest), out_k.data_ptr() + 4 * guard,
                               out_i.data_ptr() + 4 * guard if with_idx else None, ws.data_ptr(), ws.numel(),
                               int((stream or torch.cuda.current_stream()).cuda_stream))
    assert st == 0, st
    return out_k, out_i, ws


@pytest.mark.parametrize("shape,k", [((9, 700), 33), ((5, 9000), 1500), ((3, 300007), 1000), ((3, 300007), 299000)],
                         ids=lambda v: str(v))
def test_guards_null_indices_and_fault_word(shape, k):
    rows, cols = shape
    guard = 64
    keys = make_keys(rows, cols, "float32", seed=k)
    dk = to_dev(keys, "float32")
    ek, ei = expected_np(keys, "float32", True)
    for with_idx in (True, False):
        out_k, out_i, ws = raw_call(dk, k, "float32", True, with_idx=with_idx, guard=guard)
        assert lsd.lib().lsdsort_check_device(ws.data_ptr(), None) == 0
        gk, gi = bits(out_k), bits(out_i)
        assert_equal(gk[guard:-guard].reshape(rows, k), ek[:, :k], f"values (indices={with_idx})")
        assert (gk[:guard] == 0x5A5A5A5A).all() and (gk[-guard:] == 0x5A5A5A5A).all(), "guard words around the values"
        if with_idx:
            assert_equal(gi[guard:-guard].reshape(rows, k), ei[:, :k], "indices")
            assert (gi[:guard] == 0x3C3C3C3C).all() and (gi[-guard:] == 0x3C3C3C3C).all(), "guard words around the indices"
        else:
            assert (gi == 0x3C3C3C3C).all(), "no index buffer was given: nothing may be written"
    assert_equal(bits(dk), keys, "input unchanged")


@pytest.mark.parametrize("shape,k", [((9, 700), 33), ((5, 9000), 1500), ((3, 300007), 1000)], ids=lambda v: str(v))
def test_same_result_without_the_returning_add_rank_form(shape, k):
    rows, cols = shape
    keys = make_keys(rows, cols, "int32", seed=k + 1)
    dk = to_dev(keys, "int32")
    ek, ei = expected_np(keys, "int32", False)
    lsd.set_rank_method(0)
    try:
        check_case(dk, "int32", False, k, ek, ei, f"rank method 0 {rows}x{cols}")
    finally:
        lsd.set_rank_method(-1)


def test_two_streams_two_workspaces():
    rows, cols, k = 6, 200001, 500
    a = make_keys(rows, cols, "float32", seed=1)
    b = make_keys(rows, cols, "float32", seed=2)
    da, db = to_dev(a, "float32"), to_dev(b, "float32")
    serial_a = raw_call(da, k, "float32", True)
    serial_b = raw_call(db, k, "float32", False)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    s1.wait_stream(torch.cuda.current_stream())
    s2.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s1):
        par_a = raw_call(da, k, "float32", True, stream=s1)
    with torch.cuda.stream(s2):
        par_b = raw_call(db, k, "float32", False, stream=s2)
    torch.cuda.synchronize()
    for serial, par, keys, largest in ((serial_a, par_a, a, True), (serial_b, par_b, b, False)):
        assert torch.equal(serial[0], par[0]) and torch.equal(serial[1], par[1]), "streams disagree with the serial result"
        ek, ei = expected_np(keys, "float32", largest)
        assert_equal(bits(par[0])[64:-64].reshape(rows, k), ek[:, :k], "values")
        assert_equal(bits(par[1])[64:-64].reshape(rows, k), ei[:, :k], "indices")
        assert lsd.lib().lsdsort_check_device(par[2].data_ptr(), None) == 0


@pytest.mark.parametrize("shape,k", [((40, 900), 17), ((6, 12000), 300), ((2, 500009), 2000)], ids=lambda v: str(v))
def test_graph_replay_on_fresh_inputs(shape, k):
    rows, cols = shape
    L = lsd.lib()
    assert L.lsdsort_prepare_device() == 0
    dk = torch.zeros((rows, cols), dtype=torch.int32, device="cuda")
    out_k = torch.zeros((rows, k), dtype=torch.int32, device="cuda")
    out_i = torch.zeros((rows, k), dtype=torch.int32, device="cuda")
    ws = torch.empty(L.lsdsort_topk_workspace_bytes(rows, cols, k), dtype=torch.uint8, device="cuda")

    def call():
        st = L.lsdsort_topk_device(dk.data_ptr(), rows, cols, k, KEY_TYPES["int32"], 1, out_k.data_ptr(), out_i.data_ptr(),
                                   ws.data_ptr(), ws.numel(), int(torch.cuda.current_stream().cuda_stream))
        assert st == 0, st

    dk.copy_(torch.from_numpy(make_keys(rows, cols, "int32", 1).view(np.int32)))
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
        keys = make_keys(rows, cols, "int32", seed)
        if seed == 3:
            keys = np.full((rows, cols), 0xFFFFFF85, dtype=np.uint32)   # all equal
        dk.copy_(torch.from_numpy(keys.view(np.int32)))
        out_k.zero_()
        out_i.zero_()
        g.replay()
        torch.cuda.synchronize()
        fault = int(ws[:4].view(torch.int32).item())
        assert fault == 0, f"replay {seed}: fault word {fault:#x}"
        ek, ei = expected_np(keys, "int32", True)
        assert_equal(bits(out_k), ek[:, :k], f"replay {seed} values")
        assert_equal(bits(out_i), ei[:, :k], f"replay {seed} indices")
    assert L.lsdsort_check_device(ws.data_ptr(), None) == 0


def test_topk_rows_is_torch_topk():
    x = torch.randn(3, 5, 4000, device="cuda")
    for largest in (True, False):
        v, i = lsd.topk_rows(x, 10, largest=largest)
        tv, _ = torch.topk(x, 10, dim=-1, largest=largest, sorted=True)
        assert v.shape == tv.shape and i.dtype == torch.int64
        assert torch.equal(v, tv)
        assert torch.equal(torch.gather(x, -1, i), v)
    v1, i1 = lsd.GPUTopK(x[0, 0].contiguous(), 7, key_type="float32")
    assert v1.shape == (7,) and torch.equal(v1, torch.topk(x[0, 0], 7).values) and i1.dtype == torch.int32
