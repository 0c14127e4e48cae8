"""GPU suite: lsdsort_kth_multi_device (GPUKthMulti, quantile_rows), bit-exact, positions included.

Contract: slot j of row r is item ranks[j] of the stable sort of the row in the requested order, with its position -- exactly what
lsdsort_kth_device stores for that rank.  Every case is checked against TWO oracles: numpy (the sortable-key map, then
np.argsort(kind="stable") per row) and the library's own GPUKth, one call per rank.  The fault word is read after every call
(check_fault=True).

Boundaries of the implementation (lsdradixsort_amd/csrc/kth_multi.hip): rows of up to 1024 keys take one wavefront (eight rows per
workgroup), up to 16384 one workgroup -- the row is loaded once and every slot selects on the same registers --, longer ones many
workgroups per row: one histogram of the top digit for all slots, then slots that share a prefix share counters (the leader rule),
one count pass, and a pick and a locate per slot.  Slots that stop at different levels, slots that share a prefix with different
needs and slots that pick different chunks are what the input kinds and rank sets below are made for."""
import ctypes

import numpy as np
import pytest
import torch

import _row_rounds as rr
import lsdradixsort_amd as lsd
from _device_arrays import bits, to_dev
from _guarded import assert_intact, assert_unchanged, guarded, guarded_workspace, without_sentinel
from _key_oracle import KEY_TYPES32 as KEY_TYPES, MULTI_RANK32, SPECIALS32 as SPECIALS, expected_np, inputs32 as inputs

pytestmark = pytest.mark.gpu


def rank_sets(cols):
    """one rank | the adjacent pair around the median | quartiles | eight, unsorted, with a repeat -- each clipped to the row"""
    sets = [[cols // 2], [(cols - 1) // 2, cols // 2], [cols // 4, cols // 2, 3 * cols // 4],
            [cols - 1, 0, cols // 2, cols // 2, 1, cols // 4, 3 * cols // 4, cols - 2]]
    return [[min(max(r, 0), cols - 1) for r in ranks] for ranks in sets]


def check_sets(dk, keys, key_type, what, sets=None, orders=(False, True)):
    """every rank set, both orders: against numpy and against GPUKth rank by rank, values and positions bit for bit"""
    rows, cols = keys.shape
    sets = rank_sets(cols) if sets is None else sets
    for largest in orders:
        ek, ei = expected_np(keys, key_type, largest)
        single = {rank: lsd.GPUKth(dk, rank, key_type=key_type, largest=largest, check_fault=True)
                  for rank in sorted({r for ranks in sets for r in ranks})}
        for ranks in sets:
            values, indices = lsd.GPUKthMulti(dk, ranks, key_type=key_type, largest=largest, check_fault=True)
            tag = f"{what} {rows}x{cols} {key_type} largest={largest} ranks={ranks}"
            assert values.shape == (rows, len(ranks)) and indices.shape == (rows, len(ranks)) and indices.dtype == torch.int32, tag
            assert values.dtype == dk.dtype, tag
            gv, gi = bits(values), bits(indices)
            assert np.array_equal(gv, ek[:, ranks]), f"{tag}: values differ from numpy: {gv[:2]} want {ek[:2, ranks]}"
            assert np.array_equal(gi, ei[:, ranks]), f"{tag}: positions differ from numpy: {gi[:2]} want {ei[:2, ranks]}"
            for j, rank in enumerate(ranks):
                assert np.array_equal(gv[:, j], bits(single[rank][0])), f"{tag}: values of slot {j} differ from GPUKth"
                assert np.array_equal(gi[:, j], bits(single[rank][1])), f"{tag}: positions of slot {j} differ from GPUKth"
            if "all equal" in what:
                assert (gi == np.array(ranks, dtype=np.uint32)[None, :]).all(), f"{tag}: the position must equal the rank"
    assert np.array_equal(bits(dk), keys), f"{what}: input changed"


def check_shape(rows, cols, key_type):
    for name, keys in inputs(rows, cols, key_type, seed=1000 * rows + cols, families=MULTI_RANK32).items():
        check_sets(to_dev(keys, key_type), keys, key_type, name)


WAVE = [(1, 1), (9, 7), (17, 65), (9, 1000), (3, 1024)]
GROUP = [(3, 1025), (3, 4097), (2, 16384)]
LONG = [(3, 16385), (3, 70001)]


@pytest.mark.parametrize("key_type", list(KEY_TYPES))
@pytest.mark.parametrize("shape", WAVE, ids=lambda s: f"{s[0]}x{s[1]}")
def test_wave_tier(shape, key_type):
    check_shape(*shape, key_type)


@pytest.mark.parametrize("key_type", list(KEY_TYPES))
@pytest.mark.parametrize("shape", GROUP, ids=lambda s: f"{s[0]}x{s[1]}")
def test_workgroup_tier(shape, key_type):
    check_shape(*shape, key_type)


@pytest.mark.parametrize("key_type", list(KEY_TYPES))
@pytest.mark.parametrize("shape", LONG, ids=lambda s: f"{s[0]}x{s[1]}")
def test_long_tier(shape, key_type):
    check_shape(*shape, key_type)


def test_one_long_row_of_many_chunks():
    """[1 x (2^20 + 13)]: 65 chunks, so the slots pick different chunks and the remainder of each `need` matters"""
    check_shape(1, (1 << 20) + 13, "float32")


TIER_SHAPES = [(9, 1000), (3, 4097), (3, 70001)]   # one per tier, all with odd or unaligned rows


@pytest.mark.parametrize("shape", TIER_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_rank_values_only_and_one_row_input(shape):
    rows, cols = shape
    keys = inputs(rows, cols, "int32", seed=cols, families=MULTI_RANK32)["four values"]
    dk = to_dev(keys, "int32")
    ek, ei = expected_np(keys, "int32", False)
    for rank in (0, cols // 2, cols - 1):   # num_ranks = 1 is GPUKth
        v1, i1 = lsd.GPUKthMulti(dk, [rank], key_type="int32", check_fault=True)
        kv, ki = lsd.GPUKth(dk, rank, key_type="int32", check_fault=True)
        assert v1.shape == (rows, 1) and torch.equal(v1[:, 0], kv) and torch.equal(i1[:, 0], ki), rank
    ranks = rank_sets(cols)[2]
    values, indices = lsd.GPUKthMulti(dk, ranks, key_type="int32", return_indices=False, check_fault=True)
    assert indices is None and np.array_equal(bits(values), ek[:, ranks])
    v1, i1 = lsd.GPUKthMulti(dk[1], ranks, key_type="int32", check_fault=True)      # 1-D input: the whole-array case
    assert v1.shape == (3,) and i1.shape == (3,)
    assert np.array_equal(bits(v1), ek[1, ranks]) and np.array_equal(bits(i1), ei[1, ranks])


@pytest.mark.parametrize("offset", [1, 2, 3])
@pytest.mark.parametrize("shape", TIER_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_views_off_the_16_byte_line(shape, offset):
    rows, cols = shape
    for name, keys in inputs(rows, cols, "float32", seed=offset + cols, families=MULTI_RANK32).items():
        if name in ("uniform bits", "four values", "outliers"):
            check_sets(to_dev(keys, "float32", offset), keys, "float32", f"{name} offset {offset}", sets=rank_sets(cols)[2:])


def raw_call(keys, ranks, key_type, largest, with_idx, skip_bytes, short_by=0):
    """the C entry with every array inside guard zones and a workspace of exactly the reported figure"""
    rows, cols = keys.shape
    m = len(ranks)
    L = lsd.lib()
    kw, kv = guarded(keys, skip_bytes)
    ow, ov = guarded(np.zeros(rows * m, dtype=np.uint32))
    iw, iv = guarded(np.zeros(rows * m, dtype=np.uint32))
    need = L.lsdsort_kth_multi_workspace_bytes(rows, cols, m)
    assert need > 0 and need % 256 == 0
    ww, wv = guarded_workspace(need)
    torch.cuda.synchronize()
    st = L.lsdsort_kth_multi_device(kv.data_ptr(), rows, cols, (ctypes.c_size_t * m)(*ranks), m, KEY_TYPES[key_type], int(largest),
                                    ov.data_ptr(), iv.data_ptr() if with_idx else None, wv.data_ptr(), need - short_by,
                                    int(torch.cuda.current_stream().cuda_stream))
    return st, (kw, kv), (ow, ov), (iw, iv), (ww, wv)


@pytest.mark.parametrize("skip_bytes", [0, 4, 12])
@pytest.mark.parametrize("shape", TIER_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_guard_bands_exact_workspace_and_null_indices(shape, skip_bytes):
    rows, cols = shape
    keys = without_sentinel(inputs(rows, cols, "float32", seed=cols + skip_bytes, families=MULTI_RANK32)["float specials"])
    ranks = [3 * cols // 4, cols // 4, cols // 2]
    ek, ei = expected_np(keys, "float32", True)
    st, *_ = raw_call(keys, ranks, "float32", True, True, skip_bytes, short_by=1)
    assert st == lsd.errors.LSDSORT_ERR_WORKSPACE, "one byte less than the figure is refused"
    for with_idx in (True, False):
        st, (kw, kv), (ow, ov), (iw, iv), (ww, wv) = raw_call(keys, ranks, "float32", True, with_idx, skip_bytes)
        assert st == 0, st
        assert lsd.lib().lsdsort_check_device(wv.data_ptr(), None) == 0
        assert np.array_equal(bits(ov).reshape(rows, 3), ek[:, ranks]), f"values (indices={with_idx})"
        if with_idx:
            assert np.array_equal(bits(iv).reshape(rows, 3), ei[:, ranks]), "positions"
        else:
            assert (bits(iv) == 0).all(), "no index buffer was given: nothing may be written"
        assert_intact(keys=kw, values=ow, indices=iw, workspace=ww)
        assert_unchanged(kv, keys)


@pytest.mark.parametrize("shape", TIER_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_same_result_without_the_returning_add_rank_form(shape):
    rows, cols = shape
    keys = inputs(rows, cols, "int32", seed=cols + 1, families=MULTI_RANK32)["outliers"]
    dk = to_dev(keys, "int32")
    lsd.set_rank_method(0)
    try:
        for largest in (False, True):
            ek, ei = expected_np(keys, "int32", largest)
            for ranks in rank_sets(cols):
                values, indices = lsd.GPUKthMulti(dk, ranks, key_type="int32", largest=largest, check_fault=True)
                assert np.array_equal(bits(values), ek[:, ranks]) and np.array_equal(bits(indices), ei[:, ranks]), (largest, ranks)
    finally:
        lsd.set_rank_method(-1)


@pytest.mark.parametrize("shape", TIER_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_two_calls_on_one_workspace_agree(shape):
    rows, cols = shape
    keys = inputs(rows, cols, "uint32", seed=cols + 2, families=MULTI_RANK32)["four values"]
    dk = to_dev(keys, "uint32")
    ranks = rank_sets(cols)[3]
    ws = torch.empty(lsd.kth_multi_workspace_bytes(rows, cols, len(ranks)), dtype=torch.uint8, device="cuda")
    a = lsd.GPUKthMulti(dk, ranks, largest=True, workspace=ws, check_fault=True)
    b = lsd.GPUKthMulti(dk, ranks, largest=True, workspace=ws, check_fault=True)    # the same workspace, used again
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    ek, ei = expected_np(keys, "uint32", True)
    assert np.array_equal(bits(b[0]), ek[:, ranks]) and np.array_equal(bits(b[1]), ei[:, ranks])
    c = lsd.GPUKthMulti(dk, ranks[:3], largest=False, workspace=ws, check_fault=True)   # ... by a call with fewer slots
    ek, ei = expected_np(keys, "uint32", False)
    assert np.array_equal(bits(c[0]), ek[:, ranks[:3]]) and np.array_equal(bits(c[1]), ei[:, ranks[:3]])


@pytest.mark.parametrize("shape", TIER_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_graph_replay_on_changed_input(shape):
    rows, cols = shape
    ranks = [3 * cols // 4, cols // 4, cols // 2]
    c_ranks = (ctypes.c_size_t * 3)(*ranks)
    L = lsd.lib()
    assert L.lsdsort_prepare_device() == 0
    dk = torch.zeros((rows, cols), dtype=torch.int32, device="cuda")
    out_k = torch.zeros((rows, 3), dtype=torch.int32, device="cuda")
    out_i = torch.zeros((rows, 3), dtype=torch.int32, device="cuda")
    ws = torch.empty(L.lsdsort_kth_multi_workspace_bytes(rows, cols, 3), dtype=torch.uint8, device="cuda")

    def call():
        st = L.lsdsort_kth_multi_device(dk.data_ptr(), rows, cols, c_ranks, 3, KEY_TYPES["int32"], 1, out_k.data_ptr(), out_i.data_ptr(),
                                        ws.data_ptr(), ws.numel(), int(torch.cuda.current_stream().cuda_stream))
        assert st == 0, st

    kinds = inputs(rows, cols, "int32", seed=cols + 3, families=MULTI_RANK32)
    dk.copy_(torch.from_numpy(kinds["uniform bits"].view(np.int32)))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()   # warm-up: device set-up stays out of the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for name in ("four values", "outliers"):   # two replays, each on changed input
        keys = kinds[name]
        dk.copy_(torch.from_numpy(keys.view(np.int32)))
        out_k.zero_()
        out_i.zero_()
        g.replay()
        torch.cuda.synchronize()
        fault = int(ws[:4].view(torch.int32).item())
        assert fault == 0, f"replay on {name}: fault word {fault:#x}"
        ek, ei = expected_np(keys, "int32", True)
        assert np.array_equal(bits(out_k), ek[:, ranks]), f"replay on {name}: values"
        assert np.array_equal(bits(out_i), ei[:, ranks]), f"replay on {name}: positions"
    assert L.lsdsort_check_device(ws.data_ptr(), None) == 0


@pytest.mark.parametrize("name", ["WAVE32", "GROUP"])
def test_second_round_of_the_row_loops(name):
    """more rows than one round of the capped grid covers: a wave or workgroup takes a second row, whose kind differs from its first"""
    rows, cols = rr.SHAPES[name]
    keys = rr.mixed_rows(rows, cols, rr.stride_of(name, "kth"), 32, SPECIALS, seed=cols)
    dk = to_dev(keys, "float32")
    ranks = [3 * cols // 4, cols // 4, cols // 2]
    ek, ei = expected_np(keys, "float32", False)
    values, indices = lsd.GPUKthMulti(dk, ranks, key_type="float32", check_fault=True)
    gv, gi = bits(values), bits(indices)
    bad = np.flatnonzero((gv != ek[:, ranks]).any(axis=1) | (gi != ei[:, ranks]).any(axis=1))
    stride = rr.stride_of(name, "kth")
    assert bad.size == 0, f"{name}: {bad.size} rows differ, first row {bad[0]} (round {bad[0] // stride}, row {bad[0] % stride} of it)"


QS = [0.37, [0.0, 0.5, 1.0], [0.999, 0.01, 0.5, 0.05, 0.75, 0.33333334]]   # six q: twelve ranks for `linear`, more than one call


@pytest.mark.parametrize("mode", ["linear", "lower", "higher", "midpoint", "nearest"])
@pytest.mark.parametrize("shape", [(5, 1000), (3, 4097), (3, 70001), (2, 3, 1001)], ids=lambda s: "x".join(map(str, s)))
def test_quantile_rows_is_torch_quantile(shape, mode):
    """NaN-free float32 without -0.0, where torch's order is the library's: both sides run the same torch ops on the same order
    statistics, so the results are equal, not close"""
    rng = np.random.default_rng(shape[-1])
    f = rng.standard_normal(shape).astype(np.float32)
    f[f == 0] = 1.0
    f[..., ::97] = np.float32(3.5)      # ties
    f[..., 2::83] = np.float32(1e-42)   # denormal
    x = torch.from_numpy(f).cuda()
    for q in QS:
        got = lsd.quantile_rows(x, q, interpolation=mode)
        want = torch.quantile(x, torch.tensor(q, device="cuda"), dim=-1, interpolation=mode)
        assert got.shape == want.shape and got.dtype == torch.float32, (q, got.shape, want.shape)
        assert torch.equal(got, want), f"{mode} q={q}: {(got != want).sum().item()} of {want.numel()} values differ"
    got = lsd.quantile_rows(x, torch.tensor([0.25, 0.75], device="cuda"), interpolation=mode)   # q as a device tensor
    assert torch.equal(got, torch.quantile(x, torch.tensor([0.25, 0.75], device="cuda"), dim=-1, interpolation=mode))
    if len(shape) == 2:
        wide = torch.from_numpy(np.repeat(f, 2, axis=1)).cuda()[:, ::2]   # one non-contiguous input: every other column
        assert not wide.is_contiguous() and torch.equal(wide, x)
        assert torch.equal(lsd.quantile_rows(wide, QS[1], interpolation=mode), torch.quantile(x, torch.tensor(QS[1], device="cuda"), dim=-1,
                                                                                              interpolation=mode))
