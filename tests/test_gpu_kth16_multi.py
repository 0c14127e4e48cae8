"""GPU suite: lsdsort_kth16_multi_device (GPUKth16Multi, quantile16_rows), bit-exact, positions included.

Contract: slot j of row r is item ranks[j] of the stable sort of the row in the requested order, with its position -- exactly what
lsdsort_kth16_device stores for that rank.  Every case is checked against TWO oracles: numpy (the 16-bit sortable map, then
np.argsort(kind="stable") per row) and the library's own GPUKth16, one call per rank.  The fault word is read after every call
(check_fault=True), and the input is checked to be unchanged.

Boundaries of the implementation (lsdradixsort_amd/csrc/kth16_multi.hip): rows of up to 1024 keys take one wavefront (eight rows per
workgroup), up to 16384 one workgroup -- the row is loaded once and every slot selects on the same registers --, longer ones many
workgroups per row: one 2048-bin histogram of the top 11 bits for all slots, then 32 counters per leader for the low 5 bits (slots
that share a prefix share counters), one count pass, and a pick and a locate per slot; without an index buffer a long row takes a
launch sequence of its own (both levels for every slot, then the prefix is the value).  Slots that stop at different levels, slots
that share a prefix with different needs and slots that pick different chunks are what the input kinds and rank sets are made for."""
import ctypes

import numpy as np
import pytest
import torch

import _row_rounds as rr
import lsdradixsort_amd as lsd
from _device_arrays import DTYPES, bits, to_dev
from _guarded import assert_intact, guarded, guarded_workspace
from _guarded16 import assert_intact16, bits_of, guarded16
from _key_oracle import (
    ALL_TYPES16 as ALL_TYPES, KEY_TYPES16 as KEY_TYPES, MULTI_RANK16, SPECIALS16 as SPECIALS, expected_np, inputs16 as inputs,
)

pytestmark = pytest.mark.gpu


def rank_sets(cols):
    """one rank | the adjacent pair around the median | quartiles | eight, unsorted, with a repeat -- each clipped to the row"""
    sets = [[cols // 2], [(cols - 1) // 2, cols // 2], [cols // 4, cols // 2, 3 * cols // 4],
            [cols - 1, 0, cols // 2, cols // 2, 1, cols // 4, 3 * cols // 4, cols - 2]]
    return [[min(max(r, 0), cols - 1) for r in ranks] for ranks in sets]


def check_sets(dk, keys, key_type, what, sets=None, orders=(False, True)):
    """every rank set, both orders: against numpy and against GPUKth16 rank by rank, values and positions bit for bit"""
    rows, cols = keys.shape
    sets = rank_sets(cols) if sets is None else sets
    for largest in orders:
        ek, ei = expected_np(keys, key_type, largest)
        single = {rank: lsd.GPUKth16(dk, rank, key_type=key_type, largest=largest, check_fault=True)
                  for rank in sorted({r for ranks in sets for r in ranks})}
        for ranks in sets:
            values, indices = lsd.GPUKth16Multi(dk, ranks, key_type=key_type, largest=largest, check_fault=True)
            tag = f"{what} {rows}x{cols} {key_type} largest={largest} ranks={ranks}"
            assert values.shape == (rows, len(ranks)) and indices.shape == (rows, len(ranks)) and indices.dtype == torch.int32, tag
            assert values.dtype == DTYPES[key_type], tag
            gv, gi = bits(values), bits(indices)
            assert np.array_equal(gv, ek[:, ranks]), f"{tag}: values differ from numpy: {gv[:2]} want {ek[:2, ranks]}"
            assert np.array_equal(gi, ei[:, ranks]), f"{tag}: positions differ from numpy: {gi[:2]} want {ei[:2, ranks]}"
            for j, rank in enumerate(ranks):
                assert np.array_equal(gv[:, j], bits(single[rank][0])), f"{tag}: values of slot {j} differ from GPUKth16"
                assert np.array_equal(gi[:, j], bits(single[rank][1])), f"{tag}: positions of slot {j} differ from GPUKth16"
            if "all equal" in what:
                assert (gi == np.array(ranks, dtype=np.uint32)[None, :]).all(), f"{tag}: the position must equal the rank"
    assert np.array_equal(bits(dk), keys), f"{what}: input changed"


def check_shape(rows, cols, key_type):
    for name, keys in inputs(rows, cols, key_type, seed=1000 * rows + cols, families=MULTI_RANK16).items():
        check_sets(to_dev(keys, key_type), keys, key_type, name)


WAVE = [(1, 1), (9, 7), (17, 65), (9, 1000), (3, 1024)]
GROUP = [(3, 1025), (3, 4099), (2, 16384)]
LONG = [(3, 16385), (3, 70001)]


@pytest.mark.parametrize("key_type", ALL_TYPES)
@pytest.mark.parametrize("shape", WAVE, ids=lambda s: f"{s[0]}x{s[1]}")
def test_wave_tier(shape, key_type):
    check_shape(*shape, key_type)


@pytest.mark.parametrize("key_type", ALL_TYPES)
@pytest.mark.parametrize("shape", GROUP, ids=lambda s: f"{s[0]}x{s[1]}")
def test_workgroup_tier(shape, key_type):
    check_shape(*shape, key_type)


@pytest.mark.parametrize("key_type", ALL_TYPES)
@pytest.mark.parametrize("shape", LONG, ids=lambda s: f"{s[0]}x{s[1]}")
def test_long_tier(shape, key_type):
    check_shape(*shape, key_type)


def test_one_long_row_of_many_chunks():
    """[1 x (2^20 + 13)]: 65 chunks, so the slots pick different chunks and the remainder of each `need` matters"""
    check_shape(1, (1 << 20) + 13, "bfloat16")


TIER_SHAPES = [(9, 1000), (3, 4099), (3, 70001)]   # one per tier, all with odd or unaligned rows


@pytest.mark.parametrize("key_type", ["int16", "float16"])
@pytest.mark.parametrize("shape", TIER_SHAPES + [(3, 16385)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_values_only_one_rank_and_one_row_input(shape, key_type):
    """without an index buffer: the same values (the long shapes take the launch sequence without a locate, where every slot runs
    both levels: `lone minimum` and `outliers` hold slots that would have stopped after the first); one rank is GPUKth16; 1-D input"""
    rows, cols = shape
    kinds = inputs(rows, cols, key_type, seed=cols, families=MULTI_RANK16)
    for name in ("four values", "shared top 11 bits", "lone minimum", "uniform bits", "outliers"):
        keys = kinds[name]
        dk = to_dev(keys, key_type, 3)
        for largest in (False, True):
            ek, ei = expected_np(keys, key_type, largest)
            for ranks in rank_sets(cols):
                with_v, with_i = lsd.GPUKth16Multi(dk, ranks, key_type=key_type, largest=largest, check_fault=True)
                values, indices = lsd.GPUKth16Multi(dk, ranks, key_type=key_type, largest=largest, return_indices=False, check_fault=True)
                assert indices is None and values.shape == (rows, len(ranks)) and values.dtype == DTYPES[key_type]
                assert np.array_equal(bits(values), ek[:, ranks]), (name, largest, ranks)
                assert np.array_equal(bits(values), bits(with_v)) and np.array_equal(bits(with_i), ei[:, ranks]), (name, largest, ranks)
        assert np.array_equal(bits(dk), keys)
    keys = kinds["four values"]
    dk = to_dev(keys, key_type)
    ek, ei = expected_np(keys, key_type, False)
    for rank in (0, cols // 2, cols - 1):   # num_ranks = 1 is GPUKth16
        v1, i1 = lsd.GPUKth16Multi(dk, [rank], key_type=key_type, check_fault=True)
        kv, ki = lsd.GPUKth16(dk, rank, key_type=key_type, check_fault=True)
        assert v1.shape == (rows, 1) and torch.equal(v1[:, 0].view(torch.int16), kv.view(torch.int16)) and torch.equal(i1[:, 0], ki), rank
        v0, i0 = lsd.GPUKth16Multi(dk, [rank], key_type=key_type, return_indices=False, check_fault=True)
        assert i0 is None and torch.equal(v0[:, 0].view(torch.int16), kv.view(torch.int16)), rank
    ranks = rank_sets(cols)[2]
    v1, i1 = lsd.GPUKth16Multi(dk[1], ranks, key_type=key_type, check_fault=True)      # 1-D input: the whole-array case
    assert v1.shape == (3,) and i1.shape == (3,)
    assert np.array_equal(bits(v1), ek[1, ranks]) and np.array_equal(bits(i1), ei[1, ranks])
    v0, i0 = lsd.GPUKth16Multi(dk[1], ranks, key_type=key_type, return_indices=False, check_fault=True)
    assert i0 is None and v0.shape == (3,) and np.array_equal(bits(v0), ek[1, ranks])


@pytest.mark.parametrize("offset", [1, 3, 7])
@pytest.mark.parametrize("shape", TIER_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_views_off_the_16_byte_line(shape, offset):
    rows, cols = shape
    for name, keys in inputs(rows, cols, "bfloat16", seed=offset + cols, families=MULTI_RANK16).items():
        if name in ("uniform bits", "four values", "outliers"):
            check_sets(to_dev(keys, "bfloat16", offset), keys, "bfloat16", f"{name} offset {offset}", sets=rank_sets(cols)[2:])


def raw_call(keys, ranks, key_type, largest, with_idx, skip_bytes, short_by=0):
    """the C entry with every array inside guard zones and a workspace of exactly the reported figure"""
    rows, cols = keys.shape
    m = len(ranks)
    L = lsd.lib()
    kw, kv = guarded16(keys, skip_bytes, DTYPES[key_type])
    ow, ov = guarded16(np.zeros(rows * m, dtype=np.uint16), skip_bytes)
    iw, iv = guarded(np.zeros(rows * m, dtype=np.uint32))
    need = L.lsdsort_kth16_multi_workspace_bytes(rows, cols, m)
    assert need > 0 and need % 256 == 0
    ww, wv = guarded_workspace(need)
    torch.cuda.synchronize()
    st = L.lsdsort_kth16_multi_device(kv.data_ptr(), rows, cols, (ctypes.c_size_t * m)(*ranks), m, KEY_TYPES[key_type], int(largest),
                                      ov.data_ptr(), iv.data_ptr() if with_idx else None, wv.data_ptr(), need - short_by,
                                      int(torch.cuda.current_stream().cuda_stream))
    return st, (kw, kv), (ow, ov), (iw, iv), (ww, wv)


@pytest.mark.parametrize("skip_bytes", [0, 2, 6, 14])
@pytest.mark.parametrize("shape", TIER_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_guard_bands_exact_workspace_and_null_indices(shape, skip_bytes):
    rows, cols = shape
    keys = inputs(rows, cols, "float16", seed=cols + skip_bytes, families=MULTI_RANK16)["float specials"]
    ranks = [3 * cols // 4, cols // 4, cols // 2]
    ek, ei = expected_np(keys, "float16", True)
    st, *_ = raw_call(keys, ranks, "float16", True, True, skip_bytes, short_by=1)
    assert st == lsd.errors.LSDSORT_ERR_WORKSPACE, "one byte less than the figure is refused"
    for with_idx in (True, False):
        st, (kw, kv), (ow, ov), (iw, iv), (ww, wv) = raw_call(keys, ranks, "float16", True, with_idx, skip_bytes)
        assert st == 0, st
        assert lsd.lib().lsdsort_check_device(wv.data_ptr(), None) == 0
        assert int(wv[:4].view(torch.int32).item()) == 0, "fault word"
        assert np.array_equal(bits_of(ov).reshape(rows, 3), ek[:, ranks]), f"values (indices={with_idx})"
        if with_idx:
            assert np.array_equal(bits(iv).reshape(rows, 3), ei[:, ranks]), "positions"
        else:
            assert (bits(iv) == 0).all(), "no index buffer was given: nothing may be written"
        assert_intact16(keys=kw, values=ow)
        assert_intact(indices=iw, workspace=ww)
        assert np.array_equal(bits_of(kv), keys.reshape(-1)), "a read-only input was changed"


@pytest.mark.parametrize("shape", TIER_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_same_result_without_the_returning_add_rank_form(shape):
    rows, cols = shape
    keys = inputs(rows, cols, "int16", seed=cols + 1, families=MULTI_RANK16)["outliers"]
    dk = to_dev(keys, "int16")
    lsd.set_rank_method(0)
    try:
        for largest in (False, True):
            ek, ei = expected_np(keys, "int16", largest)
            for ranks in rank_sets(cols):
                values, indices = lsd.GPUKth16Multi(dk, ranks, key_type="int16", largest=largest, check_fault=True)
                assert np.array_equal(bits(values), ek[:, ranks]) and np.array_equal(bits(indices), ei[:, ranks]), (largest, ranks)
                values, _ = lsd.GPUKth16Multi(dk, ranks, key_type="int16", largest=largest, return_indices=False, check_fault=True)
                assert np.array_equal(bits(values), ek[:, ranks]), (largest, ranks)
    finally:
        lsd.set_rank_method(-1)


@pytest.mark.parametrize("shape", TIER_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_two_calls_on_one_workspace_agree(shape):
    rows, cols = shape
    keys = inputs(rows, cols, "uint16", seed=cols + 2, families=MULTI_RANK16)["four values"]
    dk = to_dev(keys, "uint16")
    ranks = rank_sets(cols)[3]
    ws = torch.empty(lsd.kth16_multi_workspace_bytes(rows, cols, len(ranks)), dtype=torch.uint8, device="cuda")
    a = lsd.GPUKth16Multi(dk, ranks, key_type="uint16", largest=True, workspace=ws, check_fault=True)
    b = lsd.GPUKth16Multi(dk, ranks, key_type="uint16", largest=True, workspace=ws, check_fault=True)   # the same workspace, used again
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    ek, ei = expected_np(keys, "uint16", True)
    assert np.array_equal(bits(b[0]), ek[:, ranks]) and np.array_equal(bits(b[1]), ei[:, ranks])
    c = lsd.GPUKth16Multi(dk, ranks[:3], key_type="uint16", largest=False, workspace=ws, check_fault=True)   # ... with fewer slots
    ek, ei = expected_np(keys, "uint16", False)
    assert np.array_equal(bits(c[0]), ek[:, ranks[:3]]) and np.array_equal(bits(c[1]), ei[:, ranks[:3]])
    d = lsd.GPUKth16Multi(dk, ranks[:3], key_type="uint16", return_indices=False, workspace=ws, check_fault=True)   # ... values only
    assert d[1] is None and np.array_equal(bits(d[0]), ek[:, ranks[:3]])


@pytest.mark.parametrize("shape,with_idx", [(s, True) for s in TIER_SHAPES] + [(TIER_SHAPES[-1], False)],
                         ids=lambda v: str(v).replace(" ", ""))
def test_graph_replay_on_changed_input(shape, with_idx):
    rows, cols = shape
    ranks = [3 * cols // 4, cols // 4, cols // 2]
    c_ranks = (ctypes.c_size_t * 3)(*ranks)
    L = lsd.lib()
    assert L.lsdsort_prepare_device() == 0
    dk = torch.zeros((rows, cols), dtype=torch.int16, device="cuda")
    out_k = torch.zeros((rows, 3), dtype=torch.int16, device="cuda")
    out_i = torch.zeros((rows, 3), dtype=torch.int32, device="cuda")
    ws = torch.empty(L.lsdsort_kth16_multi_workspace_bytes(rows, cols, 3), dtype=torch.uint8, device="cuda")

    def call():
        st = L.lsdsort_kth16_multi_device(dk.data_ptr(), rows, cols, c_ranks, 3, KEY_TYPES["int16"], 1, out_k.data_ptr(),
                                          out_i.data_ptr() if with_idx else None, ws.data_ptr(), ws.numel(),
                                          int(torch.cuda.current_stream().cuda_stream))
        assert st == 0, st

    kinds = inputs(rows, cols, "int16", seed=cols + 3, families=MULTI_RANK16)
    dk.copy_(torch.from_numpy(kinds["uniform bits"].view(np.int16)))
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
        dk.copy_(torch.from_numpy(keys.view(np.int16)))
        out_k.zero_()
        out_i.zero_()
        g.replay()
        torch.cuda.synchronize()
        fault = int(ws[:4].view(torch.int32).item())
        assert fault == 0, f"replay on {name}: fault word {fault:#x}"
        ek, ei = expected_np(keys, "int16", True)
        assert np.array_equal(bits(out_k), ek[:, ranks]), f"replay on {name}: values"
        if with_idx:
            assert np.array_equal(bits(out_i), ei[:, ranks]), f"replay on {name}: positions"
        else:
            assert (bits(out_i) == 0).all(), "no index buffer was given: nothing may be written"
    assert L.lsdsort_check_device(ws.data_ptr(), None) == 0


@pytest.mark.parametrize("name", ["WAVE16", "GROUP"])
def test_second_round_of_the_row_loops(name):
    """more rows than one round of the capped grid covers: a wave or workgroup takes a second row, whose kind differs from its first"""
    rows, cols = rr.SHAPES[name]
    stride = rr.stride_of(name, "kth16")
    keys = rr.mixed_rows(rows, cols, stride, 16, SPECIALS["bfloat16"], seed=cols)
    dk = to_dev(keys, "bfloat16")
    ranks = [3 * cols // 4, cols // 4, cols // 2]
    ek, ei = expected_np(keys, "bfloat16", False)
    values, indices = lsd.GPUKth16Multi(dk, ranks, key_type="bfloat16", check_fault=True)
    gv, gi = bits(values), bits(indices)
    bad = np.flatnonzero((gv != ek[:, ranks]).any(axis=1) | (gi != ei[:, ranks]).any(axis=1))
    assert bad.size == 0, f"{name}: {bad.size} rows differ, first row {bad[0]} (round {bad[0] // stride}, row {bad[0] % stride} of it)"


QS = [0.37, [0.0, 0.5, 1.0], [0.999, 0.01, 0.5, 0.05, 0.75, 0.33333334]]   # six q: twelve ranks for `linear`, more than one call


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=lambda d: str(d).replace("torch.", ""))
@pytest.mark.parametrize("mode", ["linear", "lower", "higher", "midpoint", "nearest"])
@pytest.mark.parametrize("shape", [(5, 1000), (3, 4097), (3, 70001), (2, 3, 1001)], ids=lambda s: "x".join(map(str, s)))
def test_quantile16_rows_is_torch_quantile_of_the_widened_rows(shape, mode, dtype):
    """NaN-free float16 / bfloat16 without zeros, where torch's order is the library's: both sides run the same torch ops on the
    same order statistics (the 16-bit values widened exactly), so the results are equal, not close.  torch.quantile itself refuses
    the 16-bit types: the reference is torch.quantile(x.float(), ...)."""
    rng = np.random.default_rng(shape[-1])
    x = torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(dtype)
    x[x == 0] = 1.0
    x[..., ::97] = 3.5                                                         # ties
    x[..., 2::83] = torch.tensor(3, dtype=torch.int16).view(dtype).item()      # a denormal
    assert not torch.isnan(x).any() and not (x == 0).any()
    x = x.cuda()
    wide = x.float()
    for q in QS:
        got = lsd.quantile16_rows(x, q, interpolation=mode)
        want = torch.quantile(wide, torch.tensor(q, device="cuda"), dim=-1, interpolation=mode)
        assert got.shape == want.shape and got.dtype == torch.float32, (q, got.shape, want.shape)
        assert torch.equal(got, want), f"{mode} q={q}: {(got != want).sum().item()} of {want.numel()} values differ"
    qd = torch.tensor([0.25, 0.75], device="cuda")                             # q as a device tensor
    assert torch.equal(lsd.quantile16_rows(x, qd, interpolation=mode), torch.quantile(wide, qd, dim=-1, interpolation=mode))
    if len(shape) == 2:
        twice = x.repeat_interleave(2, dim=1)[:, ::2]                          # one non-contiguous input: every other column
        assert not twice.is_contiguous() and torch.equal(twice, x)
        assert torch.equal(lsd.quantile16_rows(twice, QS[1], interpolation=mode),
                           torch.quantile(wide, torch.tensor(QS[1], device="cuda"), dim=-1, interpolation=mode))
