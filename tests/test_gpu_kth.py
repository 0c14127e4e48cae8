"""GPU suite: lsdsort_kth_device (GPUKth, kthvalue_rows, median_rows), bit-exact, positions included.

Contract: row r's result is item `rank` of the stable sort of the row in the requested order, with its position.  Every case is
checked against TWO oracles: numpy (the sortable-key map, then np.argsort(kind="stable") per row) and the library's own
GPUTopK(x, rank + 1, ..)[:, -1].  The fault word is read after every call (check_fault=True).

Boundaries of the implementation (lsdradixsort_amd/csrc/kth.hip): rows of up to 1024 keys take one wavefront (eight rows per
workgroup), up to 16384 one workgroup, longer ones many workgroups per row (chunks of 16384 keys or more); every row is read from
its own first 16-byte line on, so odd row lengths and offset views move the head / body / tail split."""
import numpy as np
import pytest
import torch

import lsdradixsort_amd as lsd
from _device_arrays import bits, to_dev
from _guarded import assert_intact, assert_unchanged, guarded, guarded_workspace, without_sentinel
from _key_oracle import KEY_TYPES32 as KEY_TYPES, expected_np, inputs32 as inputs

pytestmark = pytest.mark.gpu


def ranks_of(cols):
    return sorted({r for r in (0, 1, cols // 2, cols - 2, cols - 1) if 0 <= r < cols})


def check_ranks(dk, keys, key_type, what, ranks=None):
    """every rank, both orders: against numpy and against GPUTopK's last column, values and positions bit for bit"""
    rows, cols = keys.shape
    for largest in (False, True):
        ek, ei = expected_np(keys, key_type, largest)
        for rank in ranks_of(cols) if ranks is None else ranks:
            values, indices = lsd.GPUKth(dk, rank, key_type=key_type, largest=largest, check_fault=True)
            tag = f"{what} {rows}x{cols} {key_type} largest={largest} rank={rank}"
            assert values.shape == (rows,) and indices.shape == (rows,) and indices.dtype == torch.int32, tag
            gv, gi = bits(values), bits(indices)
            assert np.array_equal(gv, ek[:, rank]), f"{tag}: values differ from numpy: {gv[:4]} want {ek[:4, rank]}"
            assert np.array_equal(gi, ei[:, rank]), f"{tag}: positions differ from numpy: {gi[:4]} want {ei[:4, rank]}"
            tv, ti = lsd.GPUTopK(dk, rank + 1, key_type=key_type, largest=largest, check_fault=True)
            assert np.array_equal(gv, bits(tv[:, -1])), f"{tag}: values differ from GPUTopK"
            assert np.array_equal(gi, bits(ti[:, -1])), f"{tag}: positions differ from GPUTopK"
        if "all equal" in what:
            for rank in ranks_of(cols):
                _, indices = lsd.GPUKth(dk, rank, key_type=key_type, largest=largest, check_fault=True)
                assert (bits(indices) == rank).all(), f"{what} largest={largest}: the position must equal the rank {rank}"
    assert np.array_equal(bits(dk), keys), f"{what}: input changed"


def check_shape(rows, cols, key_type):
    for name, keys in inputs(rows, cols, key_type, seed=1000 * rows + cols).items():
        check_ranks(to_dev(keys, key_type), keys, key_type, name)


WAVE = [(rows, cols) for cols in (1, 2, 63, 64, 65, 255, 1000, 1024) for rows in (1, 9, 17)]
GROUP = [(3, 1025), (3, 4097), (3, 16384)]
LONG = [(3, 16385), (3, 32773), (3, 70001)]


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


@pytest.mark.parametrize("key_type", list(KEY_TYPES))
def test_one_long_row_of_many_chunks(key_type):
    """[1 x (2^20 + 13)]: 65 chunks, so the pick of the chunk and the remainder of `need` matter"""
    check_shape(1, (1 << 20) + 13, key_type)


TIER_SHAPES = [(9, 1000), (3, 4097), (3, 70001)]   # one per tier, all with odd or unaligned rows


@pytest.mark.parametrize("offset", [1, 2, 3])
@pytest.mark.parametrize("shape", TIER_SHAPES + [(2, 1024), (2, 16384), (2, 32768)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_views_off_the_16_byte_line(shape, offset):
    rows, cols = shape
    for name, keys in inputs(rows, cols, "float32", seed=offset + cols).items():
        if name in ("uniform bits", "four values", "float specials"):
            check_ranks(to_dev(keys, "float32", offset), keys, "float32", f"{name} offset {offset}")


@pytest.mark.parametrize("shape", [(5, 1000), (3, 4097), (3, 70001), (2, 1 << 18)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_values_against_torch_kthvalue_and_median(shape):
    """NaN-free float32 (no -0.0 either: torch calls the zeros equal) and int32, where torch's order is the library's; torch
    leaves the index among ties unspecified, so the index is checked by what it points at"""
    rows, cols = shape
    rng = np.random.default_rng(cols)
    f = rng.standard_normal((2, rows, cols)).astype(np.float32)
    f[f == 0] = 1.0
    f[..., ::97] = np.float32(np.inf)
    f[..., 1::89] = -np.float32(np.inf)
    f[..., 2::83] = np.float32(1e-42)   # denormal
    i = rng.integers(-1 << 31, 1 << 31, (2, rows, cols), dtype=np.int64).astype(np.int32)
    i[..., ::5] = 7
    for host in (f, i):
        x = torch.from_numpy(host).cuda()
        for k in sorted({1, 2, cols // 2, cols - 1, cols}):
            v, idx = lsd.kthvalue_rows(x, k)
            tv = torch.kthvalue(torch.from_numpy(host), k, dim=-1).values
            assert v.shape == tv.shape == (2, rows) and idx.dtype == torch.int64
            assert torch.equal(v.cpu(), tv), f"{host.dtype} k={k}: values differ from torch.kthvalue"
            assert torch.equal(torch.gather(x, -1, idx.unsqueeze(-1)).squeeze(-1), v), f"{host.dtype} k={k}: index"
        v, idx = lsd.median_rows(x)
        tv = torch.median(torch.from_numpy(host), dim=-1).values
        assert torch.equal(v.cpu(), tv), f"{host.dtype}: values differ from torch.median"
        assert torch.equal(torch.gather(x, -1, idx.unsqueeze(-1)).squeeze(-1), v)
        v1, i1 = lsd.kthvalue_rows(x[0, 0], 3)   # one row: 0-D results
        assert v1.shape == () and torch.equal(v1.cpu(), torch.kthvalue(torch.from_numpy(host[0, 0]), 3).values)
        assert x[0, 0, int(i1)] == v1


@pytest.mark.parametrize("shape", TIER_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_values_only_and_one_row_input(shape):
    rows, cols = shape
    keys = inputs(rows, cols, "int32", seed=cols)["four values"]
    dk = to_dev(keys, "int32")
    ek, ei = expected_np(keys, "int32", False)
    for rank in ranks_of(cols):
        values, indices = lsd.GPUKth(dk, rank, key_type="int32", return_indices=False, check_fault=True)
        assert indices is None and np.array_equal(bits(values), ek[:, rank])
        v1, i1 = lsd.GPUKth(dk[1], rank, key_type="int32", check_fault=True)      # 1-D input: the whole-array case
        assert v1.shape == () and i1.shape == ()
        assert int(bits(v1)) == ek[1, rank] and int(bits(i1)) == ei[1, rank]


def raw_call(keys, rank, key_type, largest, with_idx, skip_bytes, short_by=0):
    """the C entry with every array inside guard zones and a workspace of exactly the reported figure"""
    rows, cols = keys.shape
    L = lsd.lib()
    kw, kv = guarded(keys, skip_bytes)
    ow, ov = guarded(np.zeros(rows, dtype=np.uint32))
    iw, iv = guarded(np.zeros(rows, dtype=np.uint32))
    need = L.lsdsort_kth_workspace_bytes(rows, cols)
    assert need > 0 and need % 256 == 0
    ww, wv = guarded_workspace(need)
    torch.cuda.synchronize()
    st = L.lsdsort_kth_device(kv.data_ptr(), rows, cols, rank, KEY_TYPES[key_type], int(largest), ov.data_ptr(),
                              iv.data_ptr() if with_idx else None, wv.data_ptr(), need - short_by,
                              int(torch.cuda.current_stream().cuda_stream))
    return st, (kw, kv), (ow, ov), (iw, iv), (ww, wv)


@pytest.mark.parametrize("skip_bytes", [0, 4, 12])
@pytest.mark.parametrize("shape", TIER_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_guard_bands_exact_workspace_and_null_indices(shape, skip_bytes):
    rows, cols = shape
    keys = without_sentinel(inputs(rows, cols, "float32", seed=cols + skip_bytes)["float specials"])
    rank = cols // 2
    ek, ei = expected_np(keys, "float32", True)
    st, *_ = raw_call(keys, rank, "float32", True, True, skip_bytes, short_by=1)
    assert st == lsd.errors.LSDSORT_ERR_WORKSPACE, "one byte less than the figure is refused"
    for with_idx in (True, False):
        st, (kw, kv), (ow, ov), (iw, iv), (ww, wv) = raw_call(keys, rank, "float32", True, with_idx, skip_bytes)
        assert st == 0, st
        assert lsd.lib().lsdsort_check_device(wv.data_ptr(), None) == 0
        assert np.array_equal(bits(ov), ek[:, rank]), f"values (indices={with_idx})"
        if with_idx:
            assert np.array_equal(bits(iv), ei[:, rank]), "positions"
        else:
            assert (bits(iv) == 0).all(), "no index buffer was given: nothing may be written"
        assert_intact(keys=kw, values=ow, indices=iw, workspace=ww)
        assert_unchanged(kv, keys)


@pytest.mark.parametrize("shape", TIER_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_same_result_without_the_returning_add_rank_form(shape):
    rows, cols = shape
    keys = inputs(rows, cols, "int32", seed=cols + 1)["shared top 24 bits"]
    dk = to_dev(keys, "int32")
    lsd.set_rank_method(0)
    try:
        for largest in (False, True):
            ek, ei = expected_np(keys, "int32", largest)
            for rank in ranks_of(cols):
                values, indices = lsd.GPUKth(dk, rank, key_type="int32", largest=largest, check_fault=True)
                assert np.array_equal(bits(values), ek[:, rank]) and np.array_equal(bits(indices), ei[:, rank]), (largest, rank)
    finally:
        lsd.set_rank_method(-1)


@pytest.mark.parametrize("shape", TIER_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_two_eager_calls_agree(shape):
    rows, cols = shape
    keys = inputs(rows, cols, "uint32", seed=cols + 2)["four values"]
    dk = to_dev(keys, "uint32")
    ws = torch.empty(lsd.kth_workspace_bytes(rows, cols), dtype=torch.uint8, device="cuda")
    a = lsd.GPUKth(dk, cols // 2, largest=True, workspace=ws, check_fault=True)
    b = lsd.GPUKth(dk, cols // 2, largest=True, workspace=ws, check_fault=True)    # the same workspace, used again
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    ek, ei = expected_np(keys, "uint32", True)
    assert np.array_equal(bits(b[0]), ek[:, cols // 2]) and np.array_equal(bits(b[1]), ei[:, cols // 2])


@pytest.mark.parametrize("shape", TIER_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_graph_replay_on_changed_input(shape):
    rows, cols = shape
    rank = cols // 2
    L = lsd.lib()
    assert L.lsdsort_prepare_device() == 0
    dk = torch.zeros((rows, cols), dtype=torch.int32, device="cuda")
    out_k = torch.zeros(rows, dtype=torch.int32, device="cuda")
    out_i = torch.zeros(rows, dtype=torch.int32, device="cuda")
    ws = torch.empty(L.lsdsort_kth_workspace_bytes(rows, cols), dtype=torch.uint8, device="cuda")

    def call():
        st = L.lsdsort_kth_device(dk.data_ptr(), rows, cols, rank, KEY_TYPES["int32"], 1, out_k.data_ptr(), out_i.data_ptr(),
                                  ws.data_ptr(), ws.numel(), int(torch.cuda.current_stream().cuda_stream))
        assert st == 0, st

    kinds = inputs(rows, cols, "int32", seed=cols + 3)
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
    for name in ("four values", "shared top 24 bits"):   # two replays, each on changed input
        keys = kinds[name]
        dk.copy_(torch.from_numpy(keys.view(np.int32)))
        out_k.zero_()
        out_i.zero_()
        g.replay()
        torch.cuda.synchronize()
        fault = int(ws[:4].view(torch.int32).item())
        assert fault == 0, f"replay on {name}: fault word {fault:#x}"
        ek, ei = expected_np(keys, "int32", True)
        assert np.array_equal(bits(out_k), ek[:, rank]), f"replay on {name}: values"
        assert np.array_equal(bits(out_i), ei[:, rank]), f"replay on {name}: positions"
    assert L.lsdsort_check_device(ws.data_ptr(), None) == 0
