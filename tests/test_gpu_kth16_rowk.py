"""GPU suite: the per-row-k entries for 16-bit keys -- lsdsort_kth16_perrow_device (GPUKth16PerRow) and
lsdsort_topk16_filter_device (GPUTopK16Filter, topk16_filter_rows) -- bit-exact.

Per-row rank: row r's result is item d_ranks[r] of the stable sort of the row in the requested order, with its position; checked
against numpy (tests/_rowk16.py) and against GPUKth16 called once per distinct rank.  Filter: row r keeps the keys at least as good as
its k_r-th best and gets the fill word elsewhere, checked against np.where(sortable(x) <= sortable(T_r), x, fill); the fill word
0x7E7E occurs nowhere in the inputs.  The fault word is read after every call (check_fault=True) unless a test wants it set.

Boundaries of the implementation (lsdradixsort_amd/csrc/kth16_rowk.hip): rows of up to 1024 keys take one wavefront (eight rows per
workgroup, so the ranks and k's cycle from row to row), up to 16384 one workgroup, longer ones many workgroups per row; every row is
read from its own first 16-byte line on; the filter stores 16-byte groups where source and destination rows share their 16-byte
phase and key by key otherwise; a rank outside its row raises bit 4096 and stores nothing."""
import numpy as np
import pytest
import torch

import lsdradixsort_amd as lsd
import _rowk16 as rk
from _device_arrays import DTYPES, bits, captured, fault_word, stream_ptr, to_dev
from _guarded import assert_intact, guarded, guarded_workspace
from _guarded16 import assert_intact16, bits_of, guarded16
from _key_oracle import KEY_TYPES16 as KEY_TYPES

pytestmark = pytest.mark.gpu

FAULT_RANK = 4096


def dev_u32(values):
    """[n] uint32 -> the int32 CUDA tensor with the same bits"""
    return torch.from_numpy(np.ascontiguousarray(values, dtype=np.uint32).view(np.int32).copy()).cuda()


# ---- the two checks every shape goes through -------------------------------------------------------------------------------------
def check_perrow(dk, keys, key_type, what, against_single=True):
    """every candidate rank in some row, both orders, with and without indices"""
    rows, cols = keys.shape
    cand = rk.candidates_ranks(cols)
    at = np.arange(rows)
    for largest in (False, True):
        ek, ei = rk.expected_np(keys, key_type, largest)
        for shift in rk.shifts(cand, rows):
            ranks = rk.cycle(cand, rows, shift)
            d_ranks = dev_u32(ranks)
            tag = f"{what} {rows}x{cols} {key_type} largest={largest} ranks={ranks[:8]}"
            values, indices = lsd.GPUKth16PerRow(dk, d_ranks, key_type=key_type, largest=largest, check_fault=True)
            assert values.shape == (rows,) and indices.shape == (rows,), tag
            assert values.dtype == DTYPES[key_type] and indices.dtype == torch.int32, tag
            gv, gi = bits(values), bits(indices)
            assert np.array_equal(gv, ek[at, ranks]), f"{tag}: values differ from numpy: {gv[:4]} want {ek[at, ranks][:4]}"
            assert np.array_equal(gi, ei[at, ranks]), f"{tag}: positions differ from numpy: {gi[:4]} want {ei[at, ranks][:4]}"
            only, none = lsd.GPUKth16PerRow(dk, d_ranks, key_type=key_type, largest=largest, return_indices=False, check_fault=True)
            assert none is None and np.array_equal(bits(only), gv), f"{tag}: values only"
            if against_single:
                for rank in sorted(set(ranks.tolist())):
                    sv, si = lsd.GPUKth16(dk, rank, key_type=key_type, largest=largest, check_fault=True)
                    mine = ranks == rank
                    assert np.array_equal(gv[mine], bits(sv)[mine]), f"{tag}: values differ from GPUKth16 at rank {rank}"
                    assert np.array_equal(gi[mine], bits(si)[mine]), f"{tag}: positions differ from GPUKth16 at rank {rank}"
            if "all equal" in what:
                assert np.array_equal(gi, ranks), f"{tag}: the position must equal the rank"
            assert np.array_equal(bits(d_ranks), ranks), f"{tag}: the ranks were changed"
    assert np.array_equal(bits(dk), keys), f"{what}: input changed"


def check_filter(dk, keys, key_type, what):
    """every candidate k in some row, both orders, out of place and in place"""
    rows, cols = keys.shape
    cand = rk.candidates_k(cols)
    for largest in (False, True):
        for shift in rk.shifts(cand, rows):
            k = rk.cycle(cand, rows, shift)
            d_k = dev_u32(k)
            tag = f"{what} {rows}x{cols} {key_type} largest={largest} k={k[:8]}"
            want = rk.filter_np(keys, k, key_type, largest)
            out = lsd.GPUTopK16Filter(dk, d_k, key_type=key_type, largest=largest, fill=rk.FILL, check_fault=True)
            assert out.shape == dk.shape and out.dtype == dk.dtype and out.data_ptr() != dk.data_ptr(), tag
            got = bits(out)
            bad = np.argwhere(got != want)
            assert bad.size == 0, f"{tag}: {bad.shape[0]} words differ, first at {bad[0]}: {got[tuple(bad[0])]:#x} want {want[tuple(bad[0])]:#x}"
            on = rk.filter_on(k, cols)
            kept = (got != rk.FILL).sum(axis=1)
            assert (kept[on] >= k[on]).all(), f"{tag}: a row keeps fewer than k keys"
            assert np.array_equal(got[~on], keys[~on]), f"{tag}: a row whose filter is off differs from the input"
            if "all equal" in what:
                assert np.array_equal(got, keys), f"{tag}: a row of equal keys is never filled"
            assert np.array_equal(bits(dk), keys), f"{tag}: input changed"
            own = dk.clone()
            same = lsd.GPUTopK16Filter(own, d_k, key_type=key_type, largest=largest, fill=rk.FILL, out=own, check_fault=True)
            assert same is own and np.array_equal(bits(own), want), f"{tag}: in place differs"
            assert np.array_equal(bits(d_k), k), f"{tag}: the k's were changed"


def check_shape(rows, cols, key_type):
    for name, keys in rk.inputs(rows, cols, key_type, seed=1000 * rows + cols).items():
        dk = to_dev(keys, key_type)
        check_perrow(dk, keys, key_type, name)
        check_filter(dk, keys, key_type, name)


WAVE = [(rows, cols) for cols in (1, 2, 7, 8, 9, 63, 64, 65, 255, 1000, 1023, 1024) for rows in (1, 9, 17)]
GROUP = [(3, 1025), (3, 4099), (3, 16384)]
LONG = [(3, 16385), (3, 32773), (3, 70001)]
TIER_SHAPES = [(17, 1000), (3, 4099), (3, 70001)]   # one per tier, all with odd or unaligned rows


@pytest.mark.parametrize("key_type", rk.ALL_TYPES)
@pytest.mark.parametrize("shape", WAVE, ids=lambda s: f"{s[0]}x{s[1]}")
def test_wave_tier(shape, key_type):
    check_shape(*shape, key_type)


@pytest.mark.parametrize("key_type", rk.ALL_TYPES)
@pytest.mark.parametrize("shape", GROUP, ids=lambda s: f"{s[0]}x{s[1]}")
def test_workgroup_tier(shape, key_type):
    check_shape(*shape, key_type)


@pytest.mark.parametrize("key_type", rk.ALL_TYPES)
@pytest.mark.parametrize("shape", LONG, ids=lambda s: f"{s[0]}x{s[1]}")
def test_long_tier(shape, key_type):
    check_shape(*shape, key_type)


@pytest.mark.parametrize("key_type", ["bfloat16", "uint16"])
def test_one_long_row_of_many_chunks(key_type):
    """[1 x (2^20 + 13)]: 65 chunks -- the pick of the chunk, and an apply kernel whose chunks are not the row"""
    rows, cols = 1, (1 << 20) + 13
    for name, keys in rk.inputs(rows, cols, key_type, seed=cols).items():
        if name in ("uniform bits", "four values", "shared top 11 bits", "float specials"):
            dk = to_dev(keys, key_type, 3)
            check_perrow(dk, keys, key_type, name, against_single=name == "four values")
            check_filter(dk, keys, key_type, name)


# ---- the raw entries inside guard zones ------------------------------------------------------------------------------------------
def raw_perrow(keys, ranks, key_type, largest, with_idx, skip_bytes, out_skip=None, short_by=0, sentinel=0):
    """the C entry with every array inside guard zones and a workspace of exactly the reported figure"""
    rows, cols = keys.shape
    L = lsd.lib()
    kw, kv = guarded16(keys, skip_bytes, DTYPES[key_type])
    ow, ov = guarded16(np.full(rows, sentinel & 0xFFFF, dtype=np.uint16), skip_bytes if out_skip is None else out_skip)
    iw, iv = guarded(np.full(rows, sentinel, dtype=np.uint32))
    rw, rv = guarded(np.ascontiguousarray(ranks, dtype=np.uint32), 4)
    need = L.lsdsort_kth16_perrow_workspace_bytes(rows, cols)
    assert need > 0 and need % 256 == 0
    ww, wv = guarded_workspace(need)
    torch.cuda.synchronize()
    st = L.lsdsort_kth16_perrow_device(kv.data_ptr(), rows, cols, rv.data_ptr(), KEY_TYPES[key_type], int(largest), ov.data_ptr(),
                                       iv.data_ptr() if with_idx else None, wv.data_ptr(), need - short_by, stream_ptr())
    return st, (kw, kv), (ow, ov), (iw, iv), (rw, rv), (ww, wv)


def raw_filter(keys, k, key_type, largest, src_skip, dst_skip, in_place=False, short_by=0):
    rows, cols = keys.shape
    L = lsd.lib()
    kw, kv = guarded16(keys, src_skip, DTYPES[key_type])
    ow, ov = (kw, kv) if in_place else guarded16(np.full(rows * cols, 0x5A5A, dtype=np.uint16), dst_skip)
    rw, rv = guarded(np.ascontiguousarray(k, dtype=np.uint32), 8)
    need = L.lsdsort_topk16_filter_workspace_bytes(rows, cols)
    assert need > 0 and need % 256 == 0
    ww, wv = guarded_workspace(need)
    torch.cuda.synchronize()
    st = L.lsdsort_topk16_filter_device(kv.data_ptr(), rows, cols, rv.data_ptr(), KEY_TYPES[key_type], int(largest), rk.FILL,
                                        ov.data_ptr(), wv.data_ptr(), need - short_by, stream_ptr())
    return st, (kw, kv), (ow, ov), (rw, rv), (ww, wv)


@pytest.mark.parametrize("shape", [(9, 999), (3, 4099), (3, 70001)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_source_and_destination_at_different_offsets(shape):
    """odd cols; the source at every even byte offset 0 .. 14 against the destination at every one: where the two differ the rows do
    not share their 16-byte phase, and from row to row the phase moves (cols is odd)"""
    rows, cols = shape
    keys = rk.inputs(rows, cols, "bfloat16", seed=cols)["float specials"]
    k = rk.cycle(rk.candidates_k(cols), rows, 3)     # cols // 2, cols - 1, cols, ..
    want = rk.filter_np(keys, k, "bfloat16", True)
    ranks = rk.cycle(rk.candidates_ranks(cols), rows, 2)
    ek, ei = rk.expected_np(keys, "bfloat16", True)
    at = np.arange(rows)
    for src in range(0, 16, 2):
        for dst in range(0, 16, 2):
            st, (kw, kv), (ow, ov), (rw, rv), (ww, wv) = raw_filter(keys, k, "bfloat16", True, src, dst)
            assert st == 0, (st, src, dst)
            assert lsd.lib().lsdsort_check_device(wv.data_ptr(), None) == 0
            assert np.array_equal(bits_of(ov).reshape(rows, cols), want), f"source at +{src}, destination at +{dst}"
            assert_intact16(keys=kw, out=ow)
            assert_intact(k=rw, workspace=ww)
            assert np.array_equal(bits_of(kv), keys.reshape(-1)), "a read-only input was changed"
        st, (kw, kv), (ow, ov), (iw, iv), (rw, rv), (ww, wv) = raw_perrow(keys, ranks, "bfloat16", True, True, src, out_skip=14 - src)
        assert st == 0 and lsd.lib().lsdsort_check_device(wv.data_ptr(), None) == 0
        assert np.array_equal(bits_of(ov), ek[at, ranks]) and np.array_equal(bits(iv), ei[at, ranks]), f"per-row rank, source at +{src}"
        assert_intact16(keys=kw, values=ow)
        assert_intact(indices=iw, ranks=rw, workspace=ww)


@pytest.mark.parametrize("skip_bytes", [0, 2, 6, 14])
@pytest.mark.parametrize("shape", TIER_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_guard_bands_exact_workspace_and_null_indices(shape, skip_bytes):
    rows, cols = shape
    keys = rk.inputs(rows, cols, "float16", seed=cols + skip_bytes)["float specials"]
    at = np.arange(rows)
    ranks = rk.cycle(rk.candidates_ranks(cols), rows, skip_bytes)
    ek, ei = rk.expected_np(keys, "float16", True)
    st, *_ = raw_perrow(keys, ranks, "float16", True, True, skip_bytes, short_by=1)
    assert st == lsd.errors.LSDSORT_ERR_WORKSPACE, "one byte less than the figure is refused"
    for with_idx in (True, False):
        st, (kw, kv), (ow, ov), (iw, iv), (rw, rv), (ww, wv) = raw_perrow(keys, ranks, "float16", True, with_idx, skip_bytes)
        assert st == 0, st
        assert lsd.lib().lsdsort_check_device(wv.data_ptr(), None) == 0
        assert fault_word(wv) == 0, "fault word"
        assert np.array_equal(bits_of(ov), ek[at, ranks]), f"values (indices={with_idx})"
        if with_idx:
            assert np.array_equal(bits(iv), ei[at, ranks]), "positions"
        else:
            assert (bits(iv) == 0).all(), "no index buffer was given: nothing may be written"
        assert_intact16(keys=kw, values=ow)
        assert_intact(indices=iw, ranks=rw, workspace=ww)
        assert np.array_equal(bits_of(kv), keys.reshape(-1)), "a read-only input was changed"
        assert np.array_equal(bits(rv), ranks), "the ranks were changed"
    k = rk.cycle(rk.candidates_k(cols), rows, skip_bytes // 2)
    want = rk.filter_np(keys, k, "float16", True)
    st, *_ = raw_filter(keys, k, "float16", True, skip_bytes, skip_bytes, short_by=1)
    assert st == lsd.errors.LSDSORT_ERR_WORKSPACE, "one byte less than the figure is refused"
    for in_place in (False, True):
        st, (kw, kv), (ow, ov), (rw, rv), (ww, wv) = raw_filter(keys, k, "float16", True, skip_bytes, (skip_bytes + 6) % 16, in_place)
        assert st == 0, st
        assert lsd.lib().lsdsort_check_device(wv.data_ptr(), None) == 0
        assert fault_word(wv) == 0, "fault word"
        assert np.array_equal(bits_of(ov).reshape(rows, cols), want), f"filter (in place={in_place})"
        assert_intact16(keys=kw, out=ow)
        assert_intact(k=rw, workspace=ww)
        assert np.array_equal(bits(rv), k), "the k's were changed"


# ---- graph replay: the point of the entries ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_idx", [True, False], ids=["indices", "values"])
@pytest.mark.parametrize("shape", [(3, 70001), (17, 1000)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_perrow_graph_replay_follows_ranks_and_keys(shape, with_idx):
    rows, cols = shape
    L = lsd.lib()
    assert L.lsdsort_prepare_device() == 0
    dk = torch.zeros((rows, cols), dtype=torch.int16, device="cuda")
    d_ranks = torch.zeros(rows, dtype=torch.int32, device="cuda")
    out_k = torch.zeros(rows, dtype=torch.int16, device="cuda")
    out_i = torch.zeros(rows, dtype=torch.int32, device="cuda")
    ws = torch.empty(L.lsdsort_kth16_perrow_workspace_bytes(rows, cols), dtype=torch.uint8, device="cuda")

    def call():
        st = L.lsdsort_kth16_perrow_device(dk.data_ptr(), rows, cols, d_ranks.data_ptr(), KEY_TYPES["int16"], 1, out_k.data_ptr(),
                                           out_i.data_ptr() if with_idx else None, ws.data_ptr(), ws.numel(), stream_ptr())
        assert st == 0, st

    kinds = rk.inputs(rows, cols, "int16", seed=cols + 3)
    dk.copy_(torch.from_numpy(kinds["uniform bits"].view(np.int16)))
    g = captured(call)
    cand = rk.candidates_ranks(cols)
    at = np.arange(rows)
    for step, name in enumerate(("four values", "shared top 11 bits", "four values")):   # the keys change, then only the ranks
        keys = kinds[name]
        ranks = rk.cycle(cand, rows, step + 1)
        dk.copy_(torch.from_numpy(keys.view(np.int16)))
        d_ranks.copy_(dev_u32(ranks))
        ek, ei = rk.expected_np(keys, "int16", True)
        seen = []
        for replay in range(2):
            out_k.zero_()
            out_i.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert fault_word(ws) == 0, f"replay on {name}: fault word {fault_word(ws):#x}"
            assert np.array_equal(bits(out_k), ek[at, ranks]), f"replay on {name}, ranks {ranks}: values"
            if with_idx:
                assert np.array_equal(bits(out_i), ei[at, ranks]), f"replay on {name}, ranks {ranks}: positions"
            else:
                assert (bits(out_i) == 0).all(), "no index buffer was given: nothing may be written"
            seen.append((bits(out_k).copy(), bits(out_i).copy()))
        assert np.array_equal(seen[0][0], seen[1][0]) and np.array_equal(seen[0][1], seen[1][1]), "two replays differ"
    assert L.lsdsort_check_device(ws.data_ptr(), None) == 0


@pytest.mark.parametrize("in_place", [False, True], ids=["copy", "in place"])
@pytest.mark.parametrize("shape", [(3, 70001), (17, 1000)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_filter_graph_replay_follows_k_and_keys(shape, in_place):
    rows, cols = shape
    L = lsd.lib()
    assert L.lsdsort_prepare_device() == 0
    dk = torch.zeros((rows, cols), dtype=torch.int16, device="cuda")
    d_k = torch.zeros(rows, dtype=torch.int32, device="cuda")
    out = dk if in_place else torch.zeros((rows, cols), dtype=torch.int16, device="cuda")
    ws = torch.empty(L.lsdsort_topk16_filter_workspace_bytes(rows, cols), dtype=torch.uint8, device="cuda")

    def call():
        st = L.lsdsort_topk16_filter_device(dk.data_ptr(), rows, cols, d_k.data_ptr(), KEY_TYPES["int16"], 1, rk.FILL, out.data_ptr(),
                                            ws.data_ptr(), ws.numel(), stream_ptr())
        assert st == 0, st

    kinds = rk.inputs(rows, cols, "int16", seed=cols + 4)
    dk.copy_(torch.from_numpy(kinds["uniform bits"].view(np.int16)))
    g = captured(call)
    cand = rk.candidates_k(cols)
    for step, name in enumerate(("four values", "shared top 11 bits", "four values", "four values")):
        keys = kinds[name]
        k = rk.cycle(cand, rows, step)
        d_k.copy_(dev_u32(k))
        want = rk.filter_np(keys, k, "int16", True)
        seen = []
        for replay in range(2):
            dk.copy_(torch.from_numpy(keys.view(np.int16)))   # in place the first replay has filtered them
            if not in_place:
                out.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert fault_word(ws) == 0, f"replay on {name}: fault word {fault_word(ws):#x}"
            assert np.array_equal(bits(out), want), f"replay on {name}, k {k}"
            seen.append(bits(out).copy())
        assert np.array_equal(seen[0], seen[1]), "two replays differ"
    assert L.lsdsort_check_device(ws.data_ptr(), None) == 0


# ---- ranks outside the row --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_idx", [True, False], ids=["indices", "values"])
@pytest.mark.parametrize("shape", [(17, 1000), (3, 70001)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_rank_outside_its_row_stores_nothing_and_raises_only_its_own_bit(shape, with_idx):
    rows, cols = shape
    keys = rk.inputs(rows, cols, "bfloat16", seed=cols + 5)["float specials"]
    ranks = rk.cycle(rk.candidates_ranks(cols), rows)
    bad_rows = [1, rows - 1]
    ranks[bad_rows[0]] = cols
    ranks[bad_rows[1]] = rk.OFF
    good = np.ones(rows, dtype=bool)
    good[bad_rows] = False
    at = np.arange(rows)[good]
    SENT = 0x5A5A5A5A
    for largest in (False, True):
        ek, ei = rk.expected_np(keys, "bfloat16", largest)
        st, (kw, kv), (ow, ov), (iw, iv), (rw, rv), (ww, wv) = raw_perrow(keys, ranks, "bfloat16", largest, with_idx, 6, sentinel=SENT)
        assert st == 0, "a rank outside its row is not the host's to refuse"
        torch.cuda.synchronize()
        assert fault_word(wv) == FAULT_RANK, f"fault word {fault_word(wv):#x}: bit 4096 and no other"
        assert lsd.lib().lsdsort_check_device(wv.data_ptr(), None) == lsd.errors.LSDSORT_ERR_DEVICE_FAULT
        gv, gi = bits_of(ov), bits(iv)
        assert (gv[bad_rows] == SENT & 0xFFFF).all() and (gi[bad_rows] == SENT).all(), "something was stored for a row with a bad rank"
        assert np.array_equal(gv[good], ek[at, ranks[good]]), "the other rows' values"
        if with_idx:
            assert np.array_equal(gi[good], ei[at, ranks[good]]), "the other rows' positions"
        else:
            assert (gi == SENT).all(), "no index buffer was given: nothing may be written"
        assert_intact16(keys=kw, values=ow)
        assert_intact(indices=iw, ranks=rw, workspace=ww)
    # the Python face: check_fault raises, and a good call on the same workspace checks clean afterwards
    dk = to_dev(keys, "bfloat16")
    ws = torch.empty(lsd.kth16_perrow_workspace_bytes(rows, cols), dtype=torch.uint8, device="cuda")
    with pytest.raises(lsd.LsdsortError) as err:
        lsd.GPUKth16PerRow(dk, dev_u32(ranks), key_type="bfloat16", return_indices=with_idx, workspace=ws, check_fault=True)
    assert err.value.status == lsd.errors.LSDSORT_ERR_DEVICE_FAULT
    fine = np.where(good, ranks, 0).astype(np.uint32)
    ek, ei = rk.expected_np(keys, "bfloat16", False)
    values, indices = lsd.GPUKth16PerRow(dk, dev_u32(fine), key_type="bfloat16", return_indices=with_idx, workspace=ws, check_fault=True)
    assert fault_word(ws) == 0
    assert np.array_equal(bits(values), ek[np.arange(rows), fine])
    assert indices is None or np.array_equal(bits(indices), ei[np.arange(rows), fine])


# ---- past the grid caps of the short kernels ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(131072 + 9, 9), (4096 + 3, 1025)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_row_loops_go_round_again(shape):
    """one round of the wave tier covers 8 * 16384 rows, one of the workgroup tier 4096 (test_kth16_rowk_cpu.py holds the launch
    lines against these shapes): a second, partly filled round, whose rows carry other ranks and k's than the first round's"""
    rows, cols = shape
    stride = 8 * 16384 if cols <= 1024 else 4096
    keys = rk.without_fill(np.random.default_rng(rows).integers(0, 1 << 16, (rows, cols), dtype=np.uint32).astype(np.uint16))
    keys[::7] = 0x0100 | (keys[::7] & 3)                                          # tie runs in every seventh row
    dk = to_dev(keys, "bfloat16", 1)
    r = np.arange(rows)
    cand_r, cand_k = np.array(rk.candidates_ranks(cols), dtype=np.uint32), np.array(rk.candidates_k(cols), dtype=np.uint32)
    ranks, k = cand_r[(r + r // stride) % cand_r.size], cand_k[(r + r // stride) % cand_k.size]
    assert (ranks[:-stride] != ranks[stride:]).all() and (k[:-stride] != k[stride:]).all()
    ek, ei = rk.expected_np(keys, "bfloat16", True)
    values, indices = lsd.GPUKth16PerRow(dk, dev_u32(ranks), key_type="bfloat16", largest=True, check_fault=True)
    bad = np.flatnonzero((bits(values) != ek[r, ranks]) | (bits(indices) != ei[r, ranks]))
    assert bad.size == 0, f"{bad.size} rows differ, first row {bad[0]} = round {bad[0] // stride}, row {bad[0] % stride} of it"
    values, _ = lsd.GPUKth16PerRow(dk, dev_u32(ranks), key_type="bfloat16", largest=True, return_indices=False, check_fault=True)
    assert np.array_equal(bits(values), ek[r, ranks])
    want = rk.filter_np(keys, k, "bfloat16", True)
    out = lsd.GPUTopK16Filter(dk, dev_u32(k), key_type="bfloat16", largest=True, fill=rk.FILL, check_fault=True)
    bad = np.flatnonzero((bits(out) != want).any(axis=1))
    assert bad.size == 0, f"{bad.size} rows differ, first row {bad[0]} = round {bad[0] // stride}, row {bad[0] % stride} of it"
    own = dk.clone()
    lsd.GPUTopK16Filter(own, dev_u32(k), key_type="bfloat16", largest=True, fill=rk.FILL, out=own, check_fault=True)
    assert np.array_equal(bits(own), want), "in place"


@pytest.mark.parametrize("shape", TIER_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_same_result_without_the_returning_add_rank_form(shape):
    rows, cols = shape
    keys = rk.inputs(rows, cols, "int16", seed=cols + 1)["shared top 8 bits"]
    dk = to_dev(keys, "int16")
    lsd.set_rank_method(0)
    try:
        check_perrow(dk, keys, "int16", "shared top 8 bits, mask rank form", against_single=False)
        check_filter(dk, keys, "int16", "shared top 8 bits, mask rank form")
    finally:
        lsd.set_rank_method(-1)


# ---- the torch-shaped face ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 5, 1000), (3, 4099), (3, 70001)], ids=lambda s: "x".join(map(str, s)))
def test_topk16_filter_rows_against_torch(shape):
    """finite bfloat16 rows without +-0 (torch calls the two zeros equal, the library ranks -0.0 below +0.0): per row
    thr = torch.topk(x.float(), k_r).values[-1], then x.masked_fill(x.float() < thr, -inf)"""
    cols = shape[-1]
    g = torch.Generator(device="cuda").manual_seed(cols)
    x = torch.randn(shape, generator=g, device="cuda").to(torch.bfloat16)
    x[x == 0] = 1.0
    flat = x.view(-1, cols)
    rows = flat.shape[0]
    ks = [1, 20, 50, cols // 2, cols - 1, 1000, 2][:rows] + [7] * max(0, rows - 7)
    ks = [min(k, cols - 1) for k in ks]
    want = torch.stack([row.masked_fill(row.float() < torch.topk(row.float(), k).values[-1], float("-inf")) for row, k in zip(flat, ks)])
    want = want.view(shape)
    for k in (ks, torch.tensor(ks, dtype=torch.int64), torch.tensor(ks, dtype=torch.int32, device="cuda").view(shape[:-1])):
        got = lsd.topk16_filter_rows(x, k)
        assert got.shape == x.shape and got.dtype == x.dtype and got.data_ptr() != x.data_ptr()
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), type(k)
    # one k for every row; smallest with +inf; a fill of the caller's; off rows; in place
    got = lsd.topk16_filter_rows(x, 50)
    one = torch.stack([row.masked_fill(row.float() < torch.topk(row.float(), 50).values[-1], float("-inf")) for row in flat]).view(shape)
    assert torch.equal(got.view(torch.int16), one.view(torch.int16))
    got = lsd.topk16_filter_rows(x, 50, largest=False, fill=123.0)
    low = torch.stack([row.masked_fill(row.float() > torch.topk(row.float(), 50, largest=False).values[-1], 123.0) for row in flat]).view(shape)
    assert torch.equal(got.view(torch.int16), low.view(torch.int16))
    got = lsd.topk16_filter_rows(x, 50, largest=False)
    assert torch.equal(got.view(torch.int16), torch.where(low == 123.0, torch.tensor(float("inf"), dtype=x.dtype, device="cuda"), low).view(torch.int16))
    for off in (0, -1, cols, cols + 1, 1 << 40):
        assert torch.equal(lsd.topk16_filter_rows(x, off).view(torch.int16), x.view(torch.int16)), off
    own = x.clone()
    assert lsd.topk16_filter_rows(own, ks, inplace=True) is own and torch.equal(own.view(torch.int16), want.view(torch.int16))
    i = torch.randint(-30000, 30000, shape, generator=g, device="cuda", dtype=torch.int32).to(torch.int16)
    got = lsd.topk16_filter_rows(i, 5)
    thr = torch.topk(i.view(-1, cols).int(), 5).values[:, -1:]
    assert torch.equal(got.view(-1, cols), torch.where(i.view(-1, cols).int() < thr, torch.tensor(-32768, dtype=torch.int16, device="cuda"), i.view(-1, cols)))
