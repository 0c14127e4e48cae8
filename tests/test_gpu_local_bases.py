"""GPU suite: the local stage's bookkeeping between a digit pass's barriers (local_sort.hip: counts_to_bases on counter words and
the scan over the threads that hold words).

Bases are computed on 32-bit counter words that hold digits 2j and 2j + 1, so the cases to watch are those that put large counts
into one word, into its high half with the low one empty, and into the first and last words of a table -- for every digit width
1 .. 9 (one counter word, two, ... 256; one wave of word threads or several) and in every pass position.  The oracle is numpy's
stable sort of each bucket by its masked low bits; a payload equal to the position shows the order of equal keys.

Through lsdsort_local_sort_u32_device (the 16384-key kernels, up to three passes) and lsdsort_local_sort_halves_u32_device (the
10240-key kernel a whole sort of 2^28 keys runs: nine bits, then the rest), then the other kernels of the unit: the one-launch
sort (four byte passes), the segmented sort's workgroup tier, and one captured graph replayed twice.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 511, 512, 513, 8191, 8192, 8193, 10240, 16384]
KINDS = ["digit0", "highest", "pair", "odd", "uniform"]


def _passes(low_bits):
    """(shift, width) of the digit passes lsdsort_local_sort_u32_device runs: at most nine bits each, as even as they come."""
    count = (low_bits + 8) // 9
    out, shift = [], 0
    for i in range(count):
        width = (low_bits - shift + (count - i) - 1) // (count - i)
        out.append((shift, width))
        shift += width
    return out


def _low_bits(rng, size, passes, kind):
    """The sorted bits of a bucket's keys.  digit0: every key in digit 0 of every pass.  highest: in the highest digit (the high
    half of the table's last word).  pair: half of the keys in the highest digit and half in the one below it -- both halves of
    one word near their maxima, in random order.  odd: every key in digit 1, digit 0 empty.  uniform: random."""
    total = sum(w for _, w in passes)
    ones = np.uint32((1 << total) - 1)
    if kind == "digit0":
        return np.zeros(size, dtype=np.uint32)
    if kind == "highest":
        return np.full(size, ones, dtype=np.uint32)
    firsts = np.uint32(sum(1 << s for s, _ in passes))        # the lowest bit of every digit
    if kind == "pair":
        low = np.full(size, ones, dtype=np.uint32)
        low[: size // 2] &= ~firsts
        return rng.permutation(low)
    if kind == "odd":
        return np.full(size, firsts, dtype=np.uint32)
    return rng.integers(0, 1 << total, size=size, dtype=np.uint64).astype(np.uint32)


def _buckets(low_bits, seed):
    rng = np.random.default_rng(seed)
    passes = _passes(low_bits)
    plan = [(s, k) for k in KINDS for s in SIZES]
    bases = np.concatenate([[0], np.cumsum([s for s, _ in plan])]).astype(np.uint32)
    parts = []
    for size, kind in plan:
        high = rng.integers(0, 1 << (32 - low_bits), size=size, dtype=np.uint64).astype(np.uint32) << np.uint32(low_bits)
        parts.append(high | _low_bits(rng, size, passes, kind))
    return np.concatenate(parts), bases, plan


def _check_buckets(got, got_v, keys, vals, bases, plan, low_bits, tell):
    mask = np.uint32((1 << low_bits) - 1)
    for b, (size, kind) in enumerate(plan):
        lo, hi = int(bases[b]), int(bases[b + 1])
        order = np.argsort(keys[lo:hi] & mask, kind="stable")
        assert np.array_equal(got[lo:hi], keys[lo:hi][order]), (tell, low_bits, size, kind, "keys")
        if got_v is not None:
            assert np.array_equal(got_v[lo:hi], vals[lo:hi][order]), (tell, low_bits, size, kind, "payload order = stable order")


@pytest.mark.parametrize("with_vals", [False, True])
@pytest.mark.parametrize("low_bits", range(1, 28))
def test_buckets_by_their_low_bits(gpu, low_bits, with_vals):
    import torch

    keys, bases, plan = _buckets(low_bits, low_bits)
    vals = np.arange(keys.size, dtype=np.uint32)                  # the position: equal keys must keep their order
    d, db = gpu.to_device(keys), gpu.to_device(bases)
    dv = gpu.to_device(vals) if with_vals else None
    st = gpu.lib().lsdsort_local_sort_u32_device(d.data_ptr(), dv.data_ptr() if with_vals else None, db.data_ptr(), len(plan), low_bits,
                                                 torch.cuda.current_stream().cuda_stream)
    assert st == 0
    _check_buckets(gpu.to_host(d), gpu.to_host(dv) if with_vals else None, keys, vals, bases, plan, low_bits, "eager")


# ---- the halves entry: local_sort_kernel<20, false, false>, nine bits and then 8 - t ----------------------------------------------
@pytest.mark.parametrize("t", [0, 7])
def test_buckets_read_as_halves(gpu, t):
    import torch

    rng = np.random.default_rng(40 + t)
    free = 16 - t                                               # the bits below the group's; the sort is on free + 1 bits
    high = (0b1011001 >> (7 - t)) << (32 - t) if t else 0      # the t top bits every key shares
    num_buckets = 1 << 15
    passes = [(0, 9), (9, free - 9)] if free > 9 else [(0, 9)]
    plan = [(s, k) for k in KINDS for s in SIZES if s <= 10240]
    where = [(i * 2521 + 7) % num_buckets for i in range(len(plan))]
    assert len(set(where)) == len(plan)
    sizes = np.zeros(num_buckets, dtype=np.int64)
    sizes[where] = [s for s, _ in plan]
    bases = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    first = (sizes // 2).astype(np.uint32)                      # the first half of group 2 b, the rest of group 2 b + 1
    keys = np.zeros(int(bases[-1]), dtype=np.uint32)
    for b, (size, kind) in zip(where, plan):
        group = np.full(size, 2 * b, dtype=np.uint32)
        group[int(first[b]):] += 1
        keys[int(bases[b]):int(bases[b + 1])] = np.uint32(high) | (group << np.uint32(free)) | _low_bits(rng, size, passes, kind)

    d_half = torch.from_numpy((keys & np.uint32(0xFFFF)).astype(np.uint16).view(np.int16)).cuda()
    d_out = gpu.to_device(np.full(keys.size, 0xDEADBEEF, dtype=np.uint32))
    d_bases, d_first = gpu.to_device(bases), gpu.to_device(first)
    d_words = gpu.to_device(np.array([t, high, 17 - t], dtype=np.uint32))
    d_fault = gpu.to_device(np.zeros(1, dtype=np.uint32))
    st = gpu.lib().lsdsort_local_sort_halves_u32_device(d_out.data_ptr(), d_half.data_ptr(), d_bases.data_ptr(), d_first.data_ptr(),
                                                        num_buckets, d_words.data_ptr(), d_fault.data_ptr(),
                                                        torch.cuda.current_stream().cuda_stream)
    assert st == 0
    got = gpu.to_host(d_out)
    assert int(gpu.to_host(d_fault)[0]) == 0
    mask = np.uint32((1 << (17 - t)) - 1)
    for b, (size, kind) in zip(where, plan):
        lo, hi = int(bases[b]), int(bases[b + 1])
        order = np.argsort(keys[lo:hi] & mask, kind="stable")
        assert np.array_equal(got[lo:hi], keys[lo:hi][order]), (t, b, size, kind)


# ---- the other kernels that run the same digit pass ---------------------------------------------------------------------------------
@pytest.mark.parametrize("pairs", [False, True])
@pytest.mark.parametrize("n", [16384, 16383, 513])
def test_one_launch_sorts(gpu, n, pairs):
    """small_sort_kernel: four byte passes over the whole array.  Uniform keys, and keys whose every byte is 0xFE or 0xFF."""
    rng = np.random.default_rng(n)
    uniform = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    pair = np.uint32(0xFFFFFFFF) ^ (rng.integers(0, 16, size=n, dtype=np.uint64).astype(np.uint32) * np.uint32(0x01010101) & np.uint32(0x01010101))
    for keys in (uniform, pair):
        vals = np.arange(n, dtype=np.uint32)
        d = gpu.to_device(keys)
        dv = gpu.to_device(vals) if pairs else None
        gpu.GPULSDRadixSort(d, 8, d_vals=dv, check_fault=True)
        order = np.argsort(keys, kind="stable")
        assert np.array_equal(gpu.to_host(d), keys[order]), n
        if pairs:
            assert np.array_equal(gpu.to_host(dv), vals[order]), (n, "payload order = stable order")


@pytest.mark.parametrize("pairs", [False, True])
def test_segments_of_the_workgroup_tier(gpu, pairs):
    """segment_sort_kernel at the tier's smallest (1025) and largest (16384) sizes: one value per segment (no byte differs: no pass),
    two values a bit apart in every byte (two neighbouring digits hold everything), uniform keys."""
    import torch

    rng = np.random.default_rng(9)
    sizes = [1025, 16384, 1025, 16384, 1025, 16384]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    n = int(offsets[-1])
    keys = np.empty(n, dtype=np.uint32)
    for s, size in enumerate(sizes):
        lo, hi = int(offsets[s]), int(offsets[s + 1])
        if s < 2:
            keys[lo:hi] = np.uint32(0x9E3779B9)
        elif s < 4:
            keys[lo:hi] = np.where(rng.integers(0, 2, size=size) == 0, np.uint32(0xFEFEFEFE), np.uint32(0xFFFFFFFF))
        else:
            keys[lo:hi] = rng.integers(0, 1 << 32, size=size, dtype=np.uint64).astype(np.uint32)
    vals = np.arange(n, dtype=np.uint32)
    dk = torch.from_numpy(keys.view(np.int32)).cuda()
    do = torch.from_numpy(offsets.view(np.int32)).cuda()
    dv = torch.from_numpy(vals.view(np.int32)).cuda() if pairs else None
    gpu.GPUSortSegmented(dk, do, d_vals=dv, check_fault=True)
    torch.cuda.synchronize()
    got = dk.cpu().numpy().view(np.uint32)
    got_v = dv.cpu().numpy().view(np.uint32) if pairs else None
    for s in range(len(sizes)):
        lo, hi = int(offsets[s]), int(offsets[s + 1])
        order = np.argsort(keys[lo:hi], kind="stable")
        assert np.array_equal(got[lo:hi], keys[lo:hi][order]), (s, sizes[s], "keys")
        if pairs:
            assert np.array_equal(got_v[lo:hi], vals[lo:hi][order]), (s, sizes[s], "payload order = stable order")


def test_a_captured_graph_replayed_twice(gpu):
    """The launch captured once and replayed on fresh keys: what a pass leaves in the counter words and in the scan's partials
    must not reach the next replay."""
    import torch

    low_bits = 17
    batches = [_buckets(low_bits, 100 + r) for r in range(3)]
    bases, plan = batches[0][1], batches[0][2]
    n = int(bases[-1])
    vals = np.arange(n, dtype=np.uint32)
    d, dv, db = gpu.to_device(batches[0][0]), gpu.to_device(vals), gpu.to_device(bases)
    L = gpu.lib()

    def call():
        return L.lsdsort_local_sort_u32_device(d.data_ptr(), dv.data_ptr(), db.data_ptr(), len(plan), low_bits, torch.cuda.current_stream().cuda_stream)

    assert call() == 0                                           # the warm-up: device set-up stays out of the capture
    torch.cuda.synchronize()
    _check_buckets(gpu.to_host(d), gpu.to_host(dv), batches[0][0], vals, bases, plan, low_bits, "warm-up")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        status = call()
    assert status == 0
    for r in (1, 2):
        keys = batches[r][0]
        d.copy_(gpu.to_device(keys))
        dv.copy_(gpu.to_device(vals))
        graph.replay()
        torch.cuda.synchronize()
        _check_buckets(gpu.to_host(d), gpu.to_host(dv), keys, vals, bases, plan, low_bits, "replay %d" % r)
