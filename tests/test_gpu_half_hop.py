"""The hybrid form's half variant (half_hop.hip, rank_scatter_kernel's HALF instantiation, the half-reading branch of
local_sort_kernel<20, false, false>): the second global pass writes and the local stage reads only the low 16
bits of every key.  No reference counterpart; the RESULT has one, the sorted array: every case is compared bit-exact with
torch.sort or numpy, and with the same sort run with the variant switched off.

The local stage alone through lsdsort_local_sort_halves_u32_device, then whole sorts at the smallest size the variant exists
for (158 056 448 keys, the first n sorted in 2^15 buckets) and 12345 keys above it.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N0 = 158_056_448
SIZES = (N0, N0 + 12345)


def _u64(t):
    import torch

    return t.to(torch.int64) & 0xFFFFFFFF


def _i32(x):
    import torch

    return ((x + (1 << 31)) % (1 << 32) - (1 << 31)).to(torch.int32)


# ---- the local stage alone ---------------------------------------------------------------------------------------------
def _bucket_keys(rng, b, size, first, t, high, kind):
    """The keys of bucket b (the 15 bits below a prefix of t bits) as they lie after pass B: `first` keys of group 2 b, then
    size - first of group 2 b + 1, each part in random order."""
    free = 16 - t                                   # the bits below the group's
    low = rng.integers(0, 1 << free, size=size, dtype=np.uint64).astype(np.uint32)
    if kind == "dead_first":                        # the low nine bits the same in every key: the first local digit is no pass
        low = (low & np.uint32(((1 << free) - 1) & ~0x1FF)) | np.uint32(0x155)
    elif kind == "dead_second":                     # bits 9 .. 16 - t the same (first is 0 or size: the group bit is one of them)
        low = (low & np.uint32(0x1FF)) | np.uint32((0x2A << 9) & ((1 << free) - 1))
    g = np.full(size, 2 * b, dtype=np.uint32)
    g[first:] += 1
    keys = np.uint32(high) | (g << np.uint32(free)) | low
    if kind == "ffff_tail" and size:                # 0xFFFF halves at the bucket's tail (group 2 b + 1: bit 16 - t set)
        assert first < size and t == 0
        tail = max(1, min(size - first, 70))
        keys[size - tail:] = np.uint32(high) | (np.uint32(2 * b + 1) << np.uint32(16)) | np.uint32(0xFFFF)
    return keys


def _run_halves(gpu, keys, bases, first, t, high, num_buckets, sentinel=0xDEADBEEF):
    import torch

    d_half = torch.from_numpy((keys & np.uint32(0xFFFF)).astype(np.uint16).view(np.int16)).cuda()
    d_out = gpu.to_device(np.full(keys.size, sentinel, dtype=np.uint32))
    d_bases, d_first = gpu.to_device(bases), gpu.to_device(first)
    d_words = gpu.to_device(np.array([t, high, 17 - t], dtype=np.uint32))
    d_fault = gpu.to_device(np.zeros(1, dtype=np.uint32))
    st = gpu.lib().lsdsort_local_sort_halves_u32_device(d_out.data_ptr(), d_half.data_ptr(), d_bases.data_ptr(), d_first.data_ptr(),
                                                        num_buckets, d_words.data_ptr(), d_fault.data_ptr(),
                                                        torch.cuda.current_stream().cuda_stream)
    assert st == 0
    torch.cuda.synchronize()
    return gpu.to_host(d_out), int(gpu.to_host(d_fault)[0])


@pytest.mark.parametrize("t", [0, 1, 2, 3, 4, 5, 6, 7])
def test_local_stage_reads_halves(gpu, t):
    """Bucket sizes 0, 1, around a row of 512 and at the 10240-key capacity; first[b] = 0, size and size / 2; dead first and
    second digits; 0xFFFF halves at a tail -- at bucket numbers spread over all 2^15, so that the rebuilt upper bits differ."""
    rng = np.random.default_rng(100 + t)
    high = (0b1010101 >> (7 - t)) << (32 - t) if t else 0                  # the t top bits every key shares
    num_buckets = 1 << 15
    plan = []                                    # (size, first, kind)
    for size in (0, 1, 511, 512, 513, 10239, 10240):
        for first in sorted({0, size, size // 2}):
            plan.append((size, first, "plain"))
    for size in (513, 4000, 10240):
        plan.append((size, size, "dead_first"))
        plan.append((size, size // 2, "dead_first"))
        plan.append((size, size, "dead_second"))
        plan.append((size, 0, "dead_second"))
    if t == 0:
        for size in (1, 513, 1000, 10239, 10240):
            plan.append((size, size // 3, "ffff_tail"))
    where = np.sort(rng.choice(np.arange(1, num_buckets - 1), size=len(plan) - 2, replace=False))
    where = np.concatenate([[0], where, [num_buckets - 1]])               # the first and the last bucket among them
    sizes = np.zeros(num_buckets, dtype=np.int64)
    first = np.zeros(num_buckets, dtype=np.uint32)
    parts = []
    for b, (size, f, kind) in zip(where, plan):
        sizes[b], first[b] = size, f
        parts.append(_bucket_keys(rng, int(b), size, f, t, high, kind))
    bases = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    keys = np.concatenate(parts)
    got, fault = _run_halves(gpu, keys, bases, first, t, high, num_buckets)
    assert fault == 0
    for b, (size, f, kind), part in zip(where, plan, parts):
        lo = int(bases[b])
        assert np.array_equal(got[lo:lo + size], np.sort(part)), (t, int(b), size, f, kind)


def test_local_stage_leaves_a_bucket_above_its_capacity(gpu):
    rng = np.random.default_rng(7)
    sizes = np.array([700, 10241, 300], dtype=np.int64)
    first = np.array([350, 5000, 0], dtype=np.uint32)
    parts = [_bucket_keys(rng, b, int(sizes[b]), int(first[b]), 0, 0, "plain") for b in range(3)]
    bases = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    got, fault = _run_halves(gpu, np.concatenate(parts), bases, first, 0, 0, 3, sentinel=0x12345678)
    assert fault & 8, "a bucket of 10241 keys must raise fault bit 3"
    assert np.all(got[700:700 + 10241] == np.uint32(0x12345678)), "the bucket above the capacity was written"
    assert np.array_equal(got[:700], np.sort(parts[0])) and np.array_equal(got[700 + 10241:], np.sort(parts[2]))


# ---- whole sorts -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base(gpu):
    """Uniform keys of the larger size, made once; every case takes its first n and never changes them."""
    import torch

    gen = torch.Generator(device="cuda")
    gen.manual_seed(24)
    return torch.randint(-(1 << 31), (1 << 31) - 1, (SIZES[-1],), dtype=torch.int32, device="cuda", generator=gen)


@pytest.fixture(scope="module")
def roomy_ws(gpu):
    ws = gpu.alloc_workspace(SIZES[-1], 8)
    assert ws.numel() == gpu.lib().lsdsort_workspace_bytes_roomy(SIZES[-1], 8) > gpu.lib().lsdsort_workspace_bytes(SIZES[-1], 8, 0)
    return ws


def _shape(name, base, n):
    import torch

    k = _u64(base[:n])
    if name == "uniform":
        return base[:n].clone()
    if name == "sorted":
        return _i32(torch.sort(k).values)
    if name == "low_9_bits_dead":
        return _i32(k & 0xFFFFFE00)
    if name == "bit_16_constant_per_bucket":          # bit 16 = the bucket's lowest bit: first[b] is the bucket's size or 0
        return _i32((k & ~0x10000) | ((k >> 1) & 0x10000))
    if name.startswith("prefix_"):
        t = int(name[7:])
        return _i32((k >> t) | ((0b1011011 >> (7 - t)) << (32 - t)))
    if name == "bucket_of_12000":                     # one bucket above the 10240-key kernel, under the 16384-key one
        hot = 12000 - (n >> 15)
        return _i32(torch.cat([k[: n - hot], (k[:hot] & 0x1FFFF) | (5 << 17)]))
    if name == "half_zeros":
        return _i32(torch.where(((k >> 13) & 1) != 0, k, torch.zeros_like(k)))
    if name == "one_key_outside_the_prefix":          # t = 3 everywhere the sample looks; position 1 is not a sample's
        out = (k >> 3) | (0b101 << 29)
        out[1] = 0x12345678
        return _i32(out)
    raise AssertionError(name)


# name -> (hybrid, half) the sort must report
EXPECTED = {
    "uniform": (1, 1), "sorted": (1, 1), "low_9_bits_dead": (1, 1), "bit_16_constant_per_bucket": (1, 1),
    "prefix_1": (1, 1), "prefix_3": (1, 1), "prefix_7": (1, 1),
    "bucket_of_12000": (1, 0), "half_zeros": (0, 0), "one_key_outside_the_prefix": (0, 0),
}


def _sort_both_ways(gpu, keys, ws, want):
    """Sorts `keys` with the variant on and off in `ws`; checks the forms read back and that the outputs are equal.  Returns the
    output of the sort with the variant on."""
    import torch

    d = keys.clone()
    gpu.GPULSDRadixSort(d, 8, workspace=ws, check_fault=True)
    got = (gpu.workspace_form(ws), gpu.workspace_half(ws))
    gpu.set_half_hop(False)
    try:
        d2 = keys.clone()
        gpu.GPULSDRadixSort(d2, 8, workspace=ws, check_fault=True)
        off = (gpu.workspace_form(ws), gpu.workspace_half(ws))
    finally:
        gpu.set_half_hop(True)
    assert got == want, ("form read back (hybrid, half)", got, want)
    assert off == (want[0], 0), ("with the variant off", off)
    assert torch.equal(d, d2), "the variant changes the output"
    return d


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", list(EXPECTED))
def test_whole_sorts_with_and_without_the_variant(gpu, base, roomy_ws, name, n):
    import torch

    keys = _shape(name, base, n)
    expect = torch.sort(_u64(keys)).values
    d = _sort_both_ways(gpu, keys, roomy_ws, EXPECTED[name])
    assert torch.equal(_u64(d), expect), (name, n)


def test_timed_entry_reports_the_pass_that_ran(gpu, base, roomy_ws):
    import torch

    for name in ("uniform", "bucket_of_12000"):
        keys = _shape(name, base, N0)
        tm = gpu.GPULSDRadixSortTimed(keys, 8, workspace=roomy_ws)
        assert tm["hybrid"] == 1 and tm["passes"] == 2 and len(tm["scatter_ms"]) == 2, tm
        assert gpu.workspace_half(roomy_ws) == EXPECTED[name][1]
        # both passes and the local stage moved 1.58e8 keys: no event pair of a launch that only said no (a few microseconds)
        assert min(tm["scatter_ms"]) > 0.05 and tm["local_ms"] > 0.05, tm
        assert torch.equal(_u64(keys), torch.sort(_u64(_shape(name, base, N0))).values)


def test_plain_workspace_runs_the_full_key_form(gpu, base):
    import torch

    n = N0
    plain = int(gpu.lib().lsdsort_workspace_bytes(n, 8, 0))
    ws = torch.empty(plain, dtype=torch.uint8, device="cuda")
    keys = base[:n].clone()
    gpu.GPULSDRadixSort(keys, 8, workspace=ws, check_fault=True)
    assert (gpu.workspace_form(ws), gpu.workspace_half(ws)) == (1, 0)
    assert torch.equal(_u64(keys), torch.sort(_u64(base[:n])).values)


def test_key_base_one_word_off_16_bytes(gpu, base, roomy_ws):
    import torch

    n = N0
    buf = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    keys = buf[1:]
    assert keys.data_ptr() % 16 == 4
    keys.copy_(base[:n])
    gpu.GPULSDRadixSort(keys, 8, workspace=roomy_ws, check_fault=True)
    assert (gpu.workspace_form(roomy_ws), gpu.workspace_half(roomy_ws)) == (1, 1)
    assert torch.equal(_u64(keys), torch.sort(_u64(base[:n])).values)


def test_one_graph_replayed_on_keys_it_takes_and_keys_it_refuses(gpu, base, roomy_ws):
    import torch

    n = N0
    static_k = base[:n].clone()
    gpu.GPULSDRadixSort(static_k, 8, workspace=roomy_ws)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gpu.GPULSDRadixSort(static_k, 8, workspace=roomy_ws)
    for name in ("uniform", "bucket_of_12000", "half_zeros", "prefix_3", "uniform"):
        keys = _shape(name, base, n)
        static_k.copy_(keys)
        graph.replay()
        torch.cuda.synchronize()
        assert (gpu.workspace_form(roomy_ws), gpu.workspace_half(roomy_ws)) == EXPECTED[name], name
        assert gpu.lib().lsdsort_check_device(roomy_ws.data_ptr(), None) == 0
        assert torch.equal(_u64(static_k), torch.sort(_u64(keys)).values), name
