"""The local stage's padding positions (local_sort.hip, holds_key): a workgroup's rows past the bucket's end, and the lanes past the
end in the one partial row, take no part in a digit pass.  Padded, they were keys of the highest digit that stood last; so the
keys to watch are REAL keys of the highest digit next to them -- all low bits set, at the bucket's tail, in the wave that holds
the partial row -- and payloads, whose slots come from the same ranks.  Against numpy's stable sort, at the sizes where a wave's
count of live rows changes: around a row of 64, around a wave's first position (w * rows * 64: the waves behind it are empty),
around the 512-key step at which every wave gets one more row, and at the capacity.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# rows = ceil(size / 512); wave w starts at w * rows * 64.  2 rows: waves start at multiples of 128 (640 = wave 5, 896 = wave 7);
# 3 rows: 192 (1344 = wave 7); 7 rows: 448 (3136 = wave 7); 17 rows: 1088 (7616 = wave 7); 21 rows: 1344 (9408 = wave 7)
SIZES = [1, 63, 64, 65, 127, 128, 129, 511, 512, 513, 639, 640, 641, 704, 705, 895, 896, 897, 1024, 1025, 1343, 1344, 1345, 3073, 3135,
         3136, 3137, 8191, 8192, 8193, 8255, 8256, 8257, 8703, 8704, 8705, 10239, 10240, 10241, 16320, 16321, 16383, 16384]


def _keys(rng, n, low_bits):
    """Random keys; in the last quarter of every run of 100 keys, and in the array's last 40, all low bits set (the highest digit
    of every pass), some of them 0xFFFFFFFF itself -- the value a padded position held."""
    keys = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    top = np.uint32((1 << low_bits) - 1)
    idx = np.arange(n)
    hot = (idx % 100 >= 75) | (idx >= n - 40)
    keys[hot] |= top
    keys[hot & (idx % 3 == 0)] = np.uint32(0xFFFFFFFF)
    return keys


@pytest.mark.parametrize("low_bits", [9, 17, 27])
@pytest.mark.parametrize("with_vals", [False, True])
def test_buckets_whose_tail_is_the_highest_digit(gpu, low_bits, with_vals):
    import torch

    rng = np.random.default_rng(low_bits)
    bases = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.uint32)
    n = int(bases[-1])
    keys = np.concatenate([_keys(rng, s, low_bits) for s in SIZES])
    vals = np.arange(n, dtype=np.uint32) * np.uint32(5) + np.uint32(1)
    d, db = gpu.to_device(keys), gpu.to_device(bases)
    dv = gpu.to_device(vals) if with_vals else None
    st = gpu.lib().lsdsort_local_sort_u32_device(d.data_ptr(), dv.data_ptr() if with_vals else None, db.data_ptr(), len(SIZES), low_bits,
                                                 torch.cuda.current_stream().cuda_stream)
    assert st == 0
    got = gpu.to_host(d)
    got_v = gpu.to_host(dv) if with_vals else None
    mask = np.uint32((1 << low_bits) - 1)
    for b, size in enumerate(SIZES):
        lo, hi = int(bases[b]), int(bases[b + 1])
        order = np.argsort(keys[lo:hi] & mask, kind="stable")
        assert np.array_equal(got[lo:hi], keys[lo:hi][order]), (low_bits, size, with_vals)
        if with_vals:
            assert np.array_equal(got_v[lo:hi], vals[lo:hi][order]), (low_bits, size, "payload order = stable order")


def _whole_sort_keys(n, seed):
    """Uniform keys whose last quarter (input order) has all 18 bits below a 2^14-bucket's set, every third of those all 17 below a
    2^15-bucket's only, and whose last 5000 are 0xFFFFFFFF.  The global passes are stable, so after them every bucket's tail -- the
    partial row and the lanes before the padding -- is made of keys of the highest digit of both local passes."""
    import torch

    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    k = torch.randint(0, 1 << 32, (n,), dtype=torch.int64, device="cuda", generator=gen)
    idx = torch.arange(n, device="cuda")
    hot = idx >= n - n // 4
    k = torch.where(hot, k | torch.where(idx % 3 == 0, 0x1FFFF, 0x3FFFF), k)
    k[n - 5000:] = 0xFFFFFFFF
    return k


# The host's choice of the local stage's variant (lsdsort_api.hip hybrid_small_cap, lsd_kernels.hpp hybrid_bucket_bits), 2^14 buckets
# each: 4e7 keys -> mean 2441, the 5120-key variant (K = 10); 2^27 keys -> mean 8192, the 10240-key variant (K = 20: the flagship's
# kernel); 9e7 pairs -> mean 5493 + 6 sigma above 5120, the 8192-pair variant (K = 16); 4e7 pairs -> K = 10 with payloads.
@pytest.mark.parametrize("n,pairs", [(40_000_000 + 123, False), ((1 << 27) + 4321, False), (90_000_000 + 77, True), (40_000_000 + 5, True)])
def test_whole_sorts_whose_buckets_end_in_the_highest_digit(gpu, n, pairs):
    import torch

    k = _whole_sort_keys(n, n % 1000)
    expect = torch.sort(k, stable=True)
    d = ((k + (1 << 31)) % (1 << 32) - (1 << 31)).to(torch.int32)
    v = torch.arange(n, dtype=torch.int32, device="cuda") if pairs else None
    del k
    ws = gpu.alloc_workspace(n, 8, pairs)
    tm = gpu.GPULSDRadixSortTimed(d, 8, d_vals=v, workspace=ws)
    assert tm["hybrid"] == 1, "these keys are uniform in their top bits: the local stage must have run"
    assert gpu.lib().lsdsort_check_device(ws.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    assert torch.equal(d.to(torch.int64) & 0xFFFFFFFF, expect.values)
    if pairs:
        assert torch.equal(v.to(torch.int64), expect.indices), "payload order = stable order"


def test_records_whose_buckets_end_in_the_highest_digit(gpu):
    """Several payload arrays (sort_bucket_multi: the two passes' slots are composed through LDS, a padding lane's through its own
    position).  2^26 records with three payload arrays: buckets of 4096, local_sort_multi_kernel<16>."""
    import torch

    payloads, n = 3, (1 << 26) + 4321
    k = _whole_sort_keys(n, payloads)
    expect = torch.sort(k, stable=True)
    d = ((k + (1 << 31)) % (1 << 32) - (1 << 31)).to(torch.int32)
    del k
    idx = torch.arange(n, dtype=torch.int32, device="cuda")
    pay = [(idx * (2 * e + 3) + e).to(torch.int32) for e in range(payloads)]
    want = [p[expect.indices] for p in pay]
    ws = torch.empty(int(gpu.lib().lsdsort_workspace_bytes(n, 8, payloads)), dtype=torch.uint8, device="cuda")
    gpu.GPUSortMulti(d, pay, r=8, workspace=ws, check_fault=True)
    assert gpu.workspace_form(ws) == 1
    assert torch.equal(d.to(torch.int64) & 0xFFFFFFFF, expect.values)
    for e in range(payloads):
        assert torch.equal(pay[e], want[e]), ("payload", e)


@pytest.mark.parametrize("pairs", [False, True])
def test_one_workgroup_sorts_whose_tail_is_the_highest_digit(gpu, pairs):
    """The sort of up to 16384 items in one launch: four byte passes over the same rows."""
    rng = np.random.default_rng(5)
    for n in (1, 65, 513, 640, 641, 897, 3137, 8193, 8705, 16321, 16384):
        keys = _keys(rng, n, 32 if n % 2 else 8)
        vals = np.arange(n, dtype=np.uint32)
        d = gpu.to_device(keys)
        dv = gpu.to_device(vals) if pairs else None
        gpu.GPULSDRadixSort(d, 8, d_vals=dv, check_fault=True)
        order = np.argsort(keys, kind="stable")
        assert np.array_equal(gpu.to_host(d), keys[order]), n
        if pairs:
            assert np.array_equal(gpu.to_host(dv), vals[order]), (n, "payload order = stable order")
