"""CPU suite: the restated rules of tests/_hybrid_words.py -- the oracle of test_gpu_hybrid_edges.py -- against the constants of the
sources and against arithmetic done by hand.  What is pinned here is what the GPU cases rest on: the place and the names of the
control words, the two edges of the half variant's window, the fold of two 16-bit counts into a bucket, the upfront read's grid
(which workgroup counts which key) and the sample's positions."""
import numpy as np
import pytest

import _hybrid_words as hw


def test_control_words_are_where_the_sources_say():
    assert hw.CONTROL_BYTES == 512 and hw.HYBRID_OFFSET_WORDS == 50
    assert hw.WORD_INDEX == {"Ok": 0, "SkipLocal": 1, "Plan": 2, "Largest": 10, "LargeCount": 11, "Hopeless": 12, "Violated": 13,
                             "Differ": 14, "Prefix": 15, "Shift": 16, "LowBits": 20, "HalfOk": 21, "HalfHigh": 22, "HalfPlan": 23}
    assert hw._KERNELS["kHybridWords"] == 21 and hw._KERNELS["kHalfWords"] == 25
    assert 4 * (hw.HYBRID_OFFSET_WORDS + hw._KERNELS["kHalfWords"]) <= hw.CONTROL_BYTES
    assert (hw.LOCAL_SORT_CAP, hw.CAP_SMALL, hw.CAP_SMALL_PAIRS, hw.CAP_TINY) == (16384, 10240, 8192, 5120)
    assert (hw.MAX_PREFIX, hw.MAX_MEAN_BUCKET, hw.HALF_GROUPS) == (7, 14648, 65536)
    assert hw.MIN_ITEMS == {False: 38_000_000, True: 22_000_000} and hw.MAX_KEYS == 960_000_000


def test_the_window_and_its_capacity():
    lo, hi = hw.WINDOW
    assert (lo, hi) == (158_056_448, 330_596_351)
    assert [hw.hybrid_bucket_bits(n) for n in (lo - 1, lo, hi, hi + 1)] == [14, 15, 15, 16]
    assert [hw.in_half_window(n) for n in (lo - 1, lo, 1 << 28, hi, hi + 1)] == [False, True, True, True, False]
    assert all(hw.hybrid_small_cap(n) == 10240 for n in (lo, lo + 12345, 1 << 28, hi, hi + 1))
    assert hi >> 15 == 10088 and hi - (hi >> 15 << 15) == 32767, "balanced buckets at the top: 10088 or 10089 keys"
    # the other sizes of test_gpu_hybrid_edges.py
    assert [hw.hybrid_tried(n) for n in (37_999_999, 38_000_000, 960_000_000, 960_000_001)] == [False, True, True, False]
    assert hw.hybrid_bucket_bits(960_000_000) == 16 and hw.hybrid_small_cap(960_000_000) == 16384
    assert hw.hybrid_bucket_bits(lo, True) == 15 and hw.hybrid_small_cap(lo, True) == 8192 and hw.hybrid_tried(lo, True)


def test_the_library_agrees_on_the_window():
    from lsdradixsort_amd import lib

    L = lib()
    L.lsdsort_set_tile_config(8, -1)
    for n in (hw.WINDOW[0] - 1, hw.WINDOW[0], hw.WINDOW[1], hw.WINDOW[1] + 1):
        roomy, plain = L.lsdsort_workspace_bytes_roomy(n, 8), L.lsdsort_workspace_bytes(n, 8, 0)
        assert (roomy > plain) == hw.in_half_window(n), n


@pytest.mark.parametrize("low,high,bucket,first,lost", [
    (65535, 2412, 2412 + 65535, 65535, 0),            # the largest count a half holds: nothing lost
    (65536, 2412, 2412 + 1, 0, 65535),                # a low group of 2^16: carries into its sibling
    (65537, 2412, 2412 + 2, 1, 65535),
    (65536 + 7000, 2412, 2412 + 7001, 7000, 65535),
    (131072 + 5, 2412, 2412 + 7, 5, 131070),          # two carries
    (2412, 65536, 2412, 2412, 65536),                 # a high group of 2^16: carries out of the word
    (2412, 65536 + 7000, 2412 + 7000, 2412, 65536),
    (0, 0, 0, 0, 0), (10240, 0, 10240, 10240, 0), (0, 10240, 10240, 0, 0),
])
def test_the_fold(low, high, bucket, first, lost):
    assert hw.fold(low, high) == (bucket, first, lost)
    groups = np.zeros(1 << 16, dtype=np.int64)
    groups[[24690, 24691]] = low, high
    b, f = hw.fold_counts(groups)
    assert (int(b[12345]), int(f[12345])) == (bucket, first) and int(b.sum()) == low + high - lost
    back = hw.unpack_counts(groups)
    assert int(back.sum()) == low + high - lost and (back < 65536).all()


def test_every_folded_overflow_looks_small():
    """the point of the sum check: with a sibling of the smallest window's mean, each overflowing count of the GPU cases gives a
    bucket under the small capacity, so neither Largest nor the list can object"""
    for low, high in ((65536, 2412), (65537, 2412), (72536, 2412), (131077, 2412), (2412, 65536), (2412, 72536)):
        bucket, first, lost = hw.fold(low, high)
        assert bucket <= hw.CAP_SMALL and lost in (65535, 65536, 131070)


def test_the_upfront_reads_grid():
    """workgroup w of 256 owns keys [(w + 256 i) 16384, (w + 256 i + 1) 16384): read from kHybridHistThreads, kHybridVpt and
    kHybridHistMaxBlocks"""
    assert (hw.HIST_THREADS, hw.HIST_VPT, hw.HIST_MAX_BLOCKS) == (1024, 4, 256)
    assert hw.CHUNK_KEYS == 4096 and hw.GROUP_KEYS == 16384
    n = hw.WINDOW[1] + 1
    assert hw.hist_blocks(n) == 256 and hw.full_group_keys(n) == n
    assert hw.owned_ranges(3, n, 4) == [((3 + 256 * i) * 16384, (4 + 256 * i) * 16384) for i in range(4)]
    for lo, hi in hw.owned_ranges(3, n, 4):
        assert set(hw.owner_of(np.array([lo, lo + 4095, lo + 4096, hi - 1]), n).tolist()) == {3}
        assert hw.owner_of(lo - 1, n) == 2 and hw.owner_of(hi, n) == 4
    # the tail loop: a thread per key, workgroup after workgroup; everything for a base that is not 16-byte aligned
    m = hw.WINDOW[0] + 12345
    full = hw.full_group_keys(m)
    assert full == hw.WINDOW[0] and hw.owner_of(m - 1, m) == (m - 1 - full) // 1024 % 256
    assert hw.full_group_keys(m, aligned=False) == 0 and hw.owner_of(1024 * 257 + 5, m, aligned=False) == 1
    assert hw.hist_blocks(m, aligned=False) == 256 and hw.hist_blocks(5000, aligned=False) == 1


def test_the_samples_positions():
    assert (hw.SAMPLES, hw.SAMPLE_BLOCKS, hw.SAMPLE_THREADS, hw.SAMPLE_HOPELESS_AT) == (65536, 64, 1024, 8)
    n = hw.WINDOW[0]
    pos = hw.sample_positions(n)
    assert pos.shape == (64, 1024) and hw.sample_step(n) == 2411
    assert np.array_equal(np.sort(pos.reshape(-1)), np.arange(65536) * 2411) and pos[5, 7] == (7 * 64 + 5) * 2411
    # a contiguous run of 65536 keys is spread over the workgroups: 27 or 28 samples, one or none each
    hits = hw.sample_hits([(1_000_001, 1_000_001 + 65536)], n)
    assert hits.sum() in (27, 28) and hits.max() == 1
    # the four groups of workgroup 3 of the upfront read at the first size with 2^16 buckets: four samples in one workgroup at most
    n = hw.WINDOW[1] + 1
    hits = hw.sample_hits(hw.owned_ranges(3, n, 4), n)
    assert hits.max() == 4 < hw.SAMPLE_HOPELESS_AT and hits.sum() == 13


def test_sample_verdict_on_small_inputs():
    import torch

    n = 65536 * 4
    gen = torch.Generator().manual_seed(3)
    keys = torch.randint(-(1 << 31), (1 << 31) - 1, (n,), dtype=torch.int32, generator=gen)
    hopeless, differ = hw.sample_verdict(keys, 15)
    assert hopeless == 0 and differ >> 31 == 1
    # eight samples of workgroup 2 in one bucket, seven in another
    pos = hw.sample_positions(n)
    heavy = keys.clone()
    heavy[torch.from_numpy(pos[2, :7])] = hw.i32(torch.full((7,), 0xABCD0000) | torch.arange(7))
    assert hw.sample_verdict(heavy, 15)[0] == 0
    heavy[int(pos[2, 900])] = hw.i32(torch.tensor([0xABCD1234]))[0]
    assert hw.sample_verdict(heavy, 15)[0] == 1
    # at 2^16 buckets two neighbours share a counter: four and four
    pair = keys.clone()
    pair[torch.from_numpy(pos[9, :4])] = hw.i32(torch.full((4,), 0x12340000))
    pair[torch.from_numpy(pos[9, 4:8])] = hw.i32(torch.full((4,), 0x12350000))
    assert hw.sample_verdict(pair, 16)[0] == 1 and hw.sample_verdict(pair, 15)[0] == 1 and hw.sample_verdict(pair, 14)[0] == 1
    pair[int(pos[9, 7])] = hw.i32(torch.tensor([0x12360000]))[0]
    assert hw.sample_verdict(pair, 16)[0] == 0
    # a shared prefix: keys below 2^29 differ from keys[0] in 29 bits at most
    low = hw.i32(hw.u64(keys) >> 3 | (0b101 << 29))
    assert 32 - hw.sample_verdict(low, 15)[1].bit_length() == 3


def test_the_builder():
    import torch

    n, step = 200_000, 16
    gen = torch.Generator().manual_seed(5)
    keys = torch.randint(-(1 << 31), (1 << 31) - 1, (n,), dtype=torch.int32, generator=gen)
    field = 0x234
    out = hw.with_exact_count(keys, 20, field, 700, avoid_step=step)
    changed = (out != keys).nonzero().reshape(-1)
    was = int(((hw.u64(keys) >> 20) == field).sum())
    assert int(((hw.u64(out) >> 20) == field).sum()) == 700 and changed.numel() == 700 - was
    assert bool((changed % step != 0).all()), "a sampled position was changed"
    assert torch.equal(hw.u64(out[changed]) & 0xFFFFF, hw.u64(keys[changed]) & 0xFFFFF), "the low bits are the keys' own"
    assert not bool(((hw.u64(keys[changed]) >> 20) == field).any())
    assert torch.equal(hw.with_exact_count(out, 20, field, 700, avoid_step=step), out)
    with pytest.raises(ValueError):
        hw.with_exact_count(out, 20, field, 699, avoid_step=step)


def test_expected_words_follow_the_rules():
    """expected_words on inputs small enough to count by hand is not possible (the form starts at 3.8e7 keys); its pieces are: the
    fold and the sample above, and the key maps here"""
    import torch

    bits = torch.tensor([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0x7F800000, 0xFF800000, 0x7FC00001, 0xFFC00001, 0x3F800000])
    for (key_type, descending), xf in hw.TRANSFORMS.items():
        t = hw.to_sortable(bits, xf)
        assert torch.equal(hw.from_sortable(t, xf), bits) and int(t.min()) >= 0 and int(t.max()) < 1 << 32
        if key_type == "int32":
            signed = torch.where(bits >= 1 << 31, bits - (1 << 32), bits)
            order = torch.argsort(signed, descending=descending, stable=True)
            assert torch.equal(torch.argsort(t, stable=True), order), (key_type, descending)
    f = hw.to_sortable(bits, hw.TRANSFORMS[("float32", False)])
    # IEEE total order: -NaN < -inf < -0 < +0 < 1 < +inf < +NaN
    rank = {int(b): int(v) for b, v in zip(bits, f)}
    chain = [0xFFC00001, 0xFF800000, 0x80000000, 0, 1, 0x3F800000, 0x7F800000, 0x7FC00001]
    assert [rank[b] for b in chain] == sorted(rank[b] for b in chain)
