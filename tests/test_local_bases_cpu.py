"""CPU suite: the packed arithmetic of the local stage's counts_to_bases (local_sort.hip), as a numpy model against the plain one.

The kernel keeps eight waves' 16-bit digit counters two to a 32-bit word (digits 2j and 2j + 1).  One thread per word reads the eight
waves' words whole, keeps the running sum over the waves PACKED (both halves in one add), scans low + high across the threads, and
writes back  running sum + (off | (off + low) << 16)  -- the base of wave w inside digit d's range of the bucket.  The plain
arithmetic does the same one digit and one 16-bit counter at a time.  The model below runs the packed form in uint32 with
wrap-around, as the device does, so a carry from a low half into a high one would show as a wrong base; the test also asserts that
no intermediate field reaches 2^16.  Every field is at most the bucket's size, 16384 at the largest.
"""
import numpy as np
import pytest

WAVES = 8
CAP = 16384        # the largest bucket, segment or one-launch sort
WAVE_CAP = 2048    # a wave's share of it: 32 rows of 64


def plain_bases(counts):
    """counts[w][d] -> base[w][d] = (keys of digits below d) + (keys of digit d in the waves before w)."""
    counts = counts.astype(np.int64)
    totals = counts.sum(axis=0)
    digit_base = np.cumsum(totals) - totals
    wave_excl = np.cumsum(counts, axis=0) - counts
    return digit_base[None, :] + wave_excl


def packed_bases(counts):
    """The same through counter words, in uint32 arithmetic; returns (base[w][d], the largest field seen on the way)."""
    waves, bins = counts.shape
    assert bins % 2 == 0
    c = counts.astype(np.uint32)
    words = c[:, 0::2] | (c[:, 1::2] << np.uint32(16))                    # [w][j]
    run = np.zeros_like(words)
    total = np.zeros(bins // 2, dtype=np.uint32)
    seen = 0
    for w in range(waves):                                                # one thread per word j: the running sums stay packed
        run[w] = total
        total = total + words[w]
        seen = max(seen, int((total & np.uint32(0xFFFF)).max()), int((total >> np.uint32(16)).max()))
    low = total & np.uint32(0xFFFF)
    v = low + (total >> np.uint32(16))
    off = (np.cumsum(v, dtype=np.uint32) - v).astype(np.uint32)           # the exclusive scan across the threads
    add = off | ((off + low) << np.uint32(16))
    out = run + add[None, :]                                              # one packed add per wave
    seen = max(seen, int((out & np.uint32(0xFFFF)).max()), int((out >> np.uint32(16)).max()))
    base = np.empty((waves, bins), dtype=np.int64)
    base[:, 0::2] = out & np.uint32(0xFFFF)
    base[:, 1::2] = out >> np.uint32(16)
    return base, seen


def check(counts):
    assert counts.sum() <= CAP and counts.sum(axis=1).max() <= WAVE_CAP
    got, seen = packed_bases(counts)
    assert seen < 1 << 16, "a field reached 2^16"
    assert np.array_equal(got, plain_bases(counts))


@pytest.mark.parametrize("bins", [2, 4, 32, 256, 512])
@pytest.mark.parametrize("digit", ["first", "last", "odd"])
def test_the_whole_bucket_in_one_field(bins, digit):
    """16384 keys of one digit: the low field of word 0, the high field of the last word, a high field whose low neighbour is empty.
    The digit behind it starts at base 16384."""
    d = {"first": 0, "last": bins - 1, "odd": 1}[digit]
    counts = np.zeros((WAVES, bins), dtype=np.int64)
    counts[:, d] = WAVE_CAP
    check(counts)
    got, _ = packed_bases(counts)
    assert got[WAVES - 1, d] == CAP - WAVE_CAP
    if d + 1 < bins:
        assert (got[:, d + 1:] == CAP).all()


@pytest.mark.parametrize("bins", [2, 8, 256, 512])
@pytest.mark.parametrize("pair", ["first", "last"])
def test_both_halves_of_one_word_near_their_maxima(bins, pair):
    """8192 + 8192 in one word: its sum, 16384, lies in the high field's base and in every base behind it."""
    j = 0 if pair == "first" else bins // 2 - 1
    counts = np.zeros((WAVES, bins), dtype=np.int64)
    counts[:, 2 * j] = counts[:, 2 * j + 1] = WAVE_CAP // 2
    check(counts)


def test_uneven_waves():
    """A bucket whose rows run out: the last waves hold fewer keys or none (the padding rows count nothing)."""
    rng = np.random.default_rng(3)
    for size in (1, 2, 63, 64, 65, 511, 512, 513, 8191, 8192, 8193, 10240, 16383, 16384):
        rows = -(-size // 512)
        counts = np.zeros((WAVES, 512), dtype=np.int64)
        for w in range(WAVES):
            held = min(max(size - w * rows * 64, 0), rows * 64)
            np.add.at(counts[w], rng.integers(0, 512, held), 1)
        check(counts)


@pytest.mark.parametrize("width", range(1, 10))
def test_random_splits_over_eight_waves(width):
    rng = np.random.default_rng(width)
    bins = 1 << width
    for trial in range(20):
        counts = np.zeros((WAVES, bins), dtype=np.int64)
        for w in range(WAVES):
            held = int(rng.integers(0, WAVE_CAP + 1))
            if trial % 4 == 0:      # uniform digits
                digits = rng.integers(0, bins, held)
            elif trial % 4 == 1:    # a few hot digits, neighbours among them
                hot = rng.integers(0, bins, 3)
                digits = np.concatenate([hot, hot ^ 1])[rng.integers(0, 6, held)]
            elif trial % 4 == 2:    # one digit per wave
                digits = np.full(held, int(rng.integers(0, bins)))
            else:                   # the two ends of the table
                digits = np.where(rng.integers(0, 2, held) == 0, 0, bins - 1)
            np.add.at(counts[w], digits, 1)
        check(counts)
