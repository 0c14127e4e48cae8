"""CPU suite: the helper of the replay-and-reuse matrix (tests/_replay.py) against numpy -- the families hold what they advertise at
every size of the matrix, the oracles are np.sort / np.unique / the stable argsort, and the list of cells names every entry."""
import os
import re

import numpy as np
import pytest

import _replay as rp
import _unique as un
from _unique import KEY_TYPES


def test_constants_are_the_sources():
    have = rp.host_constants()
    assert have["kAlign"] == rp.ALIGN and have["kCtlBytes"] == rp.ALIGN
    assert have["small_sort_cap"] == rp.SMALL_SORT_CAP and rp.N_CHAINED == rp.SMALL_SORT_CAP + 1
    assert rp.N2 == un.TILE + 1 and rp.N3 == 2 * un.TILE + 1 and rp.N3 in un.SIZES
    assert rp.unique_sort_offset(rp.N3, 32, True) == 256 + 2 * 33024 and rp.unique_sort_offset(rp.N3, 64, False) == 256 + 65792


@pytest.mark.parametrize("n", rp.SIZES)
def test_families_hold_the_advertised_number_of_distinct_values(n):
    assert [name for name, _ in rp.RUNS] == ["alternating", "random8", "all_distinct", "all_equal", "random8"]
    for key_type in KEY_TYPES:
        w = un.width_of(key_type)
        for run, (name, seed) in enumerate(rp.RUNS):
            bits = rp.keys(n, key_type, run)
            assert bits.size == n and bits.dtype == un.word(w) and not bits.flags.writeable
            want = rp.DISTINCT[name] or n
            assert np.unique(bits).size == want, (n, key_type, name)
            assert not (bits == un.word(w)(rp.SENT[w])).any()
        # the second random8 is another draw of the same eight values; the run in front of every run is another family
        assert not np.array_equal(rp.keys(n, key_type, 1), rp.keys(n, key_type, 4))
        assert np.array_equal(np.unique(rp.keys(n, key_type, 1)), np.unique(rp.keys(n, key_type, 4)))
        assert np.array_equal(rp.keys(n, key_type, 1), un.families(n, w)["random8"])
    # alternating is unsorted in every order, so the warm-up moves keys
    for key_type in KEY_TYPES:
        a = un.sortable(rp.keys(n, key_type, 0), key_type)
        assert (a[1:] < a[:-1]).any() and (a[1:] > a[:-1]).any()


@pytest.mark.parametrize("n", rp.SIZES)
def test_float_runs_hold_both_zeros_and_nans_of_both_signs(n):
    f = rp.keys(n, "float32", 2)
    assert (f == 0x00000000).any() and (f == 0x80000000).any()
    nan = np.isnan(f.view(np.float32))
    assert (nan & (f >> np.uint32(31) == 0)).sum() >= 3 and (nan & (f >> np.uint32(31) == 1)).sum() >= 3
    d = rp.keys(n, "float64", 2)
    assert (d == 0).any() and (d == np.uint64(1 << 63)).any()
    nan = np.isnan(d.view(np.float64))
    assert (nan & (d >> np.uint64(63) == 0)).any() and (nan & (d >> np.uint64(63) == 1)).any()
    # the integer types take the family as it is
    assert np.array_equal(rp.keys(n, "int32", 2), un.families(n, 32)["all_distinct"])


def test_payloads_share_no_word_between_runs_or_arrays():
    n = rp.N_PARITY
    seen = np.concatenate([rp.payload(n, run, k) for run in range(len(rp.RUNS)) for k in range(3)])
    assert np.unique(seen).size == seen.size
    assert np.array_equal(rp.payload(n, 2, 1) - rp.payload(n, 2, 1)[0], np.arange(n, dtype=np.uint32))


@pytest.mark.parametrize("n", [rp.N2, rp.N3])
def test_sort_oracle_is_numpy_sort_and_stable(n):
    for key_type in KEY_TYPES:
        w = un.width_of(key_type)
        for run in range(len(rp.RUNS)):
            bits = rp.keys(n, key_type, run)
            pay = rp.payload(n, run)
            for descending in (False, True):
                got, (got_pay,) = rp.oracle_sort(bits, key_type, descending, [pay])
                assert np.array_equal(np.sort(got), np.sort(bits))
                order = got_pay - pay[0]
                assert np.array_equal(bits[order], got) and np.array_equal(order, np.argsort(un.sortable(bits, key_type, descending), kind="stable"))
                # ties keep their input order: within equal keys the positions ascend
                tie = got[1:] == got[:-1]
                assert (order[1:][tie] > order[:-1][tie]).all()
                if key_type.startswith("uint"):
                    assert np.array_equal(got, np.sort(bits)[::-1] if descending else np.sort(bits))
                elif key_type.startswith("int"):
                    want = np.sort(bits.view(np.int32 if w == 32 else np.int64))
                    assert np.array_equal(got.view(want.dtype), want[::-1] if descending else want)
                else:
                    f = got.view(np.float32 if w == 32 else np.float64)
                    f = f[~np.isnan(f)]
                    assert (np.diff(f) <= 0).all() if descending else (np.diff(f) >= 0).all()
            # and the unique oracle over the same keys is np.unique
            want = un.oracle_unique(bits, "uint%d" % w, False)
            keys, index, inverse, counts = np.unique(bits, return_index=True, return_inverse=True, return_counts=True)
            assert np.array_equal(want["keys"], keys) and np.array_equal(want["counts"], counts) and np.array_equal(want["first"], index)
            assert np.array_equal(want["inverse"], inverse.reshape(-1))


def test_histogram_and_partition_oracles():
    n = rp.N3
    for run in range(len(rp.RUNS)):
        bits = rp.keys(n, "uint32", run)
        hist = rp.oracle_histograms(bits, 8)
        assert hist.shape == (4, 256) and (hist.sum(axis=1) == n).all()
        by_bytes = bits.view(np.uint8).reshape(n, 4)   # little endian: digit g is byte g
        for g in range(4):
            assert np.array_equal(hist[g], np.bincount(by_bytes[:, g], minlength=256))
        for b in (0, 1, 3):
            out, counts = rp.oracle_partition(bits, rp.msb_buckets(bits, b), 1 << b)
            assert counts.dtype == np.uint64 and int(counts.sum()) == n and counts.size == 1 << b
            assert np.array_equal(np.sort(out), np.sort(bits)) and (np.diff(rp.msb_buckets(out, b)) >= 0).all()
            values = rp.splitters(n, b)
            assert len(values) == (1 << b) - 1 and list(values) == sorted(values)
            bucket = rp.splitter_buckets(bits, values)
            assert np.array_equal(bucket, sum((bits >= np.uint32(v)).astype(np.int64) for v in values) if values else np.zeros(n, dtype=np.int64))
            out, counts = rp.oracle_partition(bits, bucket, 1 << b)
            assert int(counts.sum()) == n and (np.diff(rp.splitter_buckets(out, values)) >= 0).all()
    # keys equal to a splitter occur in the all-distinct run, and go to the bucket above it
    values = rp.splitters(n, 3)
    bits = rp.keys(n, "uint32", 2)
    assert all((bits == np.uint32(v)).sum() == 1 for v in values)
    assert (rp.oracle_partition(bits, rp.splitter_buckets(bits, values), 8)[1] > 0).all()


def test_no_clear_of_the_library_is_a_memset_node():
    """Every clear on a path a caller may capture is lsd::launch_clear or a unit's own clear kernel.  The one hipMemsetAsync left is
    the hardware probe's (rank_scatter.hip), which allocates and synchronises and is kept out of a capture by lsdsort_prepare_device."""
    csrc = os.path.join(un.ROOT, "lsdradixsort_amd", "csrc")
    calls = {}
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".hip", ".hpp")):
            code = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, name)).read())
            count = len(re.findall(r"\bhipMemset\w*\s*\(", code))
            if count:
                calls[name] = count
    assert calls == {"rank_scatter.hip": 1}, calls
    api = open(rp.API).read()
    assert api.count("lsd::launch_clear(") == 3   # the sort's opening clear, the histogram entry's table, the partitions' opening clear


def test_every_entry_has_a_row_and_every_row_is_in_the_list():
    assert rp.ENTRIES == (
        "lsdsort_keys_device",
        "lsdsort_u32_device",
        "lsdsort_pairs_u32_device",
        "lsdsort_multi_u32_device",
        "lsdsort_keys64_device",
        "lsdsort_unique_device",
        "lsdsort_digit_histograms_u32_device",
        "lsdsort_msb_partition_u32_device",
        "lsdsort_splitter_partition_u32_device",
    )
    assert {cell["entry"] for cell in rp.CELLS} == set(rp.ENTRIES)
    assert not set(rp.ENTRIES) & set(rp.REACHED_THROUGH)
    exported = set(re.findall(r"\b(lsdsort_\w+)\(", open(un.ROOT + "/include/lsdsort.h").read()))
    assert set(rp.ENTRIES) | set(rp.REACHED_THROUGH) <= exported
    ids = [rp.cell_id(cell) for cell in rp.CELLS]
    assert len(set(ids)) == len(ids)
    # the cells the issue of this matrix names
    have = {(c["entry"], c["n"]) for c in rp.CELLS}
    assert {("lsdsort_keys_device", rp.N3), ("lsdsort_keys_device", rp.N2), ("lsdsort_keys_device", rp.N_PARITY),
            ("lsdsort_u32_device", rp.N_CHAINED), ("lsdsort_pairs_u32_device", rp.N_CHAINED), ("lsdsort_multi_u32_device", rp.N3),
            ("lsdsort_keys64_device", rp.N3), ("lsdsort_unique_device", rp.N3)} <= have
    typed = [c for c in rp.CELLS if c["entry"] == "lsdsort_keys_device" and c["n"] != rp.N_PARITY]
    assert len(typed) == 2 * 2 * 2 * 2
    assert {c["small"] for c in rp.CELLS if c["entry"] == "lsdsort_u32_device" and c["n"] == rp.N3} == {False, True}
    assert {(c["key_type"], c["descending"], c["val_bits"]) for c in rp.CELLS if c["entry"] == "lsdsort_keys64_device"} == \
        {("float64", True, 0), ("float64", True, 32), ("int64", False, 0), ("int64", False, 32)}
    assert sorted(c.get("msb_bits", c.get("log2_buckets")) for c in rp.CELLS if "partition" in c["entry"]) == [0, 0, 1, 1, 3, 3]
    assert any(c["entry"] == "lsdsort_unique_device" and "first" not in c["outputs"] and "inverse" not in c["outputs"] for c in rp.CELLS)
    assert rp.MODES == ("eager", "graph")
