"""CPU suite: every workspace size the library reports is pinned, byte for byte.

tests/test_abi.py checks bounds and monotonicity only.  The sizes here were recorded from the build before the host layer was
reorganised (tests/golden/workspace_sizes.json), so that a change to a layout's carve-up shows as a changed figure and not as
a caller's buffer that is suddenly too small.  A pull request that moves a layout on purpose records the file again
(`python tests/test_workspace_sizes.py`) and says so.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "workspace_sizes.json")


def _cases():
    from lsdradixsort_amd import errors

    sort_n = (0, 1, 4095, (1 << 19) - 1, 1 << 19, 1 << 21, 1 << 23, (1 << 24) + 5, 1 << 28, errors.LSDSORT_MAX_KEYS)
    cases = []
    for n in sort_n:
        for radix in (1, 2, 4, 8):
            for payloads in (0, 1, 2, 3):
                for algorithm in (errors.LSDSORT_ALGO_ONESWEEP, errors.LSDSORT_ALGO_STAGED):
                    cases.append(("lsdsort_workspace_bytes_ex", [n, radix, payloads, algorithm]))
    for n in sort_n:
        for msb_bits in range(5):
            cases.append(("lsdsort_msb_partition_workspace_bytes", [n, msb_bits]))
    for n in (0, 1, 4095, 1 << 19, (1 << 24) + 5, 1 << 28):
        for radix in (4, 8):
            for key_bits, val_bits in ((64, 0), (64, 32), (64, 64), (32, 64)):
                cases.append(("lsdsort_wide_workspace_bytes", [n, radix, key_bits, val_bits]))
    for n, segs in ((0, 0), (1, 1), (1000, 7), (1 << 20, 1), (1 << 20, 4096), (1 << 20, 1 << 20), ((1 << 24) + 5, 12345),
                    (1 << 28, 64), (errors.LSDSORT_MAX_KEYS, errors.LSDSORT_MAX_KEYS)):
        for pairs in (0, 1):
            cases.append(("lsdsort_segmented_workspace_bytes", [n, segs, pairs]))
    for rows, cols, k in ((0, 0, 0), (1, 1, 1), (1, 1000, 10), (64, 1 << 22, 100), (4096, 4096, 1), (4096, 4096, 4000),
                          (1 << 20, 256, 8), (8, 1 << 25, 1 << 24), (1000, 50000, 2048)):
        cases.append(("lsdsort_topk_workspace_bytes", [rows, cols, k]))
    return cases


def _measure():
    from lsdradixsort_amd import lib

    L = lib()
    for radix in range(1, 9):   # another test's pinned tile shape would change the status rows
        L.lsdsort_set_tile_config(radix, -1)
    return [[name, args, int(getattr(L, name)(*args))] for name, args in _cases()]


def test_workspace_sizes_match_the_recorded_ones():
    with open(GOLDEN) as f:
        recorded = json.load(f)
    measured = _measure()
    assert [r[:2] for r in recorded] == [m[:2] for m in measured], "the golden file's cases are not this test's"
    assert sum(1 for r in recorded if r[2] > 0) > 400, "the golden file holds refusals, not sizes"
    moved = [(m[0], m[1], r[2], m[2]) for r, m in zip(recorded, measured) if r[2] != m[2]]
    assert not moved, f"{len(moved)} workspace sizes moved (function, arguments, recorded, now): {moved[:8]}"


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    with open(GOLDEN, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(row) for row in _measure()) + "\n]\n")
    print(f"recorded {len(_cases())} sizes into {GOLDEN}")
