"""CPU suite: the workspace query and the ABI of the hybrid form's half variant (half_hop.hip).

The variant keeps its arrays BEHIND a sort's plain workspace, so every plain size stays what tests/test_workspace_sizes.py has
recorded and only the new query grows: where the variant can be attempted (8-bit digits, the sizes sorted in 2^15 buckets) by
2 n bytes of halves, 65536 words of group counts and 32768 words of bucket splits; everywhere else by nothing.
"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N0 = 158_056_448   # the first n that lsd_kernels.hpp's hybrid_bucket_bits gives 15 bucket bits (keys)
EXTRA_WORDS = 65536 + 32768


def _bucket_bits(n):
    """hybrid_bucket_bits(n, false) of lsd_kernels.hpp, restated."""
    def root_up(x):
        r = 1
        while r * r < x:
            r += 1
        return r

    if (n >> 14) + 6 * root_up(n >> 14) <= 10240:
        return 14
    return 15 if 2 * (n >> 15) + 3 * root_up(n >> 15) <= 2 * 10240 else 16


def test_the_window_starts_where_the_tests_say():
    assert _bucket_bits(N0) == 15 and _bucket_bits(N0 - 1) == 14
    assert _bucket_bits(1 << 28) == 15 and _bucket_bits(330_000_000) == 15 and _bucket_bits(400_000_000) == 16


def test_roomy_query_where_the_form_applies():
    from lsdradixsort_amd import lib

    L = lib()
    L.lsdsort_set_tile_config(8, -1)
    for n in (N0, N0 + 12345, 1 << 28, (1 << 28) + 777, 300_000_000, 330_000_000):
        assert _bucket_bits(n) == 15
        plain = L.lsdsort_workspace_bytes(n, 8, 0)
        roomy = L.lsdsort_workspace_bytes_roomy(n, 8)
        assert plain > 0 and roomy >= plain + 2 * n + 4 * EXTRA_WORDS, (n, plain, roomy)
        assert roomy % 256 == 0
        assert roomy - plain < 2 * n + 4 * EXTRA_WORDS + 4 * 256, "no more than the three arrays, each 256-byte aligned"


def test_roomy_query_equals_the_plain_one_everywhere_else():
    from lsdradixsort_amd import errors, lib

    L = lib()
    for radix in range(1, 9):
        L.lsdsort_set_tile_config(radix, -1)
    sizes = (0, 1, 4095, 1 << 19, 1 << 23, (1 << 24) + 5, 1 << 27, N0 - 1, 400_000_000, 1 << 29, errors.LSDSORT_MAX_KEYS)
    for n in sizes:
        for radix in (1, 2, 4, 8):
            assert L.lsdsort_workspace_bytes_roomy(n, radix) == L.lsdsort_workspace_bytes(n, radix, 0), (n, radix)
    for n in (N0, 1 << 28):          # inside the window, other digit widths
        for radix in (1, 2, 4):
            assert L.lsdsort_workspace_bytes_roomy(n, radix) == L.lsdsort_workspace_bytes(n, radix, 0), (n, radix)
    assert L.lsdsort_workspace_bytes_roomy(1 << 20, 7) == 0
    assert L.lsdsort_workspace_bytes_roomy(errors.LSDSORT_MAX_KEYS + 1, 8) == 0
    # another tile shape has no half-writing pass: the plain size
    assert L.lsdsort_set_tile_config(8, 0) == errors.LSDSORT_OK
    try:
        assert L.lsdsort_workspace_bytes_roomy(1 << 28, 8) == L.lsdsort_workspace_bytes(1 << 28, 8, 0)
    finally:
        L.lsdsort_set_tile_config(8, -1)


def test_python_workspace_sizes_follow_the_queries():
    import lsdradixsort_amd as lsd
    from lsdradixsort_amd import errors

    L = lsd.lib()
    L.lsdsort_set_tile_config(8, -1)
    for n in (1 << 20, 1 << 27, N0, 1 << 28):
        assert lsd.workspace_bytes(n, 8) == L.lsdsort_workspace_bytes_roomy(n, 8)
        assert lsd.workspace_bytes(n, 8, True) == L.lsdsort_workspace_bytes(n, 8, 1)
        assert lsd.workspace_bytes(n, 8, 2) == L.lsdsort_workspace_bytes(n, 8, 2)
        assert lsd.workspace_bytes(n, 4) == L.lsdsort_workspace_bytes(n, 4, 0)
        assert lsd.workspace_bytes(n, 8, False, errors.LSDSORT_ALGO_STAGED) == L.lsdsort_workspace_bytes_ex(n, 8, 0, errors.LSDSORT_ALGO_STAGED)


def test_abi_triple_is_consistent():
    """Header, exports and ctypes table name the same new entries, with the argument counts the header declares."""
    from lsdradixsort_amd import _lib

    text = open(os.path.join(ROOT, "include", "lsdsort.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = _lib.lib()
    for name, nargs in (("lsdsort_workspace_bytes_roomy", 2), ("lsdsort_set_half_hop", 1), ("lsdsort_workspace_half", 3),
                        ("lsdsort_local_sort_halves_u32_device", 8)):
        m = re.search(r"LSDSORT_API\s+[\w\s\*]+?\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert m, f"{name} is not declared in include/lsdsort.h"
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))
        assert hasattr(L, name), f"liblsdsort.so does not export {name}"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name


def test_switch_and_readback_validate_without_a_device():
    from lsdradixsort_amd import errors, lib

    L = lib()
    assert L.lsdsort_set_half_hop(0) == errors.LSDSORT_OK
    assert L.lsdsort_set_half_hop(1) == errors.LSDSORT_OK
    assert L.lsdsort_workspace_half(None, None, None) == errors.LSDSORT_ERR_INVALID_ARG
    assert L.lsdsort_local_sort_halves_u32_device(None, None, None, None, 0, None, None, None) == errors.LSDSORT_OK   # nothing to do
    assert L.lsdsort_local_sort_halves_u32_device(None, None, None, None, 4, None, None, None) == errors.LSDSORT_ERR_INVALID_ARG
    assert L.lsdsort_local_sort_halves_u32_device(None, None, None, None, 65537, None, None, None) == errors.LSDSORT_ERR_INVALID_ARG
