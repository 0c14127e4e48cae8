"""CPU suite: the oracle of the bit-exact GPU suites (tests/_key_oracle.py) against an independent statement of the order, and the
rule that the test helpers live once.

The map is held to the order written down here in other terms -- uint by value, int by two's-complement value, the float types by
the sign-magnitude integer (mag for a clear sign bit, -1 - mag for a set one) -- and, on the patterns that are numbers, to numpy's
own float comparison.  The stable row order is held to the per-row np.lexsort((positions, sortable)), the spelling half of the
suites used before they shared one.  16 bits: every pattern.  32 bits: the specials, their neighbours and 2^20 seeded patterns."""
import ast
import glob
import os
import re

import numpy as np
import pytest

import _key_oracle as ko

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL16 = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)


def patterns32():
    rng = np.random.default_rng(32)
    s = ko.SPECIALS32
    return np.unique(np.concatenate([s, s + np.uint32(1), s - np.uint32(1), rng.integers(0, 1 << 32, 1 << 20, dtype=np.uint64).astype(np.uint32)]))


def order_key(u, key_type):
    """int64 whose order is the key type's ascending order, stated without the map"""
    bits = 16 if key_type in ko.KEY_TYPES16 else 32
    u = u.astype(np.int64)
    if key_type.startswith("uint"):
        return u
    if key_type.startswith("int"):
        return np.where(u >> (bits - 1), u - (1 << bits), u)
    mag = u & ((1 << (bits - 1)) - 1)
    return np.where(u >> (bits - 1), -1 - mag, mag)


def numbers(u, key_type):
    """the patterns as floats numpy can compare"""
    if key_type == "float16":
        return u.view(np.float16)
    if key_type == "bfloat16":
        return (u.astype(np.uint32) << np.uint32(16)).view(np.float32)
    return u.view(np.float32)


CASES = [(t, ALL16, ko.sortable16_np, ko.from_sortable16_np, np.uint16) for t in ko.KEY_TYPES16] + \
        [(t, patterns32(), ko.sortable_np, ko.from_sortable_np, np.uint32) for t in ko.KEY_TYPES32]


@pytest.mark.parametrize("key_type,u,sortable,inverse,word", CASES, ids=[c[0] for c in CASES])
def test_map_is_the_order_of_the_key_type(key_type, u, sortable, inverse, word):
    up, down = sortable(u, key_type, False), sortable(u, key_type, True)
    assert up.dtype == word and down.dtype == word and up.shape == u.shape
    # a bijection: distinct keys keep distinct sortable values (on 16 bits: all 65536 of them)
    assert np.unique(up).size == u.size and np.unique(down).size == u.size
    # the order of the independent statement
    by_key = np.argsort(order_key(u, key_type), kind="stable")
    assert (np.diff(up[by_key].astype(np.int64)) > 0).all(), "ascending"
    assert (np.diff(down[by_key].astype(np.int64)) < 0).all(), "descending"
    assert np.array_equal(np.argsort(down, kind="stable"), np.argsort(up, kind="stable")[::-1]), "descending is ascending reversed"
    # the inverse undoes the map, in either direction
    assert np.array_equal(inverse(up, key_type), u) and np.array_equal(inverse(~down, key_type), u)
    assert inverse(up, key_type).dtype == word
    if "float" in key_type:
        in_order = u[np.argsort(up, kind="stable")]
        values = numbers(in_order, key_type)
        real = ~np.isnan(values)
        assert real.sum() > 0.9 * u.size and (np.diff(values[real].astype(np.float64)) >= 0).all(), "numerically non-decreasing"
        sign = np.uint32(1) << np.uint32(8 * u.itemsize - 1)
        at = np.flatnonzero(in_order == 0)[0]
        assert in_order[at - 1] == sign, "-0 comes right before +0"
        nan_at = np.flatnonzero(~real)   # NaNs by sign at the two ends, nothing between them and the infinities
        assert (in_order[nan_at[nan_at < at]] & sign).all() and not (in_order[nan_at[nan_at > at]] & sign).any()
        assert np.isneginf(values[real][0]) and np.isposinf(values[real][-1])


@pytest.mark.parametrize("key_type", list(ko.KEY_TYPES16) + list(ko.KEY_TYPES32))
def test_stable_row_order_is_the_lexsort_by_position(key_type):
    """tie-heavy rows: the values 0..7 under a random sign bit, so every row holds long runs of equal keys"""
    wide = key_type in ko.KEY_TYPES32
    word, top = (np.uint32, 31) if wide else (np.uint16, 15)
    rng = np.random.default_rng(7)
    rows, cols = 5, 397
    keys = (rng.integers(0, 8, (rows, cols)) | (rng.integers(0, 2, (rows, cols)) << top)).astype(word)
    sortable = ko.sortable_np if wide else ko.sortable16_np
    for largest in (False, True):
        ek, ei = ko.expected_np(keys, key_type, largest)
        assert ek.dtype == word and ei.dtype == np.uint32 and ek.shape == ei.shape == keys.shape
        s = sortable(keys, key_type, largest)
        for r in range(rows):
            order = np.lexsort((np.arange(cols), s[r]))
            assert np.array_equal(ei[r], order), (key_type, largest, r)
            assert np.array_equal(ek[r], keys[r][order]), (key_type, largest, r)


def test_specials_tables_hold_every_pattern_a_suite_ever_had():
    f16 = [0x0000, 0x8000, 0x7C00, 0xFC00, 0x7E00, 0xFE00, 0x7C01, 0xFC01, 0xFFFF, 0x7FFF, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x7BFF, 0xFBFF,
           0x3C00, 0xBC00]
    # the same 18 classes: +-0, +-inf, +-quiet NaN, +-signalling NaN, all ones, 0x7FFF, +-least and +-largest denormal, +-largest finite, +-1
    bf16 = [0x0000, 0x8000, 0x7F80, 0xFF80, 0x7FC0, 0xFFC0, 0x7F81, 0xFF81, 0xFFFF, 0x7FFF, 0x0001, 0x8001, 0x007F, 0x807F, 0x7F7F, 0xFF7F,
            0x3F80, 0xBF80]
    f32 = [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x7FC00000, 0xFFC00000,
           0x7F800001, 0xFFFFFFFF, 0x7FFFFFFF, 0x3F800000, 0xBF800000]
    assert set(ko.SPECIALS16) == {"float16", "bfloat16"}
    for table, want, word in ((ko.SPECIALS16["float16"], f16, np.uint16), (ko.SPECIALS16["bfloat16"], bf16, np.uint16), (ko.SPECIALS32, f32, np.uint32)):
        assert table.dtype == word and set(want) <= set(table.tolist()) and len(set(table.tolist())) == table.size
    for table, key_type in ((f16, "float16"), (bf16, "bfloat16")):   # the patterns that have a plain value do mean it
        values = numbers(np.array(table[:4] + table[-2:], dtype=np.uint16), key_type).astype(np.float64)
        assert values.tolist() == [0.0, -0.0, np.inf, -np.inf, 1.0, -1.0] and np.signbit(values[1])


def test_key_type_codes_are_the_headers():
    text = open(os.path.join(ROOT, "include", "lsdsort.h")).read()
    codes = {name: int(value) for name, value in re.findall(r"\b(LSDSORT_KEY(?:16)?_[A-Z]+\d+)\s*=\s*(\d+)", text)}
    names = {"uint": "U", "int": "I", "float": "F", "bfloat": "BF"}
    for table, prefix in ((ko.KEY_TYPES16, "LSDSORT_KEY16_"), (ko.KEY_TYPES32, "LSDSORT_KEY_"), (ko.KEY_TYPES64, "LSDSORT_KEY_")):
        for key_type, code in table.items():
            kind, bits = re.fullmatch(r"([a-z]+)(\d+)", key_type).groups()
            assert codes[prefix + names[kind] + bits] == code, key_type
    assert (ko.ALL_TYPES16, ko.ALL_TYPES32, ko.ALL_TYPES64) == (list(ko.KEY_TYPES16), list(ko.KEY_TYPES32), list(ko.KEY_TYPES64))


def test_input_families_keep_their_names_and_draws():
    """a family left out draws nothing, so a suite that picks by name sees the arrays its own copy of the function made"""
    for inputs, families, multi, key_type in ((ko.inputs16, ko.FAMILIES16, ko.MULTI_RANK16, "bfloat16"), (ko.inputs32, ko.FAMILIES32, ko.MULTI_RANK32, "float32")):
        assert list(inputs(3, 40, key_type, 5)) == list(families) and list(inputs(3, 40, key_type, 5, multi)) == list(multi)
        assert list(inputs(3, 7, key_type, 5, multi)) == list(multi[:-1]), "outliers need 8 columns"
        assert "float specials" not in inputs(3, 40, key_type.replace("bfloat", "int").replace("float", "int"), 5)
        first = inputs(3, 40, key_type, 5, families[:2])
        assert all(np.array_equal(first[name], inputs(3, 40, key_type, 5)[name]) for name in families[:2])


# ---- one definition each ------------------------------------------------------------------------------------------------------------
# helper module -> the names it alone defines at top level, over all of tests/*.py
HOME = {
    "_key_oracle.py": ("KEY_TYPES16", "KEY_TYPES32", "KEY_TYPES64", "ALL_TYPES16", "ALL_TYPES32", "ALL_TYPES64", "SPECIALS16", "SPECIALS32",
                       "sortable16_np", "sortable_np", "from_sortable16_np", "from_sortable_np", "expected_np", "inputs16", "inputs32",
                       "make_keys16", "make_keys32"),
    "_device_arrays.py": ("DTYPES", "to_dev", "bits", "stream_ptr", "fault_word", "assert_equal", "captured"),
    "_faces.py": ("lib", "no_library", "FakeCuda"),
    "_kernel_resources.py": ("sources", "code", "defined_in", "includes"),
}
# The spellings that were copied from suite to suite before the helpers had a width or a module in their name.  Each may still
# name one thing of one module's own (the filter's inputs in _rowk16.py, the segmented sort's make_keys in _seg_plan.py, the six
# wide key types in _unique.py); a second definition anywhere is a copy again.
ONCE_AT_MOST = ("_lib", "SPECIALS", "KEY_TYPES", "ALL_TYPES", "inputs", "make_keys")


def top_level_definitions():
    """{name: [files of tests/*.py that define it at top level]}: def, class, assignment (imports are not definitions)"""
    found = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "*.py"))):
        for node in ast.parse(open(path).read()).body:
            names = []
            if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)):
                names = [node.name]
            elif isinstance(node, (ast.Assign, ast.AnnAssign, ast.AugAssign)):
                targets = node.targets if isinstance(node, ast.Assign) else [node.target]
                names = [n.id for t in targets for n in ast.walk(t) if isinstance(n, ast.Name)]
            for name in names:
                found.setdefault(name, []).append(os.path.basename(path))
    return found


def test_every_shared_helper_is_defined_once():
    found = top_level_definitions()
    for home, names in HOME.items():
        for name in names:
            assert found.get(name) == [home], f"{name} is defined in {found.get(name)}"
    for name in ONCE_AT_MOST:
        assert len(found.get(name, [])) <= 1, f"{name} is defined in {found[name]}"
