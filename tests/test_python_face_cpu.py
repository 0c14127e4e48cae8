"""CPU suite: the Python package against include/lsdsort.h and against itself -- the header's numbers, the list of public names,
no torch at import, and the argument errors every wrapper raises before the library is touched."""
import ast
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    text = open(os.path.join(ROOT, "include", "lsdsort.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _enum(name):
    """{enumerator: value} of ``typedef enum <name> { ... } <name>;``."""
    body = re.search(r"typedef\s+enum\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), _header(), flags=re.S).group(1)
    pairs = re.findall(r"(LSDSORT_\w+)\s*=\s*(-?\d+)", body)
    assert len(pairs) == len([item for item in body.split(",") if item.strip()]), f"{name}: an enumerator without a value"
    return {k: int(v) for k, v in pairs}


def _define(name):
    value = re.search(r"#define\s+%s\s+(.+)" % name, _header()).group(1)
    return int(re.search(r"0x[0-9a-fA-F]+|\d+", re.sub(r"\(\s*size_t\s*\)", "", value)).group(0), 0)


def test_header_numbers_match_the_python_constants():
    from lsdradixsort_amd import _lib, errors
    from lsdradixsort_amd.dist import LoopbackWorld, ShardedSorter

    sizes = {"lsdsort_status": 10, "lsdsort_algorithm": 2, "lsdsort_key_type": 6}
    for enum, count in sizes.items():
        values = _enum(enum)
        assert len(values) == count, (enum, values)
        for name, value in values.items():
            assert getattr(errors, name) == value, name
    for name in ("LSDSORT_MAX_KEYS", "LSDSORT_MAX_PASSES", "LSDSORT_PARTITION_MSB", "LSDSORT_PARTITION_SPLITTERS"):
        assert getattr(errors, name) == _define(name), name
    assert _lib.LSDSORT_MAX_PASSES == errors.LSDSORT_MAX_PASSES
    assert errors.KEY_TYPES_32 == {"uint32": errors.LSDSORT_KEY_U32, "int32": errors.LSDSORT_KEY_I32, "float32": errors.LSDSORT_KEY_F32}
    assert errors.KEY_TYPES_64 == {"uint64": errors.LSDSORT_KEY_U64, "int64": errors.LSDSORT_KEY_I64, "float64": errors.LSDSORT_KEY_F64}
    partitions = {"msb": errors.LSDSORT_PARTITION_MSB, "splitters": errors.LSDSORT_PARTITION_SPLITTERS}
    assert ShardedSorter.PARTITIONS == partitions and LoopbackWorld.PARTITIONS == partitions
    # lsdsort_timing: four floats, the pass times, four ints, one float
    assert ctypes.sizeof(_lib.LsdsortTiming) == 4 * (4 + errors.LSDSORT_MAX_PASSES) + 4 * 4 + 4


def test_all_is_what_the_package_exports_from_api():
    import lsdradixsort_amd as lsd

    tree = ast.parse(open(os.path.join(ROOT, "lsdradixsort_amd", "__init__.py")).read())
    bound = [alias.asname or alias.name for node in tree.body
             if isinstance(node, ast.ImportFrom) and node.level == 1 and node.module == "api" for alias in node.names]
    assert bound and len(set(bound)) == len(bound)
    assert len(set(lsd.api.__all__)) == len(lsd.api.__all__)
    assert set(lsd.api.__all__) == set(bound)
    for name in bound:
        assert getattr(lsd, name) is getattr(lsd.api, name), name


def test_importing_the_package_does_not_import_torch():
    code = "import sys, lsdradixsort_amd, lsdradixsort_amd.dist; print('torch' in sys.modules)"
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "False"


@pytest.fixture
def no_library(monkeypatch):
    """The argument checks come first: the library must not even be asked for."""
    import lsdradixsort_amd as lsd

    def refuse():
        raise AssertionError("the library was reached before the arguments were checked")

    monkeypatch.setattr(lsd.api, "lib", refuse)
    return lsd


def _calls(lsd, t):
    """name -> a call of every device wrapper with the CPU tensor ``t`` where a CUDA tensor belongs."""
    return {
        "GPULSDRadixSort": lambda: lsd.GPULSDRadixSort(t),
        "GPULSDRadixSortTimed": lambda: lsd.GPULSDRadixSortTimed(t),
        "GPUSortMulti": lambda: lsd.GPUSortMulti(t, [t]),
        "GPUSortTyped": lambda: lsd.GPUSortTyped(t),
        "GPUSortSegmented": lambda: lsd.GPUSortSegmented(t, t),
        "GPUTopK": lambda: lsd.GPUTopK(t, 1),
        "GPUSortWide": lambda: lsd.GPUSortWide(t, t),
        "sort_rows": lambda: lsd.sort_rows(t.view(2, -1)),
        "sort64": lambda: lsd.sort64(t),
        "topk_rows": lambda: lsd.topk_rows(t, 1),
        "BuildHistograms": lambda: lsd.BuildHistograms(t, 8, 0),
        "BuildOffsets": lambda: lsd.BuildOffsets(t.view(2, -1), 8),
        "RankScatter": lambda: lsd.RankScatter(t, t, 8, 0),
        "DigitHistograms": lambda: lsd.DigitHistograms(t, 8),
        "MSBPartition": lambda: lsd.MSBPartition(t, 2),
        "SplitterPartition": lambda: lsd.SplitterPartition(t, [1, 2, 3]),
        "ThresholdPartition": lambda: lsd.ThresholdPartition(t, [1, 2, 3]),
    }


@pytest.mark.parametrize("name", sorted(_calls(None, None)))
def test_a_cpu_tensor_is_a_type_error(no_library, name):
    import torch

    t = torch.arange(8, dtype=torch.int32)
    with pytest.raises(TypeError):
        _calls(no_library, t)[name]()
    assert torch.equal(t, torch.arange(8, dtype=torch.int32))


def test_timed_sort_checks_its_payloads_and_typed_sort_its_tensor(no_library):
    """A payload that is no CUDA tensor is refused by both faces of the plain sort; so is a key array that is no tensor at all."""
    import torch

    t = torch.arange(8, dtype=torch.int32)
    for call in (no_library.GPULSDRadixSort, no_library.GPULSDRadixSortTimed):
        with pytest.raises(TypeError):
            call(t, d_vals=t)
    with pytest.raises(TypeError):
        no_library.GPUSortTyped([3, 1, 2])


def test_host_entries_check_their_arrays(no_library):
    good = np.arange(8, dtype=np.uint32)
    read_only = np.arange(8, dtype=np.uint32)
    read_only.flags.writeable = False
    bad = {"not uint32": np.arange(8, dtype=np.int32), "not contiguous": np.arange(16, dtype=np.uint32)[::2], "read-only": read_only}
    for why, a in bad.items():
        with pytest.raises(TypeError):
            no_library.sort(a)
        with pytest.raises(TypeError):
            no_library.sort_pairs(a, good.copy())
        with pytest.raises(TypeError):
            no_library.sort_pairs(good.copy(), a)
    with pytest.raises(ValueError):
        no_library.sort_pairs(good.copy(), np.arange(9, dtype=np.uint32))
