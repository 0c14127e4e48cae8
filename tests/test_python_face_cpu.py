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

from _faces import FakeCuda, no_library

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


def _calls(lsd, t):
    """name -> a call of every device wrapper with the CPU tensor ``t`` (int32), or one of its length in the dtype the wrapper takes,
    where a CUDA tensor belongs."""
    if t is not None:
        import torch

        i16, bf16, f32 = t.to(torch.int16), t.to(torch.bfloat16), t.to(torch.float32)
    return {
        "GPUSort16": lambda: lsd.GPUSort16(i16),
        "sort16": lambda: lsd.sort16(i16),
        "GPUTopK16": lambda: lsd.GPUTopK16(i16, 1),
        "topk16_rows": lambda: lsd.topk16_rows(bf16, 1),
        "GPUSortRows16": lambda: lsd.GPUSortRows16(i16),
        "sort_rows16": lambda: lsd.sort_rows16(bf16),
        "GPUKth": lambda: lsd.GPUKth(t, 1),
        "kthvalue_rows": lambda: lsd.kthvalue_rows(f32, 1),
        "median_rows": lambda: lsd.median_rows(t),
        "GPUKthMulti": lambda: lsd.GPUKthMulti(t, [1]),
        "quantile_rows": lambda: lsd.quantile_rows(f32, 0.5),
        "GPUKth16": lambda: lsd.GPUKth16(i16, 1),
        "kthvalue16_rows": lambda: lsd.kthvalue16_rows(bf16, 1),
        "median16_rows": lambda: lsd.median16_rows(i16),
        "GPUKth16Multi": lambda: lsd.GPUKth16Multi(i16, [1]),
        "quantile16_rows": lambda: lsd.quantile16_rows(bf16, 0.5),
        "GPUKth16PerRow": lambda: lsd.GPUKth16PerRow(i16, t[:1]),
        "GPUTopK16Filter": lambda: lsd.GPUTopK16Filter(i16, t[:1]),
        "topk16_filter_rows": lambda: lsd.topk16_filter_rows(bf16, 1),
        "GPUTopP16Filter": lambda: lsd.GPUTopP16Filter(bf16, f32[:1]),
        "topp16_filter_rows": lambda: lsd.topp16_filter_rows(bf16, 0.9),
        "GPUSample16": lambda: lsd.GPUSample16(bf16, f32[:1]),
        "sample16_rows": lambda: lsd.sample16_rows(bf16, 0.5),
        "GPULogprob16": lambda: lsd.GPULogprob16(bf16, t[:1]),
        "logprobs16_rows": lambda: lsd.logprobs16_rows(bf16.view(2, -1), t[:2]),
        "top_logprobs16_rows": lambda: lsd.top_logprobs16_rows(bf16, 1),
        "GPURunLength": lambda: lsd.GPURunLength(t),
        "GPUUnique": lambda: lsd.GPUUnique(t),
        "unique": lambda: lsd.unique(t),
        "unique_consecutive": lambda: lsd.unique_consecutive(f32),
        "GPUReduceRuns": lambda: lsd.GPUReduceRuns(t, f32),
        "GPUReduceByKey": lambda: lsd.GPUReduceByKey(t, f32),
        "reduce_by_key": lambda: lsd.reduce_by_key(t, f32),
        "reduce_consecutive": lambda: lsd.reduce_consecutive(t, t),
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


def test_the_table_holds_every_device_wrapper():
    """every ``GPU*`` name, every ``*_rows`` wrapper and the 1-D torch-shaped ones of ``__all__`` (the stage entries and the partitions
    beside them); ``workspace_form`` and ``workspace_half`` check no tensor and stay out"""
    import lsdradixsort_amd as lsd

    others = {"sort_rows16", "sort16", "sort64", "unique", "unique_consecutive", "reduce_by_key", "reduce_consecutive"}
    wrappers = {name for name in lsd.api.__all__ if name.startswith("GPU") or name.endswith("_rows") or name in others}
    assert len(wrappers) == 23 + 14 + 7
    assert wrappers <= set(_calls(None, None))


# ---- one definition of what the wrappers share (in the manner of tests/test_mass_rows_cpu.py, over the AST) ----------------------------
def _api_functions():
    """{name: FunctionDef} of the module-level functions of api.py, and the tree"""
    tree = ast.parse(open(os.path.join(ROOT, "lsdradixsort_amd", "api.py")).read())
    return {node.name: node for node in tree.body if isinstance(node, ast.FunctionDef)}, tree


def _functions_that(functions, found):
    return {name for name, node in functions.items() if any(found(n) for n in ast.walk(node))}


def test_one_workspace_path():
    functions, _ = _api_functions()
    calls = _functions_that(functions, lambda n: isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id == "_temp_workspace")
    assert calls == {"_workspace", "alloc_workspace"}, calls
    too_large = _functions_that(functions, lambda n: isinstance(n, ast.Attribute) and n.attr == "LSDSORT_ERR_TOO_LARGE")
    assert too_large == {"_workspace"}, too_large
    # and nobody builds the figure's refusal by hand beside it: LsdsortError is raised there, in alloc_workspace, and nowhere else
    raises = _functions_that(functions, lambda n: isinstance(n, ast.Raise) and "LsdsortError" in ast.dump(n))
    assert raises == {"_workspace", "alloc_workspace"}, raises


def test_one_pairing_table_of_the_16_bit_keys():
    functions, tree = _api_functions()
    pairs = [n for n in ast.walk(tree) if isinstance(n, ast.Tuple) and [getattr(e, "value", None) for e in n.elts] == ["uint16", "int16"]]
    assert len(pairs) == 1, "the dtype / key-type pairing of the 16-bit keys is written more than once"
    tables = [node for node in tree.body if isinstance(node, ast.Assign) and any(n is pairs[0] for n in ast.walk(node))]
    assert len(tables) == 1 and [t.id for t in tables[0].targets] == ["_FITS16"]
    readers = _functions_that(functions, lambda n: isinstance(n, ast.Name) and n.id == "_FITS16")
    assert readers == {"_keys16"}, readers
    # every 16-bit wrapper reaches it through _keys16 (the three logit units through _logits16), none carries the checks inline
    users = _functions_that(functions, lambda n: isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id in ("_keys16", "_logits16"))
    assert users == {"GPUSort16", "GPUTopK16", "GPUKth16", "GPUKth16Multi", "GPUKth16PerRow", "GPUTopK16Filter", "GPUSortRows16", "_logits16",
                     "GPUTopP16Filter", "GPUSample16", "GPULogprob16"}, users
    assert not _functions_that(functions, lambda n: isinstance(n, ast.Name) and n.id == "KEY_TYPES_16") - {"_keys16"}


class _Refuses:
    """stands in for the library: every size entry answers 0, nothing else may be called"""

    def __getattr__(self, name):
        assert name.endswith("_bytes"), f"{name} was called after a refused size"
        return lambda *args: 0


def test_a_refused_size_raises_the_entrys_own_error(monkeypatch):
    """status, entry name and text of the error a ``*_workspace_bytes`` figure of 0 gives, per family"""
    import torch

    import lsdradixsort_amd as lsd
    from lsdradixsort_amd import errors

    monkeypatch.setattr(lsd.api, "lib", lambda: _Refuses())

    def fake(dtype, *shape):
        return torch.zeros(shape, dtype=dtype).as_subclass(FakeCuda)

    i32, bf16, f32 = fake(torch.int32, 2, 4), fake(torch.bfloat16, 2, 4), fake(torch.float32, 2)
    rows = "too many keys or rows"
    table = {
        "lsdsort_segmented_workspace_bytes": (lambda: lsd.GPUSortSegmented(i32.view(-1), fake(torch.int32, 3)), "too many keys or segments"),
        "lsdsort_topk_workspace_bytes": (lambda: lsd.GPUTopK(i32, 1), rows),
        "lsdsort_kth_workspace_bytes": (lambda: lsd.GPUKth(i32, 1), rows),
        "lsdsort_kth_multi_workspace_bytes": (lambda: lsd.GPUKthMulti(i32, [1]), rows),
        "lsdsort_keys16_workspace_bytes": (lambda: lsd.GPUSort16(bf16.view(-1), "bfloat16"), "too many keys"),
        "lsdsort_topk16_workspace_bytes": (lambda: lsd.GPUTopK16(bf16, 1, "bfloat16"), rows),
        "lsdsort_kth16_workspace_bytes": (lambda: lsd.GPUKth16(bf16, 1, "bfloat16"), rows),
        "lsdsort_kth16_multi_workspace_bytes": (lambda: lsd.GPUKth16Multi(bf16, [1], "bfloat16"), rows),
        "lsdsort_kth16_perrow_workspace_bytes": (lambda: lsd.GPUKth16PerRow(bf16, fake(torch.int32, 2), "bfloat16"), rows),
        "lsdsort_topk16_filter_workspace_bytes": (lambda: lsd.GPUTopK16Filter(bf16, fake(torch.int32, 2), "bfloat16"), rows),
        "lsdsort_topp16_filter_workspace_bytes": (lambda: lsd.GPUTopP16Filter(bf16, f32), rows),
        "lsdsort_sample16_workspace_bytes": (lambda: lsd.GPUSample16(bf16, f32), rows),
        "lsdsort_logprob16_workspace_bytes": (lambda: lsd.GPULogprob16(bf16, fake(torch.int32, 2)), rows),
        "lsdsort_rows16_workspace_bytes": (lambda: lsd.GPUSortRows16(bf16, "bfloat16"), rows),
        "lsdsort_rle_workspace_bytes": (lambda: lsd.GPURunLength(i32.view(-1)), "too many keys"),
        "lsdsort_unique_workspace_bytes": (lambda: lsd.GPUUnique(i32.view(-1)), "too many keys"),
        "lsdsort_reduce_runs_workspace_bytes": (lambda: lsd.GPUReduceRuns(i32.view(-1), fake(torch.float32, 8)), "too many keys"),
        "lsdsort_reduce_by_key_workspace_bytes": (lambda: lsd.GPUReduceByKey(i32.view(-1), fake(torch.float32, 8)), "too many keys"),
    }
    for entry, (call, tail) in table.items():
        with pytest.raises(errors.LsdsortError) as e:
            call()
        assert e.value.status == errors.LSDSORT_ERR_TOO_LARGE and str(e.value) == f"{entry}: lsdsort status {errors.LSDSORT_ERR_TOO_LARGE}: {tail}", entry
    # the wide sorts ask even when a workspace is given, and call a figure of 0 a bad argument
    for workspace in (None, fake(torch.uint8, 4096)):
        with pytest.raises(errors.LsdsortError) as e:
            lsd.GPUSortWide(fake(torch.int64, 8), workspace=workspace)
        assert str(e.value) == f"lsdsort_wide_workspace_bytes: lsdsort status {errors.LSDSORT_ERR_INVALID_ARG}: bad (n, radix_bits)"
    # a caller's workspace is taken as it is: the figure is not asked for (the recorder refuses the device entry instead)
    with pytest.raises(AssertionError, match="lsdsort_topk_device was called"):
        lsd.GPUTopK(i32, 1, workspace=fake(torch.uint8, 4096))
    # no keys or no segments: the segmented sort's figure of 0 is no refusal
    with pytest.raises(AssertionError, match="lsdsort_segmented_device was called"):
        lsd.GPUSortSegmented(fake(torch.int32, 0), fake(torch.int32, 3))


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
