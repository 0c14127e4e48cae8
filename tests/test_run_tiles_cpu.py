"""CPU suite: what the two run units (unique.hip: run-length encode and unique; reduce_by_key.hip) share lives ONCE, in
csrc/run_tiles.hpp -- the tile constants, the group loaders and the head flags on the device side, the workspace carve-up, the sort of
the copies and the check entry's two reads on the host side -- and the units include it instead of carrying copies (DESIGN.md sections
6.18, 6.19 and 8).  Source text; hipcc for the one thing text cannot show, that the header stands on its own includes; and the
library's workspace figures against tests/golden/run_units_workspace.json, recorded from the commit before the header existed: the
shared layout code carves nothing differently.

    python tests/test_run_tiles_cpu.py          prints the figures of the library in the tree, in the fixture's form"""
import json
import os
import re
import subprocess
import sys

import pytest

import _replay as rp
import _unique as un
from _kernel_resources import CSRC, code, defined_in, hipcc, includes, sources

HEADER = "run_tiles.hpp"
UNITS = ("unique.hip", "reduce_by_key.hip")
FUNCTIONS = ("group_start", "group_flags", "load_group", "load_words32", "store_group", "tile_keys_and_heads")
CONSTANTS = ("kRunThreads", "kRunWaves", "kRunThreadKeys", "kRunTile", "kRunScanThreads", "kRunScanWaves", "kRunScanRound", "kRunMaxGrid",
             "kRunFault")
STRUCTS = ("Groups", "TileArrays", "RunLayout")
KERNELS = ("run_store_kernel",)
HOST = ("key_bits_of", "aligned_to", "store_zero_runs", "make_tile_arrays", "make_run_layout", "sort_copies", "check_copies")
GONE = (r"kRle\w*", r"kRbk\w*", "load_positions", "load_values", "load_tile_heads", "RleArrays", "RunArrays",
        "UniqueLayout", "ByKeyLayout", "rle_store_kernel", "rbk_store_kernel")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "run_units_workspace.json")


def test_each_shared_piece_is_defined_once_and_in_the_header():
    for name in FUNCTIONS:   # a definition: the line opens with the qualifiers (behind a template line or not), and the parameters follow
        found = defined_in(r"^(?:template[^\n]*\n)?__device__ __forceinline__ [\w ]+\b" + name + r"\(")
        assert found == {HEADER: 1}, f"{name} is defined in {found}"
    for name in CONSTANTS:
        found = defined_in(r"^\s*constexpr[^;\n]*\b" + name + r"\s*=")
        assert found == {HEADER: 1}, f"{name} is defined in {found}"
    for name in STRUCTS:
        found = defined_in(r"^(?:template[^\n]*\n)?struct " + name + r"\s*\{")
        assert found == {HEADER: 1}, f"{name} is defined in {found}"
    for name in KERNELS:
        found = defined_in(r"^__global__ void [^\n]*\b" + name + r"\(")
        assert found == {HEADER: 1}, f"{name} is defined in {found}"
    for name in HOST:
        found = defined_in(r"^(?:bool|int|TileArrays|RunLayout) " + name + r"\(")
        assert found == {HEADER: 1}, f"{name} is defined in {found}"
    # the units' own kernels and entries stay theirs
    header = code(sources()[HEADER])
    assert len(re.findall(r"__global__", header)) == len(KERNELS) and 'extern "C"' not in header


def test_the_old_names_are_gone_from_csrc():
    for name, text in sources().items():
        for old in GONE:
            assert not re.search(r"\b" + old + r"\b", text), (name, old)   # comments included


def test_the_two_units_include_the_header_and_nobody_else_does():
    for name, text in sources().items():
        assert (HEADER in includes(text)) == (name in UNITS), name
    assert includes(sources()[HEADER]) == {"lsd_device.hpp", "lsd_host.hpp"}
    assert re.findall(r"#include\s+(\S+)", sources()[HEADER]) == ['"lsd_device.hpp"', '"lsd_host.hpp"']


def test_the_makefile_rebuilds_the_units_when_the_header_changes():
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert HEADER in re.search(r"^HEADERS\s*:=(.*)$", makefile, flags=re.M).group(1).split()
    assert re.search(r"^\$\(BUILD\)/%\.o: %\.hip \$\(HEADERS\)$", makefile, flags=re.M)


@pytest.mark.skipif(hipcc() is None, reason="no hipcc")
def test_the_header_stands_on_its_own_includes(tmp_path):
    unit = tmp_path / "only.hip"
    unit.write_text(f'#include "{HEADER}"\n')
    p = subprocess.run([hipcc(), "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-Wno-unused-function",
                        "-Wno-unused-command-line-argument", "-I", CSRC, str(unit)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]


# ---- the workspace figures ---------------------------------------------------------------------------------------------------------
def workspace_figures():
    """The five figures over the ladder of the units' test_workspace_figures and one size above the limit: both widths or all six key
    types, with and without positions.  `unique_sort_offset` is tests/_replay.py's restatement of where the sort's workspace begins
    inside unique's."""
    from lsdradixsort_amd import errors as E
    from lsdradixsort_amd import lib

    L = lib()
    ladder = [0, 1, 2, 3, un.TILE - 1, un.TILE, un.TILE + 1, 20487, (1 << 20) + 13, un.BIG_N, 1 << 28, E.LSDSORT_MAX_KEYS, E.LSDSORT_MAX_KEYS + 1]
    return {
        "ladder": ladder,
        "rle": {str(bits): [L.lsdsort_rle_workspace_bytes(n, bits) for n in ladder] for bits in (32, 64)},
        "reduce_runs": {str(bits): [L.lsdsort_reduce_runs_workspace_bytes(n, bits) for n in ladder] for bits in (32, 64)},
        "unique": {name: {str(positions): [L.lsdsort_unique_workspace_bytes(n, kt, positions) for n in ladder] for positions in (0, 1)}
                   for kt, name in enumerate(un.KEY_TYPES)},
        "reduce_by_key": {name: [L.lsdsort_reduce_by_key_workspace_bytes(n, kt) for n in ladder] for kt, name in enumerate(un.KEY_TYPES)},
        "unique_sort_offset": {str(w): {str(positions): [rp.unique_sort_offset(n, w, bool(positions)) for n in ladder[:-1]] for positions in (0, 1)}
                               for w in (32, 64)},
    }


def test_workspace_figures_are_those_recorded_before_the_header():
    from lsdradixsort_amd import errors as E
    from lsdradixsort_amd import lib

    want = json.load(open(GOLDEN))
    got = workspace_figures()
    assert got["ladder"] == want["ladder"] and want["ladder"][-2:] == [E.LSDSORT_MAX_KEYS, E.LSDSORT_MAX_KEYS + 1]
    for name in ("rle", "reduce_runs", "unique", "reduce_by_key", "unique_sort_offset"):
        assert got[name] == want[name], name
    # the layout, exactly: what lies in front of the sort's workspace | the sort's | the tile arrays of the entry without a sort
    L = lib()
    for kt, name in enumerate(un.KEY_TYPES):
        w = un.width_of(name)
        for positions in (0, 1):
            for i, n in enumerate(want["ladder"][:-1]):
                inner = L.lsdsort_wide_workspace_bytes(n, 8, 64, 32 * positions) if w == 64 else L.lsdsort_workspace_bytes(n, 8, positions)
                inner = -(-inner // 256) * 256
                front = want["unique_sort_offset"][str(w)][str(positions)][i]
                assert want["unique"][name][str(positions)][i] == front + inner + want["rle"][str(w)][i] - 256, (name, positions, n)
                if positions:   # reduce by key: the values lie where unique's positions do
                    assert want["reduce_by_key"][name][i] == front + inner + want["reduce_runs"][str(w)][i] - 256, (name, n)
    for figures in (want["rle"], want["reduce_runs"], want["reduce_by_key"]):
        assert all(row[-1] == 0 and min(row[:-1]) > 0 for row in figures.values())


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print("{\n" + ",\n".join(f" {json.dumps(name)}: {json.dumps(value)}" for name, value in workspace_figures().items()) + "\n}")
