"""CPU suite: the row selects' tile helpers live ONCE, in csrc/select_tiles16.hpp (16-bit keys) and csrc/select_tiles32.hpp (32-bit
keys), the slots of the two multi-rank k-th value units in csrc/kth_slots.hpp, the k-th value units' pick kernel and fault bits in
csrc/radix_select.hpp, and the units include them instead of carrying copies.  Source text, and hipcc for
the one thing text cannot show: that each header stands on its own includes."""
import os
import re
import subprocess

import pytest

from _kernel_resources import CSRC, code, defined_in, hipcc, sources

H16, H32, SLOTS, SELECT = "select_tiles16.hpp", "select_tiles32.hpp", "kth_slots.hpp", "radix_select.hpp"
UNITS = {"topk16.hip": H16, "kth16.hip": H16, "kth16_multi.hip": H16, "kth16_rowk.hip": H16, "topp16.hip": H16,
         "kth.hip": H32, "kth_multi.hip": H32}
SLOT_UNITS = {"kth_multi.hip", "kth16_multi.hip"}
# helper -> the files under csrc/ that define it, each exactly once.  topk.hip's load_tile is the one exception: another shape (a
# plain pointer, one key per load, no validity mask), its own on purpose.
FUNCTIONS = {"load_tile": {H16, H32, "topk.hip"}, "load_head": {H16, H32}, "locate_tile": {H16, H32},
             "store_tile": {H16}, "store_head": {H16}, "same_phase": {H16},
             "need_of": {SLOTS}, "slot_states": {SLOTS}, "leaders": {SLOTS}, "leader_of": {SLOTS}}
STRUCTS = {"StopNever16": {H16}, "Needs": {SLOTS}, "SlotStates": {SLOTS}}
CONSTANTS = {"kNoKey": {H16}, "kHeadBit": {H16, H32}, "kNoChunk": {SELECT}, "kMaxSlots": {SLOTS},
             "kKthFaultCount": {SELECT}, "kKthFaultLocate": {SELECT}}
# host functions and kernel templates -> the one header that defines each
HOST = {"multi_too_large": SLOTS, "needs_from_ranks": SLOTS, "launch_short_slots": SLOTS}
KERNEL_TEMPLATES = {"pick_rows_kernel": SELECT, "pick_slots_kernel": SLOTS, "count_rows16_kernel": H16, "locate_rows16_kernel": H16}
# Kernel bodies of kth16_rowk.hip that repeat kth16.hip's line for line: none.  Count, pick and locate were the last three; they are
# kernel templates now, instantiated by both units (DESIGN.md section 6.14 says why that form keeps the instructions where a shared
# device function did not).
STILL_DOUBLE = set()


def test_each_helper_is_defined_once_and_in_its_header():
    for name, where in FUNCTIONS.items():   # a definition: the line opens with the qualifiers, and a body follows the parameters
        found = defined_in(r"^(?:template[^\n]*\n)?__device__ __forceinline__ [\w <>]+\b" + name + r"\(")
        assert found == {f: 1 for f in where}, f"{name} is defined in {found}"
    for name, where in STRUCTS.items():
        found = defined_in(r"^\s*struct " + name + r"\b")
        assert found == {f: 1 for f in where}, f"{name} is defined in {found}"
    for name, where in CONSTANTS.items():
        found = defined_in(r"^\s*constexpr[^;\n]*\b" + name + r"\s*=")
        assert found == {f: 1 for f in where}, f"{name} is defined in {found}"
    for name, where in HOST.items():   # a host function: the line opens with its return type
        found = defined_in(r"^(?:template[^\n]*\n)?(?:bool|int) " + name + r"\(")
        assert found == {where: 1}, f"{name} is defined in {found}"
    for name, where in KERNEL_TEMPLATES.items():
        found = defined_in(r"^template <class U>\n__global__ void __launch_bounds__\(\w+\) " + name + r"\(const typename U::Params p\)\n\{")
        assert found == {where: 1}, f"{name} is defined in {found}"
    # the pick's walk over a row's chunk counts: once for rows, once for slots, and in no unit
    found = defined_in(r"s_found\[0\] = kNoChunk;\n\s*uint32_t run = group_exclusive_scan<4>\(")
    assert found == {SELECT: 1, SLOTS: 1}, f"the pick walk is written in {found}"
    assert FUNCTIONS["load_tile"] - {H16, H32} == {"topk.hip"}   # the only helper a unit defines itself
    for table in (FUNCTIONS, STRUCTS, CONSTANTS):
        for name, where in table.items():
            assert all(f.endswith(".hpp") for f in where - {"topk.hip"}), name


def test_each_unit_includes_its_header_and_not_the_other():
    texts = sources()
    for unit, header in UNITS.items():
        included = set(re.findall(r'#include "([^"]+)"', texts[unit]))
        assert header in included and not ({H16, H32} - {header}) & included, f"{unit} includes {sorted(included)}"
    for name, text in texts.items():   # and nobody else does: the headers are those seven units'
        if name not in UNITS:
            assert not {H16, H32} & set(re.findall(r'#include "([^"]+)"', text)), name
        # the slots' header is the two multi-rank units', whatever their key width
        assert (SLOTS in re.findall(r'#include "([^"]+)"', text)) == (name in SLOT_UNITS), name


def test_the_makefile_rebuilds_the_units_when_a_header_changes():
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    headers = re.search(r"^HEADERS\s*:=(.*)$", makefile, flags=re.M).group(1).split()
    assert H16 in headers and H32 in headers and SLOTS in headers and SELECT in headers
    assert re.search(r"^\$\(BUILD\)/%\.o: %\.hip \$\(HEADERS\)$", makefile, flags=re.M)


def test_the_per_row_unit_uses_the_shared_long_select():
    for name, text in sources().items():
        assert "select_long_rowk" not in text, name
    assert len(re.findall(r"\bselect_long\(", code(sources()["kth16_rowk.hip"]))) == 3   # values only, with positions, the filter


def kernel_bodies(text, prefix):
    """{kind: the code lines of <prefix>_<kind>_kernel(const LongParams p)}, comments and blank lines aside"""
    out = {}
    for m in re.finditer(r"\b" + prefix + r"_(\w+)_kernel\(const LongParams p\)\n\{\n(.*?)\n\}\n", text, flags=re.S):
        out[m.group(1)] = [line.strip() for line in code(m.group(2)).split("\n") if line.strip()]
    return out


def test_kernel_bodies_left_double_are_the_listed_ones():
    texts = sources()
    one = kernel_bodies(texts["kth16.hip"], "kth16")
    per_row = kernel_bodies(texts["kth16_rowk.hip"], "kth16r")
    assert STILL_DOUBLE <= set(one) & set(per_row)
    assert {"hist", "scan", "value"} <= set(one) & set(per_row)                # the kernels both units still write out are read ...
    assert not {"count", "pick", "locate"} & (set(one) | set(per_row))         # ... and these three are written out in neither

    def repeats(kind):   # kth16.hip's body, more than a call or two, lies in kth16_rowk.hip's line for line and in order
        rest = iter(per_row[kind])
        return len(one[kind]) > 5 and all(line in rest for line in one[kind])

    assert {kind for kind in set(one) & set(per_row) if repeats(kind)} == STILL_DOUBLE


@pytest.mark.skipif(hipcc() is None, reason="no hipcc")
@pytest.mark.parametrize("header", [H16, H32, SLOTS, SELECT])
def test_a_header_stands_on_its_own_includes(header, tmp_path):
    unit = tmp_path / "only.hip"
    unit.write_text(f'#include "{header}"\n')
    p = subprocess.run([hipcc(), "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only", "-fsyntax-only", "-Wall", "-Werror",
                        "-Wno-unused-function", "-Wno-unused-command-line-argument", "-I", CSRC, str(unit)],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
