"""CPU suite: the row helpers of the three 16-bit mass units (topp16.hip, sample16.hip, logprob16.hip) live ONCE, in
csrc/mass_rows16.hpp, and the units include it instead of carrying copies (DESIGN.md sections 6.14 and 8); the host-side size check of
the row entries lives once in radix_select.hpp, the float key types' map and value side once in keys16_map.hpp.  Source text, and
hipcc for the one thing text cannot show: that the header stands on its own includes."""
import os
import re
import subprocess

import pytest

from _kernel_resources import CSRC, code, defined_in, hipcc, includes, sources

HEADER = "mass_rows16.hpp"
UNITS = ("topp16.hip", "sample16.hip", "logprob16.hip")
FUNCTIONS = ("read_body", "read_front", "wave_least", "best_number", "wave_add64", "log_total", "row_best_number", "chunk_best_number")
CONSTANTS = ("kAbsent",)
ALIASES = ("RowKeys",)
HOST = {"sizes_ok": "radix_select.hpp", "float16_values": "keys16_map.hpp"}   # helper -> the one header that defines it


def test_each_helper_is_defined_once_and_in_the_header():
    for name in FUNCTIONS:   # a definition: the line opens with the qualifiers (behind a template line or not), and the parameters follow
        found = defined_in(r"^(?:template[^\n]*\n)?__device__ __forceinline__ [\w ]+\b" + name + r"\(")
        assert found == {HEADER: 1}, f"{name} is defined in {found}"
    for name in CONSTANTS:
        found = defined_in(r"^\s*constexpr[^;\n]*\b" + name + r"\s*=")
        assert found == {HEADER: 1}, f"{name} is defined in {found}"
    for name in ALIASES:
        found = defined_in(r"^\s*using " + name + r"\s*=")
        assert found == {HEADER: 1}, f"{name} is defined in {found}"
    # the filter's old name for wave_least is gone, and the best kernels and the short kernels CALL the shared bodies
    texts = {name: code(text) for name, text in sources().items()}
    assert not any(re.search(r"\bwave_min\b", text) for text in texts.values())
    for unit in ("sample16.hip", "logprob16.hip"):
        assert len(re.findall(r"\bchunk_best_number\(", texts[unit])) == 1 and len(re.findall(r"\brow_best_number<WAVES>\(", texts[unit])) == 1, unit


def test_the_three_units_include_the_header_and_nobody_else_does():
    for name, text in sources().items():
        assert (HEADER in includes(text)) == (name in UNITS), name
    # the header is no user of select_tiles16.hpp (tests/test_tile_headers_cpu.py: that one is the seven selecting units') and brings
    # what it uses itself
    assert includes(sources()[HEADER]) == {"keys16_map.hpp", "lsd_device.hpp", "radix_select.hpp"}


def test_the_makefile_rebuilds_the_units_when_the_header_changes():
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert HEADER in re.search(r"^HEADERS\s*:=(.*)$", makefile, flags=re.M).group(1).split()
    assert re.search(r"^\$\(BUILD\)/%\.o: %\.hip \$\(HEADERS\)$", makefile, flags=re.M)


def test_the_host_helpers_are_defined_once():
    for name, where in HOST.items():
        found = defined_in(r"^(?:inline )?(?:bool|int) " + name + r"\(")
        assert found == {where: 1}, f"{name} is defined in {found}"
    texts = {name: code(text) for name, text in sources().items()}
    for unit in UNITS:   # the entries of the three units take key type, map and value side from the one helper
        assert "float16_values(" in texts[unit] and "Values16{" not in texts[unit] and "key16_map(" not in texts[unit], unit
    for unit in UNITS + ("kth16_rowk.hip",):
        assert "sizes_ok(" in texts[unit], unit


@pytest.mark.skipif(hipcc() is None, reason="no hipcc")
def test_the_header_stands_on_its_own_includes(tmp_path):
    unit = tmp_path / "only.hip"
    unit.write_text(f'#include "{HEADER}"\n')
    p = subprocess.run([hipcc(), "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only", "-fsyntax-only", "-Wall", "-Werror",
                        "-Wno-unused-function", "-Wno-unused-command-line-argument", "-I", CSRC, str(unit)],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
