"""hipcc's own resource remarks for one translation unit of lsdradixsort_amd/csrc, compiled for gfx950 (device code only):
what tests/test_kernel_resources.py and tests/test_segmented_cpu.py assert on; and the text of csrc/ for the header-discipline suites
(test_mass_rows_cpu.py, test_run_tiles_cpu.py, test_tile_headers_cpu.py): sources, code, defined_in, includes."""
import functools
import os
import re
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lsdradixsort_amd", "csrc")
FIELDS = {"scratch": "ScratchSize [bytes/lane]", "vgpr_spill": "VGPRs Spill", "occupancy": "Occupancy [waves/SIMD]",
          "lds_bytes": "LDS Size [bytes/block]"}


def sources():
    """{file name: text} of every .hip and .hpp under csrc/"""
    return {name: open(os.path.join(CSRC, name)).read() for name in sorted(os.listdir(CSRC)) if name.endswith((".hip", ".hpp"))}


def code(text):
    """the text without its // comments"""
    return re.sub(r"//.*", "", text)


def defined_in(pattern):
    """{file: number of definitions} over csrc/, comments aside"""
    found = {name: len(re.findall(pattern, code(text), flags=re.M)) for name, text in sources().items()}
    return {name: n for name, n in found.items() if n}


def includes(text):
    return set(re.findall(r'#include "([^"]+)"', text))


def hipcc():
    """Path of hipcc, or None where there is none."""
    path = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return path if os.path.exists(path) else None


@functools.lru_cache(maxsize=None)
def kernel_resources(source):
    """{mangled kernel name: {scratch, vgpr_spill, occupancy, lds_bytes}} of csrc/<source>."""
    with tempfile.TemporaryDirectory() as tmp:
        p = subprocess.run([hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only",
                            "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, source), "-o", os.path.join(tmp, "x.o")],
                           capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    out = {}
    for block in p.stderr.split("Function Name: ")[1:]:
        out[block.split()[0]] = {k: int(re.search(re.escape(label) + r": (\d+)", block).group(1)) for k, label in FIELDS.items()}
    assert out, "no kernel in " + source
    return out
