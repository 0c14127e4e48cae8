"""CPU suite: the kernels of stage 1 (histograms.hip), stage 2 (scans.hip), the local stage, the hybrid planner, the segmented
sort and the row selections and sorts (topk.hip, topk16.hip, kth.hip, rows16.hip) compile for gfx950 WITHOUT scratch, and with the
occupancy and the static LDS they were measured with.

A register spill in these kernels does not break a parity test -- it multiplies the kernel's memory traffic (round 3: a loop
around the local stage's body spilled 49 registers and took the stage from 0.55 to 2.07 ms; the parity tests stayed green).
hipcc's own resource remarks are the check: ScratchSize 0 and no VGPR spill for every kernel of these files (seconds to
compile; the rank-and-scatter translation units take minutes: tools/isa_diff.py --resources, profiles/pass_refactor), and against
tests/golden/kernel_resources.json (file -> mangled name -> occupancy, static LDS; the device-side counterpart of
workspace_sizes.json): the same set of kernels -- bench.py and tools/profile_bench.sh classify by name --, no fewer waves per SIMD,
the same static LDS."""
import json
import os

import pytest

from _kernel_resources import hipcc, kernel_resources

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kernel_resources.json")


@pytest.mark.parametrize("source", ["histograms.hip", "scans.hip", "local_sort.hip", "hybrid.hip", "segmented.hip", "topk.hip", "topk16.hip",
                                    "kth.hip", "rows16.hip"])
def test_no_scratch(source):
    if hipcc() is None:
        pytest.skip("no hipcc on this machine")
    got = kernel_resources(source)
    for name, r in got.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, f"{name}: scratch {r['scratch']} B/lane, {r['vgpr_spill']} VGPRs spilled"
    want = json.load(open(GOLDEN))[source]
    assert sorted(got) == sorted(want), f"kernels gone: {sorted(set(want) - set(got))}, new: {sorted(set(got) - set(want))}"
    for name, w in want.items():
        assert got[name]["occupancy"] >= w["occupancy"], f"{name}: {got[name]['occupancy']} waves/SIMD, recorded {w['occupancy']}"
        assert got[name]["lds_bytes"] == w["lds_bytes"], f"{name}: {got[name]['lds_bytes']} B of static LDS, recorded {w['lds_bytes']}"
