"""CPU suite: what the launches that serve more than one role rest on, read from the sources.

The new control-block words lie in free places -- behind the half form's, inside the block, no word of tests/_hybrid_words.py
moved -- and the planner's body exists once: in hybrid_plan.hpp, run by hybrid_plan_kernel (hybrid.hip) and by the half variant's
one-launch planner (half_hop.hip)."""
import glob
import os
import re

import _hybrid_words as hw

SLOT_WORDS = {"Shift": 4}    # name -> words: PassParams::shift of the g-th shared pass launch, g < 4


def _slot_constants():
    text = hw._text("lsd_kernels.hpp")
    return {m.group(1): hw._KERNELS["kSlotWord" + m.group(1)] for m in re.finditer(r"\bkSlotWord([A-Z]\w*)\s*=", text)}


def test_new_words_lie_behind_the_old_ones_and_inside_the_block():
    at = _slot_constants()
    assert set(at) == set(SLOT_WORDS), at
    end_of_old = hw._KERNELS["kHalfWords"]
    assert end_of_old == 25 and max(hw.WORD_INDEX.values()) < end_of_old
    taken = set()
    for name, first in at.items():
        words = set(range(first, first + SLOT_WORDS[name]))
        assert min(words) >= end_of_old, (name, first)
        assert not (words & taken), name
        taken |= words
    assert max(taken) < hw._KERNELS["kSlotWords"]
    assert 4 * (hw.HYBRID_OFFSET_WORDS + hw._KERNELS["kSlotWords"]) <= hw.CONTROL_BYTES
    # the names tests/_hybrid_words.py reads back are the ones test_hybrid_words_cpu.py pins: none of the new ones is among them
    assert not any(name.startswith("Slot") for name in hw.WORD_INDEX)


def test_no_existing_word_moved():
    assert hw.WORD_INDEX == {"Ok": 0, "SkipLocal": 1, "Plan": 2, "Largest": 10, "LargeCount": 11, "Hopeless": 12, "Violated": 13,
                             "Differ": 14, "Prefix": 15, "Shift": 16, "LowBits": 20, "HalfOk": 21, "HalfHigh": 22, "HalfPlan": 23}
    assert hw.HYBRID_OFFSET_WORDS == 50 and hw.CONTROL_BYTES == 512


def test_the_planner_body_exists_once():
    sources = {os.path.basename(p): open(p).read() for p in glob.glob(os.path.join(hw.CSRC, "*.h*"))}
    defined = [name for name, text in sources.items() if re.search(r"void\s+hybrid_plan_body\s*\(", text)]
    assert defined == ["hybrid_plan.hpp"], defined
    callers = sorted(name for name, text in sources.items() if re.search(r"hybrid_plan_body<", text))
    assert callers == ["half_hop.hip", "hybrid.hip"], callers
    # what only the body does: the verdict, the list of large buckets, the largest bucket
    for mark in (r"words\[kHybridWordOk\]\s*=", r"words\[kHybridWordLargest\]\s*=", r"large_list\[atomicAdd", r"words\[kSlotWordShift"):
        holders = [name for name, text in sources.items() if re.search(mark, text)]
        assert holders == ["hybrid_plan.hpp"], (mark, holders)
    # both kernels stay compiled next to the fused one, and the sort launches the fused one where the half variant is attempted
    half = sources["half_hop.hip"]
    for kernel in ("half_fold_kernel", "half_decide_kernel", "half_plan_kernel"):
        assert re.search(r"__global__[^;{]*\b" + kernel + r"\s*\(", half), kernel
    assert "launch_half_plan(" in sources["lsdsort_api.hip"] and "launch_half_fold(" not in sources["lsdsort_api.hip"]
