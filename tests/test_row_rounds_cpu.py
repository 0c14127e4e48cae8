"""The shapes of tests/_row_rounds.py still lie past the grid caps of the per-row kernels (no GPU needed).

test_gpu_row_rounds.py is worth what its shapes are worth: each must send the row loop of its kernel round again and end on a
partly filled round.  Here the launch lines of the ten capped kernels are read from lsdradixsort_amd/csrc and their
grid_for(items, per, cap) arguments are held against the shapes, so that raising a cap (or a tier boundary) fails this file
instead of silently turning the GPU tests into first-round tests."""
import os
import re

import pytest

import _row_rounds as rr

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lsdradixsort_amd", "csrc")
UPDATE = "update the shapes of tests/_row_rounds.py (and DESIGN.md section 6) so that every row loop still goes round again"
# <kernel>[<template arguments>] , dim3(grid_for(<items>, <per>, <cap>)): the launch macro's and launch_dynamic_lds's form alike
LAUNCH = re.compile(r"(\w+_kernel(?:<[^<>]*>)?)[>,(\s]*dim3\(grid_for\(([^,()]+),\s*(\w+)\s*,\s*(\w+)\s*\)\)")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def constant(name, *files):
    """the value of an integer constant `name = <expression of literals, other constants, + - * />` from the named sources"""
    texts = [source(f) for f in files]

    def value(word):
        if re.fullmatch(r"\d+u?", word):
            return int(word.rstrip("u"))
        for text in texts:
            m = re.search(r"constexpr[^;]*\b" + word + r"\s*=\s*([^,;]+)[,;]", text)
            if m:
                expr = re.sub(r"\(\w+_t\)", "", m.group(1))
                assert re.fullmatch(r"[\w\s+\-*/()]+", expr), f"{word} = {expr!r}: not an integer expression this test can read"
                return int(eval(re.sub(r"[A-Za-z_]\w*|\d+u", lambda t: str(value(t.group(0))), expr).replace("/", "//")))
        raise AssertionError(f"constant {word} not found in {files}: {UPDATE}")

    return value(name)


def launch_of(unit, kernel):
    """(items expression, per, cap) of the kernel's launch line(s), which must agree among themselves"""
    found = {(items.strip(), per, cap) for k, items, per, cap in LAUNCH.findall(source(unit + ".hip")) if k == kernel}
    assert found, f"{unit}.hip: no launch of {kernel} with dim3(grid_for(items, per, cap)) found any more: {UPDATE}"
    assert len(found) == 1, f"{unit}.hip: {kernel} is launched with different grids {sorted(found)}: {UPDATE}"
    items, per, cap = found.pop()
    files = (unit + ".hip", "radix_select.hpp", "lsd_kernels.hpp", "lsd_device.hpp")
    return items, constant(per, *files), constant(cap, *files)


@pytest.mark.parametrize("unit,kernel,extra,shapes", rr.LAUNCHES, ids=[f"{u}.hip {k}" for u, k, _, _ in rr.LAUNCHES])
def test_shape_goes_round_again_and_ends_on_a_partial_round(unit, kernel, extra, shapes):
    items_expr, per, cap = launch_of(unit, kernel)
    assert re.sub(r"\s", "", items_expr) == ("rows+1" if extra else "rows"), f"{unit}.hip {kernel}: grid over {items_expr!r}: {UPDATE}"
    for name in shapes:
        rows, cols = rr.SHAPES[name]
        items = rows + extra
        assert per * cap < items, f"{name} {rows}x{cols}: one round of {kernel} now covers {per} * {cap} >= {items} items: {UPDATE}"
        rest = items % (per * cap)
        assert rest != 0 and (per == 1 or rest % per != 0), \
            f"{name} {rows}x{cols}: the last round of {kernel} holds {rest} items, no partly filled workgroup ({per} each): {UPDATE}"
        if "offsets" not in kernel:
            assert per * cap == rr.stride_of(name, unit), f"{name}: {kernel} strides by {per * cap}, _row_rounds.STRIDE says otherwise"


def test_tier_boundaries_the_column_counts_rely_on():
    wave = constant("kWaveSegCap", "lsd_kernels.hpp")
    group = constant("kLocalSortCap", "lsd_kernels.hpp")
    assert (wave, group) == (rr.TIERS["wave"], rr.TIERS["group"]) == (1024, 16384), f"tier boundaries moved to {wave}, {group}: {UPDATE}"
    for name, (rows, cols) in rr.SHAPES.items():
        if name == "GROUP":
            assert cols == wave + 1 and cols % 2 == 1 and cols <= group, "GROUP: the shortest workgroup-tier row, and odd"
        else:
            assert cols <= wave, f"{name}: a wave-tier row"
    for unit in ("topk", "topk16", "kth", "kth16", "rows16"):   # the units choose their tier by these two constants
        text = source(unit + ".hip")
        assert re.search(r"cols <= \(size_t\)kWaveSegCap\b", text) and re.search(r"cols <= \(size_t\)kLocalSortCap\b", text), \
            f"{unit}.hip no longer picks its short-row kernel by kWaveSegCap and kLocalSortCap: {UPDATE}"


def test_row_kinds_differ_from_round_to_round():
    for name, (rows, cols) in rr.SHAPES.items():
        for unit in ("kth", "rows16"):
            stride = rr.stride_of(name, unit)
            if rows <= stride:
                continue
            for kinds in (4, 5):
                for shift in (0, 1):
                    kind = rr.row_kinds(rows, stride, kinds, shift)
                    assert set(kind.tolist()) == set(range(kinds))
    assert (rr.row_kinds(131081, 131072, 4) != rr.row_kinds(131081, 131072, 4, 1)).all(), "a shifted input changes every row's kind"
