"""Shapes past the grid caps of the per-row kernels (a helper module: no fixtures, no pytest settings).

The short-row kernels of topk.hip, topk16.hip, kth.hip, kth16.hip and rows16.hip are launched with a capped grid,
grid_for(items, per, cap), and every workgroup walks the rows in a grid-stride loop that carries LDS state from one row to the next.
A call with more than per * cap rows is what sends a wave or workgroup round that loop again.  test_gpu_row_rounds.py runs the
shapes below on the GPU; test_row_rounds_cpu.py reads the launch lines and fails when a raised cap leaves a shape inside the first
round.

Every shape is the smallest that goes round again AND ends on a partly filled round; the column counts put the row starts on every
phase of a 16-byte line (7 four-byte keys: all four; 13 two-byte keys: all eight) and 1025 is the shortest workgroup-tier row.
"""
import numpy as np

SHAPES = {
    "WAVE32": (131072 + 9, 7),        # top-k, k-th (32-bit): round 2 is one full workgroup and one with a single live wave
    "WAVE16": (131072 + 9, 13),       # top-k16, k-th16: the same for 2-byte keys
    "OFFS": (262144 + 5, 5),          # top-k, top-k16: third round of the short kernel, second sweep of row_offsets
    "GROUP": (4096 + 3, 1025),        # all five entries: three workgroups take a second row
    "ROWS16_WAVE": (32768 + 9, 13),   # rows16: past the wave tier's cap
}

# (unit, kernel as the launch line names it, items beyond `rows`, the shapes that must take it round again)
LAUNCHES = [
    ("topk", "topk_short_kernel<1>", 0, ("WAVE32", "OFFS")),
    ("topk16", "topk16_short_kernel<1>", 0, ("WAVE16", "OFFS")),
    ("kth", "kth_short_kernel<1>", 0, ("WAVE32",)),
    ("kth16", "kth16_short_kernel<1>", 0, ("WAVE16",)),
    ("topk", "topk_short_kernel<16>", 0, ("GROUP",)),
    ("topk16", "topk16_short_kernel<16>", 0, ("GROUP",)),
    ("kth", "kth_short_kernel<16>", 0, ("GROUP",)),
    ("kth16", "kth16_short_kernel<16>", 0, ("GROUP",)),
    ("rows16", "rows16_local_kernel<1, kWaveRegs>", 0, ("ROWS16_WAVE", "WAVE16")),
    ("rows16", "rows16_local_kernel<kGroupWaves, kGroupRegs>", 0, ("GROUP",)),
    ("topk", "topk_offsets_kernel", 1, ("OFFS",)),      # off[r] for r <= rows: rows + 1 items
    ("topk16", "topk16_offsets_kernel", 1, ("OFFS",)),
]

# rows one round of the row loop covers (per * cap): what `row // stride` and `row % stride` in a failure message refer to
STRIDE = {"wave": 8 * 16384, "group": 4096, "rows16 wave": 8 * 4096}
TIERS = {"wave": 1024, "group": 16384}   # kWaveSegCap, kLocalSortCap: the most keys of a wave-tier and of a workgroup-tier row


def stride_of(shape_name, unit):
    cols = SHAPES[shape_name][1]
    if cols > TIERS["wave"]:
        return STRIDE["group"]
    return STRIDE["rows16 wave"] if unit == "rows16" else STRIDE["wave"]


def row_kinds(rows, stride, kinds, shift=0):
    """kind of every row; row r and row r + stride -- the next row of the same wave or workgroup -- never share one.  Not r % kinds:
    every stride is a multiple of four."""
    r = np.arange(rows, dtype=np.int64)
    kind = (r + r // stride + shift) % kinds
    assert rows > stride and (kind[:-stride] != kind[stride:]).all(), "consecutive rounds must differ in kind"
    return kind


def mixed_rows(rows, cols, stride, bits, specials, seed, shift=0):
    """[rows, cols] bit patterns of `bits` bits (uint32 or uint16), each row of one kind: uniform bits | four values (tie runs) | all
    equal (the position must equal the rank) | all but the lowest digit shared (top 24 of 32 bits, top 11 of 16: every round of the
    select runs) | with `specials` (float types): those mixed in.  So consecutive rounds stop the select at different depths and
    leave different counters behind."""
    assert bits in (32, 16)
    dtype = np.uint32 if bits == 32 else np.uint16
    rng = np.random.default_rng(seed)
    kind = row_kinds(rows, stride, 5 if specials is not None else 4, shift)[:, None]
    uniform = rng.integers(0, 1 << bits, (rows, cols), dtype=np.uint64).astype(dtype)
    if bits == 32:
        four = np.array([5, 0x00010000, 0x7FFFFFFF, 0xFFFFFFF0], dtype=dtype)
        equal, shared = dtype(0x9E3779B9), dtype(0xABCDEF00) | rng.integers(0, 256, (rows, cols)).astype(dtype)
    else:
        four = np.array([5, 0x0100, 0x7FFF, 0xFFF0], dtype=dtype)
        equal, shared = dtype(0x9E37), dtype(0xABC0) | rng.integers(0, 32, (rows, cols)).astype(dtype)
    keys = np.where(kind == 0, uniform, four[rng.integers(0, 4, (rows, cols))])
    keys = np.where(kind == 2, equal, keys)
    keys = np.where(kind == 3, shared, keys)
    if specials is not None:
        if bits == 32:
            f = rng.standard_normal((rows, cols)).astype(np.float32).view(np.uint32)
        else:
            f = rng.integers(0, 1 << 16, (rows, cols), dtype=np.uint32).astype(dtype)
        f = np.where(rng.random((rows, cols)) < 0.3, specials[rng.integers(0, specials.size, (rows, cols))], f)
        keys = np.where(kind == 4, f, keys)
    return np.ascontiguousarray(keys.astype(dtype))
