"""The key map of include/lsdsort.h restated in numpy, the stable order of every row, the special bit patterns and the input
families of the select and top-k suites (a helper module: no fixtures, no pytest settings; numpy only, importable without a device).

Every bit-exact suite for typed keys holds the library against these functions, never against the package's own tables, and
test_key_oracle_cpu.py holds these functions against an independent statement of the order.  A suite imports from here; it does
not restate."""
import numpy as np

# the key-type codes of include/lsdsort.h (LSDSORT_KEY16_*, LSDSORT_KEY_*), restated
KEY_TYPES16 = {"uint16": 0, "int16": 1, "float16": 2, "bfloat16": 3}
KEY_TYPES32 = {"uint32": 0, "int32": 1, "float32": 2}
KEY_TYPES64 = {"uint64": 3, "int64": 4, "float64": 5}
ALL_TYPES16, ALL_TYPES32, ALL_TYPES64 = list(KEY_TYPES16), list(KEY_TYPES32), list(KEY_TYPES64)

# +-0, +-inf, NaNs of both signs (quiet, signalling, all ones), denormals, the largest finite values, +-1
SPECIALS16 = {
    "float16": np.array([0x0000, 0x8000, 0x7C00, 0xFC00, 0x7E00, 0xFE00, 0x7C01, 0xFC01, 0xFFFF, 0x7FFF, 0x0001, 0x8001, 0x03FF,
                         0x83FF, 0x7BFF, 0xFBFF, 0x3C00, 0xBC00], dtype=np.uint16),
    "bfloat16": np.array([0x0000, 0x8000, 0x7F80, 0xFF80, 0x7FC0, 0xFFC0, 0x7F81, 0xFF81, 0xFFFF, 0x7FFF, 0x0001, 0x8001, 0x007F,
                          0x807F, 0x7F7F, 0xFF7F, 0x3F80, 0xBF80], dtype=np.uint16),
}
SPECIALS32 = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF,
                       0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x7FFFFFFF, 0x3F800000, 0xBF800000], dtype=np.uint32)


# ---- the map --------------------------------------------------------------------------------------------------------------------
def sortable16_np(u, key_type, largest):
    """the uint16 whose unsigned order is the requested one (`largest`: descending)"""
    u = u.astype(np.uint32)
    if key_type == "int16":
        u = u ^ np.uint32(0x8000)
    elif key_type in ("float16", "bfloat16"):
        u = u ^ np.where(u & np.uint32(0x8000), np.uint32(0xFFFF), np.uint32(0x8000))
    return ((u ^ np.uint32(0xFFFF)) if largest else u).astype(np.uint16)


def from_sortable16_np(s, key_type):
    """the key whose ascending sortable value is s"""
    s = s.astype(np.uint32)
    if key_type == "int16":
        s = s ^ np.uint32(0x8000)
    elif key_type in ("float16", "bfloat16"):
        s = np.where(s & np.uint32(0x8000), s ^ np.uint32(0x8000), s ^ np.uint32(0xFFFF))
    return s.astype(np.uint16)


def sortable_np(u, key_type, descending):
    """the uint32 whose unsigned order is the requested one"""
    u = u.astype(np.uint32)
    if key_type == "int32":
        u = u ^ np.uint32(0x80000000)
    elif key_type == "float32":
        u = u ^ ((u >> np.uint32(31)) * np.uint32(0x7FFFFFFF) | np.uint32(0x80000000))
    return ~u if descending else u


def from_sortable_np(s, key_type):
    """the key whose ascending sortable value is s"""
    s = s.astype(np.uint32)
    if key_type == "int32":
        return s ^ np.uint32(0x80000000)
    if key_type == "float32":
        return np.where(s >> np.uint32(31) != 0, s ^ np.uint32(0x80000000), ~s).astype(np.uint32)
    return s


def expected_np(keys, key_type, largest):
    """keys: [rows, cols] uint16 or uint32 bits (by key_type) -> the full stable order of every row: (sorted keys, positions)"""
    s = sortable16_np(keys, key_type, largest) if key_type in KEY_TYPES16 else sortable_np(keys, key_type, largest)
    order = np.argsort(s, axis=1, kind="stable")
    return np.take_along_axis(keys, order, axis=1), order.astype(np.uint32)


# ---- input families -------------------------------------------------------------------------------------------------------------
# the families of the single-rank suites, and those of the multi-rank ones (tests/test_gpu_kth16_multi.py, test_gpu_kth_multi.py)
FAMILIES16 = ("uniform bits", "four values", "all equal", "shared top 11 bits", "shared top 8 bits", "lone minimum", "float specials")
MULTI_RANK16 = ("uniform bits", "four values", "all equal", "shared top 11 bits", "lone minimum", "float specials", "outliers")
FAMILIES32 = ("uniform bits", "four values", "all equal", "shared top 24 bits", "bit 0 only", "float specials")
MULTI_RANK32 = FAMILIES32 + ("outliers",)


def inputs16(rows, cols, key_type, seed, families=FAMILIES16):
    """name -> [rows, cols] uint16 bit patterns: those of `families`, drawn in the order below from one seeded generator (a family
    left out draws nothing).  "float specials" exists for the float types, "outliers" (which builds on "shared top 11 bits") from 8
    columns on."""
    rng = np.random.default_rng(seed)

    def rnd(hi):
        return rng.integers(0, hi, (rows, cols), dtype=np.uint32).astype(np.uint16)

    out = {}
    if "uniform bits" in families:
        out["uniform bits"] = rnd(1 << 16)
    if "four values" in families:                                                # tie runs across lanes, waves and chunks
        out["four values"] = np.array([5, 0x0100, 0x7FFF, 0xFFF0], dtype=np.uint16)[rng.integers(0, 4, (rows, cols))]
    if "all equal" in families:                                                  # the position must equal the rank
        out["all equal"] = np.full((rows, cols), 0x9E37, dtype=np.uint16)
    if "shared top 11 bits" in families:                                         # the second level decides; long rows are all ties
        out["shared top 11 bits"] = np.uint16(0xABC0) | rnd(32)
    if "shared top 8 bits" in families:
        out["shared top 8 bits"] = np.uint16(0xAB00) | rnd(256)
    if "lone minimum" in families:
        lone = np.full((rows, cols), 0x4000, dtype=np.uint16)                    # one 0x0001 among 0x4000s: the select stops after
        lone[np.arange(rows), rng.integers(0, cols, rows)] = 0x0001              # the first level or round, with a nonzero shift
        out["lone minimum"] = lone
    if "float specials" in families and key_type in SPECIALS16:
        f = rnd(1 << 16).reshape(-1)
        pick = rng.random(rows * cols) < 0.3
        f[pick] = SPECIALS16[key_type][rng.integers(0, SPECIALS16[key_type].size, int(pick.sum()))]
        out["float specials"] = f.reshape(rows, cols)
    if "outliers" in families and cols >= 8:
        # In sortable order: three keys of unique top 11 bits at each end of a row that otherwise shares its top 11 bits.  Ranks 0, 1
        # and cols - 1 finish at level 0 while the middle ranks run level 1: done and live slots side by side.
        s = out["shared top 11 bits"].copy()
        ends = np.array([0x0020, 0x0040, 0x0060, 0xFFA0, 0xFFC0, 0xFFE0], dtype=np.uint16)
        for r in range(rows):
            where = rng.choice(cols, ends.size, replace=False)
            s[r, where] = ends | rng.integers(0, 32, ends.size).astype(np.uint16)
        out["outliers"] = from_sortable16_np(s, key_type)
    return out


def inputs32(rows, cols, key_type, seed, families=FAMILIES32):
    """name -> [rows, cols] uint32: the 32-bit counterpart of inputs16 ("float specials" for float32, "outliers" on "shared top 24
    bits")"""
    rng = np.random.default_rng(seed)
    out = {}
    if "uniform bits" in families:
        out["uniform bits"] = rng.integers(0, 1 << 32, (rows, cols), dtype=np.uint64).astype(np.uint32)
    if "four values" in families:                                                # tie runs across lanes, waves and chunks
        out["four values"] = np.array([5, 0x00010000, 0x7FFFFFFF, 0xFFFFFFF0], dtype=np.uint32)[rng.integers(0, 4, (rows, cols))]
    if "all equal" in families:                                                  # the position must equal the rank
        out["all equal"] = np.full((rows, cols), 0x9E3779B9, dtype=np.uint32)
    if "shared top 24 bits" in families:                                         # every level runs
        out["shared top 24 bits"] = np.uint32(0xABCDEF00) | rng.integers(0, 256, (rows, cols)).astype(np.uint32)
    if "bit 0 only" in families:
        out["bit 0 only"] = np.uint32(0x40302010) | rng.integers(0, 2, (rows, cols)).astype(np.uint32)
    if "float specials" in families and key_type == "float32":
        f = rng.standard_normal(rows * cols).astype(np.float32).view(np.uint32).copy()
        pick = rng.random(rows * cols) < 0.3
        f[pick] = SPECIALS32[rng.integers(0, SPECIALS32.size, int(pick.sum()))]  # +-0, +-inf, NaNs of both signs, denormals
        out["float specials"] = f.reshape(rows, cols)
    if "outliers" in families and cols >= 8:
        # In sortable order: three keys of unique top bits at each end of a row that otherwise shares its top 24 bits.  Ranks 0, 1
        # and cols - 1 stop at level 0 while the middle ranks run every level: done and live slots side by side.
        s = out["shared top 24 bits"].copy()
        ends = np.array([0x00200000, 0x00400000, 0x00600000, 0xFFA00000, 0xFFC00000, 0xFFE00000], dtype=np.uint32)
        for r in range(rows):
            where = rng.choice(cols, ends.size, replace=False)
            s[r, where] = ends | rng.integers(0, 1 << 20, ends.size).astype(np.uint32)
        out["outliers"] = from_sortable_np(s, key_type)
    return out


def make_keys16(rows, cols, key_type, seed):
    """[rows, cols] uint16: random bits; the float types with 30 % specials"""
    rng = np.random.default_rng(seed)
    n = rows * cols
    keys = rng.integers(0, 1 << 16, n, dtype=np.uint32).astype(np.uint16)
    if key_type in SPECIALS16:
        pick = rng.random(n) < 0.3
        keys[pick] = SPECIALS16[key_type][rng.integers(0, SPECIALS16[key_type].size, int(pick.sum()))]
    return keys.reshape(rows, cols)


def make_keys32(rows, cols, key_type, seed):
    """[rows, cols] uint32: float32 as normal variates with 30 % specials; the integer types as random bits with a tenth each of
    0x80000000 and 0x7FFFFFFF"""
    rng = np.random.default_rng(seed)
    n = rows * cols
    if key_type == "float32":
        keys = rng.standard_normal(n).astype(np.float32).view(np.uint32).copy()
        pick = rng.random(n) < 0.3
        keys[pick] = SPECIALS32[rng.integers(0, SPECIALS32.size, int(pick.sum()))]
    else:
        keys = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        keys[rng.random(n) < 0.1] = np.uint32(0x80000000)
        keys[rng.random(n) < 0.1] = np.uint32(0x7FFFFFFF)
    return keys.reshape(rows, cols)
