"""The chunk plan of the long-row selects restated, the shapes that reach each of its regimes, and the inputs and oracles of
test_gpu_long_plan.py and test_long_plan_cpu.py (a helper module: no fixtures, no pytest settings).

Rows above kLocalSortCap = 16384 keys are cut into chunks by radix_select.hpp's chunks_for(rows, cols):

    chunk   = max(kMinChunk, ceil(rows * cols / kMaxChunks)), rounded up to kLongTile keys
    per_row = ceil(cols / chunk)                      the chunks are counted from cols, chunk 0 owns the head keys as well
    cap     = min(kMaxChunks, ceil(cols / kMinChunk)) the row stride of the per-chunk `counts` arrays of the workspace

Below 2^25 keys the chunk is kMinChunk and per_row == cap.  SHAPES names the smallest odd shapes beyond that; REGIMES says what
each must reach, and test_long_plan_cpu.py holds both against the constants read from the sources.

Inputs.  The select families (uniform bits, four values, all equal) are bit patterns; the two rows of a family differ -- another
draw, other proportions of the four values -- so that one rank is found at far-apart positions.  The sharp rows of the top-p filter
and the draw are _sample16.sharp_rows' rows built once (that helper tiles the row once per heavy key: 1.5 GiB at 2^24 keys): HEAVY
keys of a level set among -inf, NaNs of both signs and a filler at -60.  The light keys weigh below 1e-20 of the row in float64 and
floor(w * 2^32) == 0 on the device, so the helpers' M = 2^-12 -- derived for cols <= 2^17 from a truncation of cols * 2^-32 -- is
far more than these rows need at any length: only the HEAVY keys truncate.  A row of 2^24 keys that all carry mass is NOT covered
by M: such rows would need the margin re-derived from the same budget, 4 * (2.9e-5 + cols * 2^-32), never fitted to what the device
returns.  None is used here."""
import functools

import numpy as np

import _rowk16 as rk
import _topp16 as tp
from _key_oracle import SPECIALS32

MIN_CHUNK, MAX_CHUNKS, LONG_TILE, LOCAL_SORT_CAP = 16384, 2048, 4096, 16384


def chunks_for(rows, cols):
    """(chunk, per_row) of radix_select.hpp's chunks_for"""
    chunk = max(MIN_CHUNK, -(-rows * cols // MAX_CHUNKS))
    chunk = -(-chunk // LONG_TILE) * LONG_TILE
    return chunk, -(-cols // chunk)


def chunk_cap_for(cols):
    return min(MAX_CHUNKS, -(-cols // MIN_CHUNK))


SHAPES = {
    "FIVE_TILES": (2, (1 << 24) + 4099),
    "WHOLE_ROW": (2049, 16385),
    "AT_CAP": (1, (1 << 25) - 3),
    "MANY_TILES": (1, (1 << 27) + 9),
}
# name -> (chunk, per_row, cap): the table of the plan, asserted by test_long_plan_cpu.py
PLAN = {"FIVE_TILES": (20480, 820, 1025), "WHOLE_ROW": (20480, 1, 2), "AT_CAP": (16384, 2048, 2048), "MANY_TILES": (69632, 1928, 2048)}
# the regimes a shape must reach (test_long_plan_cpu.py: REGIME_HOLDS)
REGIMES = {
    "FIVE_TILES": ("odd tiles", "per_row below cap", "above 512 chunks", "partial last chunk"),
    "WHOLE_ROW": ("whole row", "per_row below cap"),
    "AT_CAP": ("at cap", "above 512 chunks", "partial last chunk"),
    "MANY_TILES": ("odd tiles", "above 512 chunks"),
}
# unit of lsdradixsort_amd/csrc -> the entries of test_gpu_long_plan.py that run it; topk.hip's plan is run by test_gpu_topk.py
UNIT_ENTRIES = {
    "topk16": ("topk16",), "kth": ("kth",), "kth16": ("kth16",), "kth_multi": ("kth_multi",), "kth16_multi": ("kth16_multi",),
    "kth16_rowk": ("kth16_perrow", "topk16_filter"), "topp16": ("topp16_filter",), "sample16": ("sample16",),
}
UNITS_TESTED_ELSEWHERE = {"topk": "test_gpu_topk.py runs (1, 2^26) and (64, 2^22)"}

KEY_TYPE = "bfloat16"          # the 16-bit entries; the 32-bit ones take float32
SKIP = {2: 6, 4: 12}           # the first row lies 3 elements into its buffer: a head of 5 (16-bit) or 1 (32-bit) keys
FAMILIES = ("uniform bits", "four values", "all equal")
FOUR = {2: np.array([5, 0x0100, 0x7FFF, 0xFFF0], dtype=np.uint16), 4: np.array([5, 0x00010000, 0x7FFFFFFF, 0xFFFFFFF0], dtype=np.uint32)}
EQUAL = {2: 0x9E37, 4: 0x9E3779B9}
TOPK = {"FIVE_TILES": 4099, "WHOLE_ROW": 70, "AT_CAP": 4099}   # topk16's k: the winners of a uniform row come from every chunk


# ---- positions ------------------------------------------------------------------------------------------------------------------------
def head_of(row, cols, size):
    """the keys of row `row` in front of its first 16-byte line, the array starting SKIP[size] bytes behind one"""
    return min(cols, (-(SKIP[size] + row * cols * size) % 16) // size)


def heads(name, size):
    rows, cols = SHAPES[name]
    return sorted({head_of(r, cols, size) for r in range(min(rows, 16))})


def chunk_at(pos, head, chunk):
    """the chunk that owns row position `pos`"""
    return 0 if pos < head else (pos - head) // chunk


def boundary_positions(rows, cols, head):
    """Row positions on both sides of what the plan cuts at, for a row with `head` head keys: the row's ends, the head's end, the
    tile boundaries of chunk 0, and the chunk boundaries c * chunk + head - 1, c * chunk + head for c in {1, 511, 512, per_row - 1}
    -- chunk 0 with the head, another wave of the pick kernels, the last, partial chunk -- and a key in the fifth tile of chunk 512
    where chunks have one."""
    chunk, per_row = chunks_for(rows, cols)
    at = {0, head - 1, head, cols // 2, cols - 1}
    for t in range(1, min(chunk, cols) // LONG_TILE + 1):
        at |= {t * LONG_TILE + head - 1, t * LONG_TILE + head}
    for c in (1, 511, 512, per_row - 1):
        if 0 < c < per_row:
            at |= {c * chunk + head - 1, c * chunk + head}
    if per_row > 512 and chunk > 4 * LONG_TILE:
        at.add(512 * chunk + head + 4 * LONG_TILE + 1)
    return sorted(p for p in at if 0 <= p < cols)


def ranks_of(name, size):
    """the ranks every select entry is asked for at a shape: boundary_positions of every head its rows have.  In the all-equal
    family the position equals the rank, so these send the pick to each of those places."""
    rows, cols = SHAPES[name]
    return sorted({p for h in heads(name, size) for p in boundary_positions(rows, cols, h)})


# ---- the select families --------------------------------------------------------------------------------------------------------------
def _row_bits(kind, r, cols, size, rng):
    dtype = {2: np.uint16, 4: np.uint32}[size]
    if kind == "all equal":
        return np.full(cols, EQUAL[size], dtype=dtype)
    if kind == "four values":      # row r draws value j with probability (1, 2, 3, 4)[(j + r) % 4] / 10
        table = np.repeat(np.arange(4), np.roll([1, 2, 3, 4], -r))
        return FOUR[size][table[rng.integers(0, 10, cols)]]
    if size == 2:
        return rng.integers(0, 1 << 16, cols, dtype=np.uint32).astype(np.uint16)
    bits = rng.integers(0, 1 << 32, cols, dtype=np.uint64).astype(np.uint32)
    pick = rng.random(cols) < 0.3
    bits[pick] = SPECIALS32[rng.integers(0, SPECIALS32.size, int(pick.sum()))]   # +-0, +-inf, NaNs of both signs, denormals
    return bits


def row_kind(r):
    """WHOLE_ROW: rows r and r + 1 never share a kind"""
    return FAMILIES[r % 3]


@functools.lru_cache(maxsize=2)
def select_keys(name, size):
    """family -> [rows, cols] bit patterns of 2- or 4-byte keys, none of them the filter tests' fill word.  WHOLE_ROW has one
    family, "cycle": row r is of kind row_kind(r)."""
    rows, cols = SHAPES[name]
    rng = np.random.default_rng(cols + size)
    if name == "WHOLE_ROW":
        out = {"cycle": np.stack([_row_bits(row_kind(r), r, cols, size, rng) for r in range(rows)])}
    else:
        out = {kind: np.stack([_row_bits(kind, r, cols, size, rng) for r in range(rows)]) for kind in FAMILIES}
    if size == 2:
        for keys in out.values():
            keys[keys == rk.FILL] ^= np.uint16(1)
    return out


def sortable32_np(u, largest):
    """float32 bit patterns -> the uint32 whose unsigned order is the requested one (include/lsdsort.h's map restated)"""
    u = u.astype(np.uint32)
    u = u ^ ((u >> np.uint32(31)) * np.uint32(0x7FFFFFFF) | np.uint32(0x80000000))
    return ~u if largest else u


def stable_at_ranks_np(keys, size, largest, ranks, first=0):
    """(values [rows, R], positions [rows, R], first values [rows, first], first positions): the items at `ranks` and the first
    `first` items of every row's STABLE sort in the requested order -- numpy's stable argsort of the sortable map"""
    s = rk.sortable16_np(keys, KEY_TYPE, largest) if size == 2 else sortable32_np(keys, largest)
    order = np.argsort(s, axis=1, kind="stable")
    at, lead = order[:, list(ranks)], order[:, :first]
    return (np.take_along_axis(keys, at, axis=1), at.astype(np.uint32), np.take_along_axis(keys, lead, axis=1), lead.astype(np.uint32))


def stable_at_ranks_torch(bits, largest, ranks):
    """stable_at_ranks_np's values and positions for float32 bit patterns held in an int32 tensor [rows, cols] on any device:
    torch.sort(stable=True) of the sortable map as int64.  test_long_plan_cpu.py shows that the two agree."""
    import torch

    u = bits.to(torch.int64) & 0xFFFFFFFF
    s = u ^ torch.where(u >> 31 != 0, 0xFFFFFFFF, 0x80000000)
    order = torch.sort(0xFFFFFFFF - s if largest else s, dim=1, stable=True).indices
    at = order[:, list(ranks)]
    return torch.gather(bits, 1, at).cpu().numpy().view(np.uint32), at.cpu().numpy().astype(np.uint32)


def equal_oracle(name, size, first=0):
    """stable_at_ranks_np for the all-equal family without a sort: the one value, and the position is the rank, in both orders"""
    rows = SHAPES[name][0]
    ranks = np.array(ranks_of(name, size), dtype=np.uint32)
    dtype = {2: np.uint16, 4: np.uint32}[size]
    return (np.full((rows, ranks.size), EQUAL[size], dtype=dtype), np.tile(ranks, (rows, 1)),
            np.full((rows, first), EQUAL[size], dtype=dtype), np.tile(np.arange(first, dtype=np.uint32), (rows, 1)))


@functools.lru_cache(maxsize=8)
def select_oracle16(name, family):
    """largest -> stable_at_ranks_np of the 16-bit family at ranks_of(name, 2), with the first TOPK[name] items: ONE stable argsort
    per family and order"""
    if family == "all equal":
        return {largest: equal_oracle(name, 2, TOPK[name]) for largest in (False, True)}
    keys = select_keys(name, 2)[family]
    return {largest: stable_at_ranks_np(keys, 2, largest, ranks_of(name, 2), TOPK[name]) for largest in (False, True)}


def spread(ranks, shift, row, rows):
    """the index into `ranks` that row `row` takes in call `shift` of a per-row entry: neighbouring rows lie half the list apart
    (two rows) or one apart, so the rows of one call want different chunks"""
    return (shift + row * (len(ranks) // 2 if rows == 2 else 1)) % len(ranks)


# ---- sharp rows for the top-p filter and the draw -------------------------------------------------------------------------------------
def sharp_positions(rows, cols, head):
    """where the heavy keys of a long sharp row are forced: for the row's own head, _sample16.placement_positions' pairs (head + b -
    1, head + b) at the first load, and at the chunk boundaries b = c * chunk of boundary_positions instead of the first alone"""
    chunk, per_row = chunks_for(rows, cols)
    return [p for p in boundary_positions(rows, cols, head) if p < 8 + head or p >= chunk - 1]


def sharp_row(set_name, cols, key_type, seed, forced):
    """(row [cols], u [HEAVY] float32, at [HEAVY], the row's Draw): _sample16.sharp_rows' construction for ONE long row, not tiled.  HEAVY keys of the
    level set at `forced` and at random positions, every one at least 0.5 % of the row; u[i] is the midpoint of the interval of the
    key at at[i]."""
    import _sample16 as sm

    levels = tp.SHARP_SETS[set_name]
    rng = np.random.default_rng(seed)
    n = sm.HEAVY
    ninf, pinf = tp.NEG_INF[key_type], tp.POS_INF[key_type]
    filler = int(tp.bits_of_values(np.array([-60.0]), key_type)[0])
    # one light key in 32 is the filler: the float64 oracle looks at every key that has mass
    light = np.array([ninf] * 15 + [filler] + [pinf + 1, ninf + 1, 0x7FFF, 0xFFFF] * 4, dtype=np.uint16)
    row = light[rng.integers(0, light.size, cols)]
    forced = sorted(set(forced))
    assert len(forced) <= n and cols > 8 * n
    rest = [int(p) for p in dict.fromkeys(rng.integers(0, cols, 4 * n).tolist()) if p not in forced][:n - len(forced)]
    at = np.sort(np.array(forced + rest, dtype=np.int64))
    assert at.size == n
    for attempt in range(100):                                          # rejection, as in sharp_rows: none too light
        heavy = levels[rng.integers(0, levels.size, n)]
        w, C, Z = sm.cdf(heavy, key_type)                               # the light keys add below 1e-20 of it
        if not (heavy == tp.FILL).any() and (w / Z >= 0.0051).all():
            break
    row[at] = heavy
    assert not (row == tp.FILL).any()
    draw = Draw(row, key_type)
    own = np.searchsorted(draw.mass, at)                                # the heavy keys among the keys that have mass
    assert np.array_equal(draw.mass[own], at)
    light = np.ones(draw.mass.size, dtype=bool)
    light[own] = False
    assert (draw.w[own] / draw.Z >= 0.005).all() and draw.w[light].sum() < 1e-20 * draw.Z
    return row, ((2 * draw.C[own] + draw.w[own]) / (2 * draw.Z)).astype(np.float32), at, draw


class Draw:
    """the float64 oracle of _sample16 for one row, its sums computed once: exact index, acceptable indices and logprob per u"""

    def __init__(self, row, key_type):
        import _sample16 as sm

        self.sm = sm
        # _sample16.weights of the row's distinct bit patterns -- the same best number, the same weight per pattern -- looked up per
        # key: a row of 2^24 keys holds a few dozen patterns
        distinct = np.flatnonzero(np.bincount(row, minlength=1 << 16)).astype(np.uint16)
        v, w, self.best = sm.weights(distinct, key_type)
        table_v, table_w = np.zeros(1 << 16), np.zeros(1 << 16)
        table_v[distinct], table_w[distinct] = v, w
        self.row, self.table_v, w = row, table_v, table_w[row]
        inc = np.cumsum(w)
        self.mass = np.flatnonzero(w > 0)           # exact_from and acceptable_from look at the keys that have mass alone
        self.w, self.C, self.Z = w[self.mass], (inc - w)[self.mass], float(inc[-1]) if w.size else 0.0
        self.log_total = float(np.log(w.sum())) if self.Z else float("nan")

    def exact(self, u):
        i = self.sm.exact_from(self.w, self.C, self.Z, u)
        return i if i < 0 else int(self.mass[i])

    def acceptable(self, u):
        return [i if i < 0 else int(self.mass[i]) for i in self.sm.acceptable_from(self.w, self.C, self.Z, u)]

    def logprob(self, i):
        """_sample16.logprob64 from the sums already made"""
        v = self.table_v[self.row[i]]
        return (0.0 if v == self.best else float(v - self.best)) - self.log_total


class Nucleus:
    """the float64 oracle of _topp16 for one row, its groups computed once: _topp16.exact_threshold and _topp16.acceptable per p"""

    def __init__(self, row, key_type):
        # _topp16.groups from the counts of the row's bit patterns instead of a sort of the row
        count = np.bincount(row, minlength=1 << 16)
        bits = np.flatnonzero(count).astype(np.uint16)
        bits = bits[np.argsort(rk.sortable16_np(bits, key_type, True))]
        self.s = rk.sortable16_np(bits, key_type, True)
        v = tp.values64(bits, key_type)
        number = ~np.isnan(v)
        w = np.zeros(v.shape)
        if number.any():
            best = v[number].max()
            with np.errstate(invalid="ignore"):
                w[number] = np.where(v[number] == best, 1.0, np.exp(v[number] - best))
        self.mass = count[bits] * w
        self.A = np.cumsum(self.mass) - self.mass
        self.Z = float(self.mass.sum())
        self.sortable = rk.sortable16_np(np.arange(1 << 16, dtype=np.uint16), key_type, True)[row]
        self.row = row

    def threshold(self, p):
        kept = self.A < float(np.float32(p)) * self.Z
        kept[0] = True
        return int(self.s[np.flatnonzero(kept).max()])

    def acceptable(self, p, m=tp.M):
        p = float(np.float32(p))
        at = np.arange(self.s.size)
        ok = ((self.A < (p + m) * self.Z) | (at == 0)) & ((self.A + self.mass >= (p - m) * self.Z) | (at == self.s.size - 1))
        return [int(x) for x in self.s[ok]]

    def midpoints(self):
        """p at the midpoint of the mass of every value that carries at least 0.5 % of the row: [n] float32"""
        heavy = self.mass >= 0.005 * self.Z
        return ((2 * self.A + self.mass) / (2 * self.Z))[heavy].astype(np.float32)

    def filtered(self, p, fill=tp.FILL):
        """the filter's output for a p below 1, bit for bit"""
        return np.where(self.sortable <= self.threshold(p), self.row, np.uint16(fill))


SHARP_SET_OF_ROW = ("near two", "around zero", "three")


@functools.lru_cache(maxsize=1)
def _sharp(name):
    import _sample16 as sm

    rows, cols = SHAPES[name]
    if name == "WHOLE_ROW":
        base = [sm.sharp_rows(s, cols, KEY_TYPE, seed=cols + j, placement=True, rows=rows) for j, s in enumerate(SHARP_SET_OF_ROW)]
        keys = np.stack([base[r % 3][0][0] for r in range(rows)])
        return keys, [b[1] for b in base], [b[2] for b in base], [Draw(b[0][0], KEY_TYPE) for b in base]
    built = [sharp_row(SHARP_SET_OF_ROW[r % 3], cols, KEY_TYPE, cols + r, sharp_positions(rows, cols, head_of(r, cols, 2))) for r in range(rows)]
    return (np.stack([b[0] for b in built]),) + tuple([b[j] for b in built] for j in (1, 2, 3))


def sharp_inputs(name):
    """(keys [rows, cols] bfloat16 bits, u, at): per distinct row the float32 u and the positions of its sharp (row, u) pairs.
    FIVE_TILES and AT_CAP: sharp_row per row, another level set, head and seed each.  WHOLE_ROW: _sample16.sharp_rows' row of
    each of the three level sets; row r is the row of set r % 3 -- neighbours never share one -- and takes pair (r // 3) % HEAVY."""
    return _sharp(name)[:3]


def draws(name):
    """the Draw of every distinct sharp row of a shape (WHOLE_ROW: of rows 0, 1, 2, which the others repeat)"""
    return _sharp(name)[3]


@functools.lru_cache(maxsize=1)
def nuclei(name):
    """the Nucleus of every distinct sharp row of a shape"""
    keys = sharp_inputs(name)[0]
    return [Nucleus(keys[j], KEY_TYPE) for j in range(min(3, keys.shape[0]))]


def whole_row_u(keys_u):
    """WHOLE_ROW: the u (or p) of every row from the three per-set lists: row r takes entry (r // 3) % len of set r % 3"""
    rows = SHAPES["WHOLE_ROW"][0]
    return np.array([keys_u[r % 3][(r // 3) % len(keys_u[r % 3])] for r in range(rows)], dtype=np.float32)


def sharp_p(name):
    """per distinct sharp row the p at the midpoint of every heavy value's mass"""
    return [nucleus.midpoints() for nucleus in nuclei(name)]


def _paired(per_row):
    """[calls][rows]: call i gives even rows their entry i and odd rows their entry n - 1 - i (a shorter list goes round): the rows
    of a call want far-apart chunks"""
    n = max(len(v) for v in per_row)
    return [np.array([v[(i if r % 2 == 0 else n - 1 - i) % len(v)] for r, v in enumerate(per_row)], dtype=np.float32) for i in range(n)]


def draw_cases(name):
    """the u [rows] of every call of the draw at a shape.  Long rows: the pairs whose heavy key sits at a forced position."""
    keys, u, at = sharp_inputs(name)
    if name == "WHOLE_ROW":
        return [whole_row_u(u)]
    rows, cols = SHAPES[name]
    forced = [set(sharp_positions(rows, cols, head_of(r, cols, 2))) for r in range(rows)]
    return _paired([[u[r][i] for i, p in enumerate(at[r]) if int(p) in forced[r]] for r in range(rows)])


def nucleus_cases(name):
    """the p [rows] of every call of the top-p filter at a shape"""
    return [whole_row_u(sharp_p(name))] if name == "WHOLE_ROW" else _paired(sharp_p(name))


def equal_draws(name, head):
    """(u [n] float32, index [n]): for a row of equal keys, u aimed at boundary_positions and the index the draw must return,
    min(cols - 1, floor(u_c * cols)) -- exact in a double: 24 bits times at most 28"""
    rows, cols = SHAPES[name]
    u = np.array([(p + 0.5) / cols for p in boundary_positions(rows, cols, head)] + [0.0, 1.0, 1.5, -1.0, np.nan], dtype=np.float32)
    index = [min(cols - 1, int(np.floor(min(max(float(x), 0.0), 1.0) * cols))) if not np.isnan(x) else 0 for x in u]
    return u, np.array(index, dtype=np.int64)
