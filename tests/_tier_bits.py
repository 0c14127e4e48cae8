"""Base rows, embeddings, flip points and the comparison engine of test_gpu_tier_bits.py and test_tier_bits_cpu.py (a helper module:
no fixtures, no pytest settings).  It stands on _topp16.py, _sample16.py, _temper16.py, _logprob16.py and _long_plan.py by import.

The three mass units -- topp16.hip's filter, sample16.hip's draw and logprob16.hip -- take a key's mass q from ONE device function and
add integers, so a row's result is an exact function of the row: it cannot depend on the size class that ran (one wavefront up to
WAVE_CAP keys, one workgroup up to GROUP_CAP, chunks above) nor on where the row's keys lie among the lanes, wave tiles and chunks.
Here a BASE ROW of B = 509 keys is embedded at offset L into rows of width W that are otherwise PADDING of zero mass (-inf, or the
negative quiet NaN), and every result is required to have the bits of the REFERENCE CONFIGURATION W = B, L = 0.  No tolerance enters:
the float64 oracle only anchors the reference configuration itself.

Equality at an arbitrary u or p proves little -- an error far below one float32 step of u Z changes nothing -- so u and p stand on
LADDERS: the 8 consecutive float32 values, 4 on each side, around the exact value at which the reference configuration's answer
flips from one key (one value) to the next, found by bisection over the bit pattern of the float32 on the device.

The engine works through an `ops` object (draw, filter, logprob on torch tensors of `ops.device`), so that it does not know the
library: test_gpu_tier_bits.py gives it the device entries, test_tier_bits_cpu.py a float64 restatement of the three size classes in
numpy, on which the engine itself is tested without a GPU -- including that a tier whose sum is off by 2^-22 of a key's mass fails it.

Part C's model: with the temperature whose float32 bits are 0x3FB8AA3B, c = float32(log2 e / T) is exactly 1, and integer logits
give q = 2^(32 + d) for d = x - best IF v_exp_f32 is exact at integers; Python integers then give Z, C, G and the filter's target."""
import functools
import math

import numpy as np

import _logprob16 as lg
import _long_plan as lp
import _sample16 as sm
import _temper16 as tm
import _topp16 as tp
from _rowk16 import sortable16_np

B = 509
WAVE_CAP, GROUP_CAP = 1024, lp.LOCAL_SORT_CAP          # kWaveSegCap, kLocalSortCap
LOAD_GROUP, LANE_ROUND, WAVE_TILE = 8, 512, 1024       # one 16-byte load, 64 lanes of them, a lane's two loads: kGroupKeys, 64 * 8, kWaveTile
WIDTHS = (B, 1024, 1025, 4099, 16384, 16385, 70001)
TIER_WIDTH = {"wave": 1024, "group": 4099, "long": 70001}   # parts B and C: one width per tier
SKIP = 3                                               # the buffer starts 3 elements behind a 16-byte line: rows have head keys
TYPES = tp.TYPES
NEG_NAN = {"bfloat16": 0xFFC0, "float16": 0xFE00}
PADS = {"-inf": tp.NEG_INF, "-nan": NEG_NAN}
T_LOG2E = np.array([0x3FB8AA3B], dtype=np.uint32).view(np.float32)[0]   # float32(log2 e): scale_of gives c == 1.0f
TEMPERATURES = (None, np.float32(0.7), np.float32(1.3), T_LOG2E)
MIN_P = np.float32(0.05)
ONE_BITS = 0x3F800000
PAIRS, LIGHT_PAIRS, LADDER = 12, 4, 8
LIGHT = 2.0 ** -10                                     # a light key weighs below this share of the row ..
CARRIES = 16.0                                         # .. and w * 2^32 >= 16 in float64: q > 0 on the device whatever its last ulp
BOUNDARY = (2.0 ** -20, 1.0 - 2.0 ** -10)
BUDGET = 8 << 20                                       # bytes of keys in one call: small widths take several ladder points a call


def tier_of(W):
    return "wave" if W <= WAVE_CAP else ("group" if W <= GROUP_CAP else "long")


def boundaries(W):
    """the row positions (up to the head keys, 0 .. 7 of them) at which a width has a lane round, a wave tile, a long tile or a chunk
    end: the first of each kind, and the last chunk boundary of the five-chunk width"""
    return [b for b in (LANE_ROUND, WAVE_TILE, lp.LONG_TILE, lp.MIN_CHUNK, 4 * lp.MIN_CHUNK) if b < W]


def offsets(W):
    """the offsets L of a width: 0 .. 9 (every phase of the 8-key load group), the row's end, and per boundary b the base row wholly in
    front of it whatever the head (b - B - 8), ending on it, across it at its middle and by four keys, and wholly behind it"""
    last = W - B
    at = set(range(10)) | {last - 1, last}
    for b in boundaries(W):
        at |= {b - B - 8, b - B, b - B // 2, b - 4, b + 8}
    return sorted(L for L in at if 0 <= L <= last)


def embed(base, W, L, pad):
    """pad * L + base + pad * (W - L - B)"""
    out = np.full(W, pad, dtype=np.uint16)
    out[L:L + B] = base
    return out


# ---- base rows ------------------------------------------------------------------------------------------------------------------------
class Base:
    """one base row with its fixed parameters: T None (no temperature array) or a float32, mp None (min-p off) or a float32"""

    def __init__(self, name, key_type, bits, T, mp):
        self.name, self.key_type, self.bits, self.T, self.mp = name, key_type, tp.without_fill(bits[None, :])[0], T, mp
        assert self.bits.shape == (B,) and not (self.bits == tp.FILL).any()

    def t(self):
        return 1.0 if self.T is None else self.T

    def __repr__(self):
        return f"{self.name} {self.key_type} T={self.T} mp={self.mp}"


def _lone(key_type, rng):
    v = 20.0 - rng.uniform(30.0, 50.0, B)
    at = rng.permutation(B)[:300]
    v[at] = 20.0 - rng.uniform(8.0, 14.0, 300)
    v[B // 2] = 20.0
    return tp.bits_of_values(v, key_type)


def _four(key_type, rng, values):
    pick = rng.integers(0, 4, B)
    pick[rng.permutation(B)[:4]] = np.arange(4)
    return tp.bits_of_values(np.array(values)[pick], key_type)


def _with_specials(key_type, rng, pos_inf):
    pinf, ninf = tp.POS_INF[key_type], tp.NEG_INF[key_type]
    nans = np.array([pinf + 1, ninf + 1, 0x7FFF, 0xFFFF, 0x7FC0 if key_type == "bfloat16" else 0x7E00, NEG_NAN[key_type]], dtype=np.uint16)
    row = tp.normal_rows(1, B, key_type, 4, int(rng.integers(1 << 30)))[0]
    order = rng.permutation(B)
    row[order[:50]] = nans[rng.integers(0, nans.size, 50)]
    row[order[50:80]] = ninf
    if pos_inf:
        row[order[80:120]] = pinf
    return row


FAMILIES = ("normal", "lone maximum", "four values", "nans", "+inf maximum")


@functools.lru_cache(maxsize=None)
def base_rows(key_type):
    """the twelve base rows of a key type: (family, temperature, min-p) fixed per row"""
    rng = np.random.default_rng(509 + TYPES.index(key_type))
    T = TEMPERATURES
    rows = [Base("normal", key_type, tp.normal_rows(1, B, key_type, 4, 11 + j)[0], T[j], (None, MIN_P, None, MIN_P)[j]) for j in range(4)]
    rows += [Base("lone maximum", key_type, _lone(key_type, rng), T[0], None), Base("lone maximum", key_type, _lone(key_type, rng), T[2], None)]
    rows += [Base("four values", key_type, _four(key_type, rng, (2.0, 1.0, -0.5, -6.0)), T[0], MIN_P),
             Base("four values", key_type, _four(key_type, rng, (3.0, 2.0, 0.5, -1.5)), T[1], None)]
    rows += [Base("nans", key_type, _with_specials(key_type, rng, False), T[0], None),
             Base("nans", key_type, _with_specials(key_type, rng, False), T[3], MIN_P)]
    rows += [Base("+inf maximum", key_type, _with_specials(key_type, rng, True), T[0], None),
             Base("+inf maximum", key_type, _with_specials(key_type, rng, True), T[2], MIN_P)]
    return tuple(rows)


def has_anchor(bits, key_type):
    """the condition under which -inf and NaN padding have zero mass: the row holds a finite number or a +inf"""
    v = tp.values64(bits, key_type)
    return bool((np.isfinite(v) | np.isposinf(v)).any())


def draw_variants(base):
    """the temperatures the draw runs a base row under: a row without one takes BOTH entries -- none, and the _ex entry with T = 1,
    which promises the same bits"""
    return [None, np.float32(1.0)] if base.T is None else [base.T]


def filter_variants(base):
    """(T, mp) likewise: a row with neither takes the plain entry and the _ex entry with T = 1 and min-p 0 (off)"""
    return [(None, None), (np.float32(1.0), np.float32(0.0))] if base.T is None and base.mp is None else [(base.T, base.mp)]


def filter_is_on(base, p):
    return (not tp.is_off(p)) or base.mp is not None


# ---- the pairs whose flip points carry the ladders --------------------------------------------------------------------------------------
def _spread(candidates, n):
    candidates = np.asarray(candidates, dtype=np.int64)
    if candidates.size <= n:
        return candidates.tolist()
    return candidates[np.unique(np.linspace(0, candidates.size - 1, n).round().astype(np.int64))].tolist()


def _choose(ok, light):
    """up to PAIRS of the candidates `ok`, the light ones first (up to half), both spread evenly over the row"""
    first = _spread(np.flatnonzero(ok & light), PAIRS // 2)
    rest = np.flatnonzero(ok)
    rest = rest[~np.isin(rest, first)]
    return sorted(first + _spread(rest, PAIRS - len(first)))


def draw_pairs(base):
    """[(i, j, C_j / Z, light)]: neighbouring mass-carrying POSITIONS of the float64 oracle under the row's T; the flip point of a
    pair is the smallest u whose index is at least j"""
    w, C, Z = tm.cdf(base.bits, base.key_type, base.t())
    mass = np.flatnonzero(w * 2.0 ** 32 >= CARRIES)
    i, j = mass[:-1], mass[1:]
    at = C[j] / Z
    ok = (at > BOUNDARY[0]) & (at < BOUNDARY[1])
    light = (w[i] / Z < LIGHT) & (w[j] / Z < LIGHT)
    return [(int(i[k]), int(j[k]), float(at[k]), bool(light[k])) for k in _choose(ok, light)]


def filter_pairs(base):
    """[(count, A / Z, light)]: neighbouring mass-carrying distinct VALUES (a, b) of the float64 oracle under the row's T, best first,
    b not beyond the strictest min-p threshold the oracle admits; `count` keys are at least as good as b, A is the mass strictly
    better than b: the flip point is the smallest p that keeps at least `count` keys"""
    s_row = sortable16_np(base.bits, base.key_type, True)
    s, first, count = np.unique(s_row, return_index=True, return_counts=True)
    g = tm.groups(base.bits, base.key_type, base.t())
    assert np.array_equal(g[0], s)
    mass, A, Z = g[1], g[2], g[3]
    carrying = np.flatnonzero(mass / count * 2.0 ** 32 >= CARRIES)
    a, b = carrying[:-1], carrying[1:]
    at = A[b] / Z
    ok = (at > BOUNDARY[0]) & (at < BOUNDARY[1])
    if base.mp is not None:
        ok &= b <= tm.minp_range_at(base.bits, base.key_type, base.t(), base.mp, s)[0]
    light = (mass[a] / Z < LIGHT) & (mass[b] / Z < LIGHT)
    return [(int((s_row <= s[b[k]]).sum()), float(at[k]), bool(light[k])) for k in _choose(ok, light)]


def bisect_flips(measure, targets):
    """per pair the smallest positive float32 bit pattern at which measure >= target: measure(bits [n] uint32) -> [n], monotone in
    the bits; below the flip at +0 and at or above it at 1.0 by construction of the pairs.  30 calls of `measure`."""
    targets = np.asarray(targets, dtype=np.int64)
    lo, hi = np.zeros(targets.size, dtype=np.int64), np.full(targets.size, ONE_BITS, dtype=np.int64)
    while (hi - lo > 1).any():
        mid = (lo + hi) // 2
        up = np.asarray(measure(mid.astype(np.uint32)), dtype=np.int64) >= targets
        hi, lo = np.where(up, mid, hi), np.where(up, lo, mid)
    assert ((hi > LADDER) & (hi < ONE_BITS - LADDER)).all(), f"a flip point at the end of the range: {hi.tolist()}"
    return hi.astype(np.uint32)


def ladders(flips):
    """[n * 8] float32: per flip point the 4 values below it and the 4 from it on"""
    bits = (np.asarray(flips, dtype=np.int64)[:, None] + np.arange(-LADDER // 2, LADDER // 2)[None, :]).reshape(-1)
    return bits.astype(np.uint32).view(np.float32)


def f32(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


# ---- logprob16's ids ---------------------------------------------------------------------------------------------------------------------
PAD_LOW = (-1, lg.INT32_MIN, -7)      # padding ids below 0 stay; those at or above the row length follow the width: W, W + 5, INT32_MAX
PAD_HIGH = (0, 5)
INT32_MAX = 2 ** 31 - 1


def base_ids(base):
    """(ids [32] int64, kind [32]): positions of the base row -- the maximum, a tie of it or of another value, the lightest keys that
    carry mass, a NaN and a -inf where the row holds one, both ends, random positions -- and padding ids: kind 0 a position, 1 a
    padding id kept as it is, 2 the width plus the id, 3 INT32_MAX"""
    rng = np.random.default_rng(B)
    v = tp.values64(base.bits, base.key_type)
    w, C, Z = tm.cdf(base.bits, base.key_type, base.t())
    number = ~np.isnan(v)
    top = np.flatnonzero(number & (v == v[number].max()))
    ids = [int(top[0]), int(top[-1]), 0, B - 1]
    values, first, count = np.unique(v[number], return_index=True, return_counts=True)
    if (count > 1).any():
        tied = values[np.flatnonzero(count > 1)[0]]
        ids += [int(x) for x in np.flatnonzero(v == tied)[:2]]
    carrying = np.flatnonzero(w * 2.0 ** 32 >= CARRIES)
    ids += [int(x) for x in carrying[np.argsort(w[carrying], kind="stable")[:6]]]
    for found in (np.flatnonzero(~number), np.flatnonzero(np.isneginf(v))):
        ids += [int(x) for x in found[:2]]
    ids = list(dict.fromkeys(ids))
    pads = [(x, 1) for x in PAD_LOW] + [(x, 2) for x in PAD_HIGH] + [(INT32_MAX, 3)]
    free = [int(x) for x in rng.permutation(B) if int(x) not in ids][:lg.MAX_SLOTS - len(ids) - len(pads)]
    both = [(x, 0) for x in ids + free] + pads
    assert len(both) == lg.MAX_SLOTS
    order = rng.permutation(lg.MAX_SLOTS)
    return np.array([both[k][0] for k in order], dtype=np.int64), np.array([both[k][1] for k in order], dtype=np.int64)


def ids_at(ids, kind, W, L, where=None):
    """the ids of a base row embedded at L into width W (`where`: the position of every base position, for a permuted row)"""
    at = ids if where is None else np.where(kind == 0, where[np.clip(ids, 0, B - 1)], ids)
    return np.where(kind == 0, at + L, np.where(kind == 2, W + ids, ids)).astype(np.int32)


# ---- the engine ----------------------------------------------------------------------------------------------------------------------------
def _torch():
    import torch
    return torch


def keys_on(ops, rows_bits, skip=SKIP):
    """[rows, W] uint16 on the host -> a contiguous [rows, W] int16 view `skip` elements into a buffer of ops.device (the to_dev of
    test_gpu_sample16.py)"""
    torch = _torch()
    rows, W = rows_bits.shape
    flat = torch.empty(rows * W + skip, dtype=torch.int16, device=ops.device)
    view = flat[skip:].view(rows, W)
    view.copy_(torch.from_numpy(np.ascontiguousarray(rows_bits).view(np.int16)))
    return view


def _f32_on(ops, values):
    return _torch().from_numpy(np.ascontiguousarray(values, dtype=np.float32).copy()).to(ops.device)


def _per_row(ops, value, rows):
    return None if value is None else _f32_on(ops, np.full(rows, value, dtype=np.float32))


def _calls(n_points, n_rows, W):
    """(R, calls): R ladder points share a call, each on its own copy of the rows"""
    R = int(min(max(BUDGET // (n_rows * W * 2), 1), n_points))
    return R, -(-n_points // R)


def _chunk(points, c, R):
    """the R points of call c (the last call is filled up with the first point) and how many of them count"""
    part = points[c * R:(c + 1) * R]
    return np.concatenate([part, np.repeat(points[:1], R - part.size)]), part.size


def run_draw(ops, key_type, rows_bits, points, T):
    """(index [n_points, n_rows] int64, logprob bits [n_points, n_rows] uint32): every row drawn at every point"""
    torch = _torch()
    n_rows, W = rows_bits.shape
    R, calls = _calls(points.size, n_rows, W)
    keys = keys_on(ops, np.tile(rows_bits, (R, 1)))
    d_T = _per_row(ops, T, R * n_rows)
    index, logprob = [], []
    for c in range(calls):
        pts, n = _chunk(points, c, R)
        i, l = ops.draw(keys, _f32_on(ops, np.repeat(pts, n_rows)), d_T, key_type)
        index.append(i.view(R, n_rows)[:n])
        logprob.append(l.view(R, n_rows)[:n])
    return torch.cat(index).cpu().numpy().astype(np.int64), torch.cat(logprob).cpu().numpy().view(np.uint32)


def run_filter(ops, key_type, rows_bits, points, T, mp, in_place=False):
    """out bits [n_points, n_rows, W] uint16 on the host: for small inputs (the reference configuration, the bisection)"""
    torch = _torch()
    n_rows, W = rows_bits.shape
    keys = keys_on(ops, np.tile(rows_bits, (points.size, 1)))
    out = ops.filter(keys, _f32_on(ops, np.repeat(points, n_rows)), _per_row(ops, mp, points.size * n_rows), _per_row(ops, T, points.size * n_rows),
                     key_type, keys if in_place else None)
    return out.contiguous().cpu().numpy().view(np.uint16).reshape(points.size, n_rows, W)


def compare_filter(ops, key_type, rows_bits, Ls, pad, points, T, mp, want, on, in_place):
    """bad [n_points, n_rows] bool: row r holds a base row at Ls[r] among `pad`; at point k its window differs from want[k] ([n_points,
    B] uint16), or a padding position does not hold the fill (on[k]) or the padding key (not on[k]).  Compared on the device."""
    torch = _torch()
    n_rows, W = rows_bits.shape
    R, calls = _calls(points.size, n_rows, W)
    master = keys_on(ops, np.tile(rows_bits, (R, 1)))
    work = keys_on(ops, np.tile(rows_bits, (R, 1))) if in_place else None
    d_T, d_mp = _per_row(ops, T, R * n_rows), _per_row(ops, mp, R * n_rows)
    window = torch.from_numpy(np.asarray(Ls, dtype=np.int64)[:, None] + np.arange(B)[None, :]).to(ops.device)          # [n_rows, B]
    is_pad = torch.ones((n_rows, W), dtype=torch.bool, device=ops.device)
    is_pad.scatter_(1, window, False)
    d_want = torch.from_numpy(np.ascontiguousarray(want).view(np.int16)).to(ops.device)
    filled = np.where(on, np.uint16(tp.FILL), np.uint16(pad)).astype(np.uint16)
    bad = []
    for c in range(calls):
        pts, n = _chunk(points, c, R)
        at = np.concatenate([np.arange(c * R, c * R + n), np.zeros(R - n, dtype=np.int64)])
        if in_place:
            work.copy_(master)
        out = ops.filter(work if in_place else master, _f32_on(ops, np.repeat(pts, n_rows)), d_mp, d_T, key_type, work if in_place else None)
        out = out.view(R, n_rows, W)
        got = out.gather(2, window[None].expand(R, n_rows, B))
        wrong = (got != d_want[torch.from_numpy(at).to(ops.device)][:, None, :]).any(2)
        in_pad = torch.from_numpy(filled[at].view(np.int16)).to(ops.device)
        wrong |= ((out != in_pad[:, None, None]) & is_pad[None]).any(2)
        bad.append(wrong[:n])
    if not in_place:
        assert torch.equal(master, keys_on(ops, np.tile(rows_bits, (R, 1)))), "the filter changed its input"
    return torch.cat(bad).cpu().numpy()


def run_logprob(ops, key_type, rows_bits, ids, T):
    """(logprob bits [rows, slots] uint32, rank [rows, slots] int64, lse bits [rows] uint32) of one call with ranks and lse"""
    torch = _torch()
    rows = rows_bits.shape[0]
    d_ids = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int32)).to(ops.device)
    logprob, rank, lse = ops.logprob(keys_on(ops, rows_bits), d_ids, _per_row(ops, T, rows), key_type)
    return logprob.cpu().numpy().view(np.uint32), rank.cpu().numpy().astype(np.int64), lse.cpu().numpy().view(np.uint32)


class Reference:
    """What the reference configuration (W = B, L = 0: copies of the base row alone, one per point) gives for a base row: its flip
    points found on `ops`, the ladders, and the results every embedding is compared with.  The results are held against the float64
    oracle's acceptance rules here, once."""

    def __init__(self, ops, base):
        self.base = base
        kt, row = base.key_type, base.bits[None, :]
        T, mp = base.T, base.mp
        # the draw
        self.draw_pairs = draw_pairs(base)
        target = np.array([j for i, j, at, light in self.draw_pairs], dtype=np.int64)
        n = target.size

        def drawn(bits):
            index, _ = ops.draw(keys_on(ops, np.tile(row, (n, 1)), 0), _f32_on(ops, f32(bits)), _per_row(ops, T, n), kt)
            return index.cpu().numpy()

        self.draw_flips = bisect_flips(drawn, target)
        self.u = np.concatenate([ladders(self.draw_flips), sm.U_CYCLE])
        self.index, self.logprob = (x[:, 0] for x in run_draw(ops, kt, row, self.u, T))
        keys = np.tile(row, (self.u.size, 1))
        tm.check_draws(self.index, keys, self.u, None if T is None else np.full(self.u.size, T, dtype=np.float32), kt, self.logprob.view(np.float32))
        if T is None:
            sm.check_rows(self.index, keys, self.u, kt, self.logprob.view(np.float32))
        on_ladder = self.index[:n * LADDER].reshape(n, LADDER)
        assert (on_ladder[:, :LADDER // 2] < target[:, None]).all() and (on_ladder[:, LADDER // 2:] >= target[:, None]).all(), \
            f"{base}: the draw does not flip where the bisection found it, in other row slots of the same configuration"
        # the filter
        self.filter_pairs = filter_pairs(base)
        self.p = tp.P_CYCLE
        self.filter_flips = np.zeros(0, dtype=np.uint32)
        if self.filter_pairs:
            count = np.array([c for c, at, light in self.filter_pairs], dtype=np.int64)

            m = count.size

            def kept(bits):   # one call: pair k in row k
                keys = keys_on(ops, np.tile(row, (m, 1)), 0)
                out = ops.filter(keys, _f32_on(ops, f32(bits)), _per_row(ops, mp, m), _per_row(ops, T, m), kt, None)
                return (out.cpu().numpy().view(np.uint16).reshape(m, B) != tp.FILL).sum(axis=1)

            self.filter_flips = bisect_flips(kept, count)
            self.p = np.concatenate([ladders(self.filter_flips), tp.P_CYCLE])
        self.on = np.array([filter_is_on(base, p) for p in self.p])
        self.out = run_filter(ops, kt, row, self.p, T, mp)[:, 0, :]
        k = self.p.size
        tm.check_rows(self.out, np.tile(row, (k, 1)), self.p, None if mp is None else np.full(k, mp, dtype=np.float32),
                      None if T is None else np.full(k, T, dtype=np.float32), kt)
        if self.filter_pairs:
            held = (self.out[:count.size * LADDER] != tp.FILL).sum(axis=1).reshape(count.size, LADDER)
            assert (held[:, :LADDER // 2] < count[:, None]).all() and (held[:, LADDER // 2:] >= count[:, None]).all(), \
                f"{base}: the filter does not flip where the bisection found it"
        # logprob16
        self.ids, self.kind = base_ids(base)
        self.lp, self.rank, self.lse = run_logprob(ops, kt, row, ids_at(self.ids, self.kind, B, 0)[None, :], T)
        lg.check_rows(self.lp.view(np.float32), self.rank, self.lse.view(np.float32), row, ids_at(self.ids, self.kind, B, 0)[None, :],
                      None if T is None else np.full(1, T, dtype=np.float32), kt)

    def ladder_count(self):
        return len(self.draw_pairs), len(self.filter_pairs)


def _first(bad):
    k, r = np.argwhere(bad)[0]
    return int(k), int(r)


def check_draw_embedded(ops, ref, W, pad_name, Ls=None, bits=None):
    """Part A for the draw: the base row of `ref` at every offset of the width, both entries where the row has no temperature.
    Returns the number of (configuration, point) comparisons."""
    base = ref.base
    pad = PADS[pad_name][base.key_type]
    Ls = offsets(W) if Ls is None else Ls
    rows_bits = np.stack([embed(base.bits if bits is None else bits, W, L, pad) for L in Ls])
    made = 0
    for T in draw_variants(base):
        index, logprob = run_draw(ops, base.key_type, rows_bits, ref.u, T)
        want = np.where(ref.index[:, None] >= 0, ref.index[:, None] + np.asarray(Ls)[None, :], -1)
        bad = (index != want) | (logprob != ref.logprob[:, None])
        if bad.any():
            k, r = _first(bad)
            raise AssertionError(f"{base}, W = {W} ({tier_of(W)} tier), L = {Ls[r]}, padding {pad_name}, entry T = {T}: at u = {ref.u[k]!r} (bits "
                                 f"{ref.u[k:k + 1].view(np.uint32)[0]:#x}) index - L = {index[k, r] - Ls[r]} logprob bits {logprob[k, r]:#x}; "
                                 f"the reference configuration gives {ref.index[k]} and {ref.logprob[k]:#x}; {int(bad.sum())} of {bad.size} differ")
        made += bad.size
    return made


def check_filter_embedded(ops, ref, W, pad_name, Ls=None, bits=None, want=None):
    """Part A for the filter: both entries where the row has neither T nor min-p, out of place and in place.  `bits`, `want`: a
    permuted base row and the reference's output permuted alike (part B)."""
    base = ref.base
    pad = PADS[pad_name][base.key_type]
    Ls = offsets(W) if Ls is None else Ls
    rows_bits = np.stack([embed(base.bits if bits is None else bits, W, L, pad) for L in Ls])
    made = 0
    for T, mp in filter_variants(base):
        for in_place in (False, True):
            bad = compare_filter(ops, base.key_type, rows_bits, Ls, pad, ref.p, T, mp, ref.out if want is None else want, ref.on, in_place)
            if bad.any():
                k, r = _first(bad)
                raise AssertionError(f"{base}, W = {W} ({tier_of(W)} tier), L = {Ls[r]}, padding {pad_name}, entry T = {T} mp = {mp}, "
                                     f"{'in place' if in_place else 'out of place'}: at p = {ref.p[k]!r} (bits {ref.p[k:k + 1].view(np.uint32)[0]:#x}) "
                                     f"the row differs from the reference configuration's; {int(bad.sum())} of {bad.size} differ")
            made += bad.size
    return made


def check_logprob_embedded(ops, ref, W, pad_name, Ls=None, bits=None, where=None):
    """Part A for logprob16: the 32 ids shifted by L (`where`: through a permutation, part B), with ranks and lse"""
    base = ref.base
    pad = PADS[pad_name][base.key_type]
    Ls = offsets(W) if Ls is None else Ls
    rows_bits = np.stack([embed(base.bits if bits is None else bits, W, L, pad) for L in Ls])
    ids = np.stack([ids_at(ref.ids, ref.kind, W, L, where) for L in Ls])
    made = 0
    for T in draw_variants(base):
        logprob, rank, lse = run_logprob(ops, base.key_type, rows_bits, ids, T)
        bad = (logprob != ref.lp) | (rank != ref.rank)
        bad[:, 0] |= lse != ref.lse[0]
        if bad.any():
            r, s = _first(bad)
            raise AssertionError(f"{base}, W = {W} ({tier_of(W)} tier), L = {Ls[r]}, padding {pad_name}, T = {T}: id {ids[r, s]} (slot {s}) gives logprob "
                                 f"bits {logprob[r, s]:#x} rank {rank[r, s]}, lse bits {lse[r]:#x}; the reference configuration {ref.lp[0, s]:#x}, "
                                 f"{ref.rank[0, s]}, {ref.lse[0]:#x}")
        made += bad.size
    return made


def permutations():
    """part B: name -> perm, the permuted row holds base[perm[k]] at k"""
    return {"reversed": np.arange(B)[::-1].copy(), "rotated": np.roll(np.arange(B), -(B // 2)), "shuffled": np.random.default_rng(B).permutation(B)}


# ---- part C: the absolute anchor on power-of-two masses -------------------------------------------------------------------------------------
MODEL_BEST = 5


@functools.lru_cache(maxsize=None)
def model_rows(key_type):
    """four rows of integer logits x = 5 + d, d in [-31, 0]: graded d with many ties, the light keys in front; (Base, d [B] int64)"""
    rng = np.random.default_rng(31)
    out = []
    for r in range(4):
        front = B // 3 + 17 * r
        d = np.concatenate([-rng.integers(12 + r, 32, front), -rng.integers(0, (6, 12, 24, 32)[r], B - front)]).astype(np.int64)
        d[front + r] = 0
        assert d.min() >= -31 and d.max() == 0
        bits = tp.bits_of_values((MODEL_BEST + d).astype(np.float64), key_type)
        assert np.array_equal(tp.values64(bits, key_type), MODEL_BEST + d), "integers are exact in both types"
        out.append((Base(f"model {r}", key_type, bits, T_LOG2E, None), d))
    return out


def model_masses(d):
    """q [B] int64 = 2^(32 + d), and Z as a Python integer"""
    q = np.left_shift(np.int64(1), (32 + d).astype(np.int64))
    return q, int(q.sum())


def model_index(d, u):
    """the device's arithmetic on exact masses: G = 0 for !(u > 0), Z - 1 for u >= 1, else min(Z - 1, floor(double(u) * double(Z)))"""
    q, Z = model_masses(d)
    u = np.float32(u)
    if not u > 0:
        G = 0
    elif u >= 1:
        G = Z - 1
    else:
        G = min(Z - 1, int(math.floor(float(u) * float(Z))))
    return int(np.searchsorted(np.cumsum(q), G, side="right"))


def model_kept(d, p):
    """[B] bool: target = ceil(double(p) * double(Z)) for p > 0, else 0; the threshold is the worst value whose strictly better
    mass is below the target, the best value for a target of 0; None where the filter is off"""
    if tp.is_off(p):
        return None
    q, Z = model_masses(d)
    p = np.float32(p)
    target = int(math.ceil(float(p) * float(Z))) if p > 0 else 0
    values = np.unique(d)[::-1]
    F, thr = 0, values[0]
    for v in values:
        if F < target:
            thr = v
        F += int(q[d == v].sum())
    return d >= thr


def model_ladders(base, d):
    """(u, p): the model's own flip points by bisection on the CPU, their ladders, and the cycles"""
    pairs = draw_pairs(base)
    flips = bisect_flips(lambda bits: [model_index(d, f32(bits)[k]) for k in range(len(pairs))], [j for i, j, at, light in pairs])
    fpairs = filter_pairs(base)
    fflips = bisect_flips(lambda bits: [B if tp.is_off(f32(bits)[k]) else int(model_kept(d, f32(bits)[k]).sum()) for k in range(len(fpairs))],
                          [c for c, at, light in fpairs])
    return np.concatenate([ladders(flips), sm.U_CYCLE]), np.concatenate([ladders(fflips), tp.P_CYCLE])


# ---- a float64 restatement of the three units, for the engine's own test without a GPU ---------------------------------------------------
class NumpyOps:
    """draw, filter and logprob of the engine's `ops` in numpy on CPU tensors: q = floor(exp2(float32((x - best) * c)) * 2^32) with
    float64's exp2, integer sums, the device's G and target.  Not the device's bits -- v_exp_f32 is not restated -- but an exact
    function of the row, which is all the engine asks.  `defect` = (tier, delta) adds delta to the mass of the first mass-carrying
    key of every row of that tier, in the draw and in the filter: what the engine must catch."""
    device = "cpu"

    def __init__(self, defect=None):
        self.defect = defect
        self.cache = {}

    def _row(self, bits, T, key_type):
        key = (bits.tobytes(), None if T is None else np.float32(T).tobytes(), key_type)
        if key not in self.cache:
            v = tp.values64(bits, key_type)
            number = ~np.isnan(v)
            c = np.float32(tm.LOG2E) if T is None else np.float32(tm.scale32(T))
            q = np.zeros(bits.size, dtype=np.int64)
            best = None
            if number.any():
                best = v[number].max()
                with np.errstate(invalid="ignore", over="ignore"):
                    e = ((v - best).astype(np.float32) * c).astype(np.float64)
                    w = np.where(v == best, 1.0, np.exp2(np.where(number & (v != best), e, -np.inf)))
                q = np.where(number, np.where(w >= 1.0, 2.0 ** 32, np.floor(w * 2.0 ** 32)), 0.0).astype(np.int64)
                if self.defect and tier_of(bits.size) == self.defect[0]:
                    q[np.flatnonzero(q)[0]] += self.defect[1]
            self.cache[key] = (v, number, best, c, q, sortable16_np(bits, key_type, True).astype(np.int64))
        return self.cache[key]

    @staticmethod
    def _bits(keys):
        return keys.contiguous().numpy().view(np.uint16)

    @staticmethod
    def _factor(c):
        return np.float32(1.0) if c == np.float32(tm.LOG2E) else np.float32(c * np.float32(0.6931471805599453))

    def draw(self, keys, u, T, key_type):
        torch = _torch()
        bits, u = self._bits(keys), u.numpy()
        index, logprob = np.full(bits.shape[0], -1, dtype=np.int32), np.full(bits.shape[0], np.nan, dtype=np.float32)
        for r in range(bits.shape[0]):
            v, number, best, c, q, s = self._row(bits[r], None if T is None else T[r].item(), key_type)
            Z = int(q.sum())
            if Z == 0:
                continue
            G = 0 if not u[r] > 0 else (Z - 1 if u[r] >= 1 else min(Z - 1, int(math.floor(float(u[r]) * float(Z)))))
            i = int(np.searchsorted(np.cumsum(q), G, side="right"))
            index[r] = i
            with np.errstate(invalid="ignore"):
                first = np.float32(0) if v[i] == best else np.float32(v[i] - best) * self._factor(c)
            logprob[r] = first - np.float32(np.log(np.float32(Z) * np.float32(2.0 ** -32)))
        return torch.from_numpy(index), torch.from_numpy(logprob)

    def filter(self, keys, p, mp, T, key_type, out):
        torch = _torch()
        bits, p = self._bits(keys), p.numpy()
        got = bits.copy()
        for r in range(bits.shape[0]):
            t = None if T is None else T[r].item()
            v, number, best, c, q, s = self._row(bits[r], t, key_type)
            off, mp_on = tp.is_off(p[r]), mp is not None and mp[r].item() > 0
            if off and not mp_on:
                continue
            keep = np.ones(bits.shape[1], dtype=bool)
            if mp_on:
                keep = s <= s.min()
                if best is not None:
                    with np.errstate(invalid="ignore", over="ignore"):
                        theta = best if np.isinf(c) else np.float32(best + min(float(1.0 if t is None else t), tm.T_MAX) * np.log(np.float32(mp[r].item())))
                        keep = (s <= s[number].min()) | (number & (v >= theta))
            if not off:
                Z = int(q.sum())
                target = int(math.ceil(float(p[r]) * float(Z))) if p[r] > 0 else 0
                order = np.argsort(s, kind="stable")
                inc = np.cumsum(q[order])
                values, start = np.unique(s[order], return_index=True)
                better = np.concatenate([[0], inc])[start]                      # the mass strictly better than each distinct value
                F = better[np.searchsorted(values, s)]
                keep &= (F < target) if target else (s == s.min())
            got[r] = np.where(keep, bits[r], np.uint16(tp.FILL))
        result = torch.from_numpy(got.view(np.int16))
        if out is not None:
            out.copy_(result)
            return out
        return result

    def logprob(self, keys, ids, T, key_type):
        torch = _torch()
        bits, ids = self._bits(keys), ids.numpy().astype(np.int64)
        rows, slots = ids.shape
        logprob, rank = np.full((rows, slots), np.nan, dtype=np.float32), np.full((rows, slots), -1, dtype=np.int32)
        lse = np.full(rows, np.nan, dtype=np.float32)
        for r in range(rows):
            v, number, best, c, q, s = self._row(bits[r], None if T is None else T[r].item(), key_type)
            Z = int(q.sum())
            log_z = np.float32(np.log(np.float32(Z) * np.float32(2.0 ** -32))) if Z else np.float32(np.nan)
            numbers = np.sort(v[number])
            for k in range(slots):
                i = ids[r, k]
                if not 0 <= i < bits.shape[1] or not number[i]:
                    continue
                rank[r, k] = numbers.size - np.searchsorted(numbers, v[i], side="right")
                with np.errstate(invalid="ignore", over="ignore"):
                    first = np.float32(0) if v[i] == best else (np.float32(-np.inf) if np.isinf(c) else np.float32(v[i] - best) * self._factor(c))
                logprob[r, k] = first - log_z
            if Z and not np.isinf(c):
                with np.errstate(invalid="ignore", over="ignore"):
                    lse[r] = np.float32(best) * self._factor(c) + log_z
        return torch.from_numpy(logprob), torch.from_numpy(rank), torch.from_numpy(lse)
