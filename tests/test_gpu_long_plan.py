"""GPU suite: the long tier of every row-select entry above 2^25 keys, where radix_select.hpp's chunk plan leaves the one regime
every other test runs (chunks of exactly 16384 keys, as many chunks per row as the `counts` stride, at most 65 chunks).

The shapes are tests/_long_plan.py's (test_long_plan_cpu.py holds them against the constants of the sources):

    FIVE_TILES (2, 2^24 + 4099)   chunks of five tiles, 820 chunks per row under a `counts` stride of 1025, a second row, a partial
                                  last chunk, 13 chunks per lane in sample16's pick
    WHOLE_ROW  (2049, 16385)      the chunk is longer than the row: one chunk per row under a stride of 2
    AT_CAP     (1, 2^25 - 3)      2048 chunks of 16384 keys: every thread of a pick kernel has eight live chunks
    MANY_TILES (1, 2^27 + 9)      chunks of 17 tiles, 1928 of them; rows of equal keys filled on the device, no host oracle

Entries: topk16, kth, kth16, kth_multi, kth16_multi, kth16_perrow, topk16_filter, topp16_filter and sample16, each through its raw C
entry with every array inside guard zones, a workspace of exactly the reported figure, and afterwards: zones intact, fault word
zero, inputs unchanged.  bfloat16 for the 16-bit entries, float32 with its specials for the 32-bit ones: the key maps have their
own tests.  The 32-bit lsdsort_topk_device is left out on purpose: test_gpu_topk.py already runs this plan at (1, 2^26) and
(64, 2^22).

References, none of them the library: the items at the wanted ranks of ONE stable argsort per (shape, family, order) -- numpy for
16-bit keys, torch.sort(stable=True) on the device for 32-bit keys (test_long_plan_cpu.py shows the two agree) --, nothing but
"the position is the rank" for rows of equal keys, and the float64 oracles of _topp16.py and _sample16.py on sharp rows, where
acceptance is equality.  Ranks, k and u aim at both sides of the chunk boundaries 1, 511, 512 and per_row - 1, at the head and at
the fifth tile of a chunk; the rows of one call want chunks far apart, so that a row stride of `chunks` in place of `chunk_cap`
(or a slot stride in the multi-rank units) returns another row's answer.

Inputs are built once per (shape, family) by _long_plan.py and uploaded once per shape (`held`); the next shape frees them."""
import ctypes

import numpy as np
import pytest
import torch

import _long_plan as lp
import _rowk16 as rk
import _sample16 as sm
import _topp16 as tp
import lsdradixsort_amd as lsd
from _guarded import GUARD, assert_intact, guarded, guarded_workspace
from _guarded16 import SENT16, assert_intact16, bits_of, guarded16

pytestmark = pytest.mark.gpu

KT16, KT32 = 3, 2                       # bfloat16 of lsdsort_key16_type, float32 of lsdsort_key_type
POISON16, POISON32 = 0x5A5A, 0x5A5A5A5A
BIG = ("FIVE_TILES", "WHOLE_ROW", "AT_CAP")
ORDERS = (False, True)

_held = {"shape": None}


def held(name, key, make):
    """what `make` returns, kept while the tests stay at shape `name`"""
    if _held["shape"] != name:
        _held.clear()
        _held["shape"] = name
        torch.cuda.empty_cache()
    if key not in _held:
        _held[key] = make()
    return _held[key]


def stream():
    return int(torch.cuda.current_stream().cuda_stream)


def families(name):
    return ("cycle",) if name == "WHOLE_ROW" else lp.FAMILIES


def select_dev(name, family, size):
    """(whole, view) of a select family on the device, the first row 3 elements behind a 16-byte line"""
    def make():
        host = lp.select_keys(name, size)[family]
        return guarded16(host, lp.SKIP[2], torch.bfloat16) if size == 2 else guarded(host, lp.SKIP[4])
    return held(name, (family, size), make)


def oracle(name, family, size):
    """largest -> (values [rows, R], positions [rows, R]) at lp.ranks_of(name, size)"""
    if size == 2:
        return {largest: o[:2] for largest, o in lp.select_oracle16(name, family).items()}
    if family == "all equal":
        return {largest: lp.equal_oracle(name, 4)[:2] for largest in ORDERS}
    rows, cols = lp.SHAPES[name]
    view = select_dev(name, family, 4)[1].view(rows, cols)
    return held(name, ("oracle32", family), lambda: {largest: lp.stable_at_ranks_torch(view, largest, lp.ranks_of(name, 4)) for largest in ORDERS})


def out16(n):
    return guarded16(np.zeros(n, dtype=np.uint16), 2)


def out32(n):
    return guarded(np.zeros(n, dtype=np.uint32))


def bits32(view):
    return view.cpu().numpy().view(np.uint32)


def workspace(figure):
    assert figure > 0 and figure % 256 == 0, figure
    return guarded_workspace(figure) + (figure,)


def settle(wv, what):
    torch.cuda.synchronize()
    assert lsd.lib().lsdsort_check_device(wv.data_ptr(), None) == 0, f"{what}: lsdsort_check_device"
    fault = int(wv[:4].view(torch.int32).item())
    assert fault == 0, f"{what}: fault word {fault:#x}"


def unchanged(name, family, size):
    host = lp.select_keys(name, size)[family].reshape(-1)
    view = select_dev(name, family, size)[1]
    got = bits_of(view) if size == 2 else bits32(view)
    assert np.array_equal(got, host), f"{name} {family}: a read-only input was changed"


def equal_rows(name, family):
    """the rows of a family that hold one value: there the position must equal the rank"""
    rows = lp.SHAPES[name][0]
    if family == "all equal":
        return np.arange(rows)
    return np.array([r for r in range(rows) if lp.row_kind(r) == "all equal"]) if family == "cycle" else np.array([], dtype=np.int64)


# ---- one rank for every row: kth16 and kth ------------------------------------------------------------------------------------------
def run_kth(name, size):
    rows, cols = lp.SHAPES[name]
    L = lsd.lib()
    fn, figure, kt = ((L.lsdsort_kth16_device, L.lsdsort_kth16_workspace_bytes, KT16) if size == 2 else
                      (L.lsdsort_kth_device, L.lsdsort_kth_workspace_bytes, KT32))
    ww, wv, need = workspace(figure(rows, cols))
    ow, ov = out16(rows) if size == 2 else out32(rows)
    iw, iv = out32(rows)
    ranks = lp.ranks_of(name, size)
    for family in families(name):
        kw, kv = select_dev(name, family, size)
        same = equal_rows(name, family)
        picked = [set() for _ in range(rows)]
        for largest in ORDERS:
            ev, ei = oracle(name, family, size)[largest]
            for j, rank in enumerate(ranks):
                for with_idx in (True, False) if j % 4 == 0 else (True,):
                    what = f"{name} {family} largest={largest} rank={rank} indices={with_idx}"
                    ov.fill_(POISON16 if size == 2 else POISON32)
                    iv.fill_(POISON32)
                    st = fn(kv.data_ptr(), rows, cols, rank, kt, int(largest), ov.data_ptr(), iv.data_ptr() if with_idx else None,
                            wv.data_ptr(), need, stream())
                    assert st == 0, (what, st)
                    settle(wv, what)
                    got = bits_of(ov) if size == 2 else bits32(ov)
                    assert np.array_equal(got, ev[:, j]), f"{what}: values {got[:4]} want {ev[:4, j]}"
                    gi = bits32(iv)
                    if with_idx:
                        assert np.array_equal(gi, ei[:, j]), f"{what}: positions {gi[:4]} want {ei[:4, j]}"
                        assert (gi[same] == rank).all(), f"{what}: the position must equal the rank in a row of equal keys"
                        for r in range(min(rows, 2)):
                            picked[r].add(lp.chunk_at(int(gi[r]), lp.head_of(r, cols, size), lp.chunks_for(rows, cols)[0]))
                    else:
                        assert (gi == POISON32).all(), f"{what}: no index buffer was given: nothing may be written"
        if name != "WHOLE_ROW":
            last = lp.chunks_for(rows, cols)[1] - 1
            assert any(512 <= c for c in picked[0]), f"{name} {family}: picks went to {sorted(picked[0])}"
            if family == "all equal":
                assert {0, 1, 511, 512, last} <= picked[0], f"{name} {family}: picks went to {sorted(picked[0])}"
            elif rows > 1:
                assert picked[0] != picked[1], f"{name} {family}: both rows picked the same chunks"
        (assert_intact16 if size == 2 else assert_intact)(keys=kw, values=ow)
        assert_intact(indices=iw, workspace=ww)
        unchanged(name, family, size)


# ---- several ranks for every row: kth16_multi and kth_multi -------------------------------------------------------------------------
def run_multi(name, size):
    rows, cols = lp.SHAPES[name]
    L = lsd.lib()
    fn, figure, kt = ((L.lsdsort_kth16_multi_device, L.lsdsort_kth16_multi_workspace_bytes, KT16) if size == 2 else
                      (L.lsdsort_kth_multi_device, L.lsdsort_kth_multi_workspace_bytes, KT32))
    ranks = lp.ranks_of(name, size)
    n_groups = -(-len(ranks) // 8)
    groups = [list(range(g, len(ranks), n_groups)) for g in range(n_groups)]   # indices into ranks: every group spans the whole row
    chunk, per_row = lp.chunks_for(rows, cols)
    if per_row > 512:
        assert all(ranks[g[-1]] - ranks[g[0]] > 512 * chunk for g in groups), "the slots of a call lie more than 512 chunks apart"
    for family in families(name):
        kw, kv = select_dev(name, family, size)
        same = equal_rows(name, family)
        for largest in ORDERS:
            ev, ei = oracle(name, family, size)[largest]
            for n, group in enumerate(groups):
                m = len(group)
                asked = [ranks[j] for j in (group if n % 2 == 0 else group[::-1])]   # any order
                cols_of = group if n % 2 == 0 else group[::-1]
                ww, wv, need = workspace(figure(rows, cols, m))
                ow, ov = out16(rows * m) if size == 2 else out32(rows * m)
                iw, iv = out32(rows * m)
                for with_idx in (True, False) if n == 0 else (True,):
                    what = f"{name} {family} largest={largest} ranks={asked} indices={with_idx}"
                    ov.fill_(POISON16 if size == 2 else POISON32)
                    iv.fill_(POISON32)
                    st = fn(kv.data_ptr(), rows, cols, (ctypes.c_size_t * m)(*asked), m, kt, int(largest), ov.data_ptr(),
                            iv.data_ptr() if with_idx else None, wv.data_ptr(), need, stream())
                    assert st == 0, (what, st)
                    settle(wv, what)
                    got = (bits_of(ov) if size == 2 else bits32(ov)).reshape(rows, m)
                    assert np.array_equal(got, ev[:, cols_of]), f"{what}: values {got[0]} want {ev[0, cols_of]}"
                    gi = bits32(iv).reshape(rows, m)
                    if with_idx:
                        assert np.array_equal(gi, ei[:, cols_of]), f"{what}: positions {gi[0]} want {ei[0, cols_of]}"
                        assert (gi[same] == np.array(asked, dtype=np.uint32)).all(), f"{what}: position == rank in a row of equal keys"
                    else:
                        assert (gi == POISON32).all(), f"{what}: no index buffer was given: nothing may be written"
                (assert_intact16 if size == 2 else assert_intact)(values=ow)
                assert_intact(indices=iw, workspace=ww)
        (assert_intact16 if size == 2 else assert_intact)(keys=kw)
        unchanged(name, family, size)


# ---- a rank or a k of its own for every row, from device memory: kth16_perrow and topk16_filter -------------------------------------
def per_row_calls(name, ranks, calls):
    """[calls][rows] indices into `ranks`: lp.spread, the shifts spaced evenly over the list"""
    rows = lp.SHAPES[name][0]
    return [np.array([lp.spread(ranks, shift, r, rows) for r in range(rows)]) for shift in range(0, len(ranks), max(1, len(ranks) // calls))]


def run_perrow(name):
    rows, cols = lp.SHAPES[name]
    L = lsd.lib()
    ww, wv, need = workspace(L.lsdsort_kth16_perrow_workspace_bytes(rows, cols))
    ow, ov = out16(rows)
    iw, iv = out32(rows)
    ranks = np.array(lp.ranks_of(name, 2), dtype=np.uint32)
    at = np.arange(rows)
    for family in families(name):
        kw, kv = select_dev(name, family, 2)
        same = equal_rows(name, family)
        for largest in ORDERS:
            ev, ei = oracle(name, family, 2)[largest]
            for n, pick in enumerate(per_row_calls(name, ranks, 4 if name == "WHOLE_ROW" else len(ranks))):
                rw, rv = guarded(ranks[pick])
                for with_idx in (True, False) if n % 4 == 0 else (True,):
                    what = f"{name} {family} largest={largest} ranks={ranks[pick][:4]} indices={with_idx}"
                    ov.fill_(POISON16)
                    iv.fill_(POISON32)
                    st = L.lsdsort_kth16_perrow_device(kv.data_ptr(), rows, cols, rv.data_ptr(), KT16, int(largest), ov.data_ptr(),
                                                       iv.data_ptr() if with_idx else None, wv.data_ptr(), need, stream())
                    assert st == 0, (what, st)
                    settle(wv, what)
                    got, gi = bits_of(ov), bits32(iv)
                    assert np.array_equal(got, ev[at, pick]), f"{what}: values {got[:4]} want {ev[at, pick][:4]}"
                    if with_idx:
                        assert np.array_equal(gi, ei[at, pick]), f"{what}: positions {gi[:4]} want {ei[at, pick][:4]}"
                        assert (gi[same] == ranks[pick][same]).all(), f"{what}: position == rank in a row of equal keys"
                    else:
                        assert (gi == POISON32).all(), f"{what}: no index buffer was given: nothing may be written"
                assert_intact(ranks=rw)
                assert np.array_equal(bits32(rv), ranks[pick]), "the ranks were changed"
        assert_intact16(keys=kw, values=ow)
        assert_intact(indices=iw, workspace=ww)
        unchanged(name, family, 2)


def run_topk16_filter(name):
    rows, cols = lp.SHAPES[name]
    L = lsd.lib()
    ww, wv, need = workspace(L.lsdsort_topk16_filter_workspace_bytes(rows, cols))
    # the output has the 16-byte phase of the keys: the 16-byte stores
    ow, ov = held(name, "filter out 6", lambda: guarded16(np.full(rows * cols, POISON16, dtype=np.uint16), lp.SKIP[2]))
    ranks = np.array(lp.ranks_of(name, 2), dtype=np.uint32)
    at = np.arange(rows)
    # every call compares 2^25 words on the host: the long shapes take one order per family (the orders are the key map's, which
    # has its own tests), rows of equal keys -- nothing is ever filled -- one call
    orders = {"cycle": ORDERS, "uniform bits": (True,), "four values": (False,), "all equal": (True,)}
    for family in families(name):
        kw, kv = select_dev(name, family, 2)
        keys = lp.select_keys(name, 2)[family]
        for largest in orders[family]:
            ev, _ = oracle(name, family, 2)[largest]
            s = rk.sortable16_np(keys, lp.KEY_TYPE, largest)
            for pick in per_row_calls(name, ranks, 2)[:1 if family == "all equal" else 2]:
                k = ranks[pick] + np.uint32(1)                          # T_r is item k_r - 1 of the stable sort: ev[r, pick[r]]
                what = f"{name} {family} largest={largest} k={k[:4]}"
                rw, rv = guarded(k)
                ov.fill_(POISON16)
                st = L.lsdsort_topk16_filter_device(kv.data_ptr(), rows, cols, rv.data_ptr(), KT16, int(largest), rk.FILL, ov.data_ptr(),
                                                    wv.data_ptr(), need, stream())
                assert st == 0, (what, st)
                settle(wv, what)
                thr = rk.sortable16_np(ev[at, pick], lp.KEY_TYPE, largest)
                want = np.where(rk.filter_on(k, cols)[:, None], np.where(s <= thr[:, None], keys, np.uint16(rk.FILL)), keys)
                got = bits_of(ov).reshape(rows, cols)
                bad = np.flatnonzero((got != want).any(axis=1))
                assert bad.size == 0, f"{what}: {bad.size} rows differ, first {bad[0]}: {int((got[bad[0]] != want[bad[0]]).sum())} words"
                assert_intact(k=rw)
        assert_intact16(keys=kw, out=ow)
        assert_intact(workspace=ww)
        unchanged(name, family, 2)


# ---- the first k of every row: topk16 ------------------------------------------------------------------------------------------------
def run_topk16(name):
    rows, cols = lp.SHAPES[name]
    k = lp.TOPK[name]
    L = lsd.lib()
    ww, wv, need = workspace(L.lsdsort_topk16_workspace_bytes(rows, cols, k))
    ow, ov = out16(rows * k)
    iw, iv = out32(rows * k)
    chunk, per_row = lp.chunks_for(rows, cols)
    for family in families(name):
        kw, kv = select_dev(name, family, 2)
        for largest in ORDERS:
            _, _, ek, ei = lp.select_oracle16(name, family)[largest]
            if family == "uniform bits":
                assert len({int(p) // chunk for p in ei[0]}) > per_row // 2, "the winners of a uniform row come from most chunks"
            for with_idx in (True, False):
                what = f"{name} {family} largest={largest} k={k} indices={with_idx}"
                ov.fill_(POISON16)
                iv.fill_(POISON32)
                st = L.lsdsort_topk16_device(kv.data_ptr(), rows, cols, k, KT16, int(largest), ov.data_ptr(), iv.data_ptr() if with_idx else None,
                                             wv.data_ptr(), need, stream())
                assert st == 0, (what, st)
                settle(wv, what)
                got, gi = bits_of(ov).reshape(rows, k), bits32(iv).reshape(rows, k)
                bad = np.flatnonzero((got != ek).any(axis=1))
                assert bad.size == 0, f"{what}: values differ in {bad.size} rows, first {bad[0]}: {got[bad[0]][:4]} want {ek[bad[0]][:4]}"
                if with_idx:
                    bad = np.flatnonzero((gi != ei).any(axis=1))
                    assert bad.size == 0, f"{what}: positions differ in {bad.size} rows, first {bad[0]}: {gi[bad[0]][:4]} want {ei[bad[0]][:4]}"
                else:
                    assert (gi == POISON32).all(), f"{what}: no index buffer was given: nothing may be written"
        assert_intact16(keys=kw, values=ow)
        assert_intact(indices=iw, workspace=ww)
        unchanged(name, family, 2)


# ---- the top-p filter and the draw on sharp rows -------------------------------------------------------------------------------------
def sharp_dev(name):
    return held(name, "sharp", lambda: guarded16(lp.sharp_inputs(name)[0], lp.SKIP[2], torch.bfloat16))


def sharp_unchanged(name):
    assert np.array_equal(bits_of(sharp_dev(name)[1]), lp.sharp_inputs(name)[0].reshape(-1)), f"{name}: a read-only input was changed"


def run_topp16(name):
    rows, cols = lp.SHAPES[name]
    L = lsd.lib()
    distinct = min(3, rows)
    nucleus = lp.nuclei(name)
    ww, wv, need = workspace(L.lsdsort_topp16_filter_workspace_bytes(rows, cols))
    kw, kv = sharp_dev(name)
    # the output has another 16-byte phase than the keys: the key-by-key stores
    ow, ov = held(name, "filter out 10", lambda: guarded16(np.full(rows * cols, POISON16, dtype=np.uint16), 10))
    cases = lp.nucleus_cases(name)
    for p in cases[::-(-len(cases) // 5)]:   # at most five calls: each compares 2^25 words on the host
        what = f"{name} p={p[:4]}"
        pw, pv = guarded(p.view(np.uint32), 8)
        ov.fill_(POISON16)
        st = L.lsdsort_topp16_filter_device(kv.data_ptr(), rows, cols, pv.data_ptr(), KT16, tp.FILL, ov.data_ptr(), wv.data_ptr(), need, stream())
        assert st == 0, (what, st)
        settle(wv, what)
        got = bits_of(ov).reshape(rows, cols)
        for r in range(rows):
            want = nucleus[r % distinct].filtered(p[r])
            if not np.array_equal(got[r], want):
                kept = got[r] != tp.FILL
                T = int(nucleus[r % distinct].sortable[kept].max()) if kept.any() else -1
                raise AssertionError(f"{what}: row {r} differs from the float64 oracle in {int((got[r] != want).sum())} words: its worst "
                                     f"kept value is {T:#x} (sortable), the oracle's {nucleus[r % distinct].threshold(p[r]):#x}")
        assert_intact(p=pw)
    assert_intact16(keys=kw, out=ow)
    assert_intact(workspace=ww)
    sharp_unchanged(name)


def draw(kv, rows, cols, u, iv, lv, wv, need, what):
    """one call of the draw: (index [rows] int64, logprob [rows] float32) after the common checks"""
    uw, uv = guarded(np.ascontiguousarray(u, dtype=np.float32).view(np.uint32), 8)
    iv.fill_(POISON32)
    lv.fill_(POISON32)
    st = lsd.lib().lsdsort_sample16_device(kv.data_ptr(), rows, cols, uv.data_ptr(), KT16, iv.data_ptr(), lv.data_ptr(), wv.data_ptr(), need, stream())
    assert st == 0, (what, st)
    settle(wv, what)
    assert_intact(u=uw)
    return iv.cpu().numpy().astype(np.int64), lv.view(torch.float32).cpu().numpy()


def run_sample16(name):
    rows, cols = lp.SHAPES[name]
    distinct = min(3, rows)
    oracles = lp.draws(name)
    ww, wv, need = workspace(lsd.lib().lsdsort_sample16_workspace_bytes(rows, cols))
    iw, iv = out32(rows)
    lw, lv = out32(rows)
    kw, kv = sharp_dev(name)
    chunk = lp.chunks_for(rows, cols)[0]
    picked = [set() for _ in range(rows)]
    for u in lp.draw_cases(name):
        what = f"{name} u={u[:4]}"
        index, logprob = draw(kv, rows, cols, u, iv, lv, wv, need, what)
        want = np.array([oracles[r % distinct].exact(u[r]) for r in range(rows)], dtype=np.int64)
        assert np.array_equal(index, want), f"{what}: index {index[:4]}, the float64 oracle's {want[:4]} (first at row {np.flatnonzero(index != want)[:1]})"
        for r in range(rows):
            lp64 = oracles[r % distinct].logprob(int(index[r]))
            assert abs(float(logprob[r]) - lp64) <= sm.LOGPROB_TOL, f"{what}: row {r}: logprob {logprob[r]!r}, float64 {lp64!r}"
            picked[r].add(lp.chunk_at(int(index[r]), lp.head_of(r, cols, 2), chunk))
    if name != "WHOLE_ROW":
        last = lp.chunks_for(rows, cols)[1] - 1
        assert {0, 1, 511, 512, last} <= picked[0], f"{name}: the draws of row 0 went to chunks {sorted(picked[0])}"
        # rows of equal keys: the index is floor(u_c * cols), which checks the chunk base arithmetic directly
        ew, ev = select_dev(name, "all equal", 2)
        for r in range(rows):
            aimed, index_of = lp.equal_draws(name, lp.head_of(r, cols, 2))
            for j in range(aimed.size):
                u = np.full(rows, 0.25, dtype=np.float32)
                u[r] = aimed[j]
                index, logprob = draw(ev, rows, cols, u, iv, lv, wv, need, f"{name} all equal row {r} u={aimed[j]!r}")
                assert index[r] == index_of[j], f"{name} all equal row {r} u={aimed[j]!r}: index {index[r]}, floor(u * cols) = {index_of[j]}"
                assert abs(float(logprob[r]) + np.log(cols)) <= sm.LOGPROB_TOL, f"{name} all equal: logprob {logprob[r]!r}, -ln(cols) = {-np.log(cols)!r}"
        assert_intact16(keys=ew)
        unchanged(name, "all equal", 2)
    assert_intact16(keys=kw)
    assert_intact(index=iw, logprob=lw, workspace=ww)
    sharp_unchanged(name)


RUN = {
    "topk16": run_topk16,
    "kth": lambda name: run_kth(name, 4),
    "kth16": lambda name: run_kth(name, 2),
    "kth_multi": lambda name: run_multi(name, 4),
    "kth16_multi": lambda name: run_multi(name, 2),
    "kth16_perrow": run_perrow,
    "topk16_filter": run_topk16_filter,
    "topp16_filter": run_topp16,
    "sample16": run_sample16,
}
CASES = [(name, entry) for name in BIG for entry in RUN]   # shape by shape: what `held` keeps serves every entry of a shape


@pytest.mark.parametrize("name,entry", CASES, ids=[f"{name}-{entry}" for name, entry in CASES])
def test_entry_at_shape(name, entry):
    RUN[entry](name)


# ---- MANY_TILES: rows of equal keys, filled on the device ----------------------------------------------------------------------------
def equal_dev():
    """(whole, view): 2^27 + 9 equal bfloat16 keys inside guard zones, 3 elements behind a 16-byte line, filled on the device"""
    def make():
        n = lp.SHAPES["MANY_TILES"][1]
        raw = torch.full((GUARD + n + GUARD + 8,), SENT16, dtype=torch.int16, device="cuda")
        lead = lp.SKIP[2] // 2
        whole = raw[lead:lead + GUARD + n + GUARD]
        view = whole[GUARD:GUARD + n]
        view.fill_(lp.EQUAL[2] - (1 << 16))
        assert view.data_ptr() % 16 == lp.SKIP[2]
        return whole, view.view(torch.bfloat16)
    return held("MANY_TILES", "equal", make)


def equal_unchanged():
    kw, kv = equal_dev()
    assert bool((kv.view(torch.int16) == lp.EQUAL[2] - (1 << 16)).all()), "a read-only input was changed"
    assert_intact16(keys=kw)


MANY_RANKS = lp.ranks_of("MANY_TILES", 2)


@pytest.mark.parametrize("entry", ["kth16", "kth16_perrow"])
def test_many_tiles_position_is_rank(entry):
    rows, cols = lp.SHAPES["MANY_TILES"]
    L = lsd.lib()
    kw, kv = equal_dev()
    figure = L.lsdsort_kth16_workspace_bytes if entry == "kth16" else L.lsdsort_kth16_perrow_workspace_bytes
    ww, wv, need = workspace(figure(rows, cols))
    ow, ov = out16(rows)
    iw, iv = out32(rows)
    for largest in ORDERS:
        for rank in MANY_RANKS:
            what = f"MANY_TILES {entry} largest={largest} rank={rank}"
            ov.fill_(POISON16)
            iv.fill_(POISON32)
            if entry == "kth16":
                st = L.lsdsort_kth16_device(kv.data_ptr(), rows, cols, rank, KT16, int(largest), ov.data_ptr(), iv.data_ptr(), wv.data_ptr(), need, stream())
            else:
                rw, rv = guarded(np.array([rank], dtype=np.uint32))
                st = L.lsdsort_kth16_perrow_device(kv.data_ptr(), rows, cols, rv.data_ptr(), KT16, int(largest), ov.data_ptr(), iv.data_ptr(),
                                                   wv.data_ptr(), need, stream())
            assert st == 0, (what, st)
            settle(wv, what)
            assert int(bits_of(ov)[0]) == lp.EQUAL[2] and int(bits32(iv)[0]) == rank, f"{what}: value {int(bits_of(ov)[0]):#x} position {int(bits32(iv)[0])}"
    assert_intact16(values=ow)
    assert_intact(indices=iw, workspace=ww)
    equal_unchanged()


@pytest.mark.parametrize("with_idx", [True, False], ids=["indices", "values"])
def test_many_tiles_multi(with_idx):
    rows, cols = lp.SHAPES["MANY_TILES"]
    L = lsd.lib()
    kw, kv = equal_dev()
    n_groups = -(-len(MANY_RANKS) // 8)
    for largest in ORDERS:
        for g in range(n_groups):
            asked = MANY_RANKS[g::n_groups]
            m = len(asked)
            what = f"MANY_TILES kth16_multi largest={largest} ranks={asked}"
            ww, wv, need = workspace(L.lsdsort_kth16_multi_workspace_bytes(rows, cols, m))
            ow, ov = out16(m)
            iw, iv = out32(m)
            iv.fill_(POISON32)
            st = L.lsdsort_kth16_multi_device(kv.data_ptr(), rows, cols, (ctypes.c_size_t * m)(*asked), m, KT16, int(largest), ov.data_ptr(),
                                              iv.data_ptr() if with_idx else None, wv.data_ptr(), need, stream())
            assert st == 0, (what, st)
            settle(wv, what)
            assert (bits_of(ov) == lp.EQUAL[2]).all(), f"{what}: values {bits_of(ov)}"
            assert np.array_equal(bits32(iv), np.array(asked if with_idx else [POISON32] * m, dtype=np.uint32)), f"{what}: positions {bits32(iv)}"
            assert_intact16(values=ow)
            assert_intact(indices=iw, workspace=ww)
    equal_unchanged()


def test_many_tiles_draw_is_floor_u_cols():
    rows, cols = lp.SHAPES["MANY_TILES"]
    kw, kv = equal_dev()
    ww, wv, need = workspace(lsd.lib().lsdsort_sample16_workspace_bytes(rows, cols))
    iw, iv = out32(rows)
    lw, lv = out32(rows)
    aimed, index_of = lp.equal_draws("MANY_TILES", lp.head_of(0, cols, 2))
    for j in range(aimed.size):
        what = f"MANY_TILES sample16 u={aimed[j]!r}"
        index, logprob = draw(kv, rows, cols, aimed[j:j + 1], iv, lv, wv, need, what)
        assert index[0] == index_of[j], f"{what}: index {index[0]}, floor(u * cols) = {index_of[j]}"
        assert abs(float(logprob[0]) + np.log(cols)) <= sm.LOGPROB_TOL, f"{what}: logprob {logprob[0]!r}, -ln(cols) = {-np.log(cols)!r}"
    assert_intact(index=iw, logprob=lw, workspace=ww)
    equal_unchanged()
