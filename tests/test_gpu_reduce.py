"""GPU suite: reduce by key (lsdsort_reduce_runs_device, lsdsort_reduce_by_key_device; csrc/reduce_by_key.hip) against the numpy oracle
of tests/_reduce.py -- bit for bit wherever the arithmetic is exact (integers, min / max, float sums whose partial sums are all
integers below 2^24), within the bound of any summation order for float sums of normal values, and the same bits on every call.
Every array is a view between guard zones (tests/_guarded.py) at the 16-byte phases 0 / 4 / 8 / 12 in turn, every workspace has
exactly the reported size, and the outputs are pre-filled with the sentinel, so a store past the count, past an array or past the
workspace shows.  Sizes are those of tests/_unique.py: around one tile, several tiles, and one size past every loop's first round."""
import functools

import numpy as np
import pytest

import _reduce as rd
import _unique as un
from _guarded import SENT32, SENT64, assert_intact, assert_unchanged, guarded, guarded_workspace

pytestmark = pytest.mark.gpu

PHASES = (0, 4, 8, 12)
# (value type, operation, value family): every integer operation on both integer types, float min / max on the specials, and the
# float sums that are exact in any order
EXACT = [(vt, op, fam) for vt in ("int32", "uint32") for op in rd.OPS for fam in ("small_ints", "wrap")] + \
        [("float32", "min", "specials"), ("float32", "max", "specials"), ("float32", "sum", "ones"), ("float32", "sum", "small_ints")]


def _host(view, dtype):
    return view.cpu().numpy().view(dtype)


def _sentinels(n, dtype=np.uint32):
    return np.full(n, SENT32 if np.dtype(dtype).itemsize == 4 else SENT64, dtype=dtype)


def _key_phase(w, case):
    return PHASES[case % 4] if w == 32 else (0, 8)[case % 2]


def _assert_exact_in_any_order(vals):
    """Every partial sum of these float32 values, in any order, is an integer below 2^24: float32 addition is exact on them."""
    v = vals.view(np.float32).astype(np.float64)
    assert np.array_equal(v, np.rint(v)) and np.abs(v).sum() < 2 ** 24


def call(lsd, entry, bits, vals, val_type, op, counts, case, key_type=None, descending=False, in_place=False, repeat=1):
    """Guarded calls of one entry ("runs" | "by_key") on the same arrays; returns {num, keys, vals[, counts]} of the first -- the host
    copies of the written prefixes -- after checking the status, the fault word, that nothing is written past the count, that the
    inputs are unchanged, that every guard zone is intact, and that every repeat gives the same bits."""
    import torch

    L = lsd.lib()
    n, w = bits.size, 8 * bits.dtype.itemsize
    code = un.KEY_CODE[key_type] if entry == "by_key" else None
    kw, dk = guarded(bits, _key_phase(w, case))
    vw, dv = guarded(vals, PHASES[(case + 1) % 4])
    if in_place:
        (ow, ok), (aw, ov) = (kw, dk), (vw, dv)
    else:
        ow, ok = guarded(_sentinels(n, bits.dtype), _key_phase(w, case + 1))
        aw, ov = guarded(_sentinels(n), PHASES[(case + 2) % 4])
    cw, dc = guarded(_sentinels(n), PHASES[(case + 3) % 4]) if counts else (None, None)
    nw, num = guarded(_sentinels(1), PHASES[case % 4])
    need = L.lsdsort_reduce_runs_workspace_bytes(n, w) if entry == "runs" else L.lsdsort_reduce_by_key_workspace_bytes(n, code)
    assert need > 0 and need % 256 == 0
    ww, ws = guarded_workspace(need)
    stream = int(torch.cuda.current_stream().cuda_stream)
    what = (entry, n, w, key_type, descending, val_type, op, counts, case, in_place)
    results = []
    for again in range(repeat):
        assert not (in_place and again)
        if again:
            for t, sent in ((ok, SENT32 if w == 32 else SENT64), (ov, SENT32), (dc, SENT32), (num, SENT32)):
                if t is not None:
                    t.fill_(sent)
        if entry == "runs":
            st = L.lsdsort_reduce_runs_device(dk.data_ptr(), dv.data_ptr(), n, w, rd.VAL_CODE[val_type], rd.OP_CODE[op], ok.data_ptr(),
                                              ov.data_ptr(), dc.data_ptr() if counts else None, num.data_ptr(), ws.data_ptr(), need, stream)
            assert st == 0, (st, what)
            assert L.lsdsort_check_device(ws.data_ptr(), stream) == 0, what
        else:
            st = L.lsdsort_reduce_by_key_device(dk.data_ptr(), dv.data_ptr(), n, code, int(descending), rd.VAL_CODE[val_type], rd.OP_CODE[op],
                                                ok.data_ptr(), ov.data_ptr(), dc.data_ptr() if counts else None, num.data_ptr(),
                                                ws.data_ptr(), need, stream)
            assert st == 0, (st, what)
            assert L.lsdsort_reduce_by_key_check_device(ws.data_ptr(), n, code, stream) == 0, what
        m = int(_host(num, np.uint32)[0])
        assert 1 <= m <= n, what
        got = {"num": m}
        for name, view, dtype, before in (("keys", ok, bits.dtype, bits), ("vals", ov, np.uint32, vals), ("counts", dc, np.uint32, None)):
            if view is None:
                continue
            whole = _host(view, dtype)
            # in place the words behind the count keep the input; otherwise the sentinel
            rest = before[m:] if in_place and before is not None else _sentinels(n - m, dtype)
            assert np.array_equal(whole[m:], rest), what + (name, "written past the count")
            got[name] = whole[:m].copy()
        results.append(got)
    if not in_place:
        assert_unchanged(dk, bits)
        assert_unchanged(dv, vals)
    assert_intact(keys=kw, vals=vw, out_keys=ow, out_vals=aw, counts=cw, num=nw, workspace=ww)
    for other in results[1:]:
        assert other["num"] == results[0]["num"] and all(np.array_equal(other[k], results[0][k]) for k in other if k != "num"), \
            what + ("a second call gave other bits",)
    return results[0]


def assert_same(got, want, what, vals=True):
    m = want["keys"].size
    assert got["num"] == m, (what, got["num"], m)
    for name in ("keys", "vals", "counts"):
        if name in got and (vals or name != "vals"):
            bad = np.flatnonzero(got[name] != want[name])
            assert bad.size == 0, (what, name, "first mismatch at", int(bad[0]), hex(int(got[name][bad[0]])), hex(int(want[name][bad[0]])))


def assert_within_sum_bound(got, bits_in_order, vals_in_order, what):
    """|got - s64| <= gamma * sum|v| per run, gamma = (L-1)u / (1 - (L-1)u), u = 2^-24: the bound of float32 summation in any order,
    so derived, not tuned (tests/_reduce.py, sum_bound)."""
    s64, bound = rd.sum_bound(bits_in_order, vals_in_order)
    err = np.abs(got["vals"].view(np.float32).astype(np.float64) - s64)
    worst = int(np.argmax(err - bound))
    assert (err <= bound).all(), (what, "run", worst, "error", err[worst], "bound", bound[worst])


# ---- 1. the runs entry, bit for bit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", un.SIZES)
@pytest.mark.parametrize("w", [32, 64])
def test_runs_families_sizes_operations_and_types(gpu, w, n):
    case = 0
    fams = rd.key_families(n, w)
    assert {"runs_T", "runs_T-1", "runs_T+1", "runs_2T+3", "all_equal"} <= set(fams)
    for name, bits in fams.items():
        for val_type, op, family in EXACT:
            vals = rd.values(n, family, val_type)
            if val_type == "float32" and op == "sum":
                _assert_exact_in_any_order(vals)
            want = rd.oracle_reduce_runs(bits, vals, val_type, op)
            for counts in (True, False):
                twice = counts and name == "recurring" and (val_type, op, family) == ("float32", "sum", "small_ints")
                got = call(gpu, "runs", bits, vals, val_type, op, counts, case, repeat=2 if twice else 1)
                assert_same(got, want, (name, n, w, val_type, op, family, counts))
                case += 1
    assert case == 2 * len(EXACT) * 9
    if n == 5 * un.TILE + 7:   # one run through six tiles: the carry through tiles without a head
        assert un.oracle_rle(fams["all_equal"])["keys"].size == 1 and -(-n // un.TILE) == 6


# ---- 2. a run of one is never touched by arithmetic --------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [32, 64])
def test_all_distinct_keys_return_the_values_bit_for_bit(gpu, w):
    case = 0
    for n in un.SIZES:
        bits = un.families(n, w)["all_distinct"]
        for val_type, family in (("float32", "specials"), ("int32", "wrap"), ("uint32", "small_ints")):
            vals = rd.values(n, family, val_type)
            for op in rd.OPS:
                got = call(gpu, "runs", bits, vals, val_type, op, case % 2 == 0, case)
                assert got["num"] == n and np.array_equal(got["keys"], bits), (n, w, val_type, op)
                assert np.array_equal(got["vals"], vals), (n, w, val_type, op, "a run of one element must keep its bits")
                if "counts" in got:
                    assert (got["counts"] == 1).all()
                case += 1


# ---- 3. float sums of normal values ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [32, 64])
def test_float_sums_of_normal_values_within_the_bound_and_deterministic(gpu, w):
    case = 0
    for n in un.SIZES:
        vals = rd.values(n, "normal", "float32")
        for name, bits in rd.key_families(n, w).items():
            got = call(gpu, "runs", bits, vals, "float32", "sum", case % 2 == 0, case, repeat=2)
            want = rd.oracle_reduce_runs(bits, vals, "float32", "sum")
            assert_same(got, want, (name, n, w), vals=False)
            assert_within_sum_bound(got, bits, vals, (name, n, w))
            case += 1


def test_float_sums_of_groups_with_nan_and_infinities(gpu):
    inf, nan = np.inf, np.nan
    groups = [[1.0, nan, 2.0], [inf, 1.0, -inf], [inf, 1.0, inf], [-inf, -2.0], [nan], [3.0, 4.0, 5.0], [inf], [-0.0], [-0.0, -0.0], [-0.0, 0.0]]
    bits = np.repeat(np.arange(len(groups), dtype=np.uint32) * 7 + 1, [len(g) for g in groups])
    vals = np.array([v for g in groups for v in g], dtype=np.float32).view(np.uint32)
    alone = sum(len(g) for g in groups[:4])
    assert np.isnan(vals.view(np.float32)[alone]) and bits[alone - 1] != bits[alone] != bits[alone + 1]
    vals[alone] = 0x7FC00123                                          # the NaN alone: a payload of its own
    got = call(gpu, "runs", bits, vals, "float32", "sum", True, 1, repeat=2)
    out = got["vals"].view(np.float32)
    assert got["num"] == len(groups) and got["counts"].tolist() == [len(g) for g in groups]
    assert np.isnan(out[0]) and np.isnan(out[1])                      # a NaN in the group; +inf with -inf
    assert out[2] == inf and out[3] == -inf and out[6] == inf         # infinities of one sign
    assert got["vals"][4] == 0x7FC00123                               # a run of one keeps its payload
    assert out[5] == 12.0
    assert got["vals"][7] == 0x80000000 and got["vals"][8] == 0x80000000 and got["vals"][9] == 0x00000000   # IEEE: -0 + -0 = -0, -0 + +0 = +0
    # the same groups unsorted, by key
    order = np.random.default_rng(5).permutation(bits.size)
    by_key = call(gpu, "by_key", bits[order], vals[order], "float32", "sum", True, 2, key_type="uint32")
    out = by_key["vals"].view(np.float32)
    assert np.array_equal(by_key["keys"], np.unique(bits)) and np.isnan(out[0]) and np.isnan(out[1]) and out[2] == inf and out[3] == -inf
    assert by_key["vals"][4] == 0x7FC00123 and out[5] == 12.0 and out[6] == inf


# ---- 4. the by-key entry -----------------------------------------------------------------------------------------------------------
BY_KEY_ROTATING = [("int32", "sum", "small_ints"), ("int32", "max", "wrap"), ("uint32", "min", "wrap"), ("float32", "min", "specials"),
                   ("float32", "max", "specials"), ("uint32", "sum", "wrap"), ("int32", "min", "small_ints"), ("uint32", "max", "small_ints")]


@pytest.mark.parametrize("descending", [False, True], ids=["ascending", "descending"])
@pytest.mark.parametrize("key_type", un.KEY_TYPES)
def test_by_key_types_directions_families_and_sizes(gpu, key_type, descending):
    w = un.width_of(key_type)
    inputs = [("specials", un.specials(key_type))]
    inputs += [((n, name), rd.shuffled(n, w, name)) for n in un.SIZES for name in rd.key_families(n, w)]
    case = 0
    for what, bits in inputs:
        n = bits.size
        order = np.argsort(un.sortable(bits, key_type, descending), kind="stable")
        # one of the exact combinations in turn, and on every input the two float sums: exact, and within the bound
        for val_type, op, family in (BY_KEY_ROTATING[case % len(BY_KEY_ROTATING)], ("float32", "sum", "small_ints"), ("float32", "sum", "normal")):
            vals = rd.values(n, family, val_type)
            want = rd.oracle_reduce_runs(bits[order], vals[order], val_type, op)
            assert np.array_equal(want["keys"], rd.oracle_reduce_by_key(bits, vals, key_type, descending, val_type, op)["keys"])
            got = call(gpu, "by_key", bits, vals, val_type, op, case % 2 == 0, case, key_type=key_type, descending=descending,
                       repeat=2 if case % 5 == 0 else 1)
            if family == "normal":
                assert_same(got, want, (what, key_type, descending, family), vals=False)
                assert_within_sum_bound(got, bits[order], vals[order], (what, key_type, descending))
            else:
                if family == "small_ints" and val_type == "float32":
                    _assert_exact_in_any_order(vals)
                assert_same(got, want, (what, key_type, descending, val_type, op, family))
            case += 1
    assert case == 3 * (1 + 9 * len(un.SIZES))


@pytest.mark.parametrize("key_type", ["uint32", "int64"])
def test_by_key_into_the_inputs_themselves(gpu, key_type):
    w = un.width_of(key_type)
    case = 0
    for n in (3, un.TILE + 1, 5 * un.TILE + 7):
        for name in ("random8", "all_distinct", "runs_T-1"):
            bits = rd.shuffled(n, w, name)
            for val_type, op, family in (("float32", "sum", "small_ints"), ("int32", "max", "wrap")):
                vals = rd.values(n, family, val_type)
                want = rd.oracle_reduce_by_key(bits, vals, key_type, case % 2 == 1, val_type, op)
                got = call(gpu, "by_key", bits, vals, val_type, op, case % 3 != 0, case, key_type=key_type, descending=case % 2 == 1,
                           in_place=True)
                assert_same(got, want, (n, name, key_type, val_type, op, "in place"))
                case += 1


# ---- 5. one size past every first round ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _big(w):
    """BIG_N keys, values from {-1, 0, 1} as int32 and as float32, and the stable order of the keys: computed once."""
    bits = un.big_keys(w)
    ints = np.random.default_rng(123 + w).integers(-1, 2, size=bits.size).astype(np.int32)
    order = np.argsort(bits, kind="stable")
    return bits, ints.view(np.uint32), ints.astype(np.float32).view(np.uint32), order


@pytest.mark.parametrize("w", [32, 64])
def test_the_size_past_every_first_round(gpu, w):
    """BIG_N keys, about BIG_DISTINCT distinct values: the scan's second round with its carried part, and more 16-byte groups than the
    copy kernel's grid has threads.  sum|v| is about 1.12e7, below 2^24: every float sum is exact."""
    bits, ints, floats, order = _big(w)
    assert bits.size == un.BIG_N and -(-bits.size // un.TILE) > un.SCAN_ROUND
    _assert_exact_in_any_order(floats)
    key_type = "uint%d" % w
    in_order = bits[order]
    for case, (val_type, op, vals) in enumerate((("float32", "sum", floats), ("int32", "max", ints))):
        want = rd.oracle_reduce_runs(in_order, vals[order], val_type, op)
        assert want["keys"].size > un.MAX_GRID * un.THREADS
        got = call(gpu, "by_key", bits, vals, val_type, op, True, case + 1, key_type=key_type)
        assert_same(got, want, ("by key", w, val_type, op))
    # the runs entry alone: on the sorted keys, and on all-equal keys -- one run across the scan's round boundary and all 4097 tiles
    sorted_vals = floats[order]
    got = call(gpu, "runs", in_order, sorted_vals, "float32", "sum", True, 3)
    assert_same(got, rd.oracle_reduce_runs(in_order, sorted_vals, "float32", "sum"), ("runs, sorted", w))
    equal = np.full(un.BIG_N, in_order[5], dtype=bits.dtype)
    for case, (val_type, op, vals) in enumerate((("float32", "sum", floats), ("int32", "max", ints))):
        want = rd.oracle_reduce_runs(equal, vals, val_type, op)
        assert want["keys"].size == 1 and want["counts"].tolist() == [un.BIG_N] and -(-un.BIG_N // un.TILE) == un.SCAN_ROUND + 1
        got = call(gpu, "runs", equal, vals, val_type, op, case != 1, case)
        assert_same(got, want, ("runs, all equal", w, val_type, op))


# ---- 6. refusals and the empty call ------------------------------------------------------------------------------------------------
def test_runs_refuses_its_inputs_as_outputs_and_an_empty_call_stores_zero(gpu):
    import torch

    L = gpu.lib()
    kw, keys = guarded(np.arange(100, dtype=np.uint32) // 3, 0)
    vw, vals = guarded(np.arange(100, dtype=np.uint32), 4)
    ow, out = guarded(_sentinels(100), 8)
    aw, agg = guarded(_sentinels(100), 12)
    nw, num = guarded(_sentinels(1), 4)
    need = L.lsdsort_reduce_runs_workspace_bytes(100, 32)
    ww, ws = guarded_workspace(need)
    stream = int(torch.cuda.current_stream().cuda_stream)
    for ok, ov in ((keys, agg), (out, vals), (keys, vals)):
        assert L.lsdsort_reduce_runs_device(keys.data_ptr(), vals.data_ptr(), 100, 32, 1, 0, ok.data_ptr(), ov.data_ptr(), None, num.data_ptr(),
                                            ws.data_ptr(), need, stream) == -1
    torch.cuda.synchronize()
    assert int(_host(num, np.uint32)[0]) == SENT32
    assert (_host(out, np.uint32) == SENT32).all() and (_host(agg, np.uint32) == SENT32).all()
    assert_unchanged(keys, np.arange(100, dtype=np.uint32) // 3)
    assert_unchanged(vals, np.arange(100, dtype=np.uint32))
    # n == 0: the count receives 0 by one store, and nothing else happens -- no pointer is needed, no workspace touched
    for entry in ("runs", "by_key"):
        num.fill_(SENT32)
        if entry == "runs":
            st = L.lsdsort_reduce_runs_device(None, None, 0, 64, 2, 0, None, None, None, num.data_ptr(), None, 0, stream)
        else:
            st = L.lsdsort_reduce_by_key_device(None, None, 0, 4, 1, 1, 2, None, None, None, num.data_ptr(), None, 0, stream)
        assert st == 0 and int(_host(num, np.uint32)[0]) == 0, entry
    assert L.lsdsort_reduce_by_key_check_device(ws.data_ptr(), 0, 4, stream) == 0
    assert_intact(keys=kw, vals=vw, out=ow, agg=aw, num=nw, workspace=ww)
    assert (_host(ws, np.uint8) == 0x7E).all()


# ---- 7. graph capture ----------------------------------------------------------------------------------------------------------------
REPLAYS = ("alternating", "random8", "all_distinct", "all_equal")   # two values / eight / a run per key / one run


@pytest.mark.parametrize("entry,key_type,val_type,op,family", [("runs", "uint32", "float32", "sum", "small_ints"),
                                                               ("runs", "uint64", "int32", "max", "wrap"),
                                                               ("by_key", "int32", "float32", "sum", "small_ints"),
                                                               ("by_key", "float64", "uint32", "min", "wrap")])
def test_graph_replays_follow_changed_keys_and_values(gpu, entry, key_type, val_type, op, family):
    """Both entries launch kernels only and rewrite every word of their state on every call: one warm-up, one capture, four replays,
    each on other keys and other values; the count and every output follow."""
    import torch

    L = gpu.lib()
    assert L.lsdsort_prepare_device() == 0
    w = un.width_of(key_type)
    n = 2 * un.TILE + 1
    code = un.KEY_CODE[key_type]
    signed = np.int32 if w == 32 else np.int64
    dk = torch.zeros(n, dtype=torch.int32 if w == 32 else torch.int64, device="cuda")
    dv = torch.zeros(n, dtype=torch.int32, device="cuda")
    out = torch.zeros_like(dk)
    agg, counts = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2))
    num = torch.zeros(1, dtype=torch.int32, device="cuda")
    need = L.lsdsort_reduce_runs_workspace_bytes(n, w) if entry == "runs" else L.lsdsort_reduce_by_key_workspace_bytes(n, code)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")

    def run():
        stream = int(torch.cuda.current_stream().cuda_stream)
        if entry == "runs":
            st = L.lsdsort_reduce_runs_device(dk.data_ptr(), dv.data_ptr(), n, w, rd.VAL_CODE[val_type], rd.OP_CODE[op], out.data_ptr(),
                                              agg.data_ptr(), counts.data_ptr(), num.data_ptr(), ws.data_ptr(), need, stream)
        else:
            st = L.lsdsort_reduce_by_key_device(dk.data_ptr(), dv.data_ptr(), n, code, 1, rd.VAL_CODE[val_type], rd.OP_CODE[op], out.data_ptr(),
                                                agg.data_ptr(), counts.data_ptr(), num.data_ptr(), ws.data_ptr(), need, stream)
        assert st == 0, st

    def keys_of(name):
        return rd.key_families(n, w)[name] if entry == "runs" else rd.shuffled(n, w, name)

    dk.copy_(torch.from_numpy(keys_of("recurring").view(signed).copy()))
    dv.copy_(torch.from_numpy(rd.values(n, family, val_type).view(np.int32).copy()))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()   # warm-up: device set-up stays out of the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    for k, name in enumerate(REPLAYS):
        bits = keys_of(name)
        vals = rd.values(n, family, val_type, seed=k + 1)
        if val_type == "float32":
            _assert_exact_in_any_order(vals)
        want = rd.oracle_reduce_runs(bits, vals, val_type, op) if entry == "runs" else \
            rd.oracle_reduce_by_key(bits, vals, key_type, True, val_type, op)
        m = want["keys"].size
        dk.copy_(torch.from_numpy(bits.view(signed).copy()))
        dv.copy_(torch.from_numpy(vals.view(np.int32).copy()))
        for t in (out, agg, counts, num):
            t.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert int(num.item()) == m, name
        assert np.array_equal(_host(out, bits.dtype)[:m], want["keys"]) and (_host(out, signed)[m:] == -1).all(), name
        assert np.array_equal(_host(agg, np.uint32)[:m], want["vals"]) and (_host(agg, np.int32)[m:] == -1).all(), name
        assert np.array_equal(_host(counts, np.uint32)[:m], want["counts"]) and (_host(counts, np.int32)[m:] == -1).all(), name
        if entry == "runs":
            assert L.lsdsort_check_device(ws.data_ptr(), None) == 0
        else:
            assert L.lsdsort_reduce_by_key_check_device(ws.data_ptr(), n, code, None) == 0


# ---- 8. the Python face against torch --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key_type", ["int32", "int64"])
def test_python_face_against_torch(gpu, key_type):
    import torch

    w = un.width_of(key_type)
    n = 2 * un.TILE + 1
    signed = np.int32 if w == 32 else np.int64

    def dev(bits, dtype=None):
        """Key words as the signed tensor of their width; 32-bit value words as `dtype`, reinterpreted."""
        if dtype is None:
            return torch.from_numpy(bits.view(signed).copy()).cuda()
        return torch.from_numpy(bits.view(np.int32).copy()).cuda().view(dtype)

    def scatter(index, v, m, op):
        if op == "sum":
            return torch.zeros(m, dtype=v.dtype, device="cuda").index_add_(0, index, v)
        return torch.zeros(m, dtype=v.dtype, device="cuda").scatter_reduce_(0, index, v, "amin" if op == "min" else "amax", include_self=False)

    x = dev(rd.shuffled(n, w, "random8"))
    y = dev(rd.key_families(n, w)["recurring"])
    ints = dev(rd.values(n, "small_ints", "int32"), torch.int32)
    floats = dev(rd.values(n, "small_ints", "float32"), torch.float32)       # NaN-free, and every sum exact
    uniq, inverse, sizes = torch.unique(x, sorted=True, return_inverse=True, return_counts=True)
    runs, run_inverse, lengths = torch.unique_consecutive(y, return_inverse=True, return_counts=True)
    for v in (ints, floats):
        for op in rd.OPS:
            keys, agg, counts = gpu.reduce_by_key(x, v, op, return_counts=True)
            assert keys.dtype == x.dtype and agg.dtype == v.dtype and counts.dtype == torch.int64
            assert torch.equal(keys, uniq) and torch.equal(counts, sizes) and torch.equal(agg, scatter(inverse, v, uniq.numel(), op)), (v.dtype, op)
            keys, agg = gpu.reduce_by_key(x, v, op, descending=True)
            assert torch.equal(keys, uniq.flip(0)) and torch.equal(agg, scatter(inverse, v, uniq.numel(), op).flip(0)), (v.dtype, op)
            keys, agg, counts = gpu.reduce_consecutive(y, v, op, return_counts=True)
            assert torch.equal(keys, runs) and torch.equal(counts, lengths) and torch.equal(agg, scatter(run_inverse, v, runs.numel(), op)), (v.dtype, op)
            assert torch.equal(gpu.reduce_consecutive(y, v, op)[1], agg)
    # the device wrappers: full-length tensors and the one-word count; the inputs themselves may take the result by key
    keys, agg, counts, num = gpu.GPUReduceByKey(x, ints, op="sum", counts=True, check_fault=True)
    m = int(num.item())
    assert keys.numel() == agg.numel() == counts.numel() == n and num.numel() == 1 and m == uniq.numel()
    assert torch.equal(keys[:m], uniq) and torch.equal(counts[:m].long(), sizes) and torch.equal(agg[:m], scatter(inverse, ints, m, "sum"))
    kz, vz = x.clone(), floats.clone()
    same_k, same_v, num = gpu.GPUReduceByKey(kz, vz, op="max", out_keys=kz, out_vals=vz, check_fault=True)
    assert same_k is kz and same_v is vz and int(num.item()) == m
    assert torch.equal(kz[:m], uniq) and torch.equal(vz[:m], scatter(inverse, floats, m, "max")) and torch.equal(kz[m:], x[m:]) and torch.equal(vz[m:], floats[m:])
    rk, ra, rc, rn = gpu.GPUReduceRuns(y, floats, op="min", counts=True, check_fault=True)
    r = int(rn.item())
    assert r == runs.numel() and torch.equal(rk[:r], runs) and torch.equal(rc[:r].long(), lengths)
    assert torch.equal(ra[:r], scatter(run_inverse, floats, r, "min"))
    for v in (ints, floats):
        for got in (gpu.reduce_by_key(x[:0], v[:0]), gpu.reduce_consecutive(x[:0], v[:0], "max"), gpu.reduce_by_key(x[:0], v[:0], return_counts=True)):
            assert all(t.numel() == 0 for t in got)
