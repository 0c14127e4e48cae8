"""GPU suite: run-length encode and unique (lsdsort_rle_device, lsdsort_unique_device; csrc/unique.hip), bit for bit against the numpy
oracle of tests/_unique.py.  Every array is a view between guard zones (tests/_guarded.py), every workspace has exactly the reported
size, and the outputs are pre-filled with the sentinel, so a store past the count, past an array or past the workspace shows.  Sizes
are named from the unit's constants: around one tile, several tiles, and one size past every loop's first round."""
import numpy as np
import pytest

import _unique as un
from _guarded import SENT32, SENT64, assert_intact, assert_unchanged, guarded, guarded_workspace

pytestmark = pytest.mark.gpu

RLE_OUTPUTS = {"neither": (False, False), "counts": (True, False), "starts": (False, True), "both": (True, True)}
UNIQUE_OUTPUTS = {"none": (), "counts": ("counts",), "first": ("first",), "inverse": ("inverse",), "all": ("counts", "first", "inverse")}
ODD = (4, 12, 8, 0)   # 16-byte phases of the 32-bit outputs: two odd 4-byte alignments among them


def _host(view, dtype):
    return view.cpu().numpy().view(dtype)


def _sentinels(n, dtype=np.uint32):
    return np.full(n, SENT32 if np.dtype(dtype).itemsize == 4 else SENT64, dtype=dtype)


def _assert_prefix(view, want, what):
    """The first len(want) words are `want`, every word behind them still holds the sentinel."""
    got = _host(view, want.dtype)
    m = want.size
    assert np.array_equal(got[:m], want), (what, "first mismatch at", int(np.flatnonzero(got[:m] != want)[0]))
    assert (got[m:] == (SENT32 if want.dtype.itemsize == 4 else SENT64)).all(), (what, "written past the count")


def run_rle(lsd, bits, counts, starts, key_skip=0, out_skip=0, twice=False):
    """One guarded call of lsdsort_rle_device, checked against the oracle."""
    import torch

    L = lsd.lib()
    n, w = bits.size, 8 * bits.dtype.itemsize
    want = un.oracle_rle(bits)
    kw, keys = guarded(bits, key_skip)
    ow, out = guarded(_sentinels(n, bits.dtype), 0)
    cw, dc = guarded(_sentinels(n), out_skip) if counts else (None, None)
    sw, ds = guarded(_sentinels(n), (out_skip + 8) % 16) if starts else (None, None)
    nw, num = guarded(_sentinels(1), out_skip)
    need = L.lsdsort_rle_workspace_bytes(n, w)
    ww, ws = guarded_workspace(need)
    stream = int(torch.cuda.current_stream().cuda_stream)
    for _ in range(2 if twice else 1):   # the second call on the same input gives the same bits
        st = L.lsdsort_rle_device(keys.data_ptr(), n, w, out.data_ptr(), dc.data_ptr() if counts else None, ds.data_ptr() if starts else None,
                                  num.data_ptr(), ws.data_ptr(), need, stream)
        assert st == 0, st
        assert L.lsdsort_check_device(ws.data_ptr(), stream) == 0
        what = (n, w, counts, starts, key_skip, out_skip)
        assert int(_host(num, np.uint32)[0]) == want["keys"].size, what
        _assert_prefix(out, want["keys"], what + ("keys",))
        if counts:
            _assert_prefix(dc, want["counts"], what + ("counts",))
        if starts:
            _assert_prefix(ds, want["starts"], what + ("starts",))
    assert_unchanged(keys, bits)
    assert_intact(keys=kw, out=ow, counts=cw, starts=sw, num=nw, workspace=ww)


def run_unique(lsd, bits, key_type, descending, outputs, want=None, key_skip=0, out_skip=0, in_place=False, twice=False):
    """One guarded call of lsdsort_unique_device, checked against the oracle (or `want`)."""
    import torch

    L = lsd.lib()
    n = bits.size
    code = un.KEY_CODE[key_type]
    want = want or un.oracle_unique(bits, key_type, descending)
    m = want["keys"].size
    kw, keys = guarded(bits, key_skip)
    ow, out = (kw, keys) if in_place else guarded(_sentinels(n, bits.dtype), 0)
    arrays = {}
    for k, name in enumerate(("counts", "first", "inverse")):
        arrays[name] = guarded(_sentinels(n), (out_skip + 4 * k) % 16) if name in outputs else (None, None)
    nw, num = guarded(_sentinels(1), out_skip)
    positions = int("first" in outputs or "inverse" in outputs)
    need = L.lsdsort_unique_workspace_bytes(n, code, positions)
    ww, ws = guarded_workspace(need)
    stream = int(torch.cuda.current_stream().cuda_stream)
    ptr = {name: (view.data_ptr() if view is not None else None) for name, (_, view) in arrays.items()}
    what = (n, key_type, descending, outputs, key_skip, out_skip, in_place)
    for _ in range(2 if twice and not in_place else 1):
        st = L.lsdsort_unique_device(keys.data_ptr(), n, code, int(descending), out.data_ptr(), ptr["counts"], ptr["first"], ptr["inverse"],
                                     num.data_ptr(), ws.data_ptr(), need, stream)
        assert st == 0, st
        assert L.lsdsort_unique_check_device(ws.data_ptr(), n, code, positions, stream) == 0
        assert int(_host(num, np.uint32)[0]) == m, what
        got_keys = _host(out, bits.dtype)
        assert np.array_equal(got_keys[:m], want["keys"]), what + ("keys",)
        # in place the words behind the count keep the input; otherwise the sentinel
        assert np.array_equal(got_keys[m:], bits[m:] if in_place else _sentinels(n - m, bits.dtype)), what + ("past the count",)
        for name in ("counts", "first"):
            if name in outputs:
                _assert_prefix(arrays[name][1], want[name], what + (name,))
        if "first" in outputs:
            first = _host(arrays["first"][1], np.uint32)[:m]
            assert np.array_equal(bits[first], want["keys"]), what
        if "inverse" in outputs:
            inverse = _host(arrays["inverse"][1], np.uint32)
            assert np.array_equal(got_keys[:m][inverse], bits), what + ("out[inverse] == x",)
            assert np.array_equal(inverse, want["inverse"]), what + ("inverse",)
    if not in_place:
        assert_unchanged(keys, bits)
    assert_intact(keys=kw, out=ow, num=nw, workspace=ww, **{name: whole for name, (whole, _) in arrays.items()})


# ---- run-length encode -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", un.SIZES)
@pytest.mark.parametrize("w", [32, 64])
def test_rle_families_sizes_and_output_combinations(gpu, w, n):
    case = 0
    for name, bits in un.families(n, w).items():
        for combo, (counts, starts) in RLE_OUTPUTS.items():
            # the keys on a 16-byte line (16-byte loads) and on a word boundary only (single words), the outputs at every phase
            key_skip = (0, w // 8)[case % 2]
            run_rle(gpu, bits, counts, starts, key_skip=key_skip, out_skip=ODD[case % 4], twice=(combo == "both"))
            case += 1


@pytest.mark.parametrize("w", [32, 64])
def test_rle_specials_compare_whole_words_and_bits(gpu, w):
    """+-0, NaN payloads and words that differ in one half only, next to each other and repeated: runs end wherever the bits change."""
    base = un.F32_SPECIALS if w == 32 else np.concatenate([un.F64_SPECIALS, un.WORD_PAIRS])
    bits = np.repeat(base, np.arange(base.size) % 3 + 1)
    assert un.oracle_rle(bits)["keys"].size == base.size
    for key_skip in (0, w // 8):
        run_rle(gpu, bits, True, True, key_skip=key_skip, out_skip=4)


def test_rle_refuses_the_keys_as_output_and_counts_an_empty_call(gpu):
    import torch

    L = gpu.lib()
    kw, keys = guarded(np.arange(100, dtype=np.uint32), 0)
    nw, num = guarded(_sentinels(1), 4)
    need = L.lsdsort_rle_workspace_bytes(100, 32)
    ww, ws = guarded_workspace(need)
    stream = int(torch.cuda.current_stream().cuda_stream)
    assert L.lsdsort_rle_device(keys.data_ptr(), 100, 32, keys.data_ptr(), None, None, num.data_ptr(), ws.data_ptr(), need, stream) == -1
    assert int(_host(num, np.uint32)[0]) == SENT32
    # n == 0: the count receives 0 by one store, and nothing else happens -- no pointer is needed, no workspace touched
    for entry in ("rle", "unique"):
        num.fill_(SENT32)
        if entry == "rle":
            st = L.lsdsort_rle_device(None, 0, 64, None, None, None, num.data_ptr(), None, 0, stream)
        else:
            st = L.lsdsort_unique_device(None, 0, 4, 1, None, None, None, None, num.data_ptr(), None, 0, stream)
        assert st == 0 and int(_host(num, np.uint32)[0]) == 0, entry
    assert L.lsdsort_unique_check_device(ws.data_ptr(), 0, 4, 1, stream) == 0
    assert_intact(keys=kw, num=nw, workspace=ww)
    assert (_host(ws, np.uint8) == 0x7E).all()


# ---- unique ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("descending", [False, True], ids=["ascending", "descending"])
@pytest.mark.parametrize("key_type", un.KEY_TYPES)
def test_unique_families_sizes_and_output_combinations(gpu, key_type, descending):
    w = un.width_of(key_type)
    case = 0
    inputs = [("specials", un.specials(key_type))]
    inputs += [((n, name), un.shuffled(n, w, name)) for n in un.SIZES for name in un.families(n, w)]
    for what, bits in inputs:
        want = un.oracle_unique(bits, key_type, descending)
        for combo, outputs in UNIQUE_OUTPUTS.items():   # every combination on every input
            # the keys on a 16-byte line and on a word boundary only, the 32-bit outputs at every phase
            run_unique(gpu, bits, key_type, descending, outputs, want, key_skip=(0, w // 8)[case % 2], out_skip=ODD[case % 4],
                       twice=(combo == "all" and case % 3 == 0))
            case += 1
    assert case == len(UNIQUE_OUTPUTS) * (1 + 8 * len(un.SIZES))


@pytest.mark.parametrize("key_type", ["float32", "float64"])
def test_unique_floats_follow_total_order_and_keep_bits_apart(gpu, key_type):
    """-0.0 and +0.0 are two values, every NaN payload is one; NaNs lie at the two ends by sign.  Through the Python face."""
    import torch

    w = un.width_of(key_type)
    bits = un.specials(key_type)[: 3 * (16 if w == 32 else 16)]
    x = torch.from_numpy(bits.view(np.int32 if w == 32 else np.int64).copy()).cuda().view(torch.float32 if w == 32 else torch.float64)
    for descending in (False, True):
        want = un.oracle_unique(bits, key_type, descending)
        values, inverse, counts, index = gpu.unique(x, return_inverse=True, return_counts=True, return_index=True, descending=descending)
        assert values.dtype == x.dtype and inverse.dtype == counts.dtype == index.dtype == torch.int64
        word = np.uint32 if w == 32 else np.uint64
        assert np.array_equal(values.cpu().numpy().view(word), want["keys"])
        assert np.array_equal(inverse.cpu().numpy(), want["inverse"]) and np.array_equal(counts.cpu().numpy(), want["counts"])
        assert np.array_equal(index.cpu().numpy(), want["first"])
    # without -0.0 and NaN the result is torch's
    plain = x[~torch.isnan(x) & ~((x == 0) & torch.signbit(x))]
    got = gpu.unique(plain, return_inverse=True, return_counts=True)
    ref = torch.unique(plain, sorted=True, return_inverse=True, return_counts=True)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
    runs, lengths = gpu.unique_consecutive(plain, return_counts=True)
    ref_runs, ref_lengths = torch.unique_consecutive(plain, return_counts=True)
    assert torch.equal(runs, ref_runs) and torch.equal(lengths, ref_lengths)


@pytest.mark.parametrize("key_type", ["int32", "int64"])
def test_python_face_against_torch(gpu, key_type):
    import torch

    w = un.width_of(key_type)
    n = 2 * un.TILE + 1
    bits = un.shuffled(n, w, "random8")
    x = torch.from_numpy(bits.view(np.int32 if w == 32 else np.int64).copy()).cuda()
    got = gpu.unique(x, return_inverse=True, return_counts=True)
    ref = torch.unique(x, sorted=True, return_inverse=True, return_counts=True)
    for a, b in zip(got, ref):
        assert a.dtype == b.dtype and torch.equal(a, b)
    assert torch.equal(gpu.unique(x), ref[0]) and torch.equal(gpu.unique(x, descending=True), ref[0].flip(0))
    y = torch.from_numpy(un.families(n, w)["recurring"].view(np.int32 if w == 32 else np.int64).copy()).cuda()
    runs, lengths = gpu.unique_consecutive(y, return_counts=True)
    ref_runs, ref_lengths = torch.unique_consecutive(y, return_counts=True)
    assert torch.equal(runs, ref_runs) and torch.equal(lengths, ref_lengths) and torch.equal(gpu.unique_consecutive(y), ref_runs)
    # the device wrappers: full-length tensors and the one-word count; the keys themselves may take the distinct keys
    keys, counts, first, inverse, num = gpu.GPUUnique(x, counts=True, first=True, inverse=True, check_fault=True)
    m = int(num.item())
    assert keys.numel() == counts.numel() == first.numel() == inverse.numel() == n and num.numel() == 1 and m == ref[0].numel()
    assert torch.equal(keys[:m], ref[0]) and torch.equal(counts[:m].long(), ref[2]) and torch.equal(inverse.long(), ref[1])
    assert torch.equal(x[first[:m].long()], ref[0])
    z = x.clone()
    same, num = gpu.GPUUnique(z, out=z, check_fault=True)
    assert same is z and torch.equal(z[: int(num.item())], ref[0]) and torch.equal(z[m:], x[m:])
    rk, rc, rs, rn = gpu.GPURunLength(y, counts=True, starts=True, check_fault=True)
    r = int(rn.item())
    assert torch.equal(rk[:r], ref_runs) and torch.equal(rc[:r].long(), ref_lengths)
    assert torch.equal(rs[:r].long(), torch.cumsum(ref_lengths, 0) - ref_lengths)
    empty = x[:0]
    assert gpu.unique(empty).numel() == 0 and gpu.unique_consecutive(empty).numel() == 0


@pytest.mark.parametrize("key_type", ["uint32", "int64"])
def test_unique_into_the_keys_themselves(gpu, key_type):
    w = un.width_of(key_type)
    for n in (3, un.TILE + 1, 5 * un.TILE + 7):
        for name in ("random8", "all_distinct", "runs_T-1"):
            run_unique(gpu, un.shuffled(n, w, name), key_type, False, UNIQUE_OUTPUTS["all"], in_place=True, out_skip=12)
            run_unique(gpu, un.shuffled(n, w, name), key_type, True, UNIQUE_OUTPUTS["none"], in_place=True, key_skip=w // 8)


# ---- one size past every loop's first round -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [32, 64])
def test_the_size_past_every_first_round(gpu, w):
    """BIG_N keys, about BIG_DISTINCT distinct values, all outputs: the scan's second round with its two carries, and more 16-byte
    groups than the copy kernel's grid has threads.  The host oracle is np.unique."""
    bits = un.big_keys(w)
    assert bits.size == un.BIG_N and -(-bits.size // un.TILE) > un.SCAN_ROUND
    keys, index, inverse, counts = np.unique(bits, return_index=True, return_inverse=True, return_counts=True)
    assert keys.size > un.MAX_GRID * un.THREADS
    want = {"keys": keys, "counts": counts.astype(np.uint32), "first": index.astype(np.uint32), "inverse": inverse.reshape(-1).astype(np.uint32)}
    run_unique(gpu, bits, "uint%d" % w, False, UNIQUE_OUTPUTS["all"], want, out_skip=4)
    # and the run-length entry alone on the sorted keys, with np.unique's counts and first positions of the sorted array
    in_order = np.sort(bits)
    run_rle(gpu, in_order, True, True, out_skip=12)


# ---- graph capture -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [32, 64])
def test_rle_graph_replays_follow_changed_keys(gpu, w):
    """lsdsort_rle_device launches kernels only and rewrites every word of its state on every call: one capture, three replays, each
    on other keys -- 8 runs per tile or so, a run per key, one run."""
    import torch

    L = gpu.lib()
    assert L.lsdsort_prepare_device() == 0
    n = 2 * un.TILE + 1
    signed = np.int32 if w == 32 else np.int64
    dk = torch.zeros(n, dtype=torch.int32 if w == 32 else torch.int64, device="cuda")
    out = torch.zeros_like(dk)
    counts, starts = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2))
    num = torch.zeros(1, dtype=torch.int32, device="cuda")
    need = L.lsdsort_rle_workspace_bytes(n, w)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")

    def call():
        st = L.lsdsort_rle_device(dk.data_ptr(), n, w, out.data_ptr(), counts.data_ptr(), starts.data_ptr(), num.data_ptr(), ws.data_ptr(),
                                  need, int(torch.cuda.current_stream().cuda_stream))
        assert st == 0, st

    dk.copy_(torch.from_numpy(un.families(n, w)["alternating"].view(signed).copy()))
    call()   # warm-up: device set-up stays out of the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for name in ("recurring", "all_distinct", "all_equal"):
        bits = un.families(n, w)[name]
        want = un.oracle_rle(bits)
        m = want["keys"].size
        dk.copy_(torch.from_numpy(bits.view(signed).copy()))
        for t_ in (out, counts, starts, num):
            t_.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert int(num.item()) == m, name
        assert np.array_equal(_host(out, bits.dtype)[:m], want["keys"]) and (_host(out, signed)[m:] == -1).all(), name
        assert np.array_equal(_host(counts, np.uint32)[:m], want["counts"]) and (_host(counts, np.int32)[m:] == -1).all(), name
        assert np.array_equal(_host(starts, np.uint32)[:m], want["starts"]) and (_host(starts, np.int32)[m:] == -1).all(), name
        assert L.lsdsort_check_device(ws.data_ptr(), None) == 0


@pytest.mark.parametrize("key_type", ["int32", "float64"])
def test_graph_replay_follows_changed_keys(gpu, key_type):
    """lsdsort_unique_device captured once and replayed four times, each time on other keys -- eight values, a run per key, one run,
    eight values drawn anew: count and every output follow.  (A second replay used to come back unsorted: the sort inside opened with
    a captured memset; tests/test_gpu_replay.py holds every entry that opened with one.)"""
    import torch

    L = gpu.lib()
    assert L.lsdsort_prepare_device() == 0
    w = un.width_of(key_type)
    n = 2 * un.TILE + 1
    code = un.KEY_CODE[key_type]
    signed = np.int32 if w == 32 else np.int64
    dk = torch.zeros(n, dtype=torch.int32 if w == 32 else torch.int64, device="cuda")
    out = torch.zeros_like(dk)
    counts, first, inverse = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(3))
    num = torch.zeros(1, dtype=torch.int32, device="cuda")
    need = L.lsdsort_unique_workspace_bytes(n, code, 1)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")

    def call():
        st = L.lsdsort_unique_device(dk.data_ptr(), n, code, 1, out.data_ptr(), counts.data_ptr(), first.data_ptr(), inverse.data_ptr(),
                                     num.data_ptr(), ws.data_ptr(), need, int(torch.cuda.current_stream().cuda_stream))
        assert st == 0, st

    dk.copy_(torch.from_numpy(un.shuffled(n, w, "alternating").view(signed).copy()))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()   # warm-up: device set-up stays out of the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    # captured on two distinct values; the last replay is another draw of the eight values of the first
    replays = [(name, un.shuffled(n, w, name)) for name in ("random8", "all_distinct", "all_equal")] + [("random8 again", un.families(n, w, 1)["random8"])]
    for name, bits in replays:
        want = un.oracle_unique(bits, key_type, True)
        m = want["keys"].size
        dk.copy_(torch.from_numpy(bits.view(signed).copy()))
        for t in (out, counts, first, inverse, num):
            t.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert int(num.item()) == m, name
        assert np.array_equal(_host(out, bits.dtype)[:m], want["keys"]) and (_host(out, signed)[m:] == -1).all(), name
        assert np.array_equal(_host(counts, np.uint32)[:m], want["counts"]) and np.array_equal(_host(first, np.uint32)[:m], want["first"]), name
        assert np.array_equal(_host(inverse, np.uint32), want["inverse"]), name
        assert L.lsdsort_unique_check_device(ws.data_ptr(), n, code, 1, None) == 0
