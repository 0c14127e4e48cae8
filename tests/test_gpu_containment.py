"""GPU suite: every device entry of include/lsdsort.h stays inside the buffers it is given.

Each case calls the C entry through gpu.lib() with guarded buffers of its own (tests/_guarded.py): 65536 sentinel elements on
either side of every array, a workspace of EXACTLY the bytes the library reports with 65536 sentinel bytes on either side, and
the arrays at chosen 16-byte phases (keys at `skip`, payload e at (skip + 4 (e + 1)) % 16) so that the key-by-key load paths
run too.  Every case asserts: the entry returns LSDSORT_OK and its check entry 0; the result is bit-exact against a CPU
reference (numpy's stable argsort of the order-preserving map, or the oracle); every guard zone is intact, the workspace's
included; read-only inputs are unchanged.  The api.py wrappers allocate outputs and workspaces themselves and would hide the
allocator's slack, so none is used here.

Inputs: seeded uniform keys with n // 7 duplicates of one value and the all-ones key (the padding value) present, never the
sentinel; the payload is the input position, so stability is part of every check.  The hybrid cases use plain uniform keys:
n // 7 duplicates would be one bucket above the local stage's capacity and the form would rightly be refused.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from _guarded import assert_intact, assert_unchanged, guarded, guarded_workspace, ptr, without_sentinel
from test_gpu_segmented import boundary_offsets
from test_gpu_segmented import expected as segmented_expected
from test_gpu_segmented import sortable_np as sortable32   # the order-preserving 32-bit map of include/lsdsort.h
from test_gpu_topk import expected_np as topk_expected

pytestmark = pytest.mark.gpu

ONES32 = np.uint32(0xFFFFFFFF)
ONES64 = np.uint64(0xFFFFFFFFFFFFFFFF)
TOP64 = np.uint64(1 << 63)
KEY32 = {"uint32": 0, "int32": 1, "float32": 2}
KEY64 = {"uint64": 3, "int64": 4, "float64": 5}
F32_SPECIALS = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x80000000, 0x00000000, 0x7F800000, 0xFF800000],
                        dtype=np.uint32)   # NaNs of both signs, -0.0, +0.0, the infinities
F64_SPECIALS = np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF, 1 << 63, 0,
                         0x7FF0000000000000, 0xFFF0000000000000], dtype=np.uint64)


def stream():
    return torch.cuda.current_stream().cuda_stream


def fill(n, value=0x5A5A5A5A, dtype=np.uint32):
    """What an output array holds before the call."""
    return np.full(n, value, dtype=dtype)


def same(view, want, what):
    """Bit-exact comparison of a device view with a host array."""
    bits = {4: np.uint32, 8: np.uint64}[view.element_size()]
    got = view.cpu().numpy().view(bits)
    want = np.ascontiguousarray(want).reshape(-1).view(bits)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{what}: {bad.size} of {got.size} elements differ, first at {bad[0]}: got {got[bad[0]]:#x} want {want[bad[0]]:#x}")


def position(n, e=0):
    """Payload array e: the input position (times e + 1, plus e, so that the arrays of one call differ); below the sentinel."""
    return (np.arange(n, dtype=np.uint64) * (e + 1) + e).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def keys32(n, seed=0):
    rng = np.random.default_rng(1000003 * seed + n)
    keys = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    if n:
        keys[rng.integers(0, n, size=n // 7)] = np.uint32(0x9E3779B9)
        keys[rng.integers(0, n)] = ONES32
    keys = without_sentinel(keys)
    keys.setflags(write=False)
    return keys


@functools.lru_cache(maxsize=None)
def keys64(n):
    rng = np.random.default_rng(77 + n)
    keys = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    if n:
        keys[rng.integers(0, n, size=n // 7)] = np.uint64(0x9E3779B97F4A7C15)
        k = min(n, F64_SPECIALS.size)
        keys[rng.permutation(n)[:k]] = F64_SPECIALS[:k]
        keys[rng.integers(0, n)] = ONES64
    keys = without_sentinel(keys)
    keys.setflags(write=False)
    return keys


def sortable64(bits, key_type, descending):
    """The 64-bit map, restated (as tests/test_gpu_wide_typed.py::_mapped does)."""
    bits = np.ascontiguousarray(bits, dtype=np.uint64)
    if key_type == "int64":
        t = bits ^ TOP64
    elif key_type == "float64":
        t = np.where(bits >> np.uint64(63) != 0, ~bits, bits ^ TOP64)
    else:
        t = bits.copy()
    return ~t if descending else t


@functools.lru_cache(maxsize=None)
def order32(n, key_type="uint32", descending=False, seed=0):
    """numpy's stable argsort of the mapped keys: computed once per input, shared by every case that sorts it."""
    keys = typed_keys32(n, key_type) if key_type != "uint32" else keys32(n, seed)
    order = np.argsort(sortable32(keys, key_type, descending), kind="stable")
    order.setflags(write=False)
    return order


@functools.lru_cache(maxsize=None)
def typed_keys32(n, key_type):
    """The keys of the typed sorts: random bit patterns (float32: NaN patterns of both signs among them) plus the specials."""
    keys = keys32(n, seed=5).copy()
    if key_type == "float32" and n:
        rng = np.random.default_rng(n)
        k = min(n, F32_SPECIALS.size)
        keys[rng.permutation(n)[:k]] = F32_SPECIALS[:k]
    keys.setflags(write=False)
    return keys


@functools.lru_cache(maxsize=None)
def order64(n, key_type, descending):
    order = np.argsort(sortable64(keys64(n), key_type, descending), kind="stable")
    order.setflags(write=False)
    return order


def check_ok(L, ws_view, n, what):
    if n:
        assert L.lsdsort_check_device(ws_view.data_ptr(), stream()) == 0, (what, "fault word")


def form_of(L, ws_view):
    hybrid = ctypes.c_int(-1)
    assert L.lsdsort_workspace_form(ws_view.data_ptr(), stream(), ctypes.byref(hybrid)) == 0
    return hybrid.value


def sort_u32(L, keys, order, r, algo, payloads, skip, workspace=None, multi=False, what=None):
    """One uint32 sort of `keys` (expected order `order`) through lsdsort_u32_device_ex, or lsdsort_multi_u32_device, in guarded
    buffers.  workspace: (whole, view) to share one; otherwise one of exactly the reported size is made.  Returns the view."""
    n = keys.size
    what = what or (n, r, algo, payloads, skip)
    kbig, kv = guarded(keys, skip)
    pay = [guarded(position(n, e), (skip + 4 * (e + 1)) % 16) for e in range(payloads)]
    if workspace is None:
        nbytes = L.lsdsort_workspace_bytes_ex(n, r, payloads, algo) if n else 1
        assert nbytes > 0
        workspace = guarded_workspace(nbytes)
    wbig, ws = workspace
    if multi:
        ptrs = (ctypes.c_void_p * payloads)(*[ptr(v) for _, v in pay])
        st = L.lsdsort_multi_u32_device(ptr(kv), ptrs, payloads, ws.data_ptr(), ws.numel(), n, r, stream())
    else:
        assert payloads <= 1
        st = L.lsdsort_u32_device_ex(ptr(kv), ptr(pay[0][1]) if payloads else None, ws.data_ptr(), ws.numel(), n, r, algo, stream())
    assert st == 0, (what, st)
    check_ok(L, ws, n, what)
    same(kv, keys[order], f"{what} keys")
    for e, (_, v) in enumerate(pay):
        same(v, position(n, e)[order], f"{what} payload {e} (stable order)")
    assert_intact(keys=kbig, workspace=wbig, **{f"payload_{e}": big for e, (big, _) in enumerate(pay)})
    return ws


# ----------------------------------------------------------------------------- lsdsort_u32_device_ex
CLASS_SIZES = [1, 4097, 16384, 16385, (1 << 19) - 1, (1 << 19) + 1, (1 << 21) + 1, (1 << 23) + 1]


@pytest.mark.parametrize("n", [0] + CLASS_SIZES)
@pytest.mark.parametrize("algo", [0, 1], ids=["chained", "staged"])
@pytest.mark.parametrize("r", [8, 4])
def test_u32_sorts_every_tile_class_and_alignment(gpu, r, algo, n):
    """Both sides of the one-launch cap and one size in every tile class; keys and pairs; every 16-byte phase."""
    L = gpu.lib()
    keys, order = keys32(n), order32(n)
    for skip in (0, 4, 8, 12):
        for pairs in (0, 1):
            sort_u32(L, keys, order, r, algo, pairs, skip)


@pytest.mark.parametrize("n", [0, (1 << 18) + 77, (1 << 21) + 5])
@pytest.mark.parametrize("algo", [0, 1], ids=["chained", "staged"])
@pytest.mark.parametrize("r", [2, 1])
def test_u32_sorts_narrow_digits(gpu, r, algo, n):
    L = gpu.lib()
    keys, order = keys32(n), order32(n)
    for skip in (0, 4):
        for pairs in (0, 1):
            sort_u32(L, keys, order, r, algo, pairs, skip)


@pytest.mark.parametrize("n", [1, 4097, 16384])
@pytest.mark.parametrize("switches", ["small_sort_off", "rank_method_0", "both"])
def test_u32_small_sizes_without_the_small_sort_and_by_peer_masks(gpu, switches, n):
    """The chained form at the sizes the one-launch sort otherwise serves, and the mask rank form there."""
    L = gpu.lib()
    keys, order = keys32(n), order32(n)
    try:
        if switches != "rank_method_0":
            assert L.lsdsort_set_small_sort(0) == 0
        if switches != "small_sort_off":
            assert L.lsdsort_set_rank_method(0) == 0
        for pairs in (0, 1):
            sort_u32(L, keys, order, 8, 0, pairs, 4)
    finally:
        L.lsdsort_set_small_sort(1)
        L.lsdsort_set_rank_method(-1)


@pytest.mark.parametrize("pairs", [0, 1], ids=["keys", "pairs"])
def test_one_workspace_serves_every_smaller_sort(gpu, pairs):
    """The guards sit at the LARGER size's reported bytes: a smaller sort that picks another tile shape must still fit."""
    L = gpu.lib()
    top = (1 << 23) + 5
    workspace = guarded_workspace(L.lsdsort_workspace_bytes(top, 8, pairs))
    for n in (top, (1 << 21) + 3, (1 << 19) - 1, 1000, 1):
        sort_u32(L, keys32(n), order32(n), 8, 0, pairs, 4, workspace=workspace)


# ----------------------------------------------------------------------------- lsdsort_multi_u32_device
@pytest.mark.parametrize("n", [0, 1, 10000, (1 << 20) + 9])
@pytest.mark.parametrize("payloads", [2, 3])
@pytest.mark.parametrize("r", [8, 4])
def test_multi_payload_sorts(gpu, r, payloads, n):
    L = gpu.lib()
    keys, order = keys32(n), order32(n)
    for skip in (0, 4):
        sort_u32(L, keys, order, r, 0, payloads, skip, multi=True)
    if n == 0:   # an empty call may come with a null array of arrays as well
        assert L.lsdsort_multi_u32_device(None, None, payloads, None, 0, 0, r, stream()) == 0


# ----------------------------------------------------------------------------- lsdsort_keys_device
def sort_typed(L, keys, order, key_type, descending, r, payload, skip):
    n = keys.size
    what = (key_type, descending, n, r, payload, skip)
    kbig, kv = guarded(keys, skip)
    vbig, vv = guarded(position(n), (skip + 4) % 16) if payload else (None, None)
    wbig, ws = guarded_workspace(L.lsdsort_workspace_bytes(n, r, int(payload)) if n else 1)
    st = L.lsdsort_keys_device(ptr(kv), ptr(vv), ws.data_ptr(), ws.numel(), n, r, KEY32[key_type], int(descending), stream())
    assert st == 0, (what, st)
    check_ok(L, ws, n, what)
    same(kv, keys[order], f"{what} keys in the typed order")
    if payload:
        same(vv, position(n)[order], f"{what} payload (stable order)")
    assert_intact(keys=kbig, payload=vbig, workspace=wbig)
    return ws


@pytest.mark.parametrize("n", [0, 1, 4097, (1 << 20) + 13])
@pytest.mark.parametrize("descending", [False, True], ids=["ascending", "descending"])
@pytest.mark.parametrize("key_type", ["int32", "float32"])
def test_typed_sorts(gpu, key_type, descending, n):
    """float32 keeps its NaN bit patterns of both signs, -0.0 and the infinities: the reference is the total-order map."""
    L = gpu.lib()
    keys, order = typed_keys32(n, key_type), order32(n, key_type, descending)
    for r in (8, 4):
        for skip in (0, 12):
            for payload in (False, True):
                sort_typed(L, keys, order, key_type, descending, r, payload, skip)


# ----------------------------------------------------------------------------- lsdsort_keys64_device, lsdsort_records_device
WIDE_SIZES = [0, 1, 4097, 16385, (1 << 20) + 5]


def sort_wide(L, oracle_mod, key_bits, val_bits, key_type, descending, n, r, skip, records):
    what = (key_bits, val_bits, key_type, descending, n, r, skip, "records" if records else "keys64")
    if key_bits == 64:
        keys, order = keys64(n), order64(n, key_type, descending)
    else:
        keys, order = keys32(n), order32(n)
    vals = None if not val_bits else position(n) if val_bits == 32 else (np.arange(n, dtype=np.uint64) << np.uint64(31)) + np.uint64(3)
    kbig, kv = guarded(keys, skip)
    vbig, vv = guarded(vals, (skip + 4) % 16 if val_bits == 32 else (skip // 8 * 8 + 8) % 16) if val_bits else (None, None)
    wbig, ws = guarded_workspace(L.lsdsort_wide_workspace_bytes(n, r, key_bits, val_bits) if n else 1)
    if records:
        st = L.lsdsort_records_device(ptr(kv), ptr(vv), key_bits, val_bits, ws.data_ptr(), ws.numel(), n, r, stream())
    else:
        st = L.lsdsort_keys64_device(ptr(kv), ptr(vv), val_bits, ws.data_ptr(), ws.numel(), n, r, KEY64[key_type], int(descending), stream())
    assert st == 0, (what, st)
    assert L.lsdsort_wide_check_device(ws.data_ptr(), n, r, key_bits, val_bits, stream()) == 0, what
    same(kv, keys[order], f"{what} keys")
    if key_bits == 64 and not val_bits:   # a second reference: std::sort of the mapped keys
        got = kv.cpu().numpy().view(np.uint64)
        assert np.array_equal(sortable64(got, key_type, descending), oracle_mod.std_sort_u64(sortable64(keys, key_type, descending))), what
    if val_bits:
        same(vv, vals[order], f"{what} payload (stable order)")
    assert_intact(keys=kbig, payload=vbig, workspace=wbig)


@pytest.mark.parametrize("n", WIDE_SIZES)
@pytest.mark.parametrize("descending", [False, True], ids=["ascending", "descending"])
@pytest.mark.parametrize("key_type", list(KEY64))
def test_keys64_sorts(gpu, oracle_mod, key_type, descending, n):
    """64/0, 64/32 and 64/64 through lsdsort_keys64_device; keys at 0 and 8 mod 16 (the 16-byte and the key-by-key split)."""
    L = gpu.lib()
    for val_bits in (0, 32, 64):
        for skip in (0, 8):
            for r in ((8, 4) if n == 4097 else (8,)):
                sort_wide(L, oracle_mod, 64, val_bits, key_type, descending, n, r, skip, records=False)


@pytest.mark.parametrize("n", WIDE_SIZES)
@pytest.mark.parametrize("key_bits,val_bits", [(64, 32), (64, 64), (32, 64)])
def test_records_sorts(gpu, oracle_mod, key_bits, val_bits, n):
    """lsdsort_records_device (uint keys, ascending); 32-bit keys at every phase a 32-bit array can have."""
    L = gpu.lib()
    for skip in ((0, 8) if key_bits == 64 else (0, 4, 8, 12)):
        for r in ((8, 4) if n == 4097 else (8,)):
            sort_wide(L, oracle_mod, key_bits, val_bits, "uint64", False, n, r, skip, records=True)
    if n == (1 << 20) + 5 and key_bits == 64 and val_bits == 64:   # a third reference for the records: the oracle's stable sort
        keys = keys64(n)
        vals = (np.arange(n, dtype=np.uint64) << np.uint64(31)) + np.uint64(3)
        ek, ev = oracle_mod.std_stable_sort_records(keys, vals)
        order = order64(n, "uint64", False)
        assert np.array_equal(ek, keys[order]) and np.array_equal(ev, vals[order])


# ----------------------------------------------------------------------------- the hybrid window's lower ends
@functools.lru_cache(maxsize=2)
def hybrid_keys(n, dist):
    rng = np.random.default_rng(n)
    keys = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    keys[rng.integers(0, n)] = ONES32
    if dist == "half_zeros":
        keys[(keys >> np.uint32(13)) & np.uint32(1) == 0] = 0    # bucket 0 holds half the keys: above the local stage's capacity
    keys = without_sentinel(keys)
    keys.setflags(write=False)
    return keys


def on_device(view, want, what):
    """The same comparison on the device (the large cases: one upload instead of one download per array)."""
    want = torch.from_numpy(np.ascontiguousarray(want).view(np.int32)).cuda()
    if not torch.equal(view, want):
        same(view, want.cpu().numpy(), what)


@functools.lru_cache(maxsize=1)
def hybrid_reference(oracle_mod, n, dist, with_payloads):
    """(sorted keys, stable order or None) by the oracle: computed once, shared by the cases at either phase."""
    keys = hybrid_keys(n, dist)
    if with_payloads:
        return oracle_mod.std_stable_sort_pairs(keys, np.arange(n, dtype=np.uint32))
    return oracle_mod.lsd_sort(keys, 8), None


@pytest.mark.parametrize("skip", [0, 4])
@pytest.mark.parametrize("dist,form", [("uniform", 1), ("half_zeros", 0)])
@pytest.mark.parametrize("r,n,payloads", [(4, (1 << 24) + 99, 0), (8, 22_000_007, 1), (8, 38_000_005, 0), (8, (1 << 25) + 4321, 3)],
                         ids=["r4_keys", "r8_pairs", "r8_keys", "r8_three_payloads"])
def test_hybrid_window_lower_ends(gpu, oracle_mod, r, n, payloads, dist, form, skip):
    """The smallest sizes at which the hybrid form is tried (hybrid_min_items), on keys the device takes and on keys it must
    refuse.  A misaligned base changes the load path of the bucket histograms, not their counts: the form is the same at
    either phase.  References: the oracle's LSD sort for keys, its std::stable_sort of (key, position) for payloads."""
    L = gpu.lib()
    keys = hybrid_keys(n, dist)
    ek, order = hybrid_reference(oracle_mod, n, dist, payloads > 0)
    what = (r, n, payloads, dist, skip)
    kbig, kv = guarded(keys, skip)
    pay = [guarded(position(n, e), (skip + 4 * (e + 1)) % 16) for e in range(payloads)]
    nbytes = L.lsdsort_workspace_bytes(n, r, payloads)
    wbig, ws = guarded_workspace(nbytes)
    if payloads > 1:
        ptrs = (ctypes.c_void_p * payloads)(*[v.data_ptr() for _, v in pay])
        st = L.lsdsort_multi_u32_device(kv.data_ptr(), ptrs, payloads, ws.data_ptr(), nbytes, n, r, stream())
    else:
        st = L.lsdsort_u32_device_ex(kv.data_ptr(), pay[0][1].data_ptr() if payloads else None, ws.data_ptr(), nbytes, n, r, 0, stream())
    assert st == 0, (what, st)
    assert L.lsdsort_check_device(ws.data_ptr(), stream()) == 0, what
    assert form_of(L, ws) == form, (what, "lsdsort_workspace_form")
    on_device(kv, ek, f"{what} keys")
    for e, (_, v) in enumerate(pay):
        on_device(v, position(n, e)[order], f"{what} payload {e} (stable order)")
    assert_intact(keys=kbig, workspace=wbig, **{f"payload_{e}": big for e, (big, _) in enumerate(pay)})


@functools.lru_cache(maxsize=1)
def refused_typed_keys(name):
    n = (1 << 24) + 99
    rng = np.random.default_rng(len(name))
    if name == "int32_below_1000":          # every key shares its top 22 bits: one bucket holds all n, seven of the eight passes are dead
        keys = rng.integers(0, 1000, size=n, dtype=np.uint64).astype(np.uint32)
    elif name == "float32_1_to_2":          # a constant top 9 bits
        keys = (1.0 + rng.random(n, dtype=np.float32) * np.float32(0.99999)).astype(np.float32).view(np.uint32).copy()
        assert ((keys >> np.uint32(23)) == 0x7F).all()
    else:                                   # half +0.0, the rest finite values of both signs
        keys = rng.standard_normal(n).astype(np.float32).view(np.uint32).copy()
        keys[rng.random(n) < 0.5] = 0
    keys.setflags(write=False)
    return keys


@functools.lru_cache(maxsize=1)
def refused_typed_order(name, key_type, descending):
    order = np.argsort(sortable32(refused_typed_keys(name), key_type, descending), kind="stable")
    order.setflags(write=False)
    return order


@pytest.mark.parametrize("skip", [0, 4])
@pytest.mark.parametrize("payload", [False, True], ids=["keys", "pairs"])
@pytest.mark.parametrize("descending", [False, True], ids=["ascending", "descending"])
@pytest.mark.parametrize("name,key_type", [("int32_below_1000", "int32"), ("float32_1_to_2", "float32"), ("float32_half_zero", "float32")])
def test_typed_sorts_whose_hybrid_attempt_is_refused(gpu, name, key_type, descending, payload, skip):
    """A typed sort gets a pass plan only where the hybrid form is tried, and that plan must never skip a pass: the last
    ordinary pass stores the inverse key transform.  Were a dead pass skipped, the output would stay in sortable form."""
    L = gpu.lib()
    keys = refused_typed_keys(name)
    n = keys.size
    order = refused_typed_order(name, key_type, descending)
    what = (name, descending, payload, skip)
    kbig, kv = guarded(keys, skip)
    vbig, vv = guarded(position(n), (skip + 4) % 16) if payload else (None, None)
    nbytes = L.lsdsort_workspace_bytes(n, 4, int(payload))
    wbig, ws = guarded_workspace(nbytes)
    st = L.lsdsort_keys_device(kv.data_ptr(), ptr(vv), ws.data_ptr(), nbytes, n, 4, KEY32[key_type], int(descending), stream())
    assert st == 0, (what, st)
    assert L.lsdsort_check_device(ws.data_ptr(), stream()) == 0, what
    assert form_of(L, ws) == 0, (what, "the hybrid form must be refused")
    on_device(kv, keys[order], f"{what} keys in the typed order")
    if payload:
        on_device(vv, order.astype(np.uint32), f"{what} payload (stable order)")
    assert_intact(keys=kbig, payload=vbig, workspace=wbig)


# ----------------------------------------------------------------------------- lsdsort_segmented_device
@pytest.mark.parametrize("skip", [0, 4])
@pytest.mark.parametrize("pairs", [False, True], ids=["keys", "pairs"])
def test_segmented_sort(gpu, pairs, skip):
    """Every size-class boundary, the 10^6 + 7 segment included, with 77 keys in front of the first segment and 131 behind
    the last that no segment covers."""
    L = gpu.lib()
    off, n = boundary_offsets(head=77, tail=131)
    segs = len(off) - 1
    keys = keys32(n, seed=3)
    vals = position(n) if pairs else None
    ek, ev = segmented_expected(keys, off, vals)
    off32 = off.astype(np.uint32)
    kbig, kv = guarded(keys, skip)
    vbig, vv = guarded(vals, (skip + 4) % 16) if pairs else (None, None)
    obig, ov = guarded(off32, (skip + 8) % 16)
    nbytes = L.lsdsort_segmented_workspace_bytes(n, segs, int(pairs))
    wbig, ws = guarded_workspace(nbytes)
    st = L.lsdsort_segmented_device(kv.data_ptr(), ptr(vv), ov.data_ptr(), segs, n, 0, 0, ws.data_ptr(), nbytes, stream())
    assert st == 0, st
    assert L.lsdsort_check_device(ws.data_ptr(), stream()) == 0
    same(kv, ek, "keys")
    if pairs:
        same(vv, ev, "payload (stable order)")
    same(kv[:77], keys[:77], "the keys in front of the first segment")
    same(kv[n - 131:], keys[n - 131:], "the keys behind the last segment")
    assert_unchanged(ov, off32, "the offsets")
    assert_intact(keys=kbig, payload=vbig, offsets=obig, workspace=wbig)


def test_segmented_sort_of_nothing(gpu):
    L = gpu.lib()
    wbig, ws = guarded_workspace(1)
    assert L.lsdsort_segmented_device(None, None, None, 0, 0, 0, 0, ws.data_ptr(), 1, stream()) == 0
    assert_intact(workspace=wbig)


# ----------------------------------------------------------------------------- lsdsort_topk_device
@pytest.mark.parametrize("key_type,largest", [("float32", True), ("uint32", False)])
@pytest.mark.parametrize("rows,cols,k", [(0, 0, 0), (9, 700, 33), (5, 9000, 1500), (3, 300007, 1000), (1, (1 << 22) + 5, 1024)],
                         ids=lambda v: str(v))
def test_topk(gpu, rows, cols, k, key_type, largest):
    """One wavefront per row, one workgroup per row, many workgroups per row; values, indices and workspace guarded."""
    L = gpu.lib()
    n = rows * cols
    keys = (typed_keys32(n, "float32") if key_type == "float32" else keys32(n, seed=9)).reshape(rows, cols)
    kbig, kv = guarded(keys, 4)
    obig, ov = guarded(fill(rows * k), 8)
    ibig, iv = guarded(fill(rows * k, 0x3C3C3C3C), 12)
    nbytes = L.lsdsort_topk_workspace_bytes(rows, cols, k) if n else 1
    wbig, ws = guarded_workspace(nbytes)
    st = L.lsdsort_topk_device(ptr(kv), rows, cols, k, KEY32[key_type], int(largest), ptr(ov), ptr(iv), ws.data_ptr(), nbytes, stream())
    assert st == 0, st
    if n:
        assert L.lsdsort_check_device(ws.data_ptr(), stream()) == 0
        ek, ei = topk_expected(keys, key_type, largest)
        same(ov, ek[:, :k], "values")
        same(iv, ei[:, :k], "indices (ties by position)")
        assert_unchanged(kv, keys, "the keys")
    assert_intact(keys=kbig, values=obig, indices=ibig, workspace=wbig)


# ----------------------------------------------------------------------------- the three partition entries
def partition_case(L, entry, keys, bits, cuts, bucket, skip):
    n = keys.size
    what = (entry, n, bits, skip)
    order = np.argsort(bucket, kind="stable")
    kbig, kv = guarded(keys, skip)
    obig, ov = guarded(fill(n), (skip + 4) % 16)
    cbig, cv = guarded(fill(1 << bits, 0x5A5A5A5A5A5A5A5A, np.uint64), 8)
    nbytes = L.lsdsort_msb_partition_workspace_bytes(n, bits)   # n = 0 too: the entry clears its control block and writes the counts
    wbig, ws = guarded_workspace(nbytes)
    args = (ptr(kv), ptr(ov), n, bits) + cuts + (cv.data_ptr(), ws.data_ptr(), nbytes, stream())
    st = getattr(L, entry)(*args)
    assert st == 0, (what, st)
    assert L.lsdsort_check_device(ws.data_ptr(), stream()) == 0, what
    same(cv, np.bincount(bucket, minlength=1 << bits).astype(np.uint64), f"{what} counts")
    same(ov, keys[order], f"{what} partitioned keys (stable)")
    assert_unchanged(kv, keys, f"{what} input")
    assert_intact(input=kbig, out=obig, counts=cbig, workspace=wbig)


PARTITION_SIZES = [0, 1, 4097, (1 << 20) + 7]


@pytest.mark.parametrize("n", PARTITION_SIZES)
@pytest.mark.parametrize("bits", [0, 1, 2, 3])
def test_msb_partition(gpu, oracle_mod, bits, n):
    L = gpu.lib()
    keys = keys32(n, seed=4)
    bucket = (keys.astype(np.uint64) >> np.uint64(32 - bits)).astype(np.int64) if bits else np.zeros(n, dtype=np.int64)
    eo, ec = oracle_mod.msb_partition(keys, bits)
    assert np.array_equal(eo, keys[np.argsort(bucket, kind="stable")]) and np.array_equal(ec, np.bincount(bucket, minlength=1 << bits))
    for skip in (0, 4):
        partition_case(L, "lsdsort_msb_partition_u32_device", keys, bits, (), bucket, skip)


@pytest.mark.parametrize("n", PARTITION_SIZES)
@pytest.mark.parametrize("cuts", [1, 3, 7])
@pytest.mark.parametrize("form", ["splitter", "threshold"])
def test_value_partitions(gpu, form, cuts, n):
    """bucket(key) = number of bounds <= key; keys equal to a bound, an empty bucket, and (thresholds) 2^32 = above every key."""
    L = gpu.lib()
    keys = keys32(n, seed=4)
    rng = np.random.default_rng(cuts + n)
    bounds = sorted(int(x) for x in rng.choice(keys, size=cuts, replace=True)) if n else list(range(1, cuts + 1))
    if cuts >= 3:
        bounds[1] = bounds[0]                                   # an empty bucket
    if form == "threshold":
        bounds[-1] = 1 << 32                                    # the last bucket stays empty, the all-ones key included
        arr = (ctypes.c_uint64 * cuts)(*bounds)
    else:
        arr = (ctypes.c_uint32 * cuts)(*bounds)
    bucket = np.zeros(n, dtype=np.int64)
    for b in bounds:
        if b < (1 << 32):
            bucket += keys >= np.uint32(b)
    bits = (cuts + 1).bit_length() - 1
    for skip in (0, 4):
        partition_case(L, f"lsdsort_{form}_partition_u32_device", keys, bits, (arr,), bucket, skip)


# ----------------------------------------------------------------------------- stage entries
@pytest.mark.parametrize("skip", [0, 4])
@pytest.mark.parametrize("r,bg", [(8, 0), (8, 3), (4, 5), (2, 9), (1, 18)])
def test_stage_tile_histograms(gpu, oracle_mod, r, bg, skip):
    L = gpu.lib()
    tile = gpu.tile_keys(r)
    keys = keys32(5 * tile + 321, seed=6)
    tiles = 6
    kbig, kv = guarded(keys, skip)
    hbig, hv = guarded(fill(tiles << r), (skip + 8) % 16)
    assert L.lsdsort_tile_histograms_u32_device(kv.data_ptr(), keys.size, r, bg, hv.data_ptr(), stream()) == 0
    same(hv, oracle_mod.tile_histograms(keys, tile, r, bg), "h[tile][digit]")
    assert_unchanged(kv, keys, "the keys")
    assert_intact(keys=kbig, hist=hbig)
    assert L.lsdsort_tile_histograms_u32_device(None, 0, r, bg, None, stream()) == 0


@pytest.mark.parametrize("tiles", [0, 1, 64, 1000])
@pytest.mark.parametrize("r", [8, 4])
def test_stage_tile_offsets(gpu, oracle_mod, r, tiles):
    L = gpu.lib()
    if tiles == 0:
        assert L.lsdsort_tile_offsets_u32_device(None, None, None, 0, r, None, stream()) == 0
        return
    hist = np.random.default_rng(r * 1000 + tiles).integers(0, 9000, size=(tiles, 1 << r), dtype=np.uint32)
    hbig, hv = guarded(hist, 4)
    lbig, lv = guarded(fill(hist.size), 8)
    gbig, gv = guarded(fill(hist.size), 12)
    nbytes = L.lsdsort_tile_offsets_scratch_bytes(tiles, r)
    sbig, sv = guarded_workspace(nbytes)
    assert L.lsdsort_tile_offsets_u32_device(hv.data_ptr(), lv.data_ptr(), gv.data_ptr(), tiles, r, sv.data_ptr(), stream()) == 0
    same(lv, oracle_mod.local_offsets(hist, r), "local offsets")
    same(gv, oracle_mod.global_offsets(hist, r), "global offsets")
    assert_unchanged(hv, hist, "the counts")
    assert_intact(hist=hbig, local=lbig, **{"global": gbig, "scratch": sbig})


@pytest.mark.parametrize("skip", [0, 4])
@pytest.mark.parametrize("r,bg", [(8, 1), (4, 2), (2, 0), (1, 31)])
def test_stage_rank_scatter(gpu, oracle_mod, r, bg, skip):
    L = gpu.lib()
    tile = gpu.tile_keys(r)
    keys = keys32(7 * tile + 11, seed=7)
    n = keys.size
    h = oracle_mod.tile_histograms(keys, tile, r, bg)
    local, glob = oracle_mod.local_offsets(h, r), oracle_mod.global_offsets(h, r)
    expect = oracle_mod.rank_scatter(keys, local, glob, tile, r, bg)
    order = np.argsort((keys >> np.uint32(r * bg)) & np.uint32((1 << r) - 1), kind="stable")
    assert np.array_equal(expect, keys[order])
    kbig, kv = guarded(keys, skip)
    vbig, vv = guarded(position(n), (skip + 4) % 16)
    gbig, gv = guarded(glob, (skip + 8) % 16)
    for with_vals in (False, True):
        obig, ov = guarded(fill(n), (skip + 12) % 16)
        pbig, pv = guarded(fill(n), skip)
        st = L.lsdsort_rank_scatter_u32_device(kv.data_ptr(), ov.data_ptr(), vv.data_ptr() if with_vals else None,
                                               pv.data_ptr() if with_vals else None, gv.data_ptr(), n, r, bg, stream())
        assert st == 0, st
        same(ov, expect, "scattered keys")
        same(pv, position(n)[order] if with_vals else fill(n), "scattered payload (or none written)")
        assert_intact(out=obig, vals_out=pbig)
    assert_unchanged(kv, keys, "the keys")
    assert_unchanged(vv, position(n), "the payload")
    assert_unchanged(gv, glob, "the global table")
    assert_intact(keys=kbig, vals=vbig, **{"global": gbig})
    assert L.lsdsort_rank_scatter_u32_device(None, None, None, None, None, 0, r, bg, stream()) == 0


@pytest.mark.parametrize("skip", [0, 4])
@pytest.mark.parametrize("r", [1, 2, 4, 8])
def test_stage_digit_histograms(gpu, oracle_mod, r, skip):
    L = gpu.lib()
    for n in (0, 1, 1023, (1 << 20) + 13):
        keys = keys32(n, seed=8)
        kbig, kv = guarded(keys, skip)
        hbig, hv = guarded(fill((32 // r) << r), (skip + 4) % 16)
        assert L.lsdsort_digit_histograms_u32_device(ptr(kv), n, r, hv.data_ptr(), stream()) == 0
        same(hv, oracle_mod.digit_histograms(keys, r).astype(np.uint32), f"n={n} [group][digit]")
        assert_unchanged(kv, keys, "the keys")
        assert_intact(keys=kbig, hist=hbig)


@pytest.mark.parametrize("with_vals", [False, True], ids=["keys", "pairs"])
@pytest.mark.parametrize("low_bits", [9, 17, 24, 27, 1])
def test_stage_local_sort(gpu, low_bits, with_vals):
    """The bucket sizes of tests/test_gpu_hybrid.py::test_local_stage_alone with bases[0] = 77: the keys in front of the first
    bucket are no bucket's and stay as they are, like the bucket above the capacity."""
    L = gpu.lib()
    sizes = [0, 1, 2, 63, 64, 65, 511, 512, 513, 1000, 4096, 8191, 8192, 16383, 16384, 16385, 0, 7, 12345]
    bases = (np.concatenate([[0], np.cumsum(sizes)]) + 77).astype(np.uint32)
    n = int(bases[-1])
    keys = keys32(n, seed=low_bits)
    mask = np.uint32((1 << low_bits) - 1)
    ek, ev = keys.copy(), position(n)
    for b, size in enumerate(sizes):
        lo, hi = int(bases[b]), int(bases[b + 1])
        if size <= 16384:
            order = np.argsort(keys[lo:hi] & mask, kind="stable") + lo
            ek[lo:hi], ev[lo:hi] = keys[order], position(n)[order]
    kbig, kv = guarded(keys, 4)
    vbig, vv = guarded(position(n), 8) if with_vals else (None, None)
    bbig, bv = guarded(bases, 12)
    st = L.lsdsort_local_sort_u32_device(kv.data_ptr(), ptr(vv), bv.data_ptr(), len(sizes), low_bits, stream())
    assert st == 0, st
    same(kv, ek, "keys: buckets sorted by their low bits, the head and the bucket above the capacity untouched")
    if with_vals:
        same(vv, ev, "payload (stable order)")
    assert_unchanged(bv, bases, "the bucket bases")
    assert_intact(keys=kbig, vals=vbig, bases=bbig)
    assert L.lsdsort_local_sort_u32_device(None, None, None, 0, low_bits, stream()) == 0
