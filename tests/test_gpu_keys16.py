"""GPU suite: 16-bit keys (lsdsort_keys16_device, GPUSort16, sort16) -- uint16, int16, float16 and bfloat16, both orders, on both
routes: the count route (count the 65536 values, scan, fill; keys only) and the widen route (map to uint32, the ordinary sort,
narrow; payloads, and small keys-only sorts).  Everything is compared bit for bit against numpy on the uint16 bit patterns: the
map of include/lsdsort.h restated here, keys only inverse(np.sort(t)), pairs the stable argsort of t."""
import contextlib

import numpy as np
import pytest

from _guarded import assert_intact, guarded, guarded_workspace
from _guarded16 import assert_intact16, bits_of, guarded16
from _key_oracle import ALL_TYPES16 as KEY_TYPES

pytestmark = pytest.mark.gpu

SIZES = [1, 7, 8, 9, 63, 64, 65, 1023, 16384, 16385, 65535, 65536, 65537, (1 << 20) + 13, (1 << 22) + 5]
WIDEN, COUNT = 0, 1


def _auto_threshold():
    """kKeys16CountMinKeys as csrc/keys16.hip states it, so that the test below straddles the threshold wherever it moves."""
    import os
    import re

    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lsdradixsort_amd", "csrc", "keys16.hip")
    with open(path) as f:
        shift = re.search(r"constexpr size_t kKeys16CountMinKeys = \(size_t\)1 << (\d+);", f.read())
    assert shift, "kKeys16CountMinKeys is no longer written as (size_t)1 << N"
    return 1 << int(shift.group(1))


AUTO_THRESHOLD = _auto_threshold()
SPECIAL = [0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x007F, 0x807F,          # +-0, +-denormals of float16 and bfloat16
           0x7C00, 0xFC00, 0x7F80, 0xFF80, 0x7BFF, 0xFBFF, 0x7F7F, 0xFF7F,          # +-inf and +-max of either type
           0x7E00, 0xFE00, 0x7FC0, 0xFFC0, 0x7C01, 0xFC01, 0x7FFF, 0xFFFF, 0x7F81]  # NaNs of both signs; INT16_MAX, -1


def _dtype(key_type):
    import torch

    return {"uint16": torch.int16, "int16": torch.int16, "float16": torch.float16, "bfloat16": torch.bfloat16}[key_type]


def _mapped(bits, key_type, descending):
    """The uint16 whose unsigned order is the requested order of the key."""
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    if key_type == "int16":
        t = bits ^ np.uint16(0x8000)
    elif key_type in ("float16", "bfloat16"):
        t = np.where(bits & np.uint16(0x8000) != 0, ~bits, bits ^ np.uint16(0x8000)).astype(np.uint16)
    else:
        t = bits.copy()
    return (~t).astype(np.uint16) if descending else t


def _unmapped(t, key_type, descending):
    t = np.ascontiguousarray(t, dtype=np.uint16)
    u = (~t).astype(np.uint16) if descending else t
    if key_type == "int16":
        return u ^ np.uint16(0x8000)
    if key_type in ("float16", "bfloat16"):
        return np.where(u & np.uint16(0x8000) != 0, u ^ np.uint16(0x8000), ~u).astype(np.uint16)
    return u.copy()


_INPUTS, _WANT = {}, {}


def _inputs(n):
    """Random 16-bit patterns: NaNs of both signs, +-inf, +-0 and denormals of both float types are in there by construction."""
    if n not in _INPUTS:
        rng = np.random.default_rng(1600 + n)
        bits = rng.integers(0, 1 << 16, size=n, dtype=np.uint16)
        k = min(n, len(SPECIAL))
        bits[:k] = np.asarray(SPECIAL[:k], dtype=np.uint16)
        rng.shuffle(bits)
        _INPUTS[n] = bits
    return _INPUTS[n]


def _want(name, bits, key_type, descending):
    """(sorted keys, stable order) of `bits`, computed once per (input, map, direction): float16 and bfloat16 share their map."""
    kind = "float" if key_type in ("float16", "bfloat16") else key_type
    key = (name, kind, descending)
    if key not in _WANT:
        t = _mapped(bits, key_type, descending)
        order = np.argsort(t, kind="stable")
        keys = _unmapped(np.sort(t), key_type, descending)
        assert np.array_equal(keys, bits[order])        # the two statements of the expected result agree
        _WANT[key] = (keys, order.astype(np.int32))
    return _WANT[key]


def _dev(bits, key_type):
    import torch

    return torch.from_numpy(np.ascontiguousarray(bits, dtype=np.uint16).view(np.int16).copy()).cuda().view(_dtype(key_type))


@contextlib.contextmanager
def _route(lsd, route):
    lsd.set_keys16_route(route)
    try:
        yield
    finally:
        lsd.set_keys16_route(-1)


def _check_all_modes(gpu, name, bits, key_type, descending):
    import torch

    n = bits.size
    keys, order = _want(name, bits, key_type, descending)
    for route in (COUNT, WIDEN):
        with _route(gpu, route):
            d = _dev(bits, key_type)
            gpu.GPUSort16(d, key_type=key_type, descending=descending, check_fault=True)
            assert np.array_equal(bits_of(d), keys), (name, "count" if route == COUNT else "widen")
    d, v = _dev(bits, key_type), torch.arange(n, dtype=torch.int32, device="cuda")
    gpu.GPUSort16(d, key_type=key_type, descending=descending, d_vals=v, check_fault=True)
    assert np.array_equal(v.cpu().numpy(), order), (name, "pairs")
    assert np.array_equal(bits_of(d), keys), (name, "pairs")


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("key_type", KEY_TYPES)
def test_both_routes_and_pairs(gpu, key_type, descending, n):
    _check_all_modes(gpu, ("random", n), _inputs(n), key_type, descending)


def _counter_patterns():
    rng = np.random.default_rng(77)
    n = (1 << 17) + 3
    return {
        "all_equal": np.full(n, 0xBF80, dtype=np.uint16),                                 # one counter past 65535; one value per wave
        "two_values": rng.permutation(np.repeat(np.array([0x0000, 0xFFFF], dtype=np.uint16), 1 << 16)),
        "every_value_once": rng.permutation(np.arange(1 << 16, dtype=np.uint16)),
        "low_half": rng.integers(0, 1 << 15, size=n, dtype=np.uint16),                     # one half of the sortable range of
        "high_half": rng.integers(1 << 15, 1 << 16, size=n, dtype=np.uint16),              # every key type, either order
        "long_runs": np.repeat(rng.integers(0, 1 << 16, size=40, dtype=np.uint16), 3277),  # whole waves of one value, then a change
    }


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("key_type", KEY_TYPES)
@pytest.mark.parametrize("name", sorted(_counter_patterns()))
def test_counter_width_and_value_ranges(gpu, name, key_type, descending):
    _check_all_modes(gpu, name, _counter_patterns()[name], key_type, descending)


@pytest.mark.parametrize("mode", ["count", "widen", "pairs"])
@pytest.mark.parametrize("phase", range(0, 16, 2))
def test_every_alignment_stays_inside(gpu, phase, mode):
    """The keys at every 2-byte phase of a 16-byte line; guard zones around the keys, the payloads and a workspace of exactly the
    reported size must be intact, and with them every key outside [0, n)."""
    from lsdradixsort_amd import errors

    L = gpu.lib()
    n = 4099
    key_type = KEY_TYPES[(phase // 2) % 4]
    descending = bool((phase // 8) & 1)
    code = errors.KEY_TYPES_16[key_type]
    bits = _inputs(n)
    keys, order = _want(("random", n), bits, key_type, descending)
    pairs = mode == "pairs"
    whole, view = guarded16(bits, phase, _dtype(key_type))
    assert view.data_ptr() % 16 == phase
    vwhole, vview = guarded(np.arange(n, dtype=np.uint32)) if pairs else (None, None)
    need = int(L.lsdsort_keys16_workspace_bytes(n, int(pairs)))
    wwhole, ws = guarded_workspace(need)
    with _route(gpu, {"count": COUNT, "widen": WIDEN, "pairs": -1}[mode]):
        st = L.lsdsort_keys16_device(view.data_ptr(), vview.data_ptr() if pairs else None, ws.data_ptr(), need, n, code,
                                     int(descending), None)
    assert st == errors.LSDSORT_OK
    assert L.lsdsort_keys16_check_device(ws.data_ptr(), n, int(pairs), None) == errors.LSDSORT_OK
    assert np.array_equal(bits_of(view), keys)
    if pairs:
        assert np.array_equal(vview.cpu().numpy(), order)
    assert_intact16(keys=whole)
    assert_intact(payloads=vwhole, workspace=wwhole)


@pytest.mark.parametrize("descending", [False, True])
def test_pairs_are_stable(gpu, descending):
    import torch

    n = 1 << 18
    rng = np.random.default_rng(5)
    values = np.array([0x0000, 0x8000, 0x3F80, 0xBF80, 0x7FC0, 0xFFC0, 0x0001, 0x7F80], dtype=np.uint16)
    bits = rng.choice(values, size=n)
    for key_type in KEY_TYPES:
        order = np.argsort(_mapped(bits, key_type, descending), kind="stable").astype(np.int32)
        d, v = _dev(bits, key_type), torch.arange(n, dtype=torch.int32, device="cuda")
        gpu.GPUSort16(d, key_type=key_type, descending=descending, d_vals=v, check_fault=True)
        assert np.array_equal(v.cpu().numpy(), order), key_type
        assert np.array_equal(bits_of(d), bits[order]), key_type


@pytest.mark.parametrize("n", [AUTO_THRESHOLD - 1, AUTO_THRESHOLD])
def test_automatic_route_on_either_side_of_the_threshold(gpu, n):
    gpu.set_keys16_route(-1)
    bits = _inputs(n)
    for key_type, descending in (("bfloat16", False), ("int16", True)):
        keys = _unmapped(np.sort(_mapped(bits, key_type, descending)), key_type, descending)   # keys only: no argsort needed
        d = _dev(bits, key_type)
        gpu.GPUSort16(d, key_type=key_type, descending=descending, check_fault=True)
        assert np.array_equal(bits_of(d), keys)


@pytest.mark.parametrize("pairs", [False, True])
def test_graph_capture_and_replay(gpu, pairs):
    """lsdsort_keys16_device allocates nothing and never synchronises: captured once, replayed on fresh keys in the same buffers."""
    import torch
    from lsdradixsort_amd import errors

    n = (1 << 20) + 13
    L = gpu.lib()
    rng = np.random.default_rng(21)
    first, second = (rng.integers(0, 1 << 16, size=n, dtype=np.uint16) for _ in range(2))
    need = int(L.lsdsort_keys16_workspace_bytes(n, int(pairs)))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")          # before the capture
    static = _dev(first, "bfloat16")
    iota = torch.arange(n, dtype=torch.int32, device="cuda")
    vals = iota.clone() if pairs else None
    assert L.lsdsort_prepare_device() == errors.LSDSORT_OK

    def call():
        return L.lsdsort_keys16_device(static.data_ptr(), vals.data_ptr() if pairs else None, ws.data_ptr(), ws.numel(), n,
                                       errors.KEY_TYPES_16["bfloat16"], 1, int(torch.cuda.current_stream().cuda_stream))

    with _route(gpu, -1 if pairs else COUNT):
        assert call() == errors.LSDSORT_OK      # warm-up outside the capture: the kernels' code objects are loaded
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            st = call()
    assert st == errors.LSDSORT_OK
    for bits in (first, second):
        static.copy_(_dev(bits, "bfloat16"))
        if pairs:
            vals.copy_(iota)
        graph.replay()
        torch.cuda.synchronize()
        assert L.lsdsort_keys16_check_device(ws.data_ptr(), n, int(pairs), None) == errors.LSDSORT_OK
        order = np.argsort(_mapped(bits, "bfloat16", True), kind="stable")
        assert np.array_equal(bits_of(static), bits[order])
        if pairs:
            assert np.array_equal(vals.cpu().numpy(), order.astype(np.int32))


@pytest.mark.parametrize("descending", [False, True])
def test_sort16_int16_matches_torch(gpu, descending):
    import torch

    for n in (0, 1, 4097, (1 << 20) + 5):
        g = torch.Generator(device="cuda").manual_seed(n + 1)
        for x in (torch.randint(-(1 << 15), 1 << 15, (n,), dtype=torch.int16, device="cuda", generator=g),
                  torch.randint(-3, 3, (n,), dtype=torch.int16, device="cuda", generator=g)):        # ties: stability shows
            keep = x.clone()
            values, indices = gpu.sort16(x, descending=descending, return_indices=True)
            want = torch.sort(x, stable=True, descending=descending)
            assert indices.dtype == torch.int64 and torch.equal(values, want.values) and torch.equal(indices, want.indices)
            assert torch.equal(gpu.sort16(x, descending=descending), want.values)                   # the count route from its size on
            assert torch.equal(x, keep)
    strided = torch.randint(-9, 9, (8194,), dtype=torch.int16, device="cuda")[::2]       # not contiguous: copied once, sorted
    keep = strided.clone()
    want = torch.sort(strided, stable=True, descending=descending)
    values, indices = gpu.sort16(strided, descending=descending, return_indices=True)
    assert values.is_contiguous() and torch.equal(values, want.values) and torch.equal(indices, want.indices)
    assert torch.equal(strided, keep)


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("key_type", ["float16", "bfloat16"])
def test_sort16_floats_match_torch_without_nan_and_negative_zero(gpu, key_type, descending):
    import torch

    g = torch.Generator(device="cuda").manual_seed(3)
    for n in (16385, (1 << 18) + 7):
        x = (torch.randn(n, dtype=torch.float32, device="cuda", generator=g) * 8).to(_dtype(key_type))   # ties by rounding
        x[x == 0] = 0.0                     # no -0.0
        x[5], x[6] = float("inf"), float("-inf")
        assert not torch.isnan(x).any() and not ((x == 0) & torch.signbit(x)).any()
        values, indices = gpu.sort16(x, descending=descending, return_indices=True)
        want = torch.sort(x, stable=True, descending=descending)
        assert torch.equal(values, want.values) and torch.equal(indices, want.indices)
        assert torch.equal(gpu.sort16(x, descending=descending), want.values)


def test_total_order_of_the_special_values(gpu):
    """-NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN for either float type, on either route."""
    f16 = np.array([0x7E00, 0x7C00, 0x3C00, 0x0001, 0x0000, 0x8000, 0x8001, 0xBC00, 0xFC00, 0xFE00, 0x7C01, 0xFFFF], dtype=np.uint16)
    want16 = np.array([0xFFFF, 0xFE00, 0xFC00, 0xBC00, 0x8001, 0x8000, 0x0000, 0x0001, 0x3C00, 0x7C00, 0x7C01, 0x7E00], dtype=np.uint16)
    bf = np.array([0x7FC0, 0x7F80, 0x3F80, 0x0001, 0x0000, 0x8000, 0x8001, 0xBF80, 0xFF80, 0xFFC0, 0x7F81, 0xFFFF], dtype=np.uint16)
    wantbf = np.array([0xFFFF, 0xFFC0, 0xFF80, 0xBF80, 0x8001, 0x8000, 0x0000, 0x0001, 0x3F80, 0x7F80, 0x7F81, 0x7FC0], dtype=np.uint16)
    for key_type, bits, want in (("float16", f16, want16), ("bfloat16", bf, wantbf)):
        for route in (COUNT, WIDEN):
            with _route(gpu, route):
                d = _dev(bits, key_type)
                gpu.GPUSort16(d, key_type=key_type, check_fault=True)
                assert np.array_equal(bits_of(d), want), (key_type, route)
                d = _dev(bits, key_type)
                gpu.GPUSort16(d, key_type=key_type, descending=True, check_fault=True)
                assert np.array_equal(bits_of(d), want[::-1]), (key_type, route)


def test_check_entry_is_clean_after_each_route(gpu):
    import torch
    from lsdradixsort_amd import errors

    L = gpu.lib()
    n = 70001
    bits = _inputs(65537)[:1].repeat(n)
    bits[::3] = 0x1234
    for route, pairs in ((COUNT, False), (WIDEN, False), (-1, True)):
        need = gpu.keys16_workspace_bytes(n, pairs)
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        d = _dev(bits, "uint16")
        v = torch.arange(n, dtype=torch.int32, device="cuda") if pairs else None
        with _route(gpu, route):
            gpu.GPUSort16(d, key_type="uint16", d_vals=v, workspace=ws)
        assert L.lsdsort_keys16_check_device(ws.data_ptr(), n, int(pairs), None) == errors.LSDSORT_OK
        assert np.array_equal(bits_of(d), np.sort(bits))
    assert L.lsdsort_keys16_check_device(ws.data_ptr(), 0, 0, None) == errors.LSDSORT_OK


def test_non_default_stream(gpu):
    import torch

    n = 65537
    bits = _inputs(n)
    keys, order = _want(("random", n), bits, "float16", True)
    s = torch.cuda.Stream()
    d, p = _dev(bits, "float16"), _dev(bits, "float16")
    v = torch.arange(n, dtype=torch.int32, device="cuda")
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), _route(gpu, COUNT):
        gpu.GPUSort16(d, key_type="float16", descending=True, stream=s, check_fault=True)
        gpu.GPUSort16(p, key_type="float16", descending=True, d_vals=v, stream=s, check_fault=True)
    s.synchronize()
    assert np.array_equal(bits_of(d), keys) and np.array_equal(bits_of(p), keys) and np.array_equal(v.cpu().numpy(), order)
