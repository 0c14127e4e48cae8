"""GPU suite: int64 / float64 keys and descending order on the 64-bit side (lsdsort_keys64_device, GPUSortWide(key_type=...),
sort64).  Everything is compared bit for bit.  Expected results come two independent ways: (1) numpy applies the order-preserving
map to the uint64 view, the mapped keys are sorted (std::sort of the oracle, or numpy's stable argsort) and the INPUT bits are
gathered; (2) where the type's native order is unambiguous, numpy / torch sort the typed view directly."""
import numpy as np
import pytest

from _key_oracle import ALL_TYPES64 as KEY_TYPES, KEY_TYPES64 as CODES

pytestmark = pytest.mark.gpu

TOP = np.uint64(1 << 63)
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
SIZES = [0, 1, 2, 255, 4097, 16385, (1 << 20) + 5]   # 16385: the first size past the one-launch small sort


def _dev(bits):
    import torch

    return torch.from_numpy(np.ascontiguousarray(bits, dtype=np.uint64).view(np.int64)).cuda()


def _bits(t):
    return t.cpu().numpy().view(np.uint64)


def _mapped(bits, key_type, descending):
    """The uint64 whose unsigned order is the requested order of the key (the map of include/lsdsort.h, restated in numpy)."""
    bits = np.ascontiguousarray(bits, dtype=np.uint64)
    if key_type == "int64":
        t = bits ^ TOP
    elif key_type == "float64":
        t = np.where(bits >> np.uint64(63) != 0, ~bits, bits ^ TOP)
    else:
        t = bits.copy()
    return ~t if descending else t


def _fill(special, n, rng, filler):
    """n keys: the special values first (cut to n), the rest from `filler`, shuffled."""
    out = filler(n)
    k = min(n, len(special))
    out[:k] = np.asarray(special[:k], dtype=np.uint64)
    rng.shuffle(out)
    return out


def _patterns(n):
    """name -> uint64 bit patterns of length n (sorted under every key type: the bits are what they are)."""
    rng = np.random.default_rng(1000 + n)
    u = lambda m: rng.integers(0, 1 << 64, size=m, dtype=np.uint64)
    i64_special = [1 << 63, (1 << 63) - 1, ONES, 0, 1,                                 # INT64_MIN, INT64_MAX, -1, 0, 1
                   0x000000057FFFFFFF, 0x0000000580000000, 0x0000000500000001, 0x00000005FFFFFFFE,   # equal high words, low words on
                   0xFFFFFFF07FFFFFFF, 0xFFFFFFF080000000, 0xFFFFFFF000000000, 0xFFFFFFF0FFFFFFFF]   # both sides of 2^31
    f64_special = [0, 1 << 63, 1, (1 << 63) | 1,                                       # +-0, +-denormal-min
                   0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF, 0x7FF0000000000000, 0xFFF0000000000000,   # +-DBL_MAX, +-inf
                   0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF,   # NaNs of both signs
                   0xC00921FB00000000, 0xC00921FB00000001, 0xC00921FB7FFFFFFF, 0xC00921FB80000000, 0xC00921FBFFFFFFFF,  # negative,
                   0x400921FB00000000, 0x400921FB80000000, 0x400921FBFFFFFFFF]                         # equal high words
    return {
        "uniform": u(n),
        "int64_edges": _fill(i64_special, n, rng, lambda m: u(m) >> rng.integers(0, 64, size=m, dtype=np.uint64)),
        "small_ids": rng.integers(0, 1 << 31, size=n, dtype=np.uint64),               # constant high word: skipped passes
        "float64_edges": _fill(f64_special, n, rng, lambda m: np.where(u(m) & np.uint64(1), u(m), rng.standard_normal(m).view(np.uint64))),
        "doubles": (np.round(rng.standard_normal(n) * 50.0) + 0.0).view(np.uint64),   # ties, no NaN, and -0.0 + 0.0 = +0.0
        "few_values": rng.choice(np.array([5, ONES, 1 << 63, 0x400921FB54442D18, 0xC00921FB54442D18], dtype=np.uint64), size=n),
    }


_CACHE = {}


def _inputs(n):
    if n not in _CACHE:
        _CACHE[n] = _patterns(n)
    return _CACHE[n]


_ORDERS = {}


def _order(n, name, key_type, descending):
    """numpy's stable argsort of the mapped keys: computed once, shared by the keys-only and the records tests."""
    key = (n, name, key_type, descending)
    if key not in _ORDERS:
        _ORDERS[key] = np.argsort(_mapped(_inputs(n)[name], key_type, descending), kind="stable").astype(np.int32)
    return _ORDERS[key]


def _check_native(bits, got, key_type, descending):
    """The second way: numpy's own sort of the typed view, where that order is unambiguous."""
    if key_type == "int64":
        want = np.sort(bits.view(np.int64))
        if descending:
            want = want[::-1]        # the values only: ties are equal bit patterns
        assert np.array_equal(got.view(np.int64), want)
    elif key_type == "float64":
        f = bits.view(np.float64)
        if np.isnan(f).any() or (bits == TOP).any():
            return                   # numpy puts every NaN last and does not order -0.0 against +0.0
        want = np.sort(f)
        if descending:
            want = want[::-1]
        assert np.array_equal(got, want.view(np.uint64))
    else:
        want = np.sort(bits)
        assert np.array_equal(got, want[::-1] if descending else want)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("key_type", KEY_TYPES)
def test_keys_only(gpu, oracle_mod, key_type, descending, n):
    for name, bits in _inputs(n).items():
        for r in ((8, 4) if n == 4097 else (8,)):
            d = _dev(bits)
            gpu.GPUSortWide(d, r=r, key_type=key_type, descending=descending, check_fault=True)
            got = _bits(d)
            t = _mapped(bits, key_type, descending)
            assert np.array_equal(_mapped(got, key_type, descending), oracle_mod.std_sort_u64(t)), (name, r)
            assert np.array_equal(got, bits[_order(n, name, key_type, descending)]), (name, r)
            _check_native(bits, got, key_type, descending)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("key_type", KEY_TYPES)
def test_records_payload_is_the_stable_argsort(gpu, key_type, descending, n):
    import torch

    for name, bits in _inputs(n).items():
        order = _order(n, name, key_type, descending)
        for vdtype in (torch.int32, torch.int64):
            for r in ((8, 4) if n == 4097 else (8,)):
                dk, dv = _dev(bits), torch.arange(n, dtype=vdtype, device="cuda")
                gpu.GPUSortWide(dk, dv, r=r, key_type=key_type, descending=descending, check_fault=True)
                assert np.array_equal(dv.cpu().numpy().astype(np.int64), order), (name, vdtype, r)
                assert np.array_equal(_bits(dk), bits[order]), (name, vdtype, r)


def test_tie_free_descending_is_the_reverse_of_ascending(gpu):
    rng = np.random.default_rng(7)
    n = 16385
    bits = rng.permutation(np.unique(rng.integers(0, 1 << 64, size=2 * n, dtype=np.uint64)))[:n].copy()
    for key_type in KEY_TYPES:
        up, down = _dev(bits), _dev(bits)
        gpu.GPUSortWide(up, key_type=key_type, check_fault=True)
        gpu.GPUSortWide(down, key_type=key_type, descending=True, check_fault=True)
        assert np.array_equal(_bits(down), _bits(up)[::-1]), key_type


def test_float64_tensor_and_total_order(gpu):
    """A float64 tensor goes in as it is; the special values come out in IEEE total order, NaNs by sign at the two ends."""
    import torch

    bits = np.array([0x7FF8000000000000, 0x7FF0000000000000, 0x3FF0000000000000, 1, 0, 1 << 63, (1 << 63) | 1, 0xBFF0000000000000,
                     0xFFF0000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)
    want = np.array([0xFFFFFFFFFFFFFFFF, 0xFFF8000000000000, 0xFFF0000000000000, 0xBFF0000000000000, (1 << 63) | 1, 1 << 63, 0, 1,
                     0x3FF0000000000000, 0x7FF0000000000000, 0x7FF0000000000001, 0x7FF8000000000000], dtype=np.uint64)
    x = torch.from_numpy(bits.view(np.float64).copy()).cuda()
    gpu.GPUSortWide(x, key_type="float64", check_fault=True)
    assert np.array_equal(x.cpu().numpy().view(np.uint64), want)
    x = torch.from_numpy(bits.view(np.float64).copy()).cuda()
    gpu.GPUSortWide(x, key_type="float64", descending=True, check_fault=True)
    assert np.array_equal(x.cpu().numpy().view(np.uint64), want[::-1])


def test_keys_not_16_byte_aligned(gpu, oracle_mod):
    """The ABI asks for 8-byte alignment: a key array that starts 8 bytes into a 16-byte line takes the one-by-one path."""
    n = 4097
    bits = np.random.default_rng(5).integers(0, 1 << 64, size=n + 1, dtype=np.uint64)
    for key_type, descending in (("int64", False), ("float64", True)):
        whole = _dev(bits)
        d = whole[1:]
        assert d.data_ptr() % 16 == 8 and d.is_contiguous()
        gpu.GPUSortWide(d, key_type=key_type, descending=descending, check_fault=True)
        t = _mapped(bits[1:], key_type, descending)
        assert np.array_equal(_bits(d), bits[1:][np.argsort(t, kind="stable")])
        assert _bits(whole)[0] == bits[0]


def test_default_arguments_still_sort_as_uint64(gpu, oracle_mod):
    """Behaviour unchanged: an int64 tensor with negative values, default arguments -> the negatives AFTER the positives."""
    import torch

    rng = np.random.default_rng(11)
    x = torch.from_numpy(rng.integers(-(1 << 63), 1 << 63, size=4097, dtype=np.int64)).cuda()
    bits = _bits(x).copy()
    gpu.GPUSortWide(x, check_fault=True)
    assert np.array_equal(_bits(x), oracle_mod.std_sort_u64(bits))
    got = x.cpu().numpy()
    assert (got[:-1] >= 0).any() and got[-1] < 0 and got[0] >= 0
    k32 = gpu.to_device(np.arange(8, dtype=np.uint32))
    v64 = torch.arange(8, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError):
        gpu.GPUSortWide(k32, v64, descending=True)
    with pytest.raises(ValueError):
        gpu.GPUSortWide(k32, v64, key_type="int64")
    with pytest.raises(TypeError):
        gpu.GPUSortWide(torch.zeros(8, dtype=torch.float64, device="cuda"))
    with pytest.raises(TypeError):
        gpu.GPUSortWide(torch.zeros(8, dtype=torch.float64, device="cuda"), key_type="int64")


@pytest.mark.parametrize("descending", [False, True])
def test_sort64_int64_matches_torch(gpu, descending):
    import torch

    for n in (0, 1, 4097, (1 << 20) + 5):
        g = torch.Generator(device="cuda").manual_seed(n + 1)
        for x in (torch.randint(-(1 << 63), (1 << 63) - 1, (n,), dtype=torch.int64, device="cuda", generator=g),
                  torch.randint(-3, 3, (n,), dtype=torch.int64, device="cuda", generator=g)):        # ties: stability shows
            keep = x.clone()
            values, indices = gpu.sort64(x, descending=descending, return_indices=True)
            want = torch.sort(x, stable=True, descending=descending)
            assert indices.dtype == torch.int64 and torch.equal(values, want.values) and torch.equal(indices, want.indices)
            assert torch.equal(gpu.sort64(x, descending=descending), want.values)
            assert torch.equal(x, keep)
    strided = torch.randint(-9, 9, (8194,), dtype=torch.int64, device="cuda")[::2]       # not contiguous: copied once, sorted
    want = torch.sort(strided, stable=True, descending=descending)
    values, indices = gpu.sort64(strided, descending=descending, return_indices=True)
    assert values.is_contiguous() and torch.equal(values, want.values) and torch.equal(indices, want.indices)


@pytest.mark.parametrize("descending", [False, True])
def test_sort64_float64_matches_torch_without_nan_and_negative_zero(gpu, descending):
    import torch

    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(16385, dtype=torch.float64, device="cuda", generator=g)
    x[::7] = x[3]                       # ties
    x[5], x[6] = float("inf"), float("-inf")
    assert not torch.isnan(x).any() and not ((x == 0) & torch.signbit(x)).any()
    values, indices = gpu.sort64(x, descending=descending, return_indices=True)
    want = torch.sort(x, stable=True, descending=descending)
    assert torch.equal(values, want.values) and torch.equal(indices, want.indices)


def test_non_default_stream(gpu):
    import torch

    n = 16385
    bits = _inputs(n)["uniform"]
    s = torch.cuda.Stream()
    d = _dev(bits)
    v = torch.arange(n, dtype=torch.int32, device="cuda")
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        gpu.GPUSortWide(d, v, key_type="int64", descending=True, stream=s, check_fault=True)
    s.synchronize()
    order = np.argsort(_mapped(bits, "int64", True), kind="stable")
    assert np.array_equal(_bits(d), bits[order]) and np.array_equal(v.cpu().numpy(), order.astype(np.int32))


def test_graph_capture_and_replay(gpu):
    """lsdsort_keys64_device allocates nothing and never synchronises: captured once, replayed on fresh keys."""
    import torch
    from lsdradixsort_amd import errors

    n = 4097
    L = gpu.lib()
    rng = np.random.default_rng(21)
    first, second = (rng.standard_normal(n).view(np.uint64) for _ in range(2))
    need = int(L.lsdsort_wide_workspace_bytes(n, 8, 64, 0))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")          # before the capture
    static = _dev(first)
    assert L.lsdsort_prepare_device() == errors.LSDSORT_OK

    def call():
        return L.lsdsort_keys64_device(static.data_ptr(), None, 0, ws.data_ptr(), ws.numel(), n, 8, CODES["float64"], 1,
                                       int(torch.cuda.current_stream().cuda_stream))

    assert call() == errors.LSDSORT_OK      # warm-up outside the capture: the kernels' code objects are loaded
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st = call()
    assert st == errors.LSDSORT_OK
    for bits in (first, second):
        static.copy_(_dev(bits))
        graph.replay()
        torch.cuda.synchronize()
        assert L.lsdsort_wide_check_device(ws.data_ptr(), n, 8, 64, 0, None) == errors.LSDSORT_OK
        assert np.array_equal(_bits(static), bits[np.argsort(_mapped(bits, "float64", True), kind="stable")])
        assert np.array_equal(_bits(static).view(np.float64), np.sort(bits.view(np.float64))[::-1])


@pytest.mark.parametrize("n", [(1 << 26) + 3, (1 << 26) + (1 << 20) + 3])
def test_int64_keys_past_the_grid_cap(gpu, n):
    """More keys than one sweep of the split and merge kernels' grid (65536 workgroups x 256 threads, four keys per thread on the
    16-byte path, one on the key-by-key path), checked on the device against torch.sort, no host copy of the array.
    16-byte aligned keys: at 2^26 + 3 every thread takes exactly ONE group of four and threads 0..2 the three left-over keys -- the
    size sits on the cap; at 2^26 + 2^20 + 3 the first 2^18 threads come round a second time (g += stride of the 16-byte loop).
    The same keys from an address 8 bytes into a 16-byte line take the key-by-key loop, five times round at either size."""
    import torch

    g = torch.Generator(device="cuda").manual_seed(9)
    base = torch.randint(-(1 << 63), (1 << 63) - 1, (n + 1,), dtype=torch.int64, device="cuda", generator=g)
    base[-3:] = torch.tensor([-(1 << 63), -1, (1 << 63) - 1], dtype=torch.int64, device="cuda")   # in the left-over keys
    want = torch.sort(base[1:]).values
    x = base[1:].clone()
    assert x.data_ptr() % 16 == 0
    gpu.GPUSortWide(x, key_type="int64", check_fault=True)
    assert torch.equal(x, want)
    del x
    first = base[0].item()
    y = base[1:]
    assert y.data_ptr() % 16 == 8 and y.is_contiguous()
    gpu.GPUSortWide(y, key_type="int64", check_fault=True)
    assert torch.equal(y, want) and base[0].item() == first
