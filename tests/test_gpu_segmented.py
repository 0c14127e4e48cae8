"""GPU suite: lsdsort_segmented_device (GPUSortSegmented, sort_rows), bit-exact against a stable reference.

Reference: the stable segmented order is np.lexsort((sortable key, segment id)) -- or, for the large shapes, torch's stable sort
of (segment id << 32 | sortable key) on the device, the same order.  Sortable keys: uint32 as is, int32 with the sign bit
flipped, float32 IEEE total order u ^ ((u >> 31) * 0x7FFFFFFF | 0x80000000); descending = ascending on the complement."""
import numpy as np
import pytest
import torch

import lsdradixsort_amd as lsd
from _device_arrays import assert_equal
from _key_oracle import sortable_np
from _seg_plan import expected_dev   # the large shapes' reference: shared with test_gpu_segmented_plan.py

pytestmark = pytest.mark.gpu

WAVE_CAP = 1024


def expected(keys, offsets, vals=None, key_type="uint32", descending=False):
    """keys (uint32 bits), offsets -> expected keys (and vals) after the segmented sort; outside [off[0], off[-1]) unchanged"""
    keys = keys.astype(np.uint32)
    out_k = keys.copy()
    out_v = None if vals is None else vals.copy()
    lo, hi = int(offsets[0]), int(offsets[-1])
    sizes = np.diff(offsets.astype(np.int64))
    seg = np.repeat(np.arange(len(sizes)), sizes)
    order = np.lexsort((sortable_np(keys[lo:hi], key_type, descending), seg)) + lo
    out_k[lo:hi] = keys[order]
    if vals is not None:
        out_v[lo:hi] = vals[order]
    return out_k, out_v


def run(keys, offsets, vals=None, key_type="uint32", descending=False, check=True):
    dk = torch.from_numpy(keys.astype(np.uint32).view(np.float32 if key_type == "float32" else np.int32)).cuda()
    do = torch.from_numpy(offsets.astype(np.uint32).view(np.int32)).cuda()
    dv = None if vals is None else torch.from_numpy(vals.astype(np.uint32).view(np.int32)).cuda()
    lsd.GPUSortSegmented(dk, do, d_vals=dv, key_type=key_type, descending=descending, check_fault=check)
    torch.cuda.synchronize()
    gk = dk.cpu().numpy().view(np.uint32)
    gv = None if dv is None else dv.cpu().numpy().view(np.uint32)
    return gk, gv


def boundary_offsets(head=0, tail=0, big=True):
    sizes = [0, 1, 2, 63, 64, 65, WAVE_CAP - 1, WAVE_CAP, WAVE_CAP + 1, 5119, 5120, 5121, 10239, 10240, 10241, 16383, 16384,
             16385, 32767, 32768, 32769]
    if big:
        sizes.append(10 ** 6 + 7)
    with_empties = []
    for s in sizes:
        with_empties += [s, 0]   # an empty segment after every one
    off = np.concatenate([[0], np.cumsum(with_empties)]) + head
    return off.astype(np.int64), int(off[-1]) + tail


def random_keys(n, seed):
    return np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


@pytest.mark.parametrize("pairs", [False, True])
def test_every_class_boundary_with_head_and_tail(pairs):
    off, n = boundary_offsets(head=77, tail=131)
    keys = random_keys(n, 1)
    vals = np.arange(n, dtype=np.uint32) if pairs else None
    gk, gv = run(keys, off, vals)
    ek, ev = expected(keys, off, vals)
    assert_equal(gk, ek, "keys")
    if pairs:
        assert_equal(gv, ev, "vals")
    assert_equal(gk[:77], keys[:77], "untouched head")
    assert_equal(gk[n - 131:], keys[n - 131:], "untouched tail")


@pytest.mark.parametrize("key_type", ["int32", "float32"])
@pytest.mark.parametrize("descending", [False, True])
def test_typed_keys_with_specials(key_type, descending):
    off, n = boundary_offsets(head=5, tail=3, big=False)
    rng = np.random.default_rng(2)
    if key_type == "float32":
        specials = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF,
                             0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x7FFFFFFF, 0x3F800000, 0xBF800000], dtype=np.uint32)
        keys = rng.standard_normal(n).astype(np.float32).view(np.uint32).copy()
        pick = rng.random(n) < 0.3
        keys[pick] = specials[rng.integers(0, specials.size, int(pick.sum()))]
    else:
        keys = random_keys(n, 3)
        keys[rng.random(n) < 0.2] = np.uint32(0x80000000)
        keys[rng.random(n) < 0.2] = np.uint32(0x7FFFFFFF)
    vals = np.arange(n, dtype=np.uint32)
    gk, gv = run(keys, off, vals, key_type=key_type, descending=descending)
    ek, ev = expected(keys, off, vals, key_type=key_type, descending=descending)
    assert_equal(gk, ek, "keys")
    assert_equal(gv, ev, "vals")


def test_heavy_values_and_constant_digits():
    rng = np.random.default_rng(4)
    sizes = [3, 100, 900, 1024, 3000, 9000, 16384, 20000, 70000]
    parts, kinds = [], []
    for s in sizes:
        for kind in range(4):
            if kind == 0:
                k = np.where(rng.random(s) < 0.5, 0, rng.integers(0, 1 << 32, s, dtype=np.uint64)).astype(np.uint32)
            elif kind == 1:
                k = np.full(s, rng.integers(0, 1 << 32, dtype=np.uint64), dtype=np.uint32)   # one value per segment
            elif kind == 2:
                k = rng.integers(0, 256, s).astype(np.uint32)                                # three constant bytes
            else:
                k = (rng.integers(0, 4, s).astype(np.uint32) << np.uint32(16)) | np.uint32(0xAB00CD)   # one live byte in the middle
            parts.append(k)
            kinds.append(s)
    keys = np.concatenate(parts)
    off = np.concatenate([[0], np.cumsum(kinds)])
    vals = np.arange(keys.size, dtype=np.uint32)
    gk, gv = run(keys, off, vals)
    ek, ev = expected(keys, off, vals)
    assert_equal(gk, ek, "keys")
    assert_equal(gv, ev, "vals (stable on duplicates)")


def test_pairs_stable_on_duplicates():
    off, n = boundary_offsets(big=False)
    keys = np.random.default_rng(5).integers(0, 7, n).astype(np.uint32)
    vals = np.arange(n, dtype=np.uint32)
    gk, gv = run(keys, off, vals)
    ek, ev = expected(keys, off, vals)
    assert_equal(gk, ek, "keys")
    assert_equal(gv, ev, "vals")


def test_lognormal_million_segments():
    rng = np.random.default_rng(6)
    sizes = np.maximum(0, rng.lognormal(np.log(100) - 0.5, 1.0, 10 ** 6)).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(sizes)])
    n = int(off[-1])
    dk = torch.randint(-(1 << 31), 1 << 31, (n,), dtype=torch.int32, device="cuda")
    dv = torch.arange(n, dtype=torch.int32, device="cuda")
    want, idx = expected_dev(dk, off)
    lsd.GPUSortSegmented(dk, torch.from_numpy(off.astype(np.int32)).cuda(), d_vals=dv, check_fault=True)
    assert torch.equal(dk, want)
    assert torch.equal(dv.to(torch.int64), idx)


def test_rows_2e14_by_2e14_workgroup_tier():
    rows = cols = 1 << 14
    dk = torch.randint(-(1 << 31), 1 << 31, (rows * cols,), dtype=torch.int32, device="cuda")
    want = torch.sort(dk.view(rows, cols).to(torch.int64) & 0xFFFFFFFF, dim=-1).values.to(torch.int32).view(-1)
    off = torch.arange(0, rows + 1, dtype=torch.int64, device="cuda").mul_(cols).to(torch.int32)
    lsd.GPUSortSegmented(dk, off, check_fault=True)
    assert torch.equal(dk, want)


@pytest.mark.parametrize("rows,cols", [(64, 1 << 22), (1, 1 << 26)])
def test_large_tier(rows, cols):
    n = rows * cols
    dk = torch.randint(-(1 << 31), 1 << 31, (n,), dtype=torch.int32, device="cuda")
    off_np = np.arange(rows + 1, dtype=np.int64) * cols
    if rows == 1:
        want = dk.clone()
        lsd.GPULSDRadixSort(want, 8, check_fault=True)
    else:
        want = torch.sort(dk.view(rows, cols).to(torch.int64) & 0xFFFFFFFF, dim=-1).values.to(torch.int32).view(-1)
    lsd.GPUSortSegmented(dk, torch.from_numpy(off_np.astype(np.int32)).cuda(), check_fault=True)
    assert torch.equal(dk, want)


def test_sort_rows_matches_torch_sort():
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn(8, 131072, device="cuda", generator=g)
    x[:, ::97] = 0.5   # ties: the index order must match the stable sort
    got, gi = lsd.sort_rows(x, descending=True, return_indices=True)
    want, wi = torch.sort(x, dim=-1, descending=True, stable=True)
    assert torch.equal(got, want) and torch.equal(gi, wi)
    xi = torch.randint(-1000, 1000, (300, 5000), dtype=torch.int32, device="cuda", generator=g)
    got, gi = lsd.sort_rows(xi, return_indices=True)
    want, wi = torch.sort(xi, dim=-1, stable=True)
    assert torch.equal(got, want) and torch.equal(gi, wi)
    assert torch.equal(lsd.sort_rows(xi, descending=True), torch.sort(xi, dim=-1, descending=True, stable=True).values)


def test_mask_rank_form_gives_the_same_result():
    off, n = boundary_offsets(head=9, tail=4)
    keys = random_keys(n, 8)
    keys[::3] = 12345   # heavy value
    vals = np.arange(n, dtype=np.uint32)
    ek, ev = expected(keys, off, vals, key_type="float32", descending=True)
    lsd.set_rank_method(0)
    try:
        gk, gv = run(keys, off, vals, key_type="float32", descending=True)
    finally:
        lsd.set_rank_method(-1)
    assert_equal(gk, ek, "keys")
    assert_equal(gv, ev, "vals")


def test_graph_capture_replays_a_new_segmentation():
    n, segs = 200000, 40
    rng = np.random.default_rng(9)
    dk = torch.empty(n, dtype=torch.int32, device="cuda")
    do = torch.empty(segs + 1, dtype=torch.int32, device="cuda")
    ws = torch.empty(lsd.segmented_workspace_bytes(n, segs), dtype=torch.uint8, device="cuda")

    def fill(seed):
        r = np.random.default_rng(seed)
        cuts = np.sort(r.integers(0, n, segs - 1))
        off = np.concatenate([[0], cuts, [n]]).astype(np.int64)
        keys = random_keys(n, seed + 100)
        dk.copy_(torch.from_numpy(keys.view(np.int32)))
        do.copy_(torch.from_numpy(off.astype(np.int32)))
        return keys, off

    fill(1)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        lsd.GPUSortSegmented(dk, do, workspace=ws, stream=s)   # warm-up: device set-up stays out of the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        lsd.GPUSortSegmented(dk, do, workspace=ws)
    for seed in (2, 3):
        keys, off = fill(seed)
        # one giant segment and many tiny ones the second time round
        if seed == 3:
            off = np.concatenate([[0], np.arange(1, segs - 1) * 3, [n - 5, n]]).astype(np.int64)
            do.copy_(torch.from_numpy(off.astype(np.int32)))
        g.replay()
        torch.cuda.synchronize()
        fault = int(ws[:4].view(torch.int32).item())
        assert fault == 0, f"replay {seed}: fault word {fault:#x}"
        ek, _ = expected(keys, off)
        assert_equal(dk.cpu().numpy().view(np.uint32), ek, f"replay {seed}")
    assert lsd.lib().lsdsort_check_device(ws.data_ptr(), None) == 0


def test_non_default_stream():
    off, n = boundary_offsets(big=False)
    keys = random_keys(n, 10)
    vals = np.arange(n, dtype=np.uint32)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dk = torch.from_numpy(keys.view(np.int32)).cuda()
        dv = torch.from_numpy(vals.view(np.int32)).cuda()
        do = torch.from_numpy(off.astype(np.int32)).cuda()
    with torch.cuda.stream(s):
        ws = torch.empty(lsd.segmented_workspace_bytes(n, off.size - 1, True), dtype=torch.uint8, device="cuda")
    lsd.GPUSortSegmented(dk, do, d_vals=dv, workspace=ws, stream=s, check_fault=True)
    s.synchronize()
    ek, ev = expected(keys, off, vals)
    assert_equal(dk.cpu().numpy().view(np.uint32), ek, "keys")
    assert_equal(dv.cpu().numpy().view(np.uint32), ev, "vals")


def test_malformed_offsets_are_reported_and_contained():
    n, pad = 50000, 4096
    keys = random_keys(n, 11)
    sentinel = np.uint32(0xDEADBEEF)
    buf = torch.full((n + 2 * pad,), int(np.int32(sentinel.view(np.int32))), dtype=torch.int32, device="cuda")
    buf[pad:pad + n] = torch.from_numpy(keys.view(np.int32)).cuda()
    dk = buf[pad:pad + n]
    # [0,100) ok | [100, 2^31) ends beyond n | (2^31, 200) descending | [200, 20000) ok | [20000, 49000) ok | [49000, 50000) ok
    off = np.array([0, 100, 1 << 31, 200, 20000, 49000, n], dtype=np.int64)
    do = torch.from_numpy(off.astype(np.uint32).view(np.int32)).cuda()
    ws = torch.empty(lsd.segmented_workspace_bytes(n, off.size - 1), dtype=torch.uint8, device="cuda")
    status = lsd.lib().lsdsort_segmented_device(dk.data_ptr(), None, do.data_ptr(), off.size - 1, n, 0, 0, ws.data_ptr(), ws.numel(),
                                                torch.cuda.current_stream().cuda_stream)
    assert status == 0
    assert lsd.lib().lsdsort_check_device(ws.data_ptr(), torch.cuda.current_stream().cuda_stream) == lsd.errors.LSDSORT_ERR_DEVICE_FAULT
    got = buf.cpu().numpy().view(np.uint32)
    assert (got[:pad] == sentinel).all() and (got[pad + n:] == sentinel).all(), "memory around the array was written"
    got = got[pad:pad + n]
    assert_equal(got[100:200], keys[100:200], "the malformed segments' keys")
    for lo, hi in ((0, 100), (200, 20000), (20000, 49000), (49000, n)):
        assert_equal(got[lo:hi], np.sort(keys[lo:hi]), f"segment [{lo}, {hi})")
