"""GPU suite: the parts of the Python face that its wrappers share -- the temporary workspace on a side stream, the one body of
the three partition faces, the timed sort with payloads, the key-type names.  Small shapes: 20000 keys is the smallest size
past the 16384-key one-launch sort (the chained form and its workspace are really used), 10000 the one-launch form, 0 the
empty call."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 20000
CUTS = [1 << 30, 1 << 31, 3 << 30]


def _keys(n, seed, distinct=None):
    rng = np.random.default_rng(seed)
    return rng.integers(0, distinct or (1 << 32), size=n, dtype=np.uint64).astype(np.uint32)


def _busy(torch, nbytes):
    """Allocations and fills on the current stream, of the size class of a workspace of ``nbytes``."""
    return [torch.full((max(nbytes // 4, 64),), 0x5A5A5A5A, dtype=torch.int32, device="cuda") for _ in range(8)]


# the library answers an empty call with several payload arrays with "invalid argument" (their addresses are null): no case of it
@pytest.mark.parametrize("face,n", [("multi", N), ("multi", 10000), ("typed", N), ("typed", 10000), ("typed", 0)])
def test_temporary_workspace_on_a_side_stream(gpu, face, n):
    """No workspace given, explicit side stream: the temporary workspace belongs to that stream, so what the current stream
    allocates and fills around the call cannot be handed its block while the passes run, and the fault check reads that
    stream's workspace.  Bit for bit the result of the same call with a workspace of its own on the current stream."""
    import torch

    keys = _keys(n, 5, distinct=1000)                       # duplicates: the payloads show the stable order
    payloads = [np.arange(n, dtype=np.uint32), _keys(n, 6)]
    if face == "multi":
        nbytes = gpu.workspace_bytes(n, 8, 2)

        def call(**kw):
            d, p = gpu.to_device(keys), [gpu.to_device(v) for v in payloads]
            torch.cuda.synchronize()
            gpu.GPUSortMulti(d, p, 8, check_fault=True, **kw)
            return [d] + p
    else:
        nbytes = gpu.workspace_bytes(n, 8, True)

        def call(**kw):
            d, p = gpu.to_device(keys), gpu.to_device(payloads[0])
            torch.cuda.synchronize()
            gpu.GPUSortTyped(d, "int32", descending=True, d_vals=p, check_fault=True, **kw)
            return [d, p]

    expect = [gpu.to_host(t) for t in call(workspace=gpu.alloc_workspace(n, 8, 2 if face == "multi" else True))]
    torch.cuda.synchronize()
    number = keys.astype(np.int64)                          # below 1000: the same number as uint32 and as int32
    order = np.argsort(-number if face == "typed" else number, kind="stable")
    for e, source in zip(expect, [keys] + payloads):
        assert np.array_equal(e, source[order]), face
    side = torch.cuda.Stream()
    for rep in range(4):
        junk = _busy(torch, nbytes)                         # still filling when the side stream starts
        got = call(stream=side)
        junk += _busy(torch, nbytes)
        side.synchronize()
        torch.cuda.synchronize()
        for g, e in zip(got, expect):
            assert np.array_equal(gpu.to_host(g), e), (face, n, rep)
        del junk, got


def test_the_three_partition_faces_agree(gpu):
    import torch

    keys = _keys(N, 11)
    d = gpu.to_device(keys)
    results = [gpu.MSBPartition(d, 2), gpu.SplitterPartition(d, CUTS), gpu.ThresholdPartition(d, CUTS)]
    torch.cuda.synchronize()
    bucket = keys >> 30
    expect = np.concatenate([keys[bucket == b] for b in range(4)])       # each bucket: the keys of its range, in input order
    for out, counts in results:
        assert counts.dtype == torch.int64 and counts.shape == (4,)
        c = counts.cpu().numpy()
        assert int(c.sum()) == N
        assert np.array_equal(c, np.bincount(bucket, minlength=4))
        assert np.array_equal(gpu.to_host(out), expect)
    for out, counts in results[1:]:
        assert torch.equal(out, results[0][0]) and torch.equal(counts, results[0][1])
    assert np.array_equal(gpu.to_host(d), keys)                          # the input is only read


def test_the_partition_faces_on_nothing_and_on_a_bad_count(gpu):
    import torch

    empty = torch.empty(0, dtype=torch.int32, device="cuda")
    for out, counts in (gpu.MSBPartition(empty, 2), gpu.SplitterPartition(empty, CUTS), gpu.ThresholdPartition(empty, CUTS)):
        assert out.numel() == 0 and out.dtype == torch.int32
        assert counts.dtype == torch.int64 and counts.cpu().tolist() == [0, 0, 0, 0]
    d = gpu.to_device(_keys(N, 12))
    for face in (gpu.SplitterPartition, gpu.ThresholdPartition):
        with pytest.raises(ValueError):
            face(d, [1 << 30, 1 << 31])


def test_timed_sort_with_payloads(gpu):
    keys = _keys(N, 13, distinct=5000)
    vals = np.arange(N, dtype=np.uint32)
    k1, v1 = gpu.to_device(keys), gpu.to_device(vals)
    k2, v2 = gpu.to_device(keys), gpu.to_device(vals)
    t = gpu.GPULSDRadixSortTimed(k1, 8, d_vals=v1)
    assert set(t) == {"total_ms", "clear_ms", "histogram_ms", "scan_ms", "scatter_ms", "passes", "tile_keys", "tiles", "hybrid",
                      "local_ms"}
    assert t["passes"] == 4 and len(t["scatter_ms"]) == 4
    gpu.GPULSDRadixSort(k2, 8, d_vals=v2, check_fault=True)
    order = np.argsort(keys, kind="stable")
    assert np.array_equal(gpu.to_host(k2), keys[order]) and np.array_equal(gpu.to_host(v2), vals[order])
    assert np.array_equal(gpu.to_host(k1), gpu.to_host(k2)) and np.array_equal(gpu.to_host(v1), gpu.to_host(v2))
    with pytest.raises(ValueError):
        gpu.GPULSDRadixSortTimed(k1, 8, d_vals=v1[:-1].contiguous())
    with pytest.raises(TypeError):
        gpu.GPULSDRadixSortTimed(k1, 8, d_vals=v1.to("cpu"))


def test_an_unknown_key_type_is_a_value_error(gpu):
    import torch

    d = gpu.to_device(_keys(N, 14))
    offsets = torch.tensor([0, N // 2, N], dtype=torch.int32, device="cuda")
    wide = torch.from_numpy(np.random.default_rng(15).integers(-(1 << 63), 1 << 63, size=N, dtype=np.int64)).cuda()
    calls = {
        "GPUSortTyped": (d, lambda: gpu.GPUSortTyped(d, key_type="int16")),
        "GPUSortSegmented": (d, lambda: gpu.GPUSortSegmented(d, offsets, key_type="int16")),
        "GPUTopK": (d, lambda: gpu.GPUTopK(d, 8, key_type="int16")),
        "GPUSortWide": (wide, lambda: gpu.GPUSortWide(wide, key_type="int16")),
    }
    for name, (tensor, call) in calls.items():
        before = tensor.clone()
        with pytest.raises(ValueError):
            call()
        torch.cuda.synchronize()
        assert torch.equal(tensor, before), name
