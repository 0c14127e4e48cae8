"""GPU suite: launches that serve more than one role of a sort that tries the hybrid form -- the half variant's
planner in one launch (half_hop.hip), its one pass-B launch that stores halves or keys as the device decided, and the first global
pass launches, which run the hybrid form's passes or the ordinary form's first ones.

Every case is compared bit for bit with torch.sort, with fault word 0 and the form and the half word read back as predicted.  Each
input is sorted twice in one workspace and then as one captured graph replayed twice, so that tickets, region tables and status
rows are reused across launches and across sorts.  The inputs the planner refuses are the ones that can go wrong here: a shared
launch that reads the other role's shift, plan or table leaves an unsorted array or a fault bit.

Sizes: the smallest at which each path exists -- 158 056 448 keys (the first n of the half window) and 2^26 keys at 8-bit digits,
2^24 keys at 4-bit digits (four shared launches), 2^26 int32 keys and 2^26 pairs."""
import pytest

pytestmark = pytest.mark.gpu

N_HALF = 158_056_448
CASES = {   # name -> (n, radix_bits, key_type, pairs, the half variant is attempted)
    "half_window_r8": (N_HALF, 8, "uint32", False, True),
    "hybrid_r8": (1 << 26, 8, "uint32", False, False),
    "hybrid_r4": (1 << 24, 4, "uint32", False, False),
    "int32_r8": (1 << 26, 8, "int32", False, False),
    "pairs_r8": (1 << 26, 8, "uint32", True, False),
}
# input -> the hybrid form runs.  (With halves where it is attempted and no bucket is listed: uniform keys of the half window.)
INPUTS = {
    "uniform": 1,
    "bucket_of_12000": 1,          # one bucket above the local stage's launch over all buckets: the full-key pass B
    "half_zeros": 0,               # the sample refuses: the ordinary form in the shared launches
    "dead_first_byte": 0,          # ... whose first pass is skipped: the second shared launch reads the caller's buffer
    "dead_second_byte": 0,         # ... whose second pass (8-bit digits; third and fourth at 4) is skipped; an odd count at 8: copy back
    "below_2_24": 0,               # a constant top byte: no upfront read; the last pass (the last two at 4) skipped
}


def _u64(t):
    import torch

    return t.view(torch.int32).to(torch.int64) & 0xFFFFFFFF


def _i32(x):
    import torch

    return ((x + (1 << 31)) % (1 << 32) - (1 << 31)).to(torch.int32)


@pytest.fixture(scope="module")
def base(gpu):
    """Uniform keys of the largest size, made once; every case takes its first n and never changes them."""
    import torch

    gen = torch.Generator(device="cuda")
    gen.manual_seed(31)
    return torch.randint(-(1 << 31), (1 << 31) - 1, (N_HALF,), dtype=torch.int32, device="cuda", generator=gen)


def _keys(name, base, n):
    import torch

    k = _u64(base[:n])
    skewed = torch.where(((k >> 13) & 1) != 0, k, torch.zeros_like(k))   # half of the keys are zero
    if name == "uniform":
        return base[:n].clone()
    if name == "bucket_of_12000":
        shift = 17 if n >= N_HALF else 18                                # a bucket of the 2^15 or of the 2^14
        hot = 12000 - (n >> (32 - shift))
        return _i32(torch.cat([k[: n - hot], (k[:hot] & ((1 << shift) - 1)) | (5 << shift)]))
    if name == "half_zeros":
        return _i32(skewed)
    if name == "dead_first_byte":
        return _i32(skewed & 0xFFFFFF00)
    if name == "dead_second_byte":
        return _i32(skewed & 0xFFFF00FF)
    if name == "below_2_24":
        return _i32(k >> 8)
    raise AssertionError(name)


def _expected(keys, key_type):
    """(sorted keys, stable order) as torch sorts them: by the unsigned bit pattern, or as int32"""
    import torch

    s = torch.sort(keys if key_type == "int32" else _u64(keys), stable=True)
    return (s.values if key_type == "int32" else _i32(s.values)), s.indices.to(torch.int32)


@pytest.mark.parametrize("name", list(INPUTS))
@pytest.mark.parametrize("case", list(CASES))
def test_twice_eager_then_one_graph_twice(gpu, base, case, name):
    import torch

    n, radix, key_type, pairs, half_tried = CASES[case]
    keys = _keys(name, base, n)
    want_keys, want_order = _expected(keys, key_type)
    hybrid = INPUTS[name]
    half = 1 if (half_tried and name == "uniform") else 0
    ws = gpu.alloc_workspace(n, radix, pairs)
    d = torch.empty_like(keys)
    v = torch.empty(n, dtype=torch.int32, device="cuda") if pairs else None

    def sort():
        if key_type == "uint32":
            gpu.GPULSDRadixSort(d, radix, d_vals=v, workspace=ws)
        else:
            gpu.GPUSortTyped(d, key_type, False, d_vals=v, r=radix, workspace=ws)

    def run(launch, tell):
        d.copy_(keys)
        if pairs:
            v.copy_(torch.arange(n, dtype=torch.int32, device="cuda"))
        launch()
        torch.cuda.synchronize()
        assert gpu.lib().lsdsort_check_device(ws.data_ptr(), None) == 0, (case, name, tell, "fault word")
        got = (gpu.workspace_form(ws), gpu.workspace_half(ws))
        assert got == (hybrid, half), (case, name, tell, "(hybrid, half) read back", got)
        assert torch.equal(d, want_keys), (case, name, tell, "keys")
        if pairs:
            assert torch.equal(v, want_order), (case, name, tell, "payloads")

    run(sort, "eager 1")
    run(sort, "eager 2")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sort()
    run(graph.replay, "replay 1")
    run(graph.replay, "replay 2")


def test_one_graph_serves_every_role(gpu, base):
    """One captured sort of the half window, replayed on keys that take each role in turn: halves, full-key pass B, the ordinary
    form with every pass, with a skipped first pass, with an odd number of passes."""
    import torch

    n = N_HALF
    ws = gpu.alloc_workspace(n, 8)
    d = base[:n].clone()
    gpu.GPULSDRadixSort(d, 8, workspace=ws)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gpu.GPULSDRadixSort(d, 8, workspace=ws)
    for name in ("uniform", "half_zeros", "bucket_of_12000", "dead_first_byte", "uniform", "dead_second_byte", "below_2_24", "uniform"):
        keys = _keys(name, base, n)
        d.copy_(keys)
        graph.replay()
        torch.cuda.synchronize()
        assert gpu.lib().lsdsort_check_device(ws.data_ptr(), None) == 0, name
        assert (gpu.workspace_form(ws), gpu.workspace_half(ws)) == (INPUTS[name], 1 if name == "uniform" else 0), name
        assert torch.equal(d, _expected(keys, "uint32")[0]), name
