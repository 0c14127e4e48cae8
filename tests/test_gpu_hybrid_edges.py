"""The hybrid form and its half variant at the edges of every decision that chooses them (hybrid.hip, half_hop.hip, make_plan of
lsdsort_api.hip).

Both are chosen on the device by a chain of defences -- the sample (Hopeless), the prefix check of the upfront read (Violated),
the planner's largest <= 16384, its total == n, and its list of buckets above the small capacity (LargeCount) -- and each of them
leaves a word in the workspace's control block.  Every case here

  * compares the sort bit-exact with torch.sort of the keys as unsigned and asks lsdsort_check_device for 0,
  * compares the reported (workspace_form, workspace_half) with the pair listed with the case,
  * compares the control words -- and, where the half variant was attempted, the 2^15 folded counts and the lower groups' counts
    it keeps in the workspace -- with what _hybrid_words.expected_words predicts from the input's own bincount,
  * and, where ONE defence is meant to stand alone, asserts that the others' words show no objection, so that a case that stops
    reaching its regime fails instead of passing for another reason.

No tolerance anywhere.  The oracle's rules are pinned by test_hybrid_words_cpu.py.  Each case prints the words it read back
(`WORDS ...`, visible with -s).

Two expectations are what the sources say, not what one might guess:
  * lsdsort_u32_device_prefixed never runs the half variant (include/lsdsort.h; its workspace is the sharded step's), so the
    window-size sorts through it report (1, 0) however roomy the workspace;
  * a key at position 0 that differs from all others in bit 29 IS the reference key: every sample then differs in bit 29, the
    prefix found is the two bits all keys do share, nothing is violated, and the sort runs the form with Prefix == 2."""
import numpy as np
import pytest

import _hybrid_words as hw
from _guarded import GUARD, SENT32, assert_intact, assert_unchanged, guarded, guarded_workspace
from _guarded16 import assert_intact16, bits_of, guarded16

pytestmark = pytest.mark.gpu

N0, TOP = hw.WINDOW                 # 158 056 448 and 330 596 351: the half variant's window
STEP0 = N0 // 65536                 # the sample's stride at N0
MIN32 = -(1 << 31)
REPORT = ("Hopeless", "Violated", "Largest", "LargeCount", "Ok", "HalfOk")


# ---- common ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base(gpu):
    """Uniform keys of the largest window size + 1, made once; every case takes its first n and never changes them."""
    import torch

    gen = torch.Generator(device="cuda")
    gen.manual_seed(4092)
    return torch.randint(MIN32, (1 << 31) - 1, (TOP + 1,), dtype=torch.int32, device="cuda", generator=gen)


@pytest.fixture(scope="module")
def ws(gpu):
    """One workspace of the largest roomy size of the window: at least the roomy size of every n up to TOP + 1."""
    import torch

    L = gpu.lib()
    nbytes = max(int(L.lsdsort_workspace_bytes_roomy(n, 8)) for n in (N0, TOP, TOP + 1))
    return torch.empty(nbytes, dtype=torch.uint8, device="cuda")


def _roomy(gpu, n):
    return int(gpu.lib().lsdsort_workspace_bytes_roomy(n, 8))


def _sorted(keys):
    """torch.sort of the keys as unsigned: the signed sort of the keys with their top bit flipped, flipped back"""
    import torch

    return torch.sort(keys.view(torch.int32) ^ MIN32).values ^ MIN32


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _after(gpu, ws):
    """(form, half) and the control words of the sort just queued in ws; its fault word must be clear"""
    assert gpu.lib().lsdsort_check_device(ws.data_ptr(), _stream()) == 0
    return (gpu.workspace_form(ws), gpu.workspace_half(ws)), hw.read_words(ws)


def _compare(gpu, label, keys, ws, form, words, want, *, half, **rules):
    """the words (and the half variant's counts) against the oracle; returns the oracle's dict"""
    import torch

    exp = hw.expected_words(keys, half=half, **rules)
    print("WORDS", label, form, {k: words[k] for k in REPORT}, "Prefix", words["Prefix"], "HalfHigh", hex(words["HalfHigh"]),
          "| predicted total", exp["total"], "of n", keys.numel())
    if want is None:
        want = (exp["Ok"], exp["HalfOk"])
    assert form == want, (label, "form read back (hybrid, half)", form, want)
    for name in hw.COMPARED:
        assert words[name] == exp[name], (label, name, words[name], exp[name])
    assert words["SkipLocal"] == 1 - exp["Ok"]
    if half and exp["bucket"] is not None:
        bucket, first = hw.read_half_counts(ws, _roomy(gpu, keys.numel()))
        assert torch.equal(bucket, exp["bucket"]), (label, "the folded bucket counts")
        assert torch.equal(first, exp["first"]), (label, "the lower groups' counts")
    return exp


def _check(gpu, label, keys, ws, want, *, expect=None, half=None, **rules):
    """Sorts a copy of `keys` (plain uint32, 8-bit digits) in `ws` and checks everything common to every case.  half: whether the
    variant is attempted; None = by the rule (window size, workspace of the roomy size, switch on).  Returns (output, words,
    oracle)."""
    import torch

    n = keys.numel()
    if half is None:
        half = hw.in_half_window(n) and ws.numel() >= _roomy(gpu, n)
    d = keys.clone()
    gpu.GPULSDRadixSort(d, 8, workspace=ws)
    form, words = _after(gpu, ws)
    exp = _compare(gpu, label, keys, ws, form, words, want, half=half, **rules)
    assert torch.equal(d, _sorted(keys) if expect is None else expect), (label, "not the sorted keys")
    return d, words, exp


def _nobody_else_objects(words):
    assert words["Hopeless"] == 0 and words["Violated"] == 0, ("the premise: neither the sample nor the prefix check refused", words)


def _sum_alone(words, exp, n, lost):
    """the premise of a case that only total == n can have refused"""
    _nobody_else_objects(words)
    assert words["Largest"] <= hw.CAP_SMALL and words["LargeCount"] == 0, ("the premise: every bucket looks small", words)
    assert exp["total"] == n - lost and words["Ok"] == 0 and words["HalfOk"] == 0


def _also_with_32_bit_counts(gpu, label, keys, ws, want_form, expect, largest):
    """The same keys with the variant switched off, and in a workspace of the plain size: the counts are 32-bit there, Largest
    is the true count, and the output is the same."""
    import torch

    n = keys.numel()
    gpu.set_half_hop(False)
    try:
        _, words, exp = _check(gpu, label + " variant off", keys, ws, (want_form, 0), expect=expect, half=False)
    finally:
        gpu.set_half_hop(True)
    assert words["Largest"] == largest and exp["total"] == n
    plain = torch.empty(int(gpu.lib().lsdsort_workspace_bytes(n, 8, 0)), dtype=torch.uint8, device="cuda")
    assert plain.numel() < _roomy(gpu, n)
    _, words, exp = _check(gpu, label + " plain workspace", keys, plain, (want_form, 0), expect=expect)
    assert words["Largest"] == largest and exp["total"] == n


# ---- a. the sum check alone (half variant, N0) ---------------------------------------------------------------------------------
SUM_BUCKET = 12345                  # groups 24690 (low half of the packed word) and 24691 (high half)
SUM_CASES = [("low", 65535), ("low", 65536), ("low", 65537), ("low", 65536 + 7000), ("low", 131072 + 5), ("high", 65536),
             ("high", 65536 + 7000), ("low_run", 65536)]


def _sum_keys(base, side, target):
    import torch

    k = base[:N0]
    if side != "low_run":
        return hw.with_exact_count(k, 16, 2 * SUM_BUCKET + (side == "high"), target, avoid_step=STEP0)
    # ONE contiguous run: the group's own keys go to its sibling (the bucket, all the sample looks at, stays theirs), then 65536
    # keys of the group with random low halves from a position the sample's stride does not divide
    u = hw.u64(k)
    out = hw.i32(torch.where((u >> 16) == 2 * SUM_BUCKET, u | 0x10000, u))
    start = 77_000_003
    assert start % STEP0 != 0 and target == 65536
    gen = torch.Generator(device="cuda")
    gen.manual_seed(77)
    out[start:start + target] = hw.i32((2 * SUM_BUCKET << 16) | torch.randint(0, 1 << 16, (target,), device="cuda", generator=gen))
    return out


@pytest.mark.parametrize("side,target", SUM_CASES)
def test_sum_check_alone_refuses_a_group_of_65536(gpu, base, ws, side, target):
    """A group of the 2^16 with 65536 keys or more carries into its sibling or out of the packed word; the folded bucket looks
    SMALL (test_hybrid_words_cpu.py: the fold table), so Largest and the list see nothing and only total == n refuses.  65535 is the
    last count that fits: nothing is lost, and Largest alone refuses."""
    import torch

    keys = _sum_keys(base, side, target)
    groups = torch.bincount(hw.u64(keys) >> 16, minlength=1 << 16)
    low, high = int(groups[2 * SUM_BUCKET]), int(groups[2 * SUM_BUCKET + 1])
    assert (high if side == "high" else low) == target
    expect = _sorted(keys)
    label = f"a {side} {target}"
    _, words, exp = _check(gpu, label, keys, ws, (0, 0), expect=expect)
    folded, first, lost = hw.fold(low, high)
    assert int(exp["bucket"][SUM_BUCKET]) == folded and int(exp["first"][SUM_BUCKET]) == first
    if target == 65535:
        _nobody_else_objects(words)
        assert lost == 0 and exp["total"] == N0 and words["Largest"] == low + high > hw.LOCAL_SORT_CAP, "Largest alone, total intact"
    else:
        assert lost in (65535, 65536, 131070)
        _sum_alone(words, exp, N0, lost)
    _also_with_32_bit_counts(gpu, label, keys, ws, 0, expect, low + high)


# ---- b. the 16-bit LDS counters of the 2^16-bucket form ------------------------------------------------------------------------
def test_sum_check_alone_refuses_an_lds_counter_that_wraps(gpu, base, ws):
    """TOP + 1 keys are the first size sorted in 2^16 buckets, counted in 16-bit halves of LDS words per workgroup.  Workgroup 3 of
    the upfront read owns keys [(3 + 256 i) 16384, + 16384): its first four groups hold one even bucket, 65536 keys -- its half
    wraps into the neighbour's, the global counts are short by 65535, and every bucket looks small."""
    import torch

    n, block, bucket = TOP + 1, 3, 0x6000
    assert hw.hybrid_bucket_bits(n) == 16 and _roomy(gpu, n) == int(gpu.lib().lsdsort_workspace_bytes(n, 8, 0))
    ranges = hw.owned_ranges(block, n, 4)
    assert hw.sample_hits(ranges, n).max() <= 4 < hw.SAMPLE_HOPELESS_AT
    keys = base[:n].clone()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(16)
    for lo, hi in ranges:
        keys[lo:hi] = hw.i32((bucket << 16) | torch.randint(0, 1 << 16, (hi - lo,), device="cuda", generator=gen))
    assert keys.data_ptr() % 16 == 0, "the ownership of keys is that of a 16-byte-aligned base"
    true = int(((hw.u64(keys) >> 16) == bucket).sum())
    assert true >= 65536
    _, words, exp = _check(gpu, "b lds half wraps", keys, ws, (0, 0), lds16_block=block)
    assert int(exp["bucket"][bucket]) == true - 65536
    _sum_alone(words, exp, n, 65535)


# ---- c. capacity boundaries in whole sorts -------------------------------------------------------------------------------------
CAP_BUCKET = 20000                  # a bucket of the 2^15: key >> 17
CAP_CASES = [("10240_lower", 10240, (1, 1)), ("10240_upper", 10240, (1, 1)), ("10241", 10241, (1, 0)), ("16384", 16384, (1, 0)),
             ("16385", 16385, (0, 0))]


@pytest.mark.parametrize("name,size,want", CAP_CASES)
def test_capacity_boundaries_in_whole_sorts(gpu, base, ws, name, size, want):
    """One bucket of exactly 10240 / 10241 keys (the planner lists cnt > small_cap: no halves) and of 16384 / 16385 (largest >
    16384: no hybrid form), made at unsampled positions.  10240 in two layouts: all keys in the bucket's lower group (first ==
    size) and all in its upper one (first == 0)."""
    import torch

    k = base[:N0]
    if name.startswith("10240_"):
        u = hw.u64(k)
        inside = (u >> 17) == CAP_BUCKET
        upper = name.endswith("upper")
        k = hw.i32(torch.where(inside, (u | 0x10000) if upper else (u & ~0x10000), u))
        keys = hw.with_exact_count(k, 16, 2 * CAP_BUCKET + int(upper), size, avoid_step=STEP0)
    else:
        keys = hw.with_exact_count(k, 17, CAP_BUCKET, size, avoid_step=STEP0)
    assert int(((hw.u64(keys) >> 17) == CAP_BUCKET).sum()) == size
    expect = _sorted(keys)
    _, words, exp = _check(gpu, "c " + name, keys, ws, want, expect=expect)
    _nobody_else_objects(words)
    assert exp["total"] == N0 and words["Largest"] == size, "the bucket is the largest, and no count is lost"
    assert words["LargeCount"] == (1 if size > hw.CAP_SMALL else 0)
    assert int(exp["bucket"][CAP_BUCKET]) == size
    if name.startswith("10240_"):
        assert int(exp["first"][CAP_BUCKET]) == (0 if name.endswith("upper") else size)
    gpu.set_half_hop(False)
    try:
        _check(gpu, "c " + name + " variant off", keys, ws, (want[0], 0), expect=expect, half=False)
    finally:
        gpu.set_half_hop(True)


# ---- d. the window's edges and the benchmark's size ----------------------------------------------------------------------------
def test_top_of_the_window_balanced(gpu, ws):
    """TOP keys with every bucket at 10088 or 10089 of the 10240 capacity, at random positions (a patterned layout would put eight
    samples of a workgroup into one bucket): 20 rows, the last partial, the largest bases."""
    import torch

    gen = torch.Generator(device="cuda")
    gen.manual_seed(2)
    keys = hw.i32(((torch.randperm(TOP, device="cuda", generator=gen) % 32768) << 17)
                  | torch.randint(0, 1 << 17, (TOP,), device="cuda", generator=gen))
    _, words, exp = _check(gpu, "d top balanced", keys, ws, (1, 1))
    assert words["Largest"] == 10089 and int(exp["bucket"].min()) == 10088 and exp["total"] == TOP


def test_top_of_the_window_uniform(gpu, base, ws):
    _, words, exp = _check(gpu, "d top uniform", base[:TOP], ws, None)
    assert words["Ok"] == 1, "uniform keys take the hybrid form"
    assert (words["HalfOk"] == 0) == (words["LargeCount"] > 0)


def test_first_size_above_the_window(gpu, base, ws):
    n = TOP + 1
    L = gpu.lib()
    assert L.lsdsort_workspace_bytes_roomy(n, 8) == L.lsdsort_workspace_bytes(n, 8, 0), "the variant is not attempted"
    _, words, _ = _check(gpu, "d top + 1", base[:n], ws, (1, 0))
    assert words["HalfOk"] == 0 and words["HalfHigh"] == 0 and words["LowBits"] == 16


def test_the_benchmarks_size_runs_the_variant(gpu, base):
    n = 1 << 28
    ws28 = gpu.alloc_workspace(n, 8)          # what GPULSDRadixSort allocates when it is given none
    assert ws28.numel() == _roomy(gpu, n) > int(gpu.lib().lsdsort_workspace_bytes(n, 8, 0))
    _check(gpu, "d 2^28", base[:n], ws28, (1, 1))


@pytest.mark.parametrize("n,form", [(38_000_000, 1), (37_999_999, 0)])
def test_lower_end_of_the_hybrid_form(gpu, base, ws, n, form):
    import torch

    keys = base[:n]
    if form:
        _check(gpu, f"d {n}", keys, ws, (1, 0))
        return
    d = keys.clone()
    gpu.GPULSDRadixSort(d, 8, workspace=ws)
    got, words = _after(gpu, ws)
    assert got == (0, 0) and not any(words.values()), "below its range the form is not tried: no word is written"
    assert torch.equal(d, _sorted(keys))


@pytest.mark.parametrize("n,form", [(960_000_000, 1), (960_000_001, 0)])
def test_upper_end_of_the_hybrid_form(gpu, n, form):
    import torch

    gen = torch.Generator(device="cuda")
    gen.manual_seed(960)
    keys = torch.randint(MIN32, (1 << 31) - 1, (n,), dtype=torch.int32, device="cuda", generator=gen)
    big = gpu.alloc_workspace(n, 8)
    if form:
        _check(gpu, f"d {n}", keys, big, (1, 0))
        return
    d = keys.clone()
    gpu.GPULSDRadixSort(d, 8, workspace=big)
    got, words = _after(gpu, big)
    assert got == (0, 0) and not any(words.values())
    assert torch.equal(d, _sorted(keys))


# ---- e. the prefix check -------------------------------------------------------------------------------------------------------
NP = N0 + 12345


@pytest.fixture(scope="module")
def prefixed(base):
    """NP keys that share the three top bits 101"""
    return hw.i32((hw.u64(base[:NP]) >> 3) | (0b101 << 29))


def _unsampled(pos, length=1):
    step = NP // 65536
    return all(p % step != 0 for p in range(pos, pos + length))


MIDDLE = NP // 2 + 1


@pytest.mark.parametrize("where", ["tail", "middle", "run_of_64"])
def test_one_key_outside_the_prefix_in_its_lowest_bit(gpu, prefixed, ws, where):
    """One key that differs from the others ONLY in bit 29, the lowest bit of the prefix, where the sample does not look: in the
    upfront read's tail loop (the last key), in the middle of the array, and as 64 equal keys at the start of a workgroup's group
    -- sixteen lanes whose first keys are equal: the heavy-value path, which counts them by ballot."""
    keys = prefixed.clone()
    if where == "tail":
        pos, length = NP - 1, 1
        assert pos >= hw.full_group_keys(NP), "the last key goes through the tail loop"
    elif where == "middle":
        pos, length = MIDDLE, 1
    else:
        pos = next(g * hw.GROUP_KEYS for g in range(NP // (2 * hw.GROUP_KEYS), NP // hw.GROUP_KEYS) if _unsampled(g * hw.GROUP_KEYS, 64))
        length = 64
        assert pos + length <= hw.full_group_keys(NP)
    assert _unsampled(pos, length)
    keys[pos:pos + length] = keys[pos] ^ (1 << 29)
    _, words, exp = _check(gpu, "e bit 29 " + where, keys, ws, (0, 0))
    assert words["Violated"] == 1 and words["Hopeless"] == 0 and words["Prefix"] == 3
    assert words["Largest"] <= hw.CAP_SMALL and exp["total"] == NP, "the premise: the prefix check alone refused"


def test_the_first_key_differs_in_bit_29(gpu, prefixed, ws):
    """keys[0] is the reference of sample and check: with ITS bit 29 flipped every sample differs in bit 29 and the prefix found
    is the two bits that all keys do share -- nothing is violated, and the form is planned for t = 2 with bit 29 inside the
    buckets (half of them empty, the others twice the size: what the oracle's bincount says decides)."""
    keys = prefixed.clone()
    keys[0] = keys[0] ^ (1 << 29)
    _, words, exp = _check(gpu, "e bit 29 first", keys, ws, None)
    assert words["Prefix"] == 2 and words["Violated"] == 0 and words["Hopeless"] == 0
    assert words["HalfHigh"] == 0x80000000 and words["LowBits"] == 15
    assert int((exp["bucket"] == 0).sum()) == (1 << 14) - 1, "bit 29 is 1 in every key but the first: half the buckets hold nothing, one holds keys[0]"


def test_one_key_differs_just_below_the_prefix(gpu, prefixed, ws):
    """the control: bit 28 is not part of the prefix, and a key that differs there must not refuse anything"""
    keys = prefixed.clone()
    assert _unsampled(MIDDLE)
    keys[MIDDLE] = keys[MIDDLE] ^ (1 << 28)
    _, words, _ = _check(gpu, "e bit 28", keys, ws, (1, 1))
    assert words["Prefix"] == 3 and words["Violated"] == 0
    assert words["HalfHigh"] == int(hw.u64(keys[:1])[0]) & 0xE0000000 == 0xA0000000


# ---- f. what must not take the variant although the workspace would allow it ---------------------------------------------------
@pytest.mark.parametrize("key_type,descending", [("int32", False), ("float32", False), ("uint32", True)])
def test_typed_keys_stay_out_of_the_variant(gpu, base, ws, key_type, descending):
    """The gate !rq.xf.on of make_plan: HalfHigh = keys[0] & ... would be taken from an unmapped key.  float32: uniform bit patterns
    (NaNs of both signs among them) with +-0, +-inf and four NaNs set by hand; IEEE total order, compared on the bits."""
    import torch

    keys = base[:N0].clone()
    if key_type == "float32":
        special = torch.tensor([0, MIN32, 0x7F800000, 0xFF800000 - (1 << 32), 0x7FC00000, 0xFFC00000 - (1 << 32), 0x7F800001,
                                0xFFFFFFFF - (1 << 32)], dtype=torch.int32, device="cuda")
        keys[1000:1008] = special
        keys[N0 - 8:] = special
    xf = hw.TRANSFORMS[(key_type, descending)]
    assert ws.numel() >= _roomy(gpu, N0)
    d = keys.view(torch.float32).clone() if key_type == "float32" else keys.clone()
    gpu.GPUSortTyped(d, key_type, descending, workspace=ws)
    form, words = _after(gpu, ws)
    _compare(gpu, f"f {key_type} descending={descending}", keys, ws, form, words, None, half=False, xf=xf)
    assert form == (1, 0) and words["HalfOk"] == 0 and words["HalfHigh"] == 0
    expect = hw.from_sortable(torch.sort(hw.to_sortable(hw.u64(keys), xf)).values, xf)
    assert torch.equal(hw.u64(d), expect)


@pytest.mark.parametrize("payloads", [1, 2])
def test_payloads_stay_out_of_the_variant(gpu, base, payloads):
    """The gate !pairs: pairs and two payload arrays in a workspace larger than the roomy size of a keys-only sort; stable."""
    import torch

    keys = base[:N0]
    wsp = gpu.alloc_workspace(N0, 8, payloads)
    assert wsp.numel() >= _roomy(gpu, N0)
    d = keys.clone()
    v = [torch.arange(N0, dtype=torch.int32, device="cuda")]
    if payloads == 2:
        v.append(v[0] * 3 + 1)
        gpu.GPUSortMulti(d, v, 8, workspace=wsp)
    else:
        gpu.GPULSDRadixSort(d, 8, d_vals=v[0], workspace=wsp)
    form, words = _after(gpu, wsp)
    _compare(gpu, f"f payloads={payloads}", keys, wsp, form, words, None, half=False, pairs=True)
    assert form == (1, 0) and words["HalfOk"] == 0
    expect = torch.sort(keys ^ MIN32, stable=True)
    assert torch.equal(d, expect.values ^ MIN32)
    assert torch.equal(v[0].to(torch.int64), expect.indices), "order among equal keys"
    if payloads == 2:
        assert torch.equal(v[1], (expect.indices * 3 + 1).to(torch.int32)), "the second payload array"


@pytest.mark.parametrize("hint", [0, 3])
def test_shard_entry_in_the_window(gpu, base, ws, hint):
    """lsdsort_u32_device_prefixed on keys that share three bits: the device finds the prefix itself, whatever the hint; the entry
    never runs the half variant (include/lsdsort.h), so a workspace of the roomy size changes nothing: (1, 0)."""
    import torch

    keys = hw.i32((hw.u64(base[:N0]) >> 3) | (0b110 << 29))
    assert ws.numel() >= _roomy(gpu, N0)
    d = keys.clone()
    assert gpu.lib().lsdsort_u32_device_prefixed(d.data_ptr(), ws.data_ptr(), ws.numel(), N0, 8, hint, _stream()) == 0
    form, words = _after(gpu, ws)
    _compare(gpu, f"f prefixed hint={hint}", keys, ws, form, words, (1, 0), half=False)
    assert words["Prefix"] == 3 and words["LowBits"] == 14
    assert torch.equal(d, _sorted(keys))


# ---- g. guard zones ------------------------------------------------------------------------------------------------------------
def _guarded_on_device(keys, skip_bytes):
    """_guarded.guarded for a tensor that is on the device already: (whole, view)"""
    import torch

    n = keys.numel()
    raw = torch.full((GUARD + n + GUARD + 4,), SENT32, dtype=torch.int32, device="cuda")
    assert raw.data_ptr() % 512 == 0 and skip_bytes % 4 == 0
    whole = raw[skip_bytes // 4:skip_bytes // 4 + GUARD + n + GUARD]
    view = whole[GUARD:GUARD + n]
    view.copy_(keys)
    assert view.data_ptr() % 16 == skip_bytes
    return whole, view


@pytest.mark.parametrize("skip", [0, 4])
def test_exact_roomy_workspace_and_one_byte_less(gpu, base, skip):
    """N0 keys in a workspace of exactly lsdsort_workspace_bytes_roomy bytes run the variant; with one byte less, and that size
    passed, they run the full-key form -- the same output, and neither writes outside keys or workspace."""
    import torch

    keys = base[:N0]
    expect = _sorted(keys)
    roomy = _roomy(gpu, N0)
    outputs = []
    for nbytes, want in ((roomy, (1, 1)), (roomy - 1, (1, 0))):
        wbig, wview = guarded_workspace(nbytes)
        kbig, kview = _guarded_on_device(keys, skip)
        gpu.GPULSDRadixSort(kview, 8, workspace=wview)
        form, words = _after(gpu, wview)
        _compare(gpu, f"g {nbytes - roomy:+d} bytes, phase {skip}", keys, wview, form, words, want, half=nbytes >= roomy)
        assert_intact(keys=kbig, workspace=wbig)
        assert torch.equal(kview, expect)
        outputs.append(kview)
        del wbig, wview
    assert torch.equal(outputs[0], outputs[1])


HALVES_SIZES = (0, 1, 513, 10240, 10241)
HALVES_AT = (0, 777, 15000, 32000, 32767)      # the buckets that hold them, of 2^15


@pytest.mark.parametrize("half_phase", [0, 2])
@pytest.mark.parametrize("t", [0, 5])
def test_local_stage_on_halves_inside_guard_zones(gpu, t, half_phase):
    """lsdsort_local_sort_halves_u32_device with halves, output, bases, first, words and fault word each a guarded view: buckets
    of 0, 1, 513 and 10240 keys sorted, one of 10241 refused (fault bit 3, its output range untouched), the read-only inputs
    unchanged, every zone intact."""
    import torch

    rng = np.random.default_rng(50 + t)
    high = (0b10110 >> (5 - t)) << (32 - t) if t else 0
    free = 16 - t
    num_buckets = 1 << 15
    sizes = np.zeros(num_buckets, dtype=np.int64)
    first = np.zeros(num_buckets, dtype=np.uint32)
    parts = []
    for b, size in zip(HALVES_AT, HALVES_SIZES):
        sizes[b], first[b] = size, size // 3
        g = np.full(size, 2 * b, dtype=np.uint32)
        g[size // 3:] += 1
        low = rng.integers(0, 1 << free, size=size, dtype=np.uint64).astype(np.uint32)
        parts.append(np.uint32(high) | (g << np.uint32(free)) | low)
    bases = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    keys = np.concatenate(parts)
    sentinel = 0x12345678
    halves = (keys & np.uint32(0xFFFF)).astype(np.uint16)
    words = np.array([t, high, 17 - t], dtype=np.uint32)
    hbig, hview = guarded16(halves, half_phase)
    obig, oview = guarded(np.full(keys.size, sentinel, dtype=np.uint32))
    bbig, bview = guarded(bases)
    fbig, fview = guarded(first)
    wbig, wview = guarded(words)
    xbig, xview = guarded(np.zeros(1, dtype=np.uint32))
    st = gpu.lib().lsdsort_local_sort_halves_u32_device(oview.data_ptr(), hview.data_ptr(), bview.data_ptr(), fview.data_ptr(), num_buckets,
                                                        wview.data_ptr(), xview.data_ptr(), _stream())
    assert st == 0
    torch.cuda.synchronize()
    assert_intact(output=obig, bases=bbig, first=fbig, words=wbig, fault=xbig)
    assert_intact16(halves=hbig)
    assert_unchanged(bview, bases, "bases")
    assert_unchanged(fview, first, "first")
    assert_unchanged(wview, words, "the three words")
    assert np.array_equal(bits_of(hview), halves), "the halves were changed"
    assert int(xview.cpu().numpy().view(np.uint32)[0]) == 8, "a bucket of 10241 keys raises fault bit 3, and nothing else is raised"
    got = oview.cpu().numpy().view(np.uint32)
    for b, size, part in zip(HALVES_AT, HALVES_SIZES, parts):
        lo = int(bases[b])
        if size > hw.CAP_SMALL:
            assert np.all(got[lo:lo + size] == np.uint32(sentinel)), "the refused bucket's output range was written"
        else:
            assert np.array_equal(got[lo:lo + size], np.sort(part)), (t, b, size)
