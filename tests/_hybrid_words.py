"""The decisions of the hybrid form and its half variant restated (hybrid.hip, half_hop.hip, make_plan of lsdsort_api.hip; DESIGN.md
4.9 to 4.9.2), and the control words a sort leaves behind (a helper module: no fixtures, no pytest settings).

Whether the hybrid form runs, and whether its half variant does, is decided on the device by a chain of defences, each of which
writes a word into the control block (the first 512 bytes of the workspace):

    Hopeless    the 65536-key sample: eight samples of one workgroup in one bucket counter
    Violated    the upfront read: some key differs from keys[0] inside the sampled prefix
    Largest     the planner: the largest bucket (above kLocalSortCap = 16384 the form is refused)
    (the sum)   the planner: the counts must sum to n -- no word of its own; it is what is left when Ok == 0 and nobody else objects
    LargeCount  the planner: buckets above the small capacity; half_decide_kernel turns any into "no halves"

read_words(ws) reads them; expected_words(keys, ...) predicts them from the keys' own bincount with the rules restated here in
plain Python.  The constants are read from the sources with regular expressions (as _long_plan.py's are pinned by
test_long_plan_cpu.py, these are by test_hybrid_words_cpu.py).

The half variant counts 2^16 groups in 16-bit halves, two to a word; so does the 2^16-bucket form in LDS.  fold() is that
arithmetic: a group of 65536 keys or more carries into its neighbour or out of the word, and the sum of all counts falls short."""
import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lsdradixsort_amd", "csrc")


# ---- constants, from the sources -----------------------------------------------------------------------------------------------
def _text(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _constants(text, known=None):
    """every `constexpr <type> kName = <integer expression>;` of a source text whose expression is made of literals, + - * << ( ),
    size_t casts and names already known"""
    out = dict(known or {})
    for m in re.finditer(r"constexpr\s+(?:size_t|int|uint32_t|unsigned)\s+(k[A-Z]\w*)\s*=\s*([^;{}]+);", text):
        expr = re.sub(r"\(\s*(?:size_t|uint32_t|int)\s*\)", "", m.group(2))
        expr = re.sub(r"\blsd::", "", expr)
        expr = re.sub(r"\b(\d+)[uUlL]+\b", r"\1", expr)
        expr = re.sub(r"\bk[A-Z]\w*\b", lambda x: str(out[x.group(0)]) if x.group(0) in out else x.group(0), expr)
        if re.fullmatch(r"[\d\s+\-*<>()]+", expr):
            out[m.group(1)] = int(eval(expr, {"__builtins__": {}}))   # digits, operators and brackets only
    return out


_KERNELS = _constants(_text("lsd_kernels.hpp"))
_API = _constants(_text("lsdsort_api.hip"), _KERNELS)
_HYBRID = _constants(_text("hybrid.hip"), _KERNELS)

LOCAL_SORT_CAP = _KERNELS["kLocalSortCap"]
CAP_SMALL = _KERNELS["kLocalSortCapSmall"]
CAP_SMALL_PAIRS = _KERNELS["kLocalSortCapSmallPairs"]
CAP_TINY = _KERNELS["kLocalSortCapTiny"]
MAX_MEAN_BUCKET = _KERNELS["kHybridMaxMeanBucket"]
MAX_PREFIX = _KERNELS["kHybridMaxPrefix"]
HALF_GROUPS = _KERNELS["kHalfGroups"]
CONTROL_BYTES = _API["kControlBytes"]
HYBRID_OFFSET_WORDS = _API["kHybridOffsetWords"]       # kPlanOffsetWords + kPlanWords + 1
MAX_KEYS = _API["kHybridMaxKeys"]
_m = re.search(r"return pairs \? \(size_t\)(\d+) \* 1000 \* 1000 : \(size_t\)(\d+) \* 1000 \* 1000;", _text("lsdsort_api.hip"))
MIN_ITEMS = {True: int(_m.group(1)) * 1000 * 1000, False: int(_m.group(2)) * 1000 * 1000}   # 8-bit digits
HIST_THREADS = _HYBRID["kHybridHistThreads"]
HIST_VPT = _HYBRID["kHybridVpt"]
HIST_MAX_BLOCKS = _HYBRID["kHybridHistMaxBlocks"]
CHUNK_KEYS = HIST_THREADS * 4                          # a chunk: one 16-byte vector per thread
GROUP_KEYS = CHUNK_KEYS * HIST_VPT                     # what a workgroup of the upfront read takes at a time
# the sample's shape, as hybrid_sample_kernel and its launcher spell it
SAMPLES = _HYBRID["kSamples"]
_m = re.search(r"launch_dynamic_lds<hybrid_sample_kernel>\(dim3\((\d+)\), dim3\((\d+)\)", _text("hybrid.hip"))
SAMPLE_BLOCKS, SAMPLE_THREADS = int(_m.group(1)), int(_m.group(2))
_m = re.search(r"\+ 1u >= (\d+)u\) words\[kHybridWordHopeless\] = 1u;", _text("hybrid.hip"))
SAMPLE_HOPELESS_AT = int(_m.group(1))

# name -> index behind HYBRID_OFFSET_WORDS: kHybridWordOk -> "Ok", kHalfWordOk -> "HalfOk"
WORD_INDEX = {m.group(1): _KERNELS["kHybridWord" + m.group(1)] for m in re.finditer(r"\bkHybridWord([A-Z]\w*)\s*=", _text("lsd_kernels.hpp"))}
WORD_INDEX.update({"Half" + m.group(1): _KERNELS["kHalfWord" + m.group(1)] for m in re.finditer(r"\bkHalfWord([A-Z]\w*)\s*=", _text("lsd_kernels.hpp"))})

WINDOW = (158_056_448, 330_596_351)     # the sizes of keys-only sorts that hybrid_bucket_bits gives 15 bits: where the half variant exists


# ---- the host rules --------------------------------------------------------------------------------------------------------------
def _root_up(x):
    r = 1
    while r * r < x:
        r += 1
    return r


def hybrid_bucket_bits(n, pairs=False):
    """lsd_kernels.hpp's hybrid_bucket_bits"""
    mean, cap = n >> 14, CAP_SMALL_PAIRS if pairs else CAP_SMALL
    if mean + 6 * _root_up(mean) <= cap:
        return 14
    mean15 = n >> 15
    return 15 if 2 * mean15 + 3 * _root_up(mean15) <= 2 * cap else 16


def hybrid_small_cap(n, pairs=False):
    """lsdsort_api.hip's hybrid_small_cap with its environment knob at the default"""
    mean = float(n >> hybrid_bucket_bits(n, pairs))
    if mean + 6.0 * math.sqrt(mean) <= float(CAP_TINY):
        return CAP_TINY
    small = CAP_SMALL_PAIRS if pairs else CAP_SMALL
    return LOCAL_SORT_CAP if mean + 1.5 * math.sqrt(mean) > float(small) else small


def hybrid_tried(n, pairs=False):
    """make_plan's try_hybrid for 8-bit digits, the default tile and switches"""
    return MIN_ITEMS[pairs] <= n <= MAX_KEYS and (n >> hybrid_bucket_bits(n, pairs)) <= MAX_MEAN_BUCKET


def in_half_window(n):
    """half_form_fits for 8-bit digits and the default tile"""
    return MIN_ITEMS[False] <= n <= MAX_KEYS and hybrid_bucket_bits(n) == 15 and (n >> 15) <= MAX_MEAN_BUCKET


def sample_step(n):
    return n // SAMPLES


def sample_positions(n):
    """[SAMPLE_BLOCKS, SAMPLE_THREADS] int64: the key that thread tid of workgroup `block` of the sample looks at"""
    tid = np.arange(SAMPLE_THREADS, dtype=np.int64)[None, :]
    block = np.arange(SAMPLE_BLOCKS, dtype=np.int64)[:, None]
    return (tid * SAMPLE_BLOCKS + block) * sample_step(n)


def full_group_keys(n, aligned=True):
    """the keys the upfront read's pipelined loop takes (whole groups of whole chunks); the rest go through its tail loop"""
    return (n // CHUNK_KEYS) // HIST_VPT * HIST_VPT * CHUNK_KEYS if aligned else 0


def hist_blocks(n, aligned=True):
    """stream_grid's grid for the upfront read"""
    blocks = -(-(n // CHUNK_KEYS) // HIST_VPT) if aligned else -(-n // (HIST_THREADS * 16))
    return max(1, min(blocks, HIST_MAX_BLOCKS))


def owner_of(pos, n, aligned=True):
    """the workgroup of the upfront read that counts the key at position pos (an integer or an integer array)"""
    pos = np.asarray(pos, dtype=np.int64)
    blocks, full = hist_blocks(n, aligned), full_group_keys(n, aligned)
    return np.where(pos < full, (pos // GROUP_KEYS) % blocks, ((pos - full) // HIST_THREADS) % blocks)


def owned_ranges(w, n, rounds):
    """[(lo, hi)]: the first `rounds` groups of workgroup w, for a 16-byte-aligned base: keys [(w + blocks i) GROUP_KEYS, + GROUP_KEYS)"""
    blocks = hist_blocks(n)
    out = [((w + blocks * i) * GROUP_KEYS, (w + blocks * i + 1) * GROUP_KEYS) for i in range(rounds)]
    assert out[-1][1] <= full_group_keys(n)
    return out


def sample_hits(ranges, n):
    """how many sampled positions inside `ranges` each workgroup of the sample looks at: [SAMPLE_BLOCKS]"""
    pos = sample_positions(n)
    inside = np.zeros(pos.shape, dtype=bool)
    for lo, hi in ranges:
        inside |= (pos >= lo) & (pos < hi)
    return inside.sum(axis=1)


# ---- the fold ------------------------------------------------------------------------------------------------------------------
def fold(low, high):
    """(bucket, first, lost) of one packed word holding the counts of groups 2 j (low) and 2 j + 1 (high): what half_fold_kernel
    makes of it, and how many keys the sum of all buckets is short by"""
    word = (int(low) + (int(high) << 16)) % (1 << 32)
    bucket, first = (word & 0xFFFF) + (word >> 16), word & 0xFFFF
    return bucket, first, int(low) + int(high) - bucket


def fold_counts(groups):
    """fold() for all 2^16 group counts at once (an int64 torch tensor or numpy array): (bucket [2^15], first [2^15])"""
    word = (groups[0::2] + (groups[1::2] << 16)) % (1 << 32)
    return (word & 0xFFFF) + (word >> 16), word & 0xFFFF


def unpack_counts(groups):
    """what a workgroup's 16-bit LDS counters hold of its own counts `groups` (2^16-bucket form: two buckets to a word), as counts
    per bucket again: [2^16]"""
    word = (groups[0::2] + (groups[1::2] << 16)) % (1 << 32)
    out = groups.clone() if hasattr(groups, "clone") else groups.copy()
    out[0::2], out[1::2] = word & 0xFFFF, word >> 16
    return out


# ---- keys ------------------------------------------------------------------------------------------------------------------------
def u64(t):
    """an int32 tensor's bit patterns as non-negative int64"""
    import torch

    return t.view(torch.int32).to(torch.int64) & 0xFFFFFFFF


def i32(x):
    """non-negative int64 values below 2^32 as int32 bit patterns"""
    import torch

    return ((x + (1 << 31)) % (1 << 32) - (1 << 31)).to(torch.int32)


TRANSFORMS = {   # (a, b, c) of lsd_kernels.hpp's KeyTransform; None: plain uint32
    ("uint32", False): None, ("uint32", True): (0, 0, 0xFFFFFFFF),
    ("int32", False): (0, 0x80000000, 0), ("int32", True): (0, 0x80000000, 0xFFFFFFFF),
    ("float32", False): (0x80000000, 0x80000000, 0), ("float32", True): (0x80000000, 0x80000000, 0xFFFFFFFF),
}


def to_sortable(u, xf):
    """lsd_kernels.hpp's to_sortable on non-negative int64 bit patterns: t = k ^ (sext(k & a) | b) ^ c"""
    if xf is None:
        return u
    a, b, c = xf
    sext = ((u & a) >> 31) * 0xFFFFFFFF
    return u ^ (sext | b) ^ c


def from_sortable(t, xf):
    if xf is None:
        return t
    a, b, c = xf
    u = t ^ c
    sext = (((u ^ 0xFFFFFFFF) & a) >> 31) * 0xFFFFFFFF
    return u ^ (sext | b)


def with_exact_count(keys, field_shift, field_value, target, *, avoid_step, seed=1):
    """A copy of `keys` (int32 bit patterns) in which exactly `target` keys have key >> field_shift == field_value: just enough keys
    at random positions that are not divisible by avoid_step (the sample never looks there) and not already in the field get the
    field's value above their own low bits."""
    import torch

    assert 0 <= field_value < 1 << (32 - field_shift)
    n = keys.numel()
    out = keys.clone()
    field = u64(out) >> field_shift
    need = target - int((field == field_value).sum())
    if need < 0:
        raise ValueError(f"{-need} keys too many hold the value already")
    gen = torch.Generator(device=keys.device)
    gen.manual_seed(seed)
    if n <= 1 << 22:
        cand = torch.randperm(n, generator=gen, device=keys.device)
    else:
        cand = torch.unique(torch.randint(0, n, (2 * need + 4096,), generator=gen, device=keys.device))
        cand = cand[torch.randperm(cand.numel(), generator=gen, device=keys.device)]
    cand = cand[(cand % avoid_step != 0) & (field[cand] != field_value)][:need]
    if cand.numel() != need:
        raise ValueError("not enough free positions")
    low = u64(out[cand]) & ((1 << field_shift) - 1)
    out[cand] = i32((field_value << field_shift) | low)
    return out


# ---- the words -------------------------------------------------------------------------------------------------------------------
def read_words(ws):
    """name -> value of the hybrid form's control words of the sort last queued in workspace tensor `ws` (synchronises)"""
    import torch

    torch.cuda.synchronize()
    words = ws[:CONTROL_BYTES].view(torch.int32).cpu().numpy().view(np.uint32)
    return {name: int(words[HYBRID_OFFSET_WORDS + index]) for name, index in WORD_INDEX.items()}


def read_half_counts(ws, roomy_bytes):
    """(bucket [2^15], first [2^15]) int64: the folded counts and the lower groups' counts the half variant keeps at the end of a
    workspace of `roomy_bytes` (make_half_layout: 2^16 words of counts, then 2^15 words of splits, each 256-byte aligned)"""
    import torch

    torch.cuda.synchronize()
    first_at = roomy_bytes - 4 * (HALF_GROUPS // 2)
    c16_at = first_at - 4 * HALF_GROUPS
    first = ws[first_at:first_at + 4 * (HALF_GROUPS // 2)].view(torch.int32)
    bucket = ws[c16_at:c16_at + 4 * (HALF_GROUPS // 2)].view(torch.int32)
    return u64(bucket), u64(first)


def _clz32(x):
    return 32 - int(x).bit_length()


def sample_verdict(keys, bucket_bits):
    """(hopeless, differ) of hybrid_sample_kernel on int32 bit patterns `keys`: every workgroup counts its samples by the bucket
    below ITS OWN samples' prefix (two neighbouring buckets to a counter at 2^16 buckets) and raises Hopeless at eight in one"""
    import torch

    n = keys.numel()
    pos = sample_positions(n)
    s = u64(keys[torch.from_numpy(pos.reshape(-1)).to(keys.device)]).cpu().numpy().reshape(pos.shape)
    d = s ^ int(u64(keys[:1])[0])
    shift = 32 - bucket_bits
    halve = 17 - shift if shift < 17 else 0
    hopeless, differ = 0, 0
    for w in range(SAMPLE_BLOCKS):
        mine = int(np.bitwise_or.reduce(d[w]))
        differ |= mine
        prefix = _clz32(mine) if mine else 32
        if prefix > MAX_PREFIX:
            prefix = 0
        counter = ((s[w] >> (shift - prefix)) & ((1 << bucket_bits) - 1)) >> halve
        if np.unique(counter, return_counts=True)[1].max() >= SAMPLE_HOPELESS_AT:
            hopeless = 1
    return hopeless, differ


def expected_words(keys, *, half, pairs=False, xf=None, lds16_block=None):
    """What a sort of `keys` (int32 bit patterns on any device; 8-bit digits, hybrid_tried sizes) must leave in its control words,
    from the keys' own bincount: Hopeless, Violated, Prefix, LowBits, Largest, LargeCount, Ok, HalfOk, HalfHigh; and beside them
    "total" (the sum of the counts the planner sees), "bucket" and, with `half`, "first" (the counts themselves; None where the
    upfront read does not run).  half: the variant is attempted (roomy workspace, window size, plain keys, switch on).  xf:
    TRANSFORMS[...] of a typed sort.  lds16_block: at 2^16 buckets, the one workgroup of the upfront read whose 16-bit LDS counters
    may overflow (asserted: nobody else's can).  Which workgroup counts a key matters for that alone: every other count is the
    same for any alignment of the key base."""
    import torch

    n = keys.numel()
    bits, cap = hybrid_bucket_bits(n, pairs), hybrid_small_cap(n, pairs)
    assert hybrid_tried(n, pairs) and (not half or (in_half_window(n) and not pairs and xf is None))
    hopeless, differ = sample_verdict(keys, bits)
    prefix = _clz32(differ) if differ else 32
    out = {"Hopeless": hopeless, "Violated": 0, "Prefix": prefix if prefix <= MAX_PREFIX else 0, "bucket": None, "first": None}
    if hopeless or prefix > MAX_PREFIX:      # the upfront read returns at once: the planner sees no counts
        largest = large = total = 0
    else:
        t = to_sortable(u64(keys), xf)
        if prefix and bool((((t ^ t[0]) >> (32 - prefix)) != 0).any()):
            out["Violated"] = 1
        if half:
            groups = torch.bincount((t >> (16 - prefix)) & 0xFFFF, minlength=1 << 16)
            bucket, out["first"] = fold_counts(groups)
        else:
            bucket = torch.bincount((t >> (32 - bits - prefix)) & ((1 << bits) - 1), minlength=1 << bits)
            if bits == 16 and lds16_block is not None:
                assert prefix == 0            # the ownership is that of a 16-byte-aligned key base: the caller checks
                full = full_group_keys(n)
                rows = t[:full].view(-1, GROUP_KEYS)[lds16_block::hist_blocks(n)].reshape(-1)
                tail = torch.arange(full, n, device=keys.device)
                tail = tail[((tail - full) // HIST_THREADS) % hist_blocks(n) == lds16_block]
                mine = torch.bincount(torch.cat([rows, t[tail]]) >> 16, minlength=1 << 16)
                assert int((bucket - mine).max()) < 65536, "another workgroup's counters could overflow as well"
                bucket = bucket - mine + unpack_counts(mine)
            else:
                assert bits < 16 or int(bucket.max()) < 65536, "a workgroup's 16-bit counters could overflow: name it"
        del t
        out["bucket"] = bucket
        largest, large, total = int(bucket.max()), int((bucket > cap).sum()), int(bucket.sum())
    out.update(Largest=largest, LargeCount=large, total=total)
    out["Ok"] = 1 if largest <= LOCAL_SORT_CAP and total == n and not out["Violated"] else 0
    out["LowBits"] = 32 - out["Prefix"] - bits
    out["HalfOk"] = 1 if half and out["Ok"] and large == 0 else 0
    p = out["Prefix"]
    out["HalfHigh"] = int(u64(keys[:1])[0]) & ~((1 << (32 - p)) - 1) & 0xFFFFFFFF if half and p else 0
    return out


COMPARED = ("Hopeless", "Violated", "Prefix", "LowBits", "Largest", "LargeCount", "Ok", "HalfOk", "HalfHigh")
