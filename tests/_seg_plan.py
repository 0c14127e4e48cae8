"""The segmented sort's plan restated, the shapes past its table and grid caps, and their inputs (a helper module: no fixtures,
no pytest settings).

lsdsort_segmented_device (lsdradixsort_amd/csrc/segmented.hip) sizes every launch and every table from (n, num_segments) alone:
seg_plan_kernel lists the segments by size class and leaves five counters in the workspace's control block, seg_layout sizes the
tables from a worst-case argument, and the large tier -- seg_tiles_kernel, then per digit pass seg_hist_kernel, the three seg_scan_*
kernels and seg_scatter_kernel -- runs with capped grids whose workgroups walk the tables in grid-stride loops.  plan() below is
that arithmetic in numpy; SHAPES are the smallest segmentations that send each capped loop round again and that fill the tables to
within one entry.  test_gpu_segmented_plan.py runs them on the GPU and holds the counters it reads back against plan();
test_seg_plan_cpu.py reads the constants and launch lines from the sources and fails when a raised cap leaves a shape inside the
first round.
"""
import numpy as np
import torch

from _key_oracle import SPECIALS32 as SPECIALS

SEG_TILE = 4096        # kSegTile: keys per large-tier tile
SCAN_BLOCK = 4096      # kScanBlock: entries per block of the flat scan
WAVE_CAP = 1024        # kWaveSegCap
GROUP_CAP = 16384      # kLocalSortCap
SUMS_ROUND = 1024      # block sums one round of seg_scan_sums_kernel's carry loop covers (its workgroup size)
CTL_BYTES = 256
ALIGN = 256
# (per workgroup, cap) of the capped launches, as their grid_for(items, per, cap) lines read
GRIDS = {"plan": (256, 2048), "wave": (8, 4096), "group": (1, 512), "items": (1, 1024), "tiles": (1, 16384)}
COUNTERS = ("wave", "group", "items", "tiles", "hist_tiles")   # kCntWave .. kCntHistTiles: u64 words 1..5 of the control block


def grid_for(items, per, cap):
    return int(min(max(-(-items // per), 1), cap))


def _align(x):
    return -(-x // ALIGN) * ALIGN


def plan(sizes, local=True, n=None):
    """What seg_plan_kernel counts and what run_segmented sizes for segments of `sizes` keys in an array of n keys (default: their
    sum).  local: the wave and workgroup tiers run; otherwise every segment of two or more keys is large, one of up to SEG_TILE
    keys a one-tile entry of the tile table with no item and no counts."""
    sizes = np.asarray(sizes, dtype=np.int64)
    segs = int(sizes.size)
    n = int(sizes.sum()) if n is None else int(n)
    assert n >= int(sizes.sum()) and (sizes >= 0).all()
    if local:
        large = sizes > GROUP_CAP
        wave = int(((sizes >= 2) & (sizes <= WAVE_CAP)).sum())
        group = int(((sizes > WAVE_CAP) & (sizes <= GROUP_CAP)).sum())
    else:
        large = sizes >= 2
        wave = group = 0
    nt = -(-sizes[large] // SEG_TILE)
    multi = nt > 1
    p = {"wave": wave, "group": group, "items": int(multi.sum()), "tiles": int(nt.sum()), "hist_tiles": int(nt[multi].sum())}
    # seg_layout
    listed = min(segs, n // 2)
    p["listed"] = listed
    p["group_cap"] = min(segs, n // (WAVE_CAP + 1))
    p["max_items"] = min(segs, n // (SEG_TILE + 1)) + 1
    p["max_hist_tiles"] = n // SEG_TILE + p["max_items"]
    p["max_tiles"] = n // SEG_TILE + listed + 1
    # run_segmented's launches
    smallest_large = GROUP_CAP + 1 if local else 2
    p["plan_grid"] = grid_for(segs, *GRIDS["plan"])
    p["wave_grid"] = grid_for(listed, *GRIDS["wave"]) if local else 0
    p["group_grid"] = grid_for(p["group_cap"], *GRIDS["group"]) if local and n > WAVE_CAP else 0
    launch_tiles = n // SEG_TILE + n // smallest_large + 1 if local else p["max_tiles"]
    p["items_grid"] = grid_for(min(segs, n // smallest_large) + 1, *GRIDS["items"]) if n >= smallest_large else 0
    p["tile_grid"] = grid_for(launch_tiles, *GRIDS["tiles"]) if n >= smallest_large else 0
    p["scan_grid"] = grid_for(p["max_hist_tiles"] * 256, SCAN_BLOCK, 1 << 30)
    p["block_sums"] = -(-p["hist_tiles"] * 256 // SCAN_BLOCK)
    return p


def workspace_bytes(p, n, pairs):
    """seg_layout's total rebuilt from plan()'s caps: control | wave list | workgroup list | items | tile table | counts | block
    sums | keys buffer | payload buffer, each aligned"""
    off = CTL_BYTES
    for nbytes in (p["listed"] * 4, p["group_cap"] * 4, p["max_items"] * 16, p["max_tiles"] * 8, p["max_hist_tiles"] * 256 * 4,
                   (p["max_hist_tiles"] * 256 // SCAN_BLOCK + 1) * 4, n * 4, n * 4 if pairs else 0):
        off = _align(off + nbytes)
    return off


def read_counters(ws):
    """the planner's counters of the last call into workspace `ws` (a uint8 device tensor): bytes 8..48 of its control block"""
    words = ws[8:48].view(torch.int64).cpu().tolist()
    return dict(zip(COUNTERS, words))


# ---- shapes ---------------------------------------------------------------------------------------------------------------------
ITEM_SEGS = 1027   # three more multi-tile segments than one round of seg_tiles_kernel's grid takes


def _ragged(segs, base, mul, mod):
    s = np.arange(segs, dtype=np.int64)
    return base + (mul * s) % mod


def _mixed_sizes():
    """ITEMS' large segments spread evenly among 3000 wave-tier and 600 workgroup-tier ones (both with their extreme sizes), an
    empty segment after every tenth"""
    large = _ragged(ITEM_SEGS, GROUP_CAP + 1, 37, 611)
    wave = _ragged(3000, 2, 37, WAVE_CAP - 1)                  # 2 .. 1024
    group = _ragged(600, WAVE_CAP + 1, 97, GROUP_CAP - WAVE_CAP)   # 1025 .. 16384
    wave[-1], group[-1] = WAVE_CAP, GROUP_CAP
    parts = (large, wave, group)
    where = np.concatenate([(np.arange(p.size) + 0.5) / p.size for p in parts])
    sizes = np.concatenate(parts)[np.argsort(where, kind="stable")]
    out = np.zeros(sizes.size + sizes.size // 10, dtype=np.int64)
    out[np.arange(sizes.size) + np.arange(sizes.size) // 10] = sizes
    return out


# name -> (segment sizes, local, head, tail): head and tail are keys outside [off[0], off[-1]) that must stay untouched
SHAPES = {
    "ITEMS": (_ragged(ITEM_SEGS, GROUP_CAP + 1, 37, 611), True, 0, 0),
    "ITEMS_TIGHT": (np.full(ITEM_SEGS, 4 * SEG_TILE + 1, dtype=np.int64), True, 0, 0),
    "ITEMS_FALLBACK": (_ragged(ITEM_SEGS, SEG_TILE + 1, 37, 611), False, 0, 0),
    "FALLBACK_TIGHT": (np.full(ITEM_SEGS, SEG_TILE + 1, dtype=np.int64), False, 0, 0),
    "TILES": (_ragged(67, (1 << 20) + 1, 4099, 8191), True, 0, 0),
    "MIXED": (_mixed_sizes(), True, 77, 131),
}
SHORT_SIZE = 100   # the graph test's first segmentation: ITEMS' (n, segs) with every segment this short


def offsets_of(name):
    """(int64 offsets, n) of a shape"""
    sizes, _, head, tail = SHAPES[name]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64) + head
    return off, int(off[-1]) + tail


def plan_of(name):
    sizes, local, _, _ = SHAPES[name]
    return plan(sizes, local, offsets_of(name)[1])


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
KINDS = ("uniform", "half zeros", "one live byte", "four values", "all equal", "float specials")


def segment_kinds(segs, key_type, shift=0):
    """kind of every segment: it rotates with the segment index, so neighbouring segments never share one"""
    kinds = len(KINDS) if key_type == "float32" else len(KINDS) - 1
    return (np.arange(segs, dtype=np.int64) + shift) % kinds


def _wrap32(x):
    """int64 values in [0, 2^32) as the int32 of the same bits"""
    return ((x + (1 << 31)) % (1 << 32) - (1 << 31)).to(torch.int32)


def make_keys(off, n, key_type, seed, device="cuda", shift=0):
    """n int32 words (the keys' bits) made on `device`: the keys of segment s = [off[s], off[s + 1]) are of kind
    segment_kinds()[s] -- uniform bits | half zeros (a heavy value) | one live byte, the other three constant (every key of a tile
    in one digit in three of the four passes) | four values (tie runs, where stability shows) | all equal | float32 only: normal
    variates with _key_oracle's SPECIALS32 mixed in.  Keys in front of off[0] and behind off[-1] are uniform."""
    g = torch.Generator(device=device).manual_seed(seed)
    segs = len(off) - 1
    sizes = torch.from_numpy(np.diff(off)).to(device)
    kind_of = torch.from_numpy(segment_kinds(segs, key_type, shift)).to(device)
    kind = torch.zeros(n, dtype=torch.int64, device=device)
    kind[int(off[0]):int(off[-1])] = torch.repeat_interleave(kind_of, sizes)
    del sizes, kind_of
    uniform = torch.randint(0, 1 << 32, (n,), generator=g, device=device, dtype=torch.int64)
    keys = uniform.clone()
    keys[(kind == 1) & (torch.rand(n, generator=g, device=device) < 0.5)] = 0
    keys = torch.where(kind == 2, 0x5A00C3E1 | (uniform & 0x00FF0000), keys)
    four = torch.tensor([5, 0x00010000, 0x7FFFFFFF, 0xFFFFFFF0], dtype=torch.int64, device=device)
    keys = torch.where(kind == 3, four[(uniform >> 7) & 3], keys)
    keys = torch.where(kind == 4, torch.full_like(keys, 0x9E3779B9), keys)
    if key_type == "float32":
        f = torch.randn(n, generator=g, device=device).view(torch.int32).to(torch.int64) & 0xFFFFFFFF
        special = torch.tensor(SPECIALS.tolist(), dtype=torch.int64, device=device)[(uniform >> 9) % len(SPECIALS)]
        f = torch.where(torch.rand(n, generator=g, device=device) < 0.3, special, f)
        keys = torch.where(kind == 5, f, keys)
    return _wrap32(keys)


def expected_dev(d_keys, offsets_np, key_type="uint32", descending=False):
    """the stable segmented order on the device (large shapes): stable torch.sort of segment id << 32 | sortable key; returns
    (keys, source index).  Independent of the code under test; test_gpu_segmented.py uses it too."""
    u = d_keys.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    if key_type == "int32":
        u = u ^ 0x80000000
    elif key_type == "float32":
        u = u ^ (((u >> 31) * 0x7FFFFFFF) | 0x80000000)
    if descending:
        u = u ^ 0xFFFFFFFF
    lo, hi = int(offsets_np[0]), int(offsets_np[-1])
    sizes = torch.from_numpy(np.diff(offsets_np.astype(np.int64))).to(d_keys.device)
    seg = torch.repeat_interleave(torch.arange(sizes.numel(), device=d_keys.device), sizes)
    comp = (seg << 32) | u[lo:hi]
    _, idx = torch.sort(comp, stable=True)
    del comp, seg, u
    idx = idx + lo
    out = d_keys.clone()
    out[lo:hi] = d_keys[idx]
    return out, idx
