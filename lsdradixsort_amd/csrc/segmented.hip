// segmented.hip -- many independent segments of one array in one call (lsdsort_segmented_device).
//
// No counterpart in the reference (it sorts one array, LSDRadixSort.cu:839-910).  Segment s = keys [off[s], off[s + 1]).  Segment
// sizes are known only on the device and the entry does not synchronise, so a PLANNER kernel reads the offsets, checks them and
// lists every segment of two or more keys in one of three size classes; the tiers that follow are launched with fixed grids sized
// from (n, num_segments), walk their lists and let surplus workgroups leave (the pattern of local_sort_list_kernel):
//   wave      2 .. kWaveSegCap keys      one wavefront per segment, keys in its registers and its own LDS slice, no barrier
//   workgroup .. kLocalSortCap (16384)   one workgroup per segment in LDS (local_sort.hip sort_segment, sort_bucket's passes)
//   large     above                      four staged passes over ragged tiles that never cross a segment (below)
// In the wave and workgroup tiers a digit that is the same for every key of the segment (AND and OR of its keys agree on it) is no
// pass at all.  Both tiers rank with the returning LDS add, whose lane order the library probes on the device; where that form is
// not in force (lsdsort_set_rank_method(0), a failed probe) the planner sends EVERY segment of two or more keys to the large tier,
// which ranks with wave ballots then: same result, slower.
//
// Large tier, per 8-bit digit pass (DESIGN.md section 4.4's staged form, 12 B/key/pass, made segment-aware):
//   tile table  each large segment is cut into tiles of kSegTile keys, the last one short; a segment of one tile (fallback only)
//               needs no table of counts: its digit offsets are its own
//   histograms  hist[(segment block)][digit][tile within segment] per tile: the blocks of the multi-tile segments one after another
//   scan        ONE flat exclusive scan over all blocks
//   scatter     tile t of segment s puts its digit-d keys at off[s] + scan(s, d, t) - scan(s, 0, 0), in tile order (stable)
// Work ping-pongs through a workspace buffer of n words (2n with payloads); four passes end back in place.
//
// Offsets: a segment whose end is below its start or beyond n raises kSegFaultBit in the workspace's fault word and is left
// alone (lsdsort_check_device: LSDSORT_ERR_DEVICE_FAULT).  Every access stays inside [0, n): listed segments are checked ones.
#define LSDSORT_BUILD 1
#include "../../include/lsdsort.h"

#include "lsd_device.hpp"
#include "lsd_host.hpp"

namespace lsd {
namespace {

constexpr uint32_t kSegTile = 4096;          // keys per large-tier tile: 256 threads x 16
constexpr int kSegThreads = 256;
constexpr int kSegKeys = (int)kSegTile / kSegThreads;
constexpr int kSegWaves = kSegThreads / kWave;
constexpr uint32_t kOneTile = 0xFFFFFFFFu;   // tile table: the tile is a whole segment (.x = the segment)
constexpr uint32_t kSkipTile = 0xFFFFFFFEu;  // tile table: nothing (a segment that did not fit the tables, below)
constexpr uint32_t kScanBlock = 4096;        // entries per block of the flat scan
constexpr int kWaveTierWaves = 8;            // segments per workgroup of the wave tier
constexpr int kWaveRows = kWaveSegCap / kWave;
constexpr int kWaveSliceWords = kWaveSegCap + 256;   // per wave: keys, then 256 digit counters

// control block (the workspace's first 256 bytes): word 0 is the fault word every entry keeps there, then the planner's 64-bit
// counters from byte 8 (64 bits: no sum of sizes, however the offsets overlap, wraps one round to an index already handed out)
enum : int { kCtlFault = 0 };
enum : int { kCntWave = 1, kCntGroup = 2, kCntItems = 3, kCntTiles = 4, kCntHistTiles = 5 };   // index into the u64 view
typedef unsigned long long u64;
// Fault bits besides kSegFaultBit: tables that do not describe the offsets (never expected: a tier then skips the entry, and no
// key is read or written outside the array)
constexpr uint32_t kSegFaultList = 128u, kSegFaultTile = 256u, kSegFaultDest = 512u;
__device__ __forceinline__ uint32_t clamp_count(u64 count, uint32_t cap) { return count < cap ? (uint32_t)count : cap; }


// Workspace: control | wave list | workgroup list | items (uint4 per multi-tile segment) | tile table (uint2 per tile)
//            | counts [hist tiles][256] | scan block sums | keys buffer | payload buffer
struct SegLayout {
    size_t wave_list, group_list, items, tiles, hist, sums, alt_keys, alt_vals, total;
    size_t max_items, max_tiles, max_hist_tiles;
};
SegLayout seg_layout(size_t n, size_t segs, bool pairs)
{
    SegLayout L{};
    const size_t listed = min_sz(segs, n / 2);                       // segments of two or more keys
    L.max_items = min_sz(segs, n / (kSegTile + 1)) + 1;              // segments of more than one tile
    L.max_hist_tiles = n / kSegTile + L.max_items;                   // their tiles
    L.max_tiles = n / kSegTile + listed + 1;                         // every large-tier tile, the fallback's one-tile segments included
    size_t off = kCtlBytes;
    L.wave_list = off;   off = align_up(off + listed * 4);
    L.group_list = off;  off = align_up(off + min_sz(segs, n / (kWaveSegCap + 1)) * 4);
    L.items = off;       off = align_up(off + L.max_items * 16);
    L.tiles = off;       off = align_up(off + L.max_tiles * 8);
    L.hist = off;        off = align_up(off + L.max_hist_tiles * 256 * 4);
    L.sums = off;        off = align_up(off + (L.max_hist_tiles * 256 / kScanBlock + 1) * 4);
    L.alt_keys = off;    off = align_up(off + n * 4);
    L.alt_vals = off;    off = align_up(off + (pairs ? n * 4 : 0));
    L.total = off;
    return L;
}

struct PlanParams {
    const uint32_t* offsets;
    uint32_t segs, n;
    uint32_t local;               // 1: the wave and workgroup tiers run (returning-add rank form in force)
    uint32_t* ctl;
    u64* cnt;                     // ctl viewed as 64-bit words
    uint32_t* wave_list;
    uint32_t* group_list;
    uint4* items;                 // {segment, first tile, first hist tile, tiles}
    uint2* tiles;                 // {item, tile within segment}, {segment, kOneTile} or {-, kSkipTile}
    uint32_t wave_cap, group_cap, item_cap, tile_cap, hist_cap;   // what the workspace holds
};

// One atomic per wave for the lanes that append.  (At 10^6 segments the planner takes 0.20 ms either way: the atomics of every wave
// still meet on one word -- DESIGN.md section 6.3.)
__device__ __forceinline__ u64 wave_append(u64* counter, bool want)
{
    const uint64_t m = __ballot(want);
    if (m == 0ull) return 0ull;
    const uint32_t leader = (uint32_t)__builtin_ctzll(m);
    u64 base = 0ull;
    if (lane_index() == leader) base = atomicAdd(counter, (u64)__popcll(m));
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)base, (int)leader, kWave);
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(base >> 32), (int)leader, kWave);
    return (((u64)hi << 32) | lo) + mbcnt_add(m, 0u);
}

// One thread per segment: check, classify, list.  Lists are in no particular order (segments are independent); a large segment
// takes its tiles and its block of counts by atomic add, and the flat scan later reads where that block begins.
// Well-formed offsets never fill a table (the segments are disjoint).  Malformed ones can make checked segments overlap, and
// their sizes then sum beyond n: whatever does not fit is not listed (fault bit), and every reader clamps a count to its table.
__global__ void __launch_bounds__(256) seg_plan_kernel(const PlanParams p)
{
    // s0 is uniform, so every lane of a wave reaches the ballots of wave_append together
    for (uint32_t s0 = blockIdx.x * blockDim.x; s0 < p.segs; s0 += gridDim.x * blockDim.x) {
        const uint32_t s = s0 + threadIdx.x;
        uint32_t lo = 0u, hi = 0u;
        if (s < p.segs) {
            lo = p.offsets[s];
            hi = p.offsets[s + 1];
            if (hi < lo || hi > p.n) {
                atomicOr(p.ctl + kCtlFault, kSegFaultBit);
                lo = hi = 0u;
            }
        }
        const uint32_t size = hi - lo;
        const bool to_wave = p.local && size >= 2u && size <= (uint32_t)kWaveSegCap;
        const bool to_group = p.local && size > (uint32_t)kWaveSegCap && size <= (uint32_t)kLocalSortCap;
        const u64 at_wave = wave_append(p.cnt + kCntWave, to_wave);
        const u64 at_group = wave_append(p.cnt + kCntGroup, to_group);
        if (size < 2u) continue;
        bool fits = true;
        if (to_wave) {
            if (at_wave < p.wave_cap) p.wave_list[at_wave] = s;
            else fits = false;
        } else if (to_group) {
            if (at_group < p.group_cap) p.group_list[at_group] = s;
            else fits = false;
        } else {
            const uint32_t nt = (size + kSegTile - 1u) / kSegTile;
            const u64 first64 = atomicAdd(p.cnt + kCntTiles, (u64)nt);
            fits = first64 + nt <= p.tile_cap;
            const uint32_t first = (uint32_t)(first64 < p.tile_cap ? first64 : p.tile_cap);
            if (fits && nt == 1u) {
                p.tiles[first] = make_uint2(s, kOneTile);
            } else if (fits) {
                const u64 hf = atomicAdd(p.cnt + kCntHistTiles, (u64)nt);
                fits = hf + nt <= p.hist_cap;
                const u64 at = fits ? atomicAdd(p.cnt + kCntItems, 1ull) : p.item_cap;
                if (at < p.item_cap) p.items[at] = make_uint4(s, first, (uint32_t)hf, nt);
                else fits = false;
            }
            // tiles claimed inside the table but not listed: marked empty, so that nobody reads an unwritten entry
            if (!fits)
                for (uint32_t t = first; t < p.tile_cap && t - first < nt; t++) p.tiles[t] = make_uint2(0u, kSkipTile);
        }
        if (!fits) atomicOr(p.ctl + kCtlFault, kSegFaultBit);
    }
}

// the control block starts at zero (a kernel rather than a memset: one kind of node in a captured graph)
__global__ void __launch_bounds__(64) seg_clear_kernel(uint32_t* ctl)
{
    ctl[threadIdx.x] = 0u;
}

// the tile table's entries of the multi-tile segments: a workgroup per segment
__global__ void __launch_bounds__(256) seg_tiles_kernel(const PlanParams p)
{
    const uint32_t count = clamp_count(p.cnt[kCntItems], p.item_cap);
    for (uint32_t it = blockIdx.x; it < count; it += gridDim.x) {
        const uint4 item = p.items[it];
        for (uint32_t t = threadIdx.x; t < item.w; t += blockDim.x) p.tiles[item.y + t] = make_uint2(it, t);
    }
}

// ---- wave tier ------------------------------------------------------------------------------------------------------------
// One wavefront per segment of at most kWaveSegCap keys: lane l's register i holds position 64 i + l.  Per digit pass: zero the
// wave's 256 counters, rank = returning LDS add (lane order within a row, rows in order: stable), exclusive scan of the counters
// across the wave (four per lane), keys to LDS at base + rank, back in position order.  Only this wave touches its slice, and a
// wave's LDS operations are served in order: no barrier anywhere.
template <bool PAIRS>
__global__ void __launch_bounds__(kWaveTierWaves * kWave) seg_wave_kernel(const SegSortParams p)
{
    __shared__ uint32_t smem[kWaveTierWaves * kWaveSliceWords];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    lds_u32* const s_keys = (lds_u32*)smem + wave * kWaveSliceWords;
    volatile lds_u32* const s_cnt = (volatile lds_u32*)(s_keys + kWaveSegCap);
    const uint32_t listed = clamp_count(*p.list_count, p.list_cap);
    for (uint32_t item = blockIdx.x * kWaveTierWaves + wave; item < listed; item += gridDim.x * kWaveTierWaves) {
        const uint32_t s = p.list[item];
        if (s >= p.num_segments) {   // (uniform) never: the planner lists checked segments of 2 .. kWaveSegCap keys
            if (lane == 0u) atomicOr(p.fault, kSegFaultList);
            continue;
        }
        const uint32_t lo = p.offsets[s], hi = p.offsets[s + 1], size = hi - lo;
        if (hi < lo || hi > p.n || size > (uint32_t)kWaveSegCap) {
            if (lane == 0u) atomicOr(p.fault, kSegFaultList);
            continue;
        }
        uint32_t* const seg = p.keys + lo;
        uint32_t* const seg_vals = PAIRS ? p.vals + lo : nullptr;
        const uint32_t rows = (size + 63u) / 64u;
        uint32_t key[kWaveRows], rank[kWaveRows], val[PAIRS ? kWaveRows : 1];
        uint32_t any = 0u, all = ~0u;
#pragma unroll
        for (int i = 0; i < kWaveRows; i++) {
            const uint32_t pos = (uint32_t)i * 64u + lane;
            key[i] = 0xFFFFFFFFu;
            if ((uint32_t)i < rows && pos < size) {
                uint32_t k = seg[pos];
                if (p.xin.on) k = to_sortable(k, p.xin);
                key[i] = k;
                any |= k;
                all &= k;
                if (PAIRS) val[i] = seg_vals[pos];
            }
        }
        any = wave_or(any);
        all = wave_and(all);
        uint32_t todo = 0;   // bit b: digit b differs somewhere in the segment
#pragma unroll
        for (int b = 0; b < 4; b++) todo |= (((any ^ all) >> (8 * b)) & 0xFFu) ? 1u << b : 0u;
        while (todo) {
            const uint32_t shift = 8u * (uint32_t)__builtin_ctz(todo);
            todo &= todo - 1u;
            const bool last = todo == 0u;
#pragma unroll
            for (int j = 0; j < 4; j++) s_cnt[j * 64 + lane] = 0u;
            wave_sync();
#pragma unroll
            for (int i = 0; i < kWaveRows; i++) {
                if ((uint32_t)i < rows && (uint32_t)i * 64u + lane < size)
                    rank[i] = __hip_atomic_fetch_add((lds_u32*)&s_cnt[(key[i] >> shift) & 0xFFu], 1u, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_WAVEFRONT);
            }
            wave_sync();
            uint32_t c[4], sum = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                c[j] = s_cnt[lane * 4 + j];
                sum += c[j];
            }
            uint32_t base = wave_inclusive_scan(sum) - sum;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                s_cnt[lane * 4 + j] = base;
                base += c[j];
            }
            wave_sync();
#pragma unroll
            for (int i = 0; i < kWaveRows; i++) {
                if ((uint32_t)i < rows && (uint32_t)i * 64u + lane < size) {
                    const uint32_t q = s_cnt[(key[i] >> shift) & 0xFFu] + rank[i];
                    s_keys[q] = key[i];
                    rank[i] = q;
                }
            }
            wave_sync();
            if (last) {
                for (uint32_t q = lane; q < size; q += 64u) seg[q] = p.xout.on ? from_sortable(s_keys[q], p.xout) : s_keys[q];
            } else {
#pragma unroll
                for (int i = 0; i < kWaveRows; i++)
                    if ((uint32_t)i < rows && (uint32_t)i * 64u + lane < size) key[i] = s_keys[(uint32_t)i * 64u + lane];
            }
            if (PAIRS) {
                wave_sync();
#pragma unroll
                for (int i = 0; i < kWaveRows; i++)
                    if ((uint32_t)i < rows && (uint32_t)i * 64u + lane < size) s_keys[rank[i]] = val[i];
                wave_sync();
                if (last) {
                    for (uint32_t q = lane; q < size; q += 64u) seg_vals[q] = s_keys[q];
                } else {
#pragma unroll
                    for (int i = 0; i < kWaveRows; i++)
                        if ((uint32_t)i < rows && (uint32_t)i * 64u + lane < size) val[i] = s_keys[(uint32_t)i * 64u + lane];
                }
            }
            wave_sync();   // the next pass (or segment) writes this slice again
        }
    }
}

// ---- large tier -----------------------------------------------------------------------------------------------------------
struct LargeParams {
    const uint32_t* in;
    uint32_t* out;
    const uint32_t* vals_in;      // null: keys only
    uint32_t* vals_out;
    const uint32_t* offsets;
    const u64* cnt;
    const uint4* items;
    const uint2* tiles;
    uint32_t* hist;               // counts, then (in place) their flat exclusive scan
    uint32_t* sums;
    uint32_t tile_cap, hist_cap, item_cap;   // table sizes: counts are clamped to them
    uint32_t segs, n;
    uint32_t* fault;
    uint32_t shift;
    KeyTransform xin, xout;       // first pass / last pass
};

struct TileRef {
    uint32_t lo, size;            // keys [lo, lo + size) of the array
    uint32_t seg_lo, seg_size;
    uint32_t t, nt, hf;           // tile within segment, tiles of segment, first hist tile (nt > 1 only)
    bool ok;                      // false: an entry that does not describe a checked segment (never expected; skipped)
};
__device__ __forceinline__ TileRef tile_ref(const LargeParams& p, uint32_t j)
{
    const uint2 e = p.tiles[j];
    TileRef r{};
    uint32_t s;
    if (e.y == kOneTile) {
        s = e.x; r.t = 0u; r.nt = 1u; r.hf = 0u;
    } else {
        if (e.x >= p.item_cap) return r;
        const uint4 item = p.items[e.x];
        s = item.x; r.t = e.y; r.nt = item.w; r.hf = item.z;
        if (r.nt < 2u || r.t >= r.nt || r.hf > p.hist_cap || r.nt > p.hist_cap - r.hf) return r;
    }
    if (s >= p.segs) return r;
    r.seg_lo = p.offsets[s];
    const uint32_t seg_hi = p.offsets[s + 1];
    if (seg_hi < r.seg_lo || seg_hi > p.n) return r;
    r.seg_size = seg_hi - r.seg_lo;
    if ((r.seg_size + kSegTile - 1u) / kSegTile != r.nt) return r;
    r.lo = r.seg_lo + r.t * kSegTile;
    r.size = seg_hi - r.lo < kSegTile ? seg_hi - r.lo : kSegTile;
    r.ok = true;
    return r;
}

// hist[(hf + t) block layout]: entry (segment block, d, t) = hf * 256 + d * nt + t
__global__ void __launch_bounds__(kSegThreads) seg_hist_kernel(const LargeParams p)
{
    __shared__ uint32_t s_hist[256];
    const uint32_t tid = threadIdx.x, count = clamp_count(p.cnt[kCntTiles], p.tile_cap);
    for (uint32_t j = blockIdx.x; j < count; j += gridDim.x) {
        if (p.tiles[j].y >= kSkipTile) continue;   // uniform: a one-tile segment needs no counts
        const TileRef r = tile_ref(p, j);
        if (!r.ok) {   // uniform
            if (tid == 0u) atomicOr(p.fault, kSegFaultTile);
            continue;
        }
        s_hist[tid] = 0u;
        __syncthreads();
        for (uint32_t q = tid; q < r.size; q += kSegThreads) {
            uint32_t k = p.in[r.lo + q];
            if (p.xin.on) k = to_sortable(k, p.xin);
            atomicAdd(&s_hist[(k >> p.shift) & 0xFFu], 1u);
        }
        __syncthreads();
        p.hist[(size_t)r.hf * 256u + tid * r.nt + r.t] = s_hist[tid];
        __syncthreads();
    }
}

// flat exclusive scan of hist[0, hist tiles x 256): block sums, their scan (one workgroup), then each block in place
__global__ void __launch_bounds__(256) seg_scan_reduce_kernel(const LargeParams p)
{
    __shared__ uint32_t s_part[4];
    const uint32_t total = clamp_count(p.cnt[kCntHistTiles], p.hist_cap) * 256u, b0 = blockIdx.x * kScanBlock;
    if (b0 >= total) return;
    uint32_t sum = 0;
    for (uint32_t q = b0 + threadIdx.x; q < b0 + kScanBlock && q < total; q += 256u) sum += p.hist[q];
    sum = wave_sum(sum);
    if ((threadIdx.x & 63u) == 0u) s_part[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) p.sums[blockIdx.x] = s_part[0] + s_part[1] + s_part[2] + s_part[3];
}

__global__ void __launch_bounds__(1024) seg_scan_sums_kernel(const LargeParams p)
{
    __shared__ uint32_t s_part[16];
    const uint32_t total = clamp_count(p.cnt[kCntHistTiles], p.hist_cap) * 256u;
    const uint32_t blocks = (total + kScanBlock - 1u) / kScanBlock;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t carry = 0;
    for (uint32_t c0 = 0; c0 < blocks; c0 += 1024u) {
        const uint32_t q = c0 + tid;
        const uint32_t v = q < blocks ? p.sums[q] : 0u;
        uint32_t all = 0;
        const uint32_t before = group_exclusive_scan<16>(v, lane, wave, s_part, &all);
        if (q < blocks) p.sums[q] = carry + before;
        carry += all;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) seg_scan_down_kernel(const LargeParams p)
{
    constexpr uint32_t E = kScanBlock / 256u;   // consecutive entries per thread
    __shared__ uint32_t s_part[4];
    const uint32_t total = clamp_count(p.cnt[kCntHistTiles], p.hist_cap) * 256u, b0 = blockIdx.x * kScanBlock;
    if (b0 >= total) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t first = b0 + tid * E;
    uint32_t v[E], sum = 0;
#pragma unroll
    for (uint32_t e = 0; e < E; e++) {
        v[e] = first + e < total ? p.hist[first + e] : 0u;
        sum += v[e];
    }
    uint32_t run = p.sums[blockIdx.x] + group_exclusive_scan<4>(sum, lane, wave, s_part);
#pragma unroll
    for (uint32_t e = 0; e < E; e++) {
        if (first + e < total) p.hist[first + e] = run;
        run += v[e];
    }
}

// One tile per iteration: wave w holds tile positions [1024 w, 1024 (w + 1)), lane l's register i position 1024 w + 64 i + l.
// Rank within the wave (LDS_ADD: returning add, lane-ordered; otherwise 8 ballots and a wave-private count), wave bases per digit,
// keys into LDS in digit order, then out linearly: key at tile slot q with digit d goes to gdelta[d] + q.
template <bool PAIRS, bool LDS_ADD>
__global__ void __launch_bounds__(kSegThreads) seg_scatter_kernel(const LargeParams p)
{
    __shared__ uint32_t s_keys[kSegTile];
    __shared__ uint32_t s_vals[PAIRS ? kSegTile : 1];
    __shared__ uint32_t s_cnt_raw[kSegWaves * 256];
    __shared__ uint32_t s_gdelta[256];
    __shared__ uint32_t s_part[kSegWaves];
    volatile lds_u32* const s_cnt = (volatile lds_u32*)(lds_u32*)s_cnt_raw;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t count = clamp_count(p.cnt[kCntTiles], p.tile_cap);
    for (uint32_t j = blockIdx.x; j < count; j += gridDim.x) {
        if (p.tiles[j].y == kSkipTile) continue;   // uniform
        const TileRef r = tile_ref(p, j);
        if (!r.ok) {   // uniform
            if (tid == 0u) atomicOr(p.fault, kSegFaultTile);
            continue;
        }
        uint32_t key[kSegKeys], rank[kSegKeys], val[PAIRS ? kSegKeys : 1];
#pragma unroll
        for (int i = 0; i < kSegKeys; i++) {
            const uint32_t pos = wave * 1024u + (uint32_t)i * 64u + lane;
            key[i] = 0xFFFFFFFFu;
            if (pos < r.size) {
                uint32_t k = p.in[r.lo + pos];
                if (p.xin.on) k = to_sortable(k, p.xin);
                key[i] = k;
                if (PAIRS) val[i] = p.vals_in[r.lo + pos];
            }
        }
#pragma unroll
        for (int j4 = 0; j4 < 4; j4++) s_cnt[wave * 256 + j4 * 64 + lane] = 0u;
        wave_sync();
#pragma unroll
        for (int i = 0; i < kSegKeys; i++) {
            const bool valid = wave * 1024u + (uint32_t)i * 64u + lane < r.size;
            const uint32_t d = (key[i] >> p.shift) & 0xFFu;
            if (LDS_ADD) {
                if (valid)
                    rank[i] = __hip_atomic_fetch_add((lds_u32*)&s_cnt[wave * 256 + d], 1u, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_WAVEFRONT);
            } else {
                const uint64_t peers = match_ballot<8>(d) & __ballot(valid);
                const uint32_t rk = mbcnt_add(peers, s_cnt[wave * 256 + d]);
                wave_sync();
                if (valid && (peers >> lane) == 1ull) s_cnt[wave * 256 + d] = rk + 1u;   // the highest lane of its peers
                wave_sync();
                rank[i] = rk;
            }
        }
        __syncthreads();
        // thread d: wave bases inside the digit, the digit's offset in the tile, its global destination
        {
            const uint32_t d = tid;
            uint32_t wave_excl[kSegWaves], total = 0;
#pragma unroll
            for (int w = 0; w < kSegWaves; w++) {
                wave_excl[w] = total;
                total += s_cnt[w * 256 + d];
            }
            const uint32_t excl = group_exclusive_scan<kSegWaves>(total, lane, wave, s_part);
#pragma unroll
            for (int w = 0; w < kSegWaves; w++) s_cnt[w * 256 + d] = excl + wave_excl[w];
            uint32_t gbase;
            if (r.nt == 1u) {
                gbase = r.seg_lo + excl;
            } else {
                const size_t block = (size_t)r.hf * 256u;
                gbase = r.seg_lo + p.hist[block + d * r.nt + r.t] - p.hist[block];
            }
            s_gdelta[d] = gbase - excl;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kSegKeys; i++) {
            if (wave * 1024u + (uint32_t)i * 64u + lane < r.size) {
                const uint32_t q = s_cnt[wave * 256 + ((key[i] >> p.shift) & 0xFFu)] + rank[i];
                s_keys[q] = key[i];
                if (PAIRS) s_vals[q] = val[i];
            }
        }
        __syncthreads();
        for (uint32_t q = tid; q < r.size; q += kSegThreads) {
            const uint32_t k = s_keys[q];
            const uint32_t dst = s_gdelta[(k >> p.shift) & 0xFFu] + q;
            if (dst - r.seg_lo >= r.seg_size) {   // counts that do not describe the keys: never expected, never written
                atomicOr(p.fault, kSegFaultDest);
                continue;
            }
            p.out[dst] = p.xout.on ? from_sortable(k, p.xout) : k;
            if (PAIRS) p.vals_out[dst] = s_vals[q];
        }
        __syncthreads();   // the next tile reuses the LDS
    }
}

template <bool PAIRS>
hipError_t launch_scatter(bool lds_add, uint32_t grid, const LargeParams& lp, hipStream_t stream)
{
    if (lds_add) hipLaunchKernelGGL((seg_scatter_kernel<PAIRS, true>), dim3(grid), dim3(kSegThreads), 0, stream, lp);
    else hipLaunchKernelGGL((seg_scatter_kernel<PAIRS, false>), dim3(grid), dim3(kSegThreads), 0, stream, lp);
    return hipGetLastError();
}

int run_segmented(uint32_t* keys, uint32_t* vals, const uint32_t* offsets, size_t segs, size_t n, const KeyTransform& xf,
                  void* d_ws, size_t ws_bytes, hipStream_t stream)
{
    if (n > LSDSORT_MAX_KEYS || segs > LSDSORT_MAX_KEYS) return LSDSORT_ERR_TOO_LARGE;
    if (!keys || !offsets) return LSDSORT_ERR_INVALID_ARG;
    const bool pairs = vals != nullptr;
    const SegLayout L = seg_layout(n, segs, pairs);
    if (!workspace_ok(d_ws, ws_bytes, L.total)) return LSDSORT_ERR_WORKSPACE;
    int rank_method = 0;
    LSD_TRY(device_rank_method(8, &rank_method));
    const bool local = rank_method == kRankLdsAdd;

    char* ws = static_cast<char*>(d_ws);
    uint32_t* ctl = reinterpret_cast<uint32_t*>(ws);
    PlanParams pp{};
    pp.offsets = offsets;
    pp.segs = (uint32_t)segs;
    pp.n = (uint32_t)n;
    pp.local = local ? 1u : 0u;
    pp.ctl = ctl;
    pp.cnt = reinterpret_cast<u64*>(ws);
    pp.wave_list = reinterpret_cast<uint32_t*>(ws + L.wave_list);
    pp.group_list = reinterpret_cast<uint32_t*>(ws + L.group_list);
    pp.items = reinterpret_cast<uint4*>(ws + L.items);
    pp.tiles = reinterpret_cast<uint2*>(ws + L.tiles);
    pp.wave_cap = (uint32_t)min_sz(segs, n / 2);
    pp.group_cap = (uint32_t)min_sz(segs, n / (kWaveSegCap + 1));
    pp.item_cap = (uint32_t)L.max_items;
    pp.tile_cap = (uint32_t)L.max_tiles;
    pp.hist_cap = (uint32_t)L.max_hist_tiles;
    static_assert(kCtlBytes == 64 * sizeof(uint32_t), "one word per thread");
    hipLaunchKernelGGL(seg_clear_kernel, dim3(1), dim3(64), 0, stream, ctl);
    hipLaunchKernelGGL(seg_plan_kernel, dim3(grid_for(segs, 256, 2048)), dim3(256), 0, stream, pp);
    LSD_HIP(hipGetLastError());

    const size_t listed = min_sz(segs, n / 2);
    if (local) {
        SegSortParams sp{};
        sp.keys = keys;
        sp.vals = vals;
        sp.offsets = offsets;
        sp.xin = xf;
        sp.xout = xf;
        sp.num_segments = (uint32_t)segs;
        sp.n = (uint32_t)n;
        sp.fault = ctl + kCtlFault;
        sp.list = pp.wave_list;
        sp.list_count = pp.cnt + kCntWave;
        sp.list_cap = pp.wave_cap;
        const uint32_t wave_grid = grid_for(listed, kWaveTierWaves, 4096);   // measured: wider grids are slower (2.30 -> 2.50 ms at 2^20 x 256)
        if (pairs) hipLaunchKernelGGL(seg_wave_kernel<true>, dim3(wave_grid), dim3(kWaveTierWaves * kWave), 0, stream, sp);
        else hipLaunchKernelGGL(seg_wave_kernel<false>, dim3(wave_grid), dim3(kWaveTierWaves * kWave), 0, stream, sp);
        LSD_HIP(hipGetLastError());
        if (n > (size_t)kWaveSegCap) {
            sp.list = pp.group_list;
            sp.list_count = pp.cnt + kCntGroup;
            sp.list_cap = pp.group_cap;
            LSD_HIP(launch_segment_sort(sp, grid_for(min_sz(segs, n / (kWaveSegCap + 1)), 1, 512), stream));   // two per CU
        }
    }
    // the large tier: with the local tiers in force only segments above kLocalSortCap keys reach it
    const size_t smallest_large = local ? (size_t)kLocalSortCap + 1 : 2;
    if (n < smallest_large) return LSDSORT_OK;
    const size_t max_tiles = local ? n / kSegTile + n / smallest_large + 1 : L.max_tiles;
    hipLaunchKernelGGL(seg_tiles_kernel, dim3(grid_for(min_sz(segs, n / smallest_large) + 1, 1, 1024)), dim3(256), 0, stream, pp);
    LSD_HIP(hipGetLastError());
    // 64 x 2^22: 8.0 ms with 2048 workgroups walking the table, 6.9 with one per tile (whose empty launches cost 18 us each where no
    // segment is large), 7.07 with 16384
    const uint32_t tile_grid = grid_for(max_tiles, 1, 16384);
    const uint32_t scan_grid = grid_for(L.max_hist_tiles * 256, kScanBlock, 1u << 30);
    uint32_t* alt_keys = reinterpret_cast<uint32_t*>(ws + L.alt_keys);
    uint32_t* alt_vals = pairs ? reinterpret_cast<uint32_t*>(ws + L.alt_vals) : nullptr;
    for (int pass = 0; pass < 4; pass++) {
        LargeParams lp{};
        const bool even = (pass & 1) == 0;
        lp.in = even ? keys : alt_keys;
        lp.out = even ? alt_keys : keys;
        lp.vals_in = even ? vals : alt_vals;
        lp.vals_out = even ? alt_vals : vals;
        lp.offsets = offsets;
        lp.cnt = pp.cnt;
        lp.items = pp.items;
        lp.tiles = pp.tiles;
        lp.hist = reinterpret_cast<uint32_t*>(ws + L.hist);
        lp.sums = reinterpret_cast<uint32_t*>(ws + L.sums);
        lp.tile_cap = pp.tile_cap;
        lp.hist_cap = pp.hist_cap;
        lp.item_cap = pp.item_cap;
        lp.segs = (uint32_t)segs;
        lp.n = (uint32_t)n;
        lp.fault = ctl + kCtlFault;
        lp.shift = 8u * (uint32_t)pass;
        if (pass == 0) lp.xin = xf;
        if (pass == 3) lp.xout = xf;
        hipLaunchKernelGGL(seg_hist_kernel, dim3(tile_grid), dim3(kSegThreads), 0, stream, lp);
        hipLaunchKernelGGL(seg_scan_reduce_kernel, dim3(scan_grid), dim3(256), 0, stream, lp);
        hipLaunchKernelGGL(seg_scan_sums_kernel, dim3(1), dim3(1024), 0, stream, lp);
        hipLaunchKernelGGL(seg_scan_down_kernel, dim3(scan_grid), dim3(256), 0, stream, lp);
        LSD_HIP(hipGetLastError());
        LSD_HIP(pairs ? launch_scatter<true>(local, tile_grid, lp, stream) : launch_scatter<false>(local, tile_grid, lp, stream));
    }
    return LSDSORT_OK;
}

}  // namespace
}  // namespace lsd

extern "C" {

size_t lsdsort_segmented_workspace_bytes(size_t n, size_t num_segments, int pairs)
{
    if (n > LSDSORT_MAX_KEYS || num_segments > LSDSORT_MAX_KEYS) return 0;
    return lsd::seg_layout(n, num_segments, pairs != 0).total;
}

int lsdsort_segmented_device(void* d_keys, uint32_t* d_vals, const uint32_t* d_offsets, size_t num_segments, size_t n, int key_type,
                             int descending, void* d_workspace, size_t workspace_bytes, void* hip_stream)
{
    lsd::KeyTransform xf;
    LSD_TRY(lsd::key_transform(key_type, descending, &xf));
    if (n > LSDSORT_MAX_KEYS || num_segments > LSDSORT_MAX_KEYS) return LSDSORT_ERR_TOO_LARGE;
    if ((n > 0 || num_segments > 0) && (!d_keys || !d_offsets)) return LSDSORT_ERR_INVALID_ARG;
    if (n == 0 || num_segments == 0) return LSDSORT_OK;
    return lsd::run_segmented(static_cast<uint32_t*>(d_keys), d_vals, d_offsets, num_segments, n, xf, d_workspace, workspace_bytes,
                              static_cast<hipStream_t>(hip_stream));
}

}  // extern "C"
