// rows16.hip -- the stable sort of every row of a [rows x cols] array of 16-bit keys, with each key's position in its row
// (lsdsort_rows16_device).  The 16-bit sibling of the segmented sort for regular rows: the host knows every
// size, so nothing is planned on the device.
//
// No counterpart in the reference (it sorts one whole array of uint32, LSDRadixSort.cu:839-910).  The map of keys16_map.hpp is
// applied where a key is read and undone where it is stored.  An item travels as ONE word, sortable16 << 16 | index: the digit
// passes look at the key bytes only (shifts 16 and 24), the index rides for free, and a 16-bit key needs at most TWO 8-bit passes.
// Routes, by cols (the host chooses):
//   cols <= kWaveSegCap (1024)     wave tier: one wavefront per row, eight rows per workgroup, 16 items per lane, no workgroup barrier
//   cols <= kLocalSortCap (16384)  workgroup tier: one workgroup per row, 512 threads x 32 items
//                                  both: the row is read once as 2-byte keys into LDS, sorted there (a byte that is the same in
//                                  every key of the row is no pass), and leaves as 2-byte keys and 4-byte positions: 2 + 2 + 4 B/key
//   cols <= LSDSORT_ROWS16_NATIVE_MAX_COLS  long tier: two global LSD passes, low byte then high byte, over tiles of kLongTile
//                                  consecutive row positions.  Per pass: a histogram kernel (one workgroup per tile, counts laid out
//                                  [row][digit][tile]), a per-row scan (one workgroup per row: the rows are regular, so the
//                                  destination of a run is r cols + keys of the row with a smaller digit + keys of that digit in
//                                  earlier tiles), and a scatter kernel that sorts the tile by the digit in LDS and stores the runs.
//                                  Pass 1 reads the raw rows and writes a uint32 sortable key and a uint32 position per item into the
//                                  workspace; pass 2 reads those and writes the outputs.  2, 2 + 8, 4, 8 + 6 = 30 B/key.
//   longer rows, lsdsort_set_rows16_route(0), or the returning-LDS-add rank form not in force:
//                                  widen route: keys to sortable uint32 words with their positions in the workspace, the segmented
//                                  sort on the pairs, one kernel that un-maps and narrows.
// Ranking is the other tiers': one returning LDS add per key on wave-private counters, whose lane order the library probes.  A wave
// owns consecutive positions (register i of lane l: the wave's first position + 64 i + l), so ranks follow positions: stable.
// Key reads and writes: a row starts at any even address.  Every tile is split BY ITS ADDRESS into the keys in front of its first
// 16-byte line, whole groups of eight (one 16-byte access), and the keys behind the last whole group, one by one.
// d_out_keys may be d_keys: a row (local tiers), the whole array (long tier, widen route) is read before its first output is stored.
#define LSDSORT_BUILD 1
#include "../../include/lsdsort.h"

#include <atomic>

#include "keys16_map.hpp"
#include "lsd_device.hpp"
#include "lsd_host.hpp"

namespace lsd {
namespace {

// Rows of at least this many keys take the native route under the automatic rule (lsdsort_set_rows16_route(-1)).  1 = every row:
// the native route is ahead of the widen route in every class that was measured, the wave class included -- bfloat16 normal
// keys, descending, with positions: [2^20 x 256] 1.23 against 5.08 ms, [2^17 x 1024] 0.47 against 2.02, [2^14 x 2^14] 1.27 against
// 4.31, [1024 x 131072] 1.65 against 5.95 (profiles/rows16_perf.jsonl).  Rows below 256 keys: not measured.
constexpr size_t kRows16NativeMinCols = 1;

std::atomic<int> g_rows16_route{-1};   // lsdsort_set_rows16_route: -1 by size, 0 widen, 1 native wherever it exists

constexpr uint32_t kRowsFaultDest = 4096u;   // fault word: a destination outside its row (never expected; not stored)
constexpr uint32_t kPad = 0xFFFFFFFFu;       // an item that does not exist: the highest digit in every pass, at the highest positions
constexpr int kGroupThreads = 512, kGroupWaves = kGroupThreads / kWave;
constexpr int kWaveRegs = kWaveSegCap / kWave;                  // 16 items per lane
constexpr int kGroupRegs = kLocalSortCap / kGroupThreads;       // 32 items per thread
constexpr uint32_t kLongTile = 8192;                            // long tier: 512 threads x 16; keys AND positions of a tile in LDS
constexpr int kLongRegs = (int)kLongTile / kGroupThreads;
constexpr int kHistThreads = 256;
constexpr int kPlainThreads = 256;
constexpr int kMiscWords = 32;               // per group: the scan's partials [0, 8), OR of the keys [8, 16), AND [16, 24)
static_assert(LSDSORT_ROWS16_NATIVE_MAX_COLS >= 262144 && LSDSORT_ROWS16_NATIVE_MAX_COLS % kLongTile == 0, "the long tier's cap");
static_assert(kLongTile <= 65536 && kLocalSortCap <= 65536, "an index within a tile fits the low half-word");

// ---- a tile between global memory and LDS ---------------------------------------------------------------------------------------
// s_items[q] = sortable(src[q]) << 16 | q, q < size, by thread t of `threads`: 16-byte loads from the tile's first 16-byte line on.
__device__ __forceinline__ void stage_raw(const uint16_t* src, uint32_t size, const Key16Map& m, lds_u32* s_items, uint32_t t,
                                          uint32_t threads)
{
    const uint32_t to_line = keys_to_line(src);
    const uint32_t head = to_line < size ? to_line : size;
    const uint32_t groups = (size - head) / kGroupKeys, tail0 = head + groups * kGroupKeys;
    auto one = [&](uint32_t q) { s_items[q] = (to_sortable16(src[q], m) << 16) | q; };
    if (t < head) one(t);
    if (t < size - tail0) one(tail0 + t);
    for (uint32_t g = t; g < groups; g += threads) {
        const uint32_t q = head + g * kGroupKeys;
        const uint4 v = *reinterpret_cast<const uint4*>(src + q);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) {
            s_items[q + 2u * i] = (to_sortable16(w[i] & 0xFFFFu, m) << 16) | (q + 2u * i);
            s_items[q + 2u * i + 1u] = (to_sortable16(w[i] >> 16, m) << 16) | (q + 2u * i + 1u);
        }
    }
}

// The sorted row leaves: dst[q] = the key of s_items[q] in the caller's type, idx[q] (may be null) its low half-word, q < size.
__device__ __forceinline__ void store_row(const lds_u32* s_items, uint32_t size, const Key16Map& m, uint16_t* dst, uint32_t* idx, uint32_t t,
                                          uint32_t threads)
{
    const uint32_t to_line = keys_to_line(dst);
    const uint32_t head = to_line < size ? to_line : size;
    const uint32_t groups = (size - head) / kGroupKeys, tail0 = head + groups * kGroupKeys;
    auto key_at = [&](uint32_t q) { return from_sortable16(s_items[q] >> 16, m); };
    if (t < head) dst[t] = (uint16_t)key_at(t);
    if (t < size - tail0) dst[tail0 + t] = (uint16_t)key_at(tail0 + t);
    for (uint32_t g = t; g < groups; g += threads) {
        const uint32_t q = head + g * kGroupKeys;
        uint32_t w[4];
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) w[i] = key_at(q + 2u * i) | (key_at(q + 2u * i + 1u) << 16);
        *reinterpret_cast<uint4*>(dst + q) = make_uint4(w[0], w[1], w[2], w[3]);
    }
    if (idx)
        for (uint32_t q = t; q < size; q += threads) idx[q] = s_items[q] & 0xFFFFu;
}

// ---- the digit pass of a group of WAVES wavefronts over up to WAVES x 64 x K items in LDS ----------------------------------------
template <int WAVES, int K>
struct Group {
    lds_u32* s_items;             // [WAVES * 64 * K]
    volatile lds_u32* s_cnt;      // [WAVES][256]: counts, then bases
    lds_u32* s_misc;              // [kMiscWords]
    uint32_t tid, lane, wave;     // tid: the thread within the group
    uint32_t size, rows, wbase;   // rows = ceil(size / (WAVES * 64)), uniform, 1 .. K; register i: position wbase + 64 i
};
template <int WAVES, int K>
constexpr uint32_t group_words() { return (uint32_t)(WAVES * 64 * K + WAVES * 256 + kMiscWords); }

template <int WAVES, int K>
__device__ __forceinline__ Group<WAVES, K> group_at(uint32_t* smem, uint32_t size)
{
    Group<WAVES, K> g;
    g.lane = threadIdx.x & 63u;
    g.wave = WAVES == 1 ? 0u : threadIdx.x >> 6;
    g.tid = g.wave * 64u + g.lane;
    g.s_items = (lds_u32*)smem;
    g.s_cnt = (volatile lds_u32*)(g.s_items + WAVES * 64 * K);
    g.s_misc = (lds_u32*)(g.s_cnt + WAVES * 256);
    g.size = size;
    g.rows = (size + (uint32_t)(WAVES * 64) - 1u) / (uint32_t)(WAVES * 64);
    g.wbase = g.wave * g.rows * 64u + g.lane;
    return g;
}

// LDS -> registers in position order; past the end: kPad
template <int WAVES, int K>
__device__ __forceinline__ void read_items(const Group<WAVES, K>& g, uint32_t (&item)[K])
{
#pragma unroll
    for (int i = 0; i < K; i++) {
        item[i] = kPad;
        if ((uint32_t)i < g.rows) {
            const uint32_t pos = g.wbase + (uint32_t)i * 64u;
            if (pos < g.size) item[i] = g.s_items[pos];
        }
    }
}

// Which of the two key bytes differ somewhere in the group's items: bit 0 the low byte (shift 16), bit 1 the high byte (shift 24).
template <int WAVES, int K>
__device__ __forceinline__ uint32_t live_bytes(const Group<WAVES, K>& g, const uint32_t (&item)[K])
{
    uint32_t any = 0u, all = ~0u;
#pragma unroll
    for (int i = 0; i < K; i++) {
        if ((uint32_t)i < g.rows && g.wbase + (uint32_t)i * 64u < g.size) {
            any |= item[i];
            all &= item[i];
        }
    }
    any = wave_or(any);
    all = wave_and(all);
    if (WAVES > 1) {
        if (g.lane == 0u) {
            g.s_misc[8 + g.wave] = any;
            g.s_misc[16 + g.wave] = all;
        }
        __syncthreads();
#pragma unroll
        for (int w = 0; w < WAVES; w++) {
            any |= g.s_misc[8 + w];
            all &= g.s_misc[16 + w];
        }
    }
    const uint32_t differ = any ^ all;
    return ((differ >> 16) & 0xFFu ? 1u : 0u) | ((differ >> 24) ? 2u : 0u);
}

// One pass over item[] (position order) on the byte at `shift`: afterwards the items lie in s_items in their new order.  Items past
// the end take part as kPad and stay behind every real one.  s_start (may be null): [256] where each digit's run starts.
template <int WAVES, int K>
__device__ __forceinline__ void digit_pass(const Group<WAVES, K>& g, const uint32_t (&item)[K], uint32_t shift, lds_u32* s_start)
{
    volatile lds_u32* const mine = g.s_cnt + g.wave * 256u;
#pragma unroll
    for (int j = 0; j < 4; j++) mine[j * 64 + g.lane] = 0u;
    wave_sync();
    uint32_t rank[K];
#pragma unroll
    for (int i = 0; i < K; i++) {
        if ((uint32_t)i < g.rows)
            rank[i] = __hip_atomic_fetch_add((lds_u32*)&mine[(item[i] >> shift) & 0xFFu], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    }
    group_sync<WAVES>();
    if (WAVES == 1) {   // four digits per lane
        uint32_t c[4], sum = 0u;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            c[j] = mine[g.lane * 4u + j];
            sum += c[j];
        }
        uint32_t base = wave_inclusive_scan(sum) - sum;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            mine[g.lane * 4u + j] = base;
            if (s_start) s_start[g.lane * 4u + j] = base;
            base += c[j];
        }
    } else {            // one thread per digit: the waves' bases inside the digit's run, the runs by an exclusive scan
        uint32_t total = 0u, wave_excl[WAVES];
        if (g.tid < 256u) {
#pragma unroll
            for (int w = 0; w < WAVES; w++) {
                wave_excl[w] = total;
                total += g.s_cnt[w * 256 + g.tid];
            }
        }
        const uint32_t excl = group_exclusive_scan<WAVES>(total, g.lane, g.wave, g.s_misc);
        if (g.tid < 256u) {
#pragma unroll
            for (int w = 0; w < WAVES; w++) g.s_cnt[w * 256 + g.tid] = excl + wave_excl[w];
            if (s_start) s_start[g.tid] = excl;
        }
    }
    group_sync<WAVES>();
#pragma unroll
    for (int i = 0; i < K; i++) {
        if ((uint32_t)i < g.rows) g.s_items[mine[(item[i] >> shift) & 0xFFu] + rank[i]] = item[i];
    }
    group_sync<WAVES>();
}

// ---- wave and workgroup tiers ---------------------------------------------------------------------------------------------------
struct LocalParams {
    const uint16_t* keys;
    uint16_t* out_keys;
    uint32_t* out_idx;            // null: keys only
    uint32_t rows, cols;
    Key16Map map;
};

// WAVES = 1: a wavefront per row, eight rows in flight per workgroup; WAVES = 8: the workgroup per row.
template <int WAVES, int K>
__global__ void __launch_bounds__(kGroupThreads) rows16_local_kernel(const LocalParams p)
{
    constexpr uint32_t kGroups = WAVES == 1 ? (uint32_t)kGroupWaves : 1u;
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const uint32_t group = WAVES == 1 ? threadIdx.x >> 6 : 0u;
    const Group<WAVES, K> g = group_at<WAVES, K>(smem + group * group_words<WAVES, K>(), p.cols);
    // `row` is the same for every thread of a group (a wave, or the whole workgroup): its barriers are reached together
    for (uint32_t row = blockIdx.x * kGroups + group; row < p.rows; row += gridDim.x * kGroups) {
        const size_t at = (size_t)row * p.cols;
        stage_raw(p.keys + at, g.size, p.map, g.s_items, g.tid, (uint32_t)(WAVES * 64));
        group_sync<WAVES>();
        uint32_t item[K];
        read_items(g, item);
        uint32_t todo = live_bytes(g, item);   // uniform
        while (todo) {
            const uint32_t shift = 16u + 8u * (uint32_t)__builtin_ctz(todo);
            todo &= todo - 1u;
            digit_pass(g, item, shift, nullptr);
            if (todo) read_items(g, item);
        }
        store_row(g.s_items, g.size, p.map, p.out_keys + at, p.out_idx ? p.out_idx + at : nullptr, g.tid, (uint32_t)(WAVES * 64));
        group_sync<WAVES>();   // the next row is staged into the same LDS
    }
}

// ---- long tier ------------------------------------------------------------------------------------------------------------------
struct LongParams {
    const uint16_t* keys;
    uint16_t* out_keys;
    uint32_t* out_idx;            // null: keys only
    uint32_t* mid_key;            // [rows][cols] sortable values after pass 1
    uint32_t* mid_pos;            // [rows][cols] their positions
    uint32_t* hist;               // [rows][256][tiles]: counts, then (in place) where each tile's run of the digit starts in the row
    uint32_t rows, cols, tiles;   // tiles per row
    Key16Map map;
    uint32_t* fault;
};

// One tile per workgroup.  PASS 1: the low byte of the sortable value of the raw keys; PASS 2: the high byte of pass 1's output.
template <int PASS>
__global__ void __launch_bounds__(kHistThreads) rows16_hist_kernel(const LongParams p)
{
    __shared__ uint32_t s_hist[256];
    const uint32_t row = blockIdx.x / p.tiles, tile = blockIdx.x % p.tiles;
    if (row >= p.rows) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    s_hist[tid] = 0u;
    __syncthreads();
    const uint32_t lo = tile * kLongTile, size = p.cols - lo < kLongTile ? p.cols - lo : kLongTile;
    const size_t at = (size_t)row * p.cols + lo;
    if (PASS == 1) {
        const uint16_t* const src = p.keys + at;
        const uint32_t to_line = keys_to_line(src);
        const uint32_t head = to_line < size ? to_line : size;
        const uint32_t groups = (size - head) / kGroupKeys, tail0 = head + groups * kGroupKeys;
        if (tid < 64u) {   // wave 0: the keys outside the whole groups
            const bool in_head = lane < head, in_tail = lane >= 8u && lane - 8u < size - tail0;
            uint32_t k = 0u;
            if (in_head) k = src[lane];
            if (in_tail) k = src[tail0 + lane - 8u];
            count_digit(s_hist, in_head || in_tail, to_sortable16(k, p.map) & 0xFFu, lane);
        }
        for (uint32_t g0 = 0; g0 < groups; g0 += kHistThreads) {   // uniform
            const uint32_t g = g0 + tid;
            const bool valid = g < groups;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (valid) v = *reinterpret_cast<const uint4*>(src + head + g * kGroupKeys);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int i = 0; i < 4; i++) {
                count_digit(s_hist, valid, to_sortable16(w[i] & 0xFFFFu, p.map) & 0xFFu, lane);
                count_digit(s_hist, valid, to_sortable16(w[i] >> 16, p.map) & 0xFFu, lane);
            }
        }
    } else {
        const uint32_t* const src = p.mid_key + at;
        for (uint32_t q0 = 0; q0 < size; q0 += kHistThreads) {   // uniform
            const uint32_t q = q0 + tid;
            const bool valid = q < size;
            const uint32_t k = valid ? src[q] : 0u;
            count_digit(s_hist, valid, (k >> 8) & 0xFFu, lane);
        }
    }
    __syncthreads();
    p.hist[((size_t)row * 256u + tid) * p.tiles + tile] = s_hist[tid];
}

// One workgroup per row, one thread per digit: counts [digit][tile] -> the run's start within the row.
__global__ void __launch_bounds__(256) rows16_scan_kernel(const LongParams p)
{
    __shared__ uint32_t s_part[4];
    const uint32_t row = blockIdx.x, tid = threadIdx.x;
    if (row >= p.rows) return;
    uint32_t* const mine = p.hist + ((size_t)row * 256u + tid) * p.tiles;
    uint32_t total = 0u;
    for (uint32_t t = 0; t < p.tiles; t++) total += mine[t];
    uint32_t run = group_exclusive_scan<4>(total, tid & 63u, tid >> 6, s_part);
    for (uint32_t t = 0; t < p.tiles; t++) {
        const uint32_t v = mine[t];
        mine[t] = run;
        run += v;
    }
}

template <int PASS>
constexpr uint32_t scatter_words() { return group_words<kGroupWaves, kLongRegs>() + 512u + (PASS == 2 ? kLongTile : 0u); }

// One tile per workgroup: the tile sorted by the pass's digit in LDS, then the runs of each digit stored where the scan says.
// In LDS an item is sortable << 16 | its index within the tile; the position rides beside it in the workspace (pass 1 writes
// tile start + index, pass 2 looks the index up in s_pos).
template <int PASS>
__global__ void __launch_bounds__(kGroupThreads) rows16_scatter_kernel(const LongParams p)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const uint32_t row = blockIdx.x / p.tiles, tile = blockIdx.x % p.tiles;
    if (row >= p.rows) return;
    const uint32_t lo = tile * kLongTile, size = p.cols - lo < kLongTile ? p.cols - lo : kLongTile;
    const size_t row_at = (size_t)row * p.cols, at = row_at + lo;
    const Group<kGroupWaves, kLongRegs> g = group_at<kGroupWaves, kLongRegs>(smem, size);
    lds_u32* const s_start = g.s_misc + kMiscWords;
    lds_u32* const s_gdelta = s_start + 256;
    lds_u32* const s_pos = s_gdelta + 256;   // PASS 2 only
    uint32_t item[kLongRegs];
    if (PASS == 1) {
        stage_raw(p.keys + at, size, p.map, g.s_items, g.tid, (uint32_t)kGroupThreads);
        __syncthreads();
        read_items(g, item);
    } else {
#pragma unroll
        for (int i = 0; i < kLongRegs; i++) {
            item[i] = kPad;
            if ((uint32_t)i < g.rows) {
                const uint32_t pos = g.wbase + (uint32_t)i * 64u;
                if (pos < size) {
                    item[i] = (p.mid_key[at + pos] << 16) | pos;
                    s_pos[pos] = p.mid_pos[at + pos];
                }
            }
        }
    }
    constexpr uint32_t shift = PASS == 1 ? 16u : 24u;
    digit_pass(g, item, shift, s_start);   // its barriers also put s_pos and s_start behind us
    if (g.tid < 256u) s_gdelta[g.tid] = p.hist[((size_t)row * 256u + g.tid) * p.tiles + tile] - s_start[g.tid];
    __syncthreads();
    for (uint32_t q = g.tid; q < size; q += (uint32_t)kGroupThreads) {
        const uint32_t w = g.s_items[q];
        const uint32_t dst = s_gdelta[(w >> shift) & 0xFFu] + q;
        if (dst >= p.cols) {   // counts that do not describe the keys: never expected, never written
            atomicOr(p.fault, kRowsFaultDest);
            continue;
        }
        if (PASS == 1) {
            p.mid_key[row_at + dst] = w >> 16;
            p.mid_pos[row_at + dst] = lo + (w & 0xFFFFu);
        } else {
            p.out_keys[row_at + dst] = (uint16_t)from_sortable16(w >> 16, p.map);
            if (p.out_idx) p.out_idx[row_at + dst] = s_pos[w & 0xFFFFu];
        }
    }
}

// ---- widen route ----------------------------------------------------------------------------------------------------------------
// the control block starts at zero (a kernel rather than a memset: one kind of node in a captured graph)
__global__ void __launch_bounds__(64) rows16_clear_kernel(uint32_t* ctl)
{
    ctl[threadIdx.x] = 0u;
}

// every key widened to its sortable value with its position in its row beside it, and the rows as segments: off[r] = r cols
__global__ void __launch_bounds__(kPlainThreads) rows16_widen_kernel(const uint16_t* __restrict__ keys, uint32_t n, uint32_t rows, uint32_t cols,
                                                                    Key16Map m, uint32_t* __restrict__ wide, uint32_t* __restrict__ idx,
                                                                    uint32_t* __restrict__ off)
{
    const uint32_t first = blockIdx.x * blockDim.x + threadIdx.x, step = gridDim.x * blockDim.x;
    for (uint32_t r = first; r <= rows; r += step) off[r] = r * cols;
    for (uint32_t q = first; q < n; q += step) {
        wide[q] = to_sortable16(keys[q], m);
        if (idx) idx[q] = q % cols;
    }
}

// un-map, narrow, and the positions where the caller wants them
__global__ void __launch_bounds__(kPlainThreads) rows16_finish_kernel(const uint32_t* __restrict__ sorted, const uint32_t* __restrict__ pos, uint32_t n,
                                                                     Key16Map m, uint16_t* __restrict__ out_keys, uint32_t* __restrict__ out_idx)
{
    for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < n; q += gridDim.x * blockDim.x) {
        out_keys[q] = (uint16_t)from_sortable16(sorted[q] & 0xFFFFu, m);
        if (out_idx) out_idx[q] = pos[q];
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
size_t tiles_for(size_t cols) { return (cols + kLongTile - 1) / kLongTile; }

// Workspace.  Widen route: control | offsets | the widened keys | their positions | the segmented sort of rows x cols pairs.
// Native routes: control | counts [rows][256][tiles] | pass 1's keys | pass 1's positions (the local tiers use the control block
// alone).  The figure is the larger of the two whatever the route: a caller's buffer serves both.
struct Rows16Layout {
    size_t w_offsets, w_keys, w_idx, w_seg, w_seg_bytes, w_total;   // widen route
    size_t hist, mid_key, mid_pos, n_total;                         // long tier
    size_t total;
};
Rows16Layout rows16_layout(size_t rows, size_t cols)
{
    Rows16Layout L{};
    const size_t n = rows * cols;
    size_t off = kCtlBytes;
    L.w_offsets = off;  off = align_up(off + (rows + 1) * 4);
    L.w_keys = off;     off = align_up(off + n * 4);
    L.w_idx = off;      off = align_up(off + n * 4);
    L.w_seg = off;
    L.w_seg_bytes = lsdsort_segmented_workspace_bytes(n, rows, 1);
    L.w_total = align_up(off + L.w_seg_bytes);
    off = kCtlBytes;
    L.hist = off;       off = align_up(off + rows * 256 * tiles_for(cols) * 4);
    L.mid_key = off;    off = align_up(off + n * 4);
    L.mid_pos = off;    off = align_up(off + n * 4);
    L.n_total = off;
    L.total = L.w_total > L.n_total ? L.w_total : L.n_total;
    return L;
}

int run_widen(const uint16_t* keys, size_t rows, size_t cols, const Key16Map& map, uint16_t* out_keys, uint32_t* out_idx, char* ws,
              const Rows16Layout& L, hipStream_t stream)
{
    uint32_t* const ctl = reinterpret_cast<uint32_t*>(ws);
    uint32_t* const offsets = reinterpret_cast<uint32_t*>(ws + L.w_offsets);
    uint32_t* const wide = reinterpret_cast<uint32_t*>(ws + L.w_keys);
    uint32_t* const idx = out_idx ? reinterpret_cast<uint32_t*>(ws + L.w_idx) : nullptr;
    const size_t n = rows * cols;
    const uint32_t grid = grid_for(n > rows + 1 ? n : rows + 1, 1024, 8192);
    static_assert(kCtlBytes == 64 * sizeof(uint32_t), "one word per thread");
    hipLaunchKernelGGL(rows16_clear_kernel, dim3(1), dim3(64), 0, stream, ctl);
    hipLaunchKernelGGL(rows16_widen_kernel, dim3(grid), dim3(kPlainThreads), 0, stream, keys, (uint32_t)n, (uint32_t)rows, (uint32_t)cols, map,
                       wide, idx, offsets);
    LSD_HIP(hipGetLastError());
    LSD_TRY(lsdsort_segmented_device(wide, idx, offsets, rows, n, LSDSORT_KEY_U32, 0, ws + L.w_seg, L.w_seg_bytes, stream));
    hipLaunchKernelGGL(rows16_finish_kernel, dim3(grid), dim3(kPlainThreads), 0, stream, static_cast<const uint32_t*>(wide),
                       static_cast<const uint32_t*>(idx), (uint32_t)n, map, out_keys, out_idx);
    LSD_HIP(hipGetLastError());
    LSD_HIP(launch_keep_fault(ctl, reinterpret_cast<const uint32_t*>(ws + L.w_seg), stream));
    return LSDSORT_OK;
}

int run_native(const uint16_t* keys, size_t rows, size_t cols, const Key16Map& map, uint16_t* out_keys, uint32_t* out_idx, char* ws,
               const Rows16Layout& L, hipStream_t stream)
{
    uint32_t* const ctl = reinterpret_cast<uint32_t*>(ws);
    hipLaunchKernelGGL(rows16_clear_kernel, dim3(1), dim3(64), 0, stream, ctl);
    LSD_HIP(hipGetLastError());
    if (cols <= (size_t)kLocalSortCap) {
        const LocalParams lp{keys, out_keys, out_idx, (uint32_t)rows, (uint32_t)cols, map};
        if (cols <= (size_t)kWaveSegCap) {
            constexpr size_t lds = (size_t)kGroupWaves * group_words<1, kWaveRegs>() * sizeof(uint32_t);
            LSD_HIP((launch_dynamic_lds<rows16_local_kernel<1, kWaveRegs>>(dim3(grid_for(rows, kGroupWaves, 4096)), dim3(kGroupThreads), lds,
                                                                           stream, lp)));
        } else {
            constexpr size_t lds = (size_t)group_words<kGroupWaves, kGroupRegs>() * sizeof(uint32_t);
            LSD_HIP((launch_dynamic_lds<rows16_local_kernel<kGroupWaves, kGroupRegs>>(dim3(grid_for(rows, 1, 4096)), dim3(kGroupThreads), lds,
                                                                                      stream, lp)));
        }
        return LSDSORT_OK;
    }
    LongParams p{};
    p.keys = keys;
    p.out_keys = out_keys;
    p.out_idx = out_idx;
    p.mid_key = reinterpret_cast<uint32_t*>(ws + L.mid_key);
    p.mid_pos = reinterpret_cast<uint32_t*>(ws + L.mid_pos);
    p.hist = reinterpret_cast<uint32_t*>(ws + L.hist);
    p.rows = (uint32_t)rows;
    p.cols = (uint32_t)cols;
    p.tiles = (uint32_t)tiles_for(cols);
    p.map = map;
    p.fault = ctl;
    const dim3 tile_grid((uint32_t)(rows * p.tiles)), row_grid((uint32_t)rows);
    hipLaunchKernelGGL(rows16_hist_kernel<1>, tile_grid, dim3(kHistThreads), 0, stream, p);
    hipLaunchKernelGGL(rows16_scan_kernel, row_grid, dim3(256), 0, stream, p);
    LSD_HIP(hipGetLastError());
    LSD_HIP((launch_dynamic_lds<rows16_scatter_kernel<1>>(tile_grid, dim3(kGroupThreads), scatter_words<1>() * sizeof(uint32_t), stream, p)));
    hipLaunchKernelGGL(rows16_hist_kernel<2>, tile_grid, dim3(kHistThreads), 0, stream, p);
    hipLaunchKernelGGL(rows16_scan_kernel, row_grid, dim3(256), 0, stream, p);
    LSD_HIP(hipGetLastError());
    LSD_HIP((launch_dynamic_lds<rows16_scatter_kernel<2>>(tile_grid, dim3(kGroupThreads), scatter_words<2>() * sizeof(uint32_t), stream, p)));
    return LSDSORT_OK;
}

}  // namespace
}  // namespace lsd

extern "C" {

int lsdsort_set_rows16_route(int route)
{
    if (route < -1 || route > 1) return LSDSORT_ERR_INVALID_ARG;
    lsd::g_rows16_route.store(route, std::memory_order_relaxed);
    return LSDSORT_OK;
}

size_t lsdsort_rows16_workspace_bytes(size_t rows, size_t cols)
{
    if (rows > LSDSORT_MAX_KEYS || cols > LSDSORT_MAX_KEYS) return 0;
    if (rows != 0 && cols > LSDSORT_MAX_KEYS / rows) return 0;
    return lsd::rows16_layout(rows, cols).total;
}

int lsdsort_rows16_device(const void* d_keys, size_t rows, size_t cols, int key_type, int descending, void* d_out_keys, uint32_t* d_out_idx,
                          void* d_workspace, size_t workspace_bytes, void* hip_stream)
{
    Key16Map map;
    LSD_TRY(key16_map(key_type, descending, &map));
    if (rows > LSDSORT_MAX_KEYS || (rows != 0 && cols > LSDSORT_MAX_KEYS / rows)) return LSDSORT_ERR_TOO_LARGE;
    if (rows == 0 || cols == 0) return LSDSORT_OK;
    if (!d_keys || !d_out_keys || (((uintptr_t)d_keys | (uintptr_t)d_out_keys) & 1)) return LSDSORT_ERR_INVALID_ARG;
    const lsd::Rows16Layout L = lsd::rows16_layout(rows, cols);
    if (!lsd::workspace_ok(d_workspace, workspace_bytes, L.total)) return LSDSORT_ERR_WORKSPACE;
    int rank_method = 0;
    LSD_TRY(lsd::device_rank_method(8, &rank_method));
    const int route = lsd::g_rows16_route.load(std::memory_order_relaxed);
    const bool exists = cols <= (size_t)LSDSORT_ROWS16_NATIVE_MAX_COLS && rank_method == lsd::kRankLdsAdd;
    const bool native = exists && (route == 1 || (route == -1 && cols >= lsd::kRows16NativeMinCols));
    return (native ? lsd::run_native : lsd::run_widen)(static_cast<const uint16_t*>(d_keys), rows, cols, map, static_cast<uint16_t*>(d_out_keys),
                                                       d_out_idx, static_cast<char*>(d_workspace), L, static_cast<hipStream_t>(hip_stream));
}

}  // extern "C"
