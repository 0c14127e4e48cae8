// radix_select.hpp -- the counting radix SELECT of one key per row, once: what topk.hip, topk16.hip and kth.hip share.
//
// Most significant digit first: count the digit of the keys that still match the prefix found so far, walk the counts from the
// best end to the bin that holds the wanted key, append that bin's digit to the prefix, lower `need` by the keys in better bins,
// stop where the stop rule says the rest is decided.  Three size classes (those of segmented.hip, by cols): one wavefront per row
// and one workgroup per row (select_short: the row in registers, 8-bit digits in 256 LDS counters), and many chunks per row
// (clear_select, hist_level, scan_level: wider digits, kBins counters per row in the workspace, one launch per level and step).
// A unit brings how a tile is loaded and what marks a missing key (the counting functors; the loaders themselves are
// select_tiles16.hpp's and select_tiles32.hpp's), what it does with (prefix, shift, need) afterwards, its __global__ wrappers and
// its entries.  Internal linkage: every unit's kernels keep their own symbols.  The k-th value units also share their fault bits
// and the pick of their long rows, a kernel template that each of them instantiates under its own name (pick_rows_kernel).
#pragma once

#include <stddef.h>

#include "lsd_device.hpp"
#include "lsd_host.hpp"

namespace lsd {
namespace {

constexpr int kRegs = 16;                     // keys per lane of a tile
constexpr uint32_t kWaveTile = 64u * kRegs;   // keys of one wave's tile
constexpr uint32_t kBins = 2048;              // long rows: counters per row (11-bit digits)
constexpr uint32_t kLongThreads = 256, kLongWaves = kLongThreads / kWave, kLongTile = kLongThreads * kRegs;
constexpr uint32_t kMinChunk = 16384, kMaxChunks = 2048;

// ---- rows and chunks by address -------------------------------------------------------------------------------------------------
// One row by address: key p of the row is keys[p]; keys [0, head) lie in front of the row's first 16-byte line, the `body` keys
// from there on are keys[head + q], q < body, and q = kLineKeys g is the start of a 16-byte line.
template <class Key>
struct Row {
    static constexpr uint32_t kLineKeys = 16u / (uint32_t)sizeof(Key);
    const Key* keys;
    uint32_t head, body;
};
template <class Key>
__device__ __forceinline__ Row<Key> row_of(const Key* keys, uint32_t row, uint32_t cols)
{
    Row<Key> r;
    r.keys = keys + (size_t)row * cols;
    const uint32_t to_line = keys_to_line(r.keys);
    r.head = to_line < cols ? to_line : cols;
    r.body = cols - r.head;
    return r;
}

// Chunk c of a row is body positions [lo, hi) -- in EVERY kernel of a unit -- and chunk 0 owns the head keys as well.  A row whose
// head is not empty may leave its last chunk empty (lo == hi): the chunks are counted from cols.
struct ChunkRange {
    uint32_t lo, hi;
};
template <class Key>
__device__ __forceinline__ ChunkRange chunk_of(const Row<Key>& r, uint32_t chunk, uint32_t c)
{
    ChunkRange g;
    g.lo = c * chunk < r.body ? c * chunk : r.body;
    g.hi = r.body - g.lo < chunk ? r.body : g.lo + chunk;
    return g;
}

// ---- digit levels of the long rows and stop rules -------------------------------------------------------------------------------
struct Levels32 {   // 32-bit keys: 11, 11 and 10 bits
    static constexpr int kLevels = 3;
    static constexpr uint32_t kNoLevel = 32u;   // the shift of a row state no level has run on
    static constexpr uint32_t bits(int level) { return level == 2 ? 10u : 11u; }
    static constexpr uint32_t shift(int level) { return level == 0 ? 21u : (level == 1 ? 10u : 0u); }
};
struct Levels16 {   // 16-bit keys: 11 and 5 bits
    static constexpr int kLevels = 2;
    static constexpr uint32_t kNoLevel = 16u;
    static constexpr uint32_t bits(int level) { return level == 0 ? 11u : 5u; }
    static constexpr uint32_t shift(int level) { return level == 0 ? 5u : 0u; }
};

// `count` keys in the found bin, `need` of the keys under the new prefix wanted: is the rest decided?
struct StopTopk {   // every key under the prefix wins
    static __device__ __forceinline__ bool stops(uint32_t count, uint32_t need) { return count == need; }
};
struct StopKth {    // one key under the prefix: it is the one (the `need`-th of several equal-prefix keys is not yet known by value)
    static __device__ __forceinline__ bool stops(uint32_t count, uint32_t) { return count == 1u; }
};

// ---- short rows: the row in the registers of WAVES wavefronts -------------------------------------------------------------------
struct Selected {
    uint32_t prefix, shift, need;
};

// ROUNDS rounds of 8-bit digits from the top.  s_cnt: 256 counters, s_found: 3 words, both this row's own.  `count(round, shift,
// prefix, add)` calls add(key) for each of the caller's keys that exists and matches: every key in round 0, later those with
// ((key >> shift) >> 8) == prefix.  Counts that do not reach `need` raise `fault_bit` and select nothing: (0, 0, 0).
// `fault` is a reference to the caller's pointer so that it is read where the bit is raised, as in the hand-written loops: read at
// the call, the kernel-argument load moves in front of the loop and the short kernels' registers are allocated differently.
template <int WAVES, int ROUNDS, class Stop, class Count>
__device__ __forceinline__ Selected select_short(volatile lds_u32* s_cnt, volatile lds_u32* s_found, uint32_t wave, uint32_t lane,
                                                 uint32_t need, uint32_t* const& fault, uint32_t fault_bit, Count count)
{
    uint32_t prefix = 0u, shift = 8u * (uint32_t)(ROUNDS - 1);
#pragma unroll 1
    for (int round = 0; round < ROUNDS; round++) {
        shift = 8u * (uint32_t)(ROUNDS - 1) - 8u * (uint32_t)round;
        if (wave == 0u) {
#pragma unroll
            for (int j = 0; j < 4; j++) s_cnt[j * 64 + lane] = 0u;
            if (lane == 0u) s_found[0] = 0xFFFFFFFFu;
        }
        group_sync<WAVES>();
        count(round, shift, prefix, [&](uint32_t key) __attribute__((always_inline)) {
            __hip_atomic_fetch_add((lds_u32*)&s_cnt[(key >> shift) & 0xFFu], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        });
        group_sync<WAVES>();
        if (wave == 0u) {   // four bins per lane, from the best end
            uint32_t c[4], sum = 0u;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                c[j] = s_cnt[lane * 4u + j];
                sum += c[j];
            }
            uint32_t run = wave_inclusive_scan(sum) - sum;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if (run < need && need - run <= c[j]) {   // at most one bin of the row
                    s_found[0] = lane * 4u + j;
                    s_found[1] = run;
                    s_found[2] = c[j];
                }
                run += c[j];
            }
        }
        group_sync<WAVES>();
        const uint32_t bin = s_found[0], before = s_found[1], count_in_bin = s_found[2];
        group_sync<WAVES>();   // the next round writes s_found again
        if (bin > 0xFFu) {     // (uniform) the counts do not reach `need`: nothing is selected
            if (wave == 0u && lane == 0u) atomicOr(fault, fault_bit);
            prefix = 0u;
            shift = 0u;
            need = 0u;
            break;
        }
        prefix = (prefix << 8) | bin;
        need -= before;
        if (Stop::stops(count_in_bin, need)) break;   // uniform
    }
    return Selected{prefix, shift, need};
}

// ---- long rows: one launch per level and step -----------------------------------------------------------------------------------
// Row state in the workspace (uint4): x prefix, y shift (kNoLevel: no level has run), z need, w done (the select stopped: later
// levels return at once).

// control block, counters and row states of a call (a kernel rather than memsets: one kind of node in a captured graph)
__device__ __forceinline__ void clear_select(uint32_t at, uint32_t step, uint32_t* ctl, uint32_t* hist, uint32_t hist_words, uint4* state,
                                             uint32_t rows, uint32_t need, uint32_t no_level)
{
    if (at < (uint32_t)(kCtlBytes / 4)) ctl[at] = 0u;
    for (uint32_t q = at; q < hist_words; q += step) hist[q] = 0u;
    if (state)
        for (uint32_t r = at; r < rows; r += step) state[r] = make_uint4(0u, no_level, need, 0u);
}

// One chunk of one row per workgroup of kLongThreads: `count(row, c, st, lane, wave)` adds the digit of every key of chunk c under
// the row's prefix into s_hist (kBins LDS counters, count_digit); the non-zero ones are flushed into hist[row] by global atomics.
template <class LP, class Count>
__device__ __forceinline__ void hist_level(const LP& p, uint32_t* s_hist, Count count)
{
    const uint32_t row = blockIdx.x / p.chunks, c = blockIdx.x % p.chunks;
    if (row >= p.out.rows) return;
    const uint4 st = p.state[row];
    if (st.w != 0u) return;   // uniform
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for (uint32_t b = tid; b < kBins; b += kLongThreads) s_hist[b] = 0u;
    __syncthreads();
    count(row, c, st, lane, wave);
    __syncthreads();
    uint32_t* const out = p.hist + (size_t)row * kBins;
    for (uint32_t b = tid; b < kBins; b += kLongThreads) {
        const uint32_t v = s_hist[b];
        if (v != 0u) atomicAdd(out + b, v);
    }
}

// One workgroup of 256 per row: walk the bins from the best end to the one that holds the wanted key; the counters go back to
// zero.  s_part: 4 words, s_found: 3.  Counts that do not reach the row's need raise `fault_bit` and end the row's select.
template <class L, int LEVEL, class Stop, class LP>
__device__ __forceinline__ void scan_level(const LP& p, uint32_t* s_part, uint32_t* s_found, uint32_t fault_bit)
{
    const uint32_t row = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (row >= p.out.rows) return;
    const uint4 st = p.state[row];
    if (st.w != 0u) return;   // uniform
    uint32_t* const h = p.hist + (size_t)row * kBins;
    constexpr uint32_t E = kBins / 256u;
    uint32_t c[E], sum = 0u;
#pragma unroll
    for (uint32_t e = 0; e < E; e++) {
        c[e] = h[tid * E + e];
        h[tid * E + e] = 0u;
        sum += c[e];
    }
    if (tid == 0u) s_found[0] = 0xFFFFFFFFu;
    uint32_t run = group_exclusive_scan<4>(sum, lane, wave, s_part);
    const uint32_t need = st.z;
#pragma unroll
    for (uint32_t e = 0; e < E; e++) {
        if (run < need && need - run <= c[e]) {   // at most one bin of the row
            s_found[0] = tid * E + e;
            s_found[1] = run;
            s_found[2] = c[e];
        }
        run += c[e];
    }
    __syncthreads();
    if (tid != 0u) return;
    const uint32_t bin = s_found[0], before = s_found[1], count = s_found[2];
    // A found bin has a non-zero count, and the level's hist kernel counts under a mask of bits(LEVEL) bits: found means below
    // 1 << bits(LEVEL).  Otherwise s_found[0] is still 0xFFFFFFFF: kBins, every counter the walk reads, separates the two at
    // every level.
    if (bin >= kBins) {   // no bin of the walk: nothing is selected
        atomicOr(p.out.fault, fault_bit);
        p.state[row] = make_uint4(0u, 0u, 0u, 1u);
        return;
    }
    const uint32_t prefix = LEVEL == 0 ? bin : ((st.x << L::bits(LEVEL)) | bin);
    const uint32_t left = need - before;
    p.state[row] = make_uint4(prefix, L::shift(LEVEL), left, (LEVEL == L::kLevels - 1 || Stop::stops(count, left)) ? 1u : 0u);
}

// ---- the k-th value units: the pick of the long rows ------------------------------------------------------------------------------
constexpr uint32_t kKthFaultCount = 1024u;    // fault word: the digit counts of a row do not reach a rank (never expected)
// fault word: no key was located for a row or slot, or a values-only state is no whole value (never expected; nothing stored)
constexpr uint32_t kKthFaultLocate = 2048u;
constexpr uint32_t kNoChunk = 0xFFFFFFFFu;

// The kernels behind the levels that do not depend on the unit are kernel TEMPLATES, here, in select_tiles16.hpp and in
// kth_slots.hpp: a template is optimised once, as a kernel, so each instantiation is the code the unit's own kernel was (a shared
// device function is not: DESIGN.md section 6.14).  A unit names itself to them by a struct U of its own -- it is what tells two
// units' instantiations apart in a kernel trace, every LongParams being lsd::(anonymous)::LongParams:
//   U::Levels   Levels32 or Levels16
//   U::Params   the unit's LongParams
//   U::kBadW    single-rank units: the state w of a row that was refused from the start, 0 where the unit has no such rows;
//               U::kFaultBad (needed only where kBadW is not 0) is the bit such a row is reported by
//
// One workgroup per row: the chunk that holds the `need`-th key under the prefix, and which of that chunk's such keys it is.  A row
// that was refused from the start (kth16_rowk.hip: a rank outside the row) is reported here, by its own bit, and has nothing picked.
template <class U>
__global__ void __launch_bounds__(256) pick_rows_kernel(const typename U::Params p)
{
    __shared__ uint32_t s_part[4];
    __shared__ uint32_t s_found[2];
    const uint32_t row = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (row >= p.out.rows) return;
    const uint4 st = p.state[row];
    if constexpr (U::kBadW != 0u) {
        if (st.y == U::Levels::kNoLevel && st.w == U::kBadW) {   // uniform
            if (tid == 0u) {
                atomicOr(p.out.fault, U::kFaultBad);
                p.state[row] = make_uint4(0u, 0u, 0u, kNoChunk);
            }
            return;
        }
    }
    const uint32_t* const counts = p.counts + (size_t)row * p.chunk_cap;
    constexpr uint32_t E = kMaxChunks / 256u;
    uint32_t c[E], sum = 0u;
#pragma unroll
    for (uint32_t e = 0; e < E; e++) {
        c[e] = tid * E + e < p.chunks ? counts[tid * E + e] : 0u;
        sum += c[e];
    }
    if (tid == 0u) s_found[0] = kNoChunk;
    uint32_t run = group_exclusive_scan<4>(sum, lane, wave, s_part);
    const uint32_t need = st.y < U::Levels::kNoLevel ? st.z : 0u;
#pragma unroll
    for (uint32_t e = 0; e < E; e++) {
        if (run < need && need - run <= c[e]) {   // at most one chunk of the row
            s_found[0] = tid * E + e;
            s_found[1] = need - run;
        }
        run += c[e];
    }
    __syncthreads();
    if (tid != 0u) return;
    const uint32_t chunk = s_found[0];
    if (chunk == kNoChunk) {   // the keys under the prefix are fewer than `need`: nothing is located
        atomicOr(p.out.fault, kKthFaultLocate);
        p.state[row] = make_uint4(0u, 0u, 0u, kNoChunk);
        return;
    }
    p.state[row] = make_uint4(st.x, st.y, s_found[1], chunk);
}

// off[r] = r * stride, r <= rows: the rows as segments of the segmented sort
__device__ __forceinline__ void row_offsets(uint32_t at, uint32_t step, uint32_t* off, uint32_t rows, uint32_t stride)
{
    for (uint32_t r = at; r <= rows; r += step) off[r] = r * stride;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
// Long rows are cut into chunks of a multiple of kLongTile keys, about kMaxChunks of them over the whole array.
struct Chunks {
    uint32_t chunk, per_row;
};
Chunks chunks_for(size_t rows, size_t cols)
{
    const size_t n = rows * cols;
    size_t chunk = max_sz(kMinChunk, (n + kMaxChunks - 1) / kMaxChunks);
    chunk = (chunk + kLongTile - 1) / kLongTile * kLongTile;
    return Chunks{(uint32_t)chunk, (uint32_t)((cols + chunk - 1) / chunk)};
}
size_t chunk_cap_for(size_t cols) { return min_sz(kMaxChunks, (cols + kMinChunk - 1) / kMinChunk); }
// a [rows][cols] array a row entry takes: no more than LSDSORT_MAX_KEYS rows, and no more keys in all (no product that can overflow)
bool sizes_ok(size_t rows, size_t cols) { return rows <= LSDSORT_MAX_KEYS && (rows == 0 || cols <= LSDSORT_MAX_KEYS / rows); }

// The select's part of a workspace: control | row states | [offsets of rows + 1 segments] | counters [rows][kBins] | chunk counts
// of `count_bytes` each -- the last two for rows above kLocalSortCap keys only.  A unit's own arrays follow from `end`.
struct SelectLayout {
    size_t state, offsets, hist, counts, end;
};
SelectLayout select_layout(size_t rows, size_t cols, bool with_offsets, size_t count_bytes)
{
    SelectLayout L{};
    const bool is_long = cols > (size_t)kLocalSortCap;
    size_t off = kCtlBytes;
    L.state = off;    off = align_up(off + rows * 16);
    L.offsets = off;  off = align_up(off + (with_offsets ? (rows + 1) * 4 : 0));
    L.hist = off;     off = align_up(off + (is_long ? rows * kBins * 4 : 0));
    L.counts = off;   off = align_up(off + (is_long ? rows * chunk_cap_for(cols) * count_bytes : 0));
    L.end = off;
    return L;
}

// ---- the top-k units (topk.hip, topk16.hip) -------------------------------------------------------------------------------------
constexpr uint32_t kTopkFaultCount = 1024u;   // fault word: the digit counts of a row do not reach k (never expected)
constexpr uint32_t kTopkFaultDest = 2048u;    // fault word: a winner's slot is not below k (never expected; not stored)

// Top-k's sort route takes over where k * kLargeKDen > cols * kLargeKNum.  By bytes the 32-bit select route costs at most 20 B per
// key of the row plus the sort of k items, the sort route 12 B per key (copy with positions) plus the sort of the whole row and the
// gather: the select stays ahead until k is most of the row.  The 16-bit top-k inherits the 3/4: it is NOT
// tuned for 2-byte keys, where the select is cheaper still.
constexpr size_t kLargeKNum = 3, kLargeKDen = 4;
bool sort_route(size_t cols, size_t k) { return k * kLargeKDen > cols * kLargeKNum; }
// the most keys a sort-route call with this (rows, k) can have: it takes the sort route only if cols < 4 k / 3
size_t sort_route_keys(size_t rows, size_t cols, size_t k)
{
    return min_sz(min_sz(rows * cols, rows * ((k * kLargeKDen + kLargeKNum - 1) / kLargeKNum)), LSDSORT_MAX_KEYS);
}
// The sort route's workspace: control | offsets | `sort_keys` keys as uint32 | their positions | segmented sort of that many pairs.
struct SortRouteLayout {
    size_t offsets, keys, idx, seg, seg_bytes, total;
};
SortRouteLayout sort_route_layout(size_t rows, size_t sort_keys)
{
    SortRouteLayout L{};
    size_t off = kCtlBytes;
    L.offsets = off;  off = align_up(off + (rows + 1) * 4);
    L.keys = off;     off = align_up(off + sort_keys * 4);
    L.idx = off;      off = align_up(off + sort_keys * 4);
    L.seg = off;
    L.seg_bytes = lsdsort_segmented_workspace_bytes(sort_keys, rows, 1);
    L.total = align_up(off + L.seg_bytes);
    return L;
}

// The long rows' select: the fields every unit's LongParams has (keys, cols, chunk, chunks, chunk_cap, state, hist, counts) are
// filled from the layout, then the unit's clear kernel and, per level, its hist and scan kernels run.  Afterwards the row states
// hold (prefix, shift, need) and lp serves the unit's own kernels.  `clear(grid, block, ctl, hist, hist_words, state, rows)`
// launches the unit's clear kernel: the control block, the counters, and the row states at no level with the rows' needs.
template <class LP>
struct LevelKernels {
    void (*hist)(const LP);
    void (*scan)(const LP);
};
template <class LP, class Key, size_t LEVELS, class Clear>
int select_long(LP& lp, const Key* keys, size_t rows, size_t cols, char* ws, const SelectLayout& L, Clear clear,
                const LevelKernels<LP> (&levels)[LEVELS], hipStream_t stream)
{
    const Chunks ch = chunks_for(rows, cols);
    lp.keys = keys;
    lp.cols = (uint32_t)cols;
    lp.chunk = ch.chunk;
    lp.chunks = ch.per_row;
    lp.chunk_cap = (uint32_t)chunk_cap_for(cols);
    lp.state = reinterpret_cast<uint4*>(ws + L.state);
    lp.hist = reinterpret_cast<uint32_t*>(ws + L.hist);
    lp.counts = reinterpret_cast<decltype(lp.counts)>(ws + L.counts);
    if (lp.chunks > lp.chunk_cap) return LSDSORT_ERR_INVALID_ARG;   // never: chunks are at least kMinChunk keys
    clear(dim3(grid_for(rows * kBins, 1024, 4096)), dim3(256), reinterpret_cast<uint32_t*>(ws), lp.hist, (uint32_t)(rows * kBins), lp.state,
          (uint32_t)rows);
    for (const LevelKernels<LP>& level : levels) {
        hipLaunchKernelGGL(level.hist, dim3((uint32_t)(rows * lp.chunks)), dim3(kLongThreads), 0, stream, lp);
        hipLaunchKernelGGL(level.scan, dim3((uint32_t)rows), dim3(256), 0, stream, lp);
    }
    LSD_HIP(hipGetLastError());
    return LSDSORT_OK;
}
// one `need` for all rows, as a kernel argument: the clear kernel of topk.hip, topk16.hip, kth.hip and kth16.hip
using ClearKernel = void (*)(uint32_t*, uint32_t*, uint32_t, uint4*, uint32_t, uint32_t);
template <class LP, class Key, size_t LEVELS>
int select_long(LP& lp, const Key* keys, size_t rows, size_t cols, uint32_t need, char* ws, const SelectLayout& L, ClearKernel clear,
                const LevelKernels<LP> (&levels)[LEVELS], hipStream_t stream)
{
    auto launch = [&](dim3 grid, dim3 block, uint32_t* ctl, uint32_t* hist, uint32_t hist_words, uint4* state, uint32_t nrows) {
        hipLaunchKernelGGL(clear, grid, block, 0, stream, ctl, hist, hist_words, state, nrows, need);
    };
    return select_long(lp, keys, rows, cols, ws, L, launch, levels, stream);
}

}  // namespace
}  // namespace lsd
