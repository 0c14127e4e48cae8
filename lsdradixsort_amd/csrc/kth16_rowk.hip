// kth16_rowk.hip -- the 16-bit row selects with a k of their own for EVERY row, read from device memory:
//   lsdsort_kth16_perrow_device    kth16.hip's contract with row r's rank in d_ranks[r]
//   lsdsort_topk16_filter_device   the top-k filter of a sampling step: row r keeps the keys at least as good as its k_r-th best
//                                  (every duplicate of that value included), the others become `fill_bits`
// A batch of requests with mixed top_k is one call, and a captured graph follows a changed k: the values are read by the kernels,
// never by the host, and no launch is sized from them.
//
// No counterpart in the reference (it sorts one whole array of uint32, LSDRadixSort.cu:839-910).  The select is radix_select.hpp's
// with Levels16, in kth16.hip's three size classes:
//   cols <= kWaveSegCap (1024)      one wavefront per row, eight rows per workgroup; `need` is loaded once per row, uniformly
//   cols <= kLocalSortCap (16384)   one workgroup of 16 wavefronts per row: the same
//   longer                          many workgroups per row.  select_long launches this unit's clear kernel, which writes the row
//                                   states from the device array, then the two levels.  Per-row rank: count, pick and locate, or
//                                   without an index buffer both levels and the value kernel, as in kth16.hip.
//                                   Filter: both levels (the state then holds the whole threshold), then ONE apply kernel over the
//                                   same chunks reads a tile, compares and stores.
// The filter's short kernels compare and store the registers the select ran on: one read and one write of the row (4 B/key by byte
// accounting; long rows 2 reads + 1 read + 1 write = 8 B/key).  A kept key is stored as from_sortable16(to_sortable16(key)), which
// is the key bit for bit (the map is a bijection of the 16-bit words).  A row is stored by 16-byte groups where source and
// destination rows share their 16-byte phase (in place always), otherwise key by key.  In place every position is read and written by
// the same lane, a row's select has ended before its first store (registers in the short tiers, a kernel boundary in the long one).
//
// A rank outside its row cannot be refused by the host.  Such a row of the per-row entry stores nothing, raises kRowkFaultRank and
// no other bit, and leaves every other row as it is: short tiers skip the row; the clear kernel gives a long one a done state
// (w = kBadRow) that hist, scan, count and locate pass over, and the kernel that would have reported "nothing located" for it
// (pick, or the value kernel) reports kRowkFaultRank instead.  The filter has no such rank: k_r == 0 or k_r >= cols is "filter
// off" (state w = kOffRow), the row is copied, or left alone in place.
//
// The loaders, locate_tile, the filter's stores, the hist-level body and the value kernel's body are select_tiles16.hpp's, shared
// with the other 16-bit row selects.  The count, pick and locate kernels are kth16.hip's too: kernel templates (count_rows16_kernel
// and locate_rows16_kernel there, pick_rows_kernel in radix_select.hpp), the pick with this unit's bad-rank branch in front, behind
// `if constexpr` on the unit.  Every launch is sized from (rows,
// cols) and from whether an index buffer was given; phases are ordered by kernel boundaries; every store into the outputs is guarded
// by row < rows and stays within the row.  Nothing here ranks with the returning add: the result does not depend on
// lsdsort_set_rank_method.
#define LSDSORT_BUILD 1
#include "../../include/lsdsort.h"

#include "keys16_map.hpp"
#include "lsd_device.hpp"
#include "lsd_host.hpp"
#include "radix_select.hpp"
#include "select_tiles16.hpp"

namespace lsd {
namespace {

constexpr uint32_t kRowkFaultRank = 4096u;     // fault word: d_ranks[r] >= cols for some row (the caller's error; nothing stored for it)
constexpr uint32_t kBadRow = 2u, kOffRow = 3u; // row state w: done from the start (1: the select stopped or fell short)

struct Outputs {
    uint16_t* keys;       // [rows], the caller's 16-bit words
    uint32_t* idx;        // [rows] positions, may be null
    uint32_t rows;
    uint32_t* fault;
    __device__ __forceinline__ size_t at(uint32_t row, uint32_t) const { return row; }   // locate_tile's store: one slot per row
};

// ---- short rows: one wavefront (WAVES = 1, eight rows per workgroup) or one workgroup (WAVES = 16) per row ----------------------
struct ShortParams {
    const uint16_t* keys;
    const uint32_t* ranks;   // [rows], device: the 0-based rank (per-row entry) or k (filter) of every row
    uint32_t cols;
    Key16Map map;
    Outputs out;             // the filter: rows and fault only
    uint16_t* dst;           // the filter: [rows][cols], may be `keys`
    uint32_t fill;
};

template <int WAVES>
__global__ void __launch_bounds__(WAVES == 1 ? 512 : 1024) kth16r_short_kernel(const ShortParams p)
{
    constexpr int kGroups = WAVES == 1 ? 8 : 1;      // rows in flight per workgroup
    constexpr int kSlice = 256 + 8 + WAVES;          // per row: digit counters, the found bin, per-wave counts
    __shared__ uint32_t smem[kGroups * kSlice];
    const uint32_t lane = threadIdx.x & 63u, wave_of_block = threadIdx.x >> 6;
    const uint32_t group = WAVES == 1 ? wave_of_block : 0u, wave = WAVES == 1 ? 0u : wave_of_block;
    volatile lds_u32* const s_cnt = (volatile lds_u32*)((lds_u32*)smem + group * kSlice);
    volatile lds_u32* const s_found = s_cnt + 256;
    volatile lds_u32* const s_wc = s_cnt + 264;
    // `row` is the same for every thread of a group (a wave, or the whole workgroup): its barriers are reached together
    for (uint32_t row = blockIdx.x * kGroups + group; row < p.out.rows; row += gridDim.x * kGroups) {
        const uint32_t rank_load = p.ranks[row];   // issued in front of the row's loads and used behind them: no wait of its own
        const Row16 r = row_of(p.keys, row, p.cols);
        const uint32_t q0 = wave * kWaveTile;
        uint32_t t[kRegs];
        load_tile(r, q0, r.body, lane, p.map, t);
        const uint32_t h = wave == 0u ? load_head(r, lane, p.map) : kNoKey;
        const uint32_t rank = (uint32_t)__builtin_amdgcn_readfirstlane((int)rank_load);   // one value per row
        if (rank >= p.cols) {   // (uniform) the caller's error: nothing is stored for the row, and no other bit is raised
            if (wave == 0u && lane == 0u) atomicOr(p.out.fault, kRowkFaultRank);
            continue;
        }
        // round 0: every key there is; round 1: those whose top byte is the prefix (kNoKey never is)
        auto count = [&](int round, uint32_t, uint32_t prefix, auto add) __attribute__((always_inline)) {
            auto one = [&](uint32_t key) __attribute__((always_inline)) {
                if (round == 0 ? key != kNoKey : (key >> 8) == prefix) add(key);
            };
#pragma unroll
            for (int i = 0; i < kRegs; i++) one(t[i]);
            one(h);
        };
        const Selected sel = select_short<WAVES, 2, StopKth>(s_cnt, s_found, wave, lane, rank + 1u, p.out.fault, kKthFaultCount, count);
        uint32_t base = 0u;
        const bool found = locate_tile<WAVES>(t, h, q0, r, sel.prefix, sel.shift, sel.need, base, s_wc, wave, lane, row, 0u, p.out, p.map);
        if (!found && sel.need != 0u && wave == 0u && lane == 0u) atomicOr(p.out.fault, kKthFaultLocate);
        group_sync<WAVES>();
    }
}

// The filter: the select at need = k_r, then the same registers are compared and stored.  Where the select stopped with one key
// under a prefix of fewer than 16 bits, that key is the threshold and (key >> shift) <= prefix keeps exactly the keys up to it.
template <int WAVES>
__global__ void __launch_bounds__(WAVES == 1 ? 512 : 1024) topk16f_short_kernel(const ShortParams p)
{
    constexpr int kGroups = WAVES == 1 ? 8 : 1;
    constexpr int kSlice = 256 + 8;                  // per row: digit counters, the found bin
    __shared__ uint32_t smem[kGroups * kSlice];
    const uint32_t lane = threadIdx.x & 63u, wave_of_block = threadIdx.x >> 6;
    const uint32_t group = WAVES == 1 ? wave_of_block : 0u, wave = WAVES == 1 ? 0u : wave_of_block;
    volatile lds_u32* const s_cnt = (volatile lds_u32*)((lds_u32*)smem + group * kSlice);
    volatile lds_u32* const s_found = s_cnt + 256;
    const bool in_place = p.dst == p.keys;
    for (uint32_t row = blockIdx.x * kGroups + group; row < p.out.rows; row += gridDim.x * kGroups) {
        const uint32_t k = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.ranks[row]);   // one value per row
        const bool off = k == 0u || k >= p.cols;   // (uniform) the filter is off: the row is copied
        if (off && in_place) continue;
        const Row16 r = row_of(p.keys, row, p.cols);
        const uint32_t q0 = wave * kWaveTile;
        uint32_t t[kRegs];
        load_tile(r, q0, r.body, lane, p.map, t);
        const uint32_t h = wave == 0u ? load_head(r, lane, p.map) : kNoKey;
        uint32_t prefix = 0xFFFFu, shift = 0u;   // every key there is
        bool selected = true;
        if (!off) {
            auto count = [&](int round, uint32_t, uint32_t pre, auto add) __attribute__((always_inline)) {
                auto one = [&](uint32_t key) __attribute__((always_inline)) {
                    if (round == 0 ? key != kNoKey : (key >> 8) == pre) add(key);
                };
#pragma unroll
                for (int i = 0; i < kRegs; i++) one(t[i]);
                one(h);
            };
            const Selected sel = select_short<WAVES, 2, StopKth>(s_cnt, s_found, wave, lane, k, p.out.fault, kKthFaultCount, count);
            prefix = sel.prefix;
            shift = sel.shift;
            selected = sel.need != 0u;   // else the counts fell short (never; the fault bit is set): nothing is stored
        }
        if (selected) {
            uint16_t* const orow = p.dst + (size_t)row * p.cols;
            store_tile(orow, same_phase(orow, r.keys), r, q0, r.body, lane, t, prefix, shift, p.fill, p.map);
            if (wave == 0u) store_head(orow, r, lane, h, prefix, shift, p.fill, p.map);
        }
        group_sync<WAVES>();
    }
}

// ---- long rows ------------------------------------------------------------------------------------------------------------------
// Row state in the workspace (uint4).  During the select: x prefix, y shift (16: no level has run), z need, w done (1: the select
// stopped; kBadRow / kOffRow: from the start).  After the pick: x prefix, y shift, z which of the chunk's keys under the prefix is
// the wanted one (1-based; 0: none), w the chunk that holds it.
struct LongParams {
    const uint16_t* keys;
    uint32_t cols;
    uint32_t chunk, chunks;       // body positions per chunk (a multiple of kLongTile), chunks per row
    uint32_t chunk_cap;           // row stride of `counts`
    uint4* state;
    uint32_t* hist;               // [rows][kBins], zero on entry to every level
    uint32_t* counts;             // [rows][chunk_cap]: keys under the prefix, per chunk (per-row entry with indices)
    Key16Map map;
    Outputs out;
    uint16_t* dst;                // the filter: [rows][cols], may be `keys`
    uint32_t fill;
};

// Control block, counters and row states of a call, the states from the device array.  Per-row entry: need = rank + 1, a rank
// outside the row gives a done state.  FILTER: need = k, k == 0 or k >= cols gives the "off" state.  With state == nullptr (short
// rows) it is the control block alone.
template <bool FILTER>
__global__ void __launch_bounds__(256) kth16r_clear_kernel(uint32_t* ctl, uint32_t* hist, uint32_t hist_words, uint4* state, uint32_t rows,
                                                           const uint32_t* ranks, uint32_t cols)
{
    const uint32_t at = blockIdx.x * blockDim.x + threadIdx.x, step = gridDim.x * blockDim.x;
    if (at < (uint32_t)(kCtlBytes / 4)) ctl[at] = 0u;
    for (uint32_t q = at; q < hist_words; q += step) hist[q] = 0u;
    if (!state) return;
    for (uint32_t r = at; r < rows; r += step) {
        const uint32_t v = ranks[r];
        if (FILTER) state[r] = (v == 0u || v >= cols) ? make_uint4(0u, Levels16::kNoLevel, 0u, kOffRow) : make_uint4(0u, Levels16::kNoLevel, v, 0u);
        else state[r] = v >= cols ? make_uint4(0u, Levels16::kNoLevel, 0u, kBadRow) : make_uint4(0u, Levels16::kNoLevel, v + 1u, 0u);
    }
}

// one chunk of one row per workgroup: the digit of every key under the row's prefix, counted in LDS (hist_level16); a done row returns at once
template <int LEVEL>
__global__ void __launch_bounds__(kLongThreads) kth16r_hist_kernel(const LongParams p)
{
    __shared__ uint32_t s_hist[kBins];
    hist_level16<LEVEL>(p, s_hist);
}

// One workgroup per row: walk the bins from the best end to the one that holds the wanted key; the counters go back to zero.
template <int LEVEL, class Stop>
__global__ void __launch_bounds__(256) kth16r_scan_kernel(const LongParams p)
{
    __shared__ uint32_t s_part[4];
    __shared__ uint32_t s_found[3];
    scan_level<Levels16, LEVEL, Stop>(p, s_part, s_found, kKthFaultCount);
}

// Count, pick and locate are kth16.hip's: the kernel templates of select_tiles16.hpp and radix_select.hpp, under this unit's name.
// Count and locate pass a row whose rank lies outside it by; the pick reports it, by its own bit, and has nothing picked for it.
struct Kth16Rowk {
    using Levels = Levels16;
    using Params = LongParams;
    static constexpr uint32_t kBadW = kBadRow, kFaultBad = kRowkFaultRank;
};
constexpr auto kth16r_count_kernel = count_rows16_kernel<Kth16Rowk>;
constexpr auto kth16r_pick_kernel = pick_rows_kernel<Kth16Rowk>;
constexpr auto kth16r_locate_kernel = locate_rows16_kernel<Kth16Rowk>;

// Values only: after both levels the prefix is the row's whole sortable value (shift 0, need not 0).  A row whose rank lies outside
// it is reported by its own bit; anything else is a row whose counts fell short (its fault bit is set) -- never.  Nothing is stored
// for either.
__global__ void __launch_bounds__(256) kth16r_value_kernel(const LongParams p)
{
    store_values16<kBadRow>(blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x, p, kKthFaultLocate, kRowkFaultRank);
}

// The filter over one chunk of one row per workgroup, the chunks of the select: after both levels the state holds the row's whole
// threshold (shift 0, need not 0); an "off" row is copied, or left alone in place.  Anything else is a row whose counts fell short
// (its fault bit is set) -- never: nothing is stored for it.
__global__ void __launch_bounds__(kLongThreads) topk16f_apply_kernel(const LongParams p)
{
    const uint32_t row = blockIdx.x / p.chunks, c = blockIdx.x % p.chunks;
    if (row >= p.out.rows) return;
    const uint4 st = p.state[row];
    const bool off = st.y == Levels16::kNoLevel && st.w == kOffRow;   // uniform
    if (off ? p.dst == p.keys : !(st.y == 0u && st.z != 0u)) return;
    const uint32_t prefix = off ? 0xFFFFu : (st.x & 0xFFFFu);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const Row16 r = row_of(p.keys, row, p.cols);
    const ChunkRange g = chunk_of(r, p.chunk, c);
    uint16_t* const orow = p.dst + (size_t)row * p.cols;
    const bool vec = same_phase(orow, r.keys);
    if (c == 0u && wave == 0u) store_head(orow, r, lane, load_head(r, lane, p.map), prefix, 0u, p.fill, p.map);   // uniform
    for (uint32_t tile = g.lo; tile < g.hi; tile += kLongTile) {   // uniform
        const uint32_t q0 = tile + wave * kWaveTile;
        uint32_t t[kRegs];
        load_tile(r, q0, g.hi, lane, p.map, t);
        store_tile(orow, vec, r, q0, g.hi, lane, t, prefix, 0u, p.fill, p.map);
    }
}

// Workspace of the per-row entry, kth16.hip's: control | row states (16 B per row) | counters [rows][2048] | chunk counts (4 B per
// chunk) -- the last two for rows above kLocalSortCap keys only.  The filter's has no chunk counts.
using RowkLayout = SelectLayout;
RowkLayout perrow_layout(size_t rows, size_t cols) { return select_layout(rows, cols, false, 4); }
RowkLayout filter_layout(size_t rows, size_t cols) { return select_layout(rows, cols, false, 0); }

// select_long's clear launch with the needs from the device array, and the two level sequences: the select that stops at one key,
// and the one that runs both levels whatever it finds (values only, and the filter: the state then holds the whole value).
template <bool FILTER>
auto clear_from(const uint32_t* ranks, size_t cols, hipStream_t stream)
{
    return [=](dim3 grid, dim3 block, uint32_t* ctl, uint32_t* hist, uint32_t hist_words, uint4* state, uint32_t rows) {
        hipLaunchKernelGGL(kth16r_clear_kernel<FILTER>, grid, block, 0, stream, ctl, hist, hist_words, state, rows, ranks, (uint32_t)cols);
    };
}
const LevelKernels<LongParams> kLevelsKth[] = {{kth16r_hist_kernel<0>, kth16r_scan_kernel<0, StopKth>},
                                               {kth16r_hist_kernel<1>, kth16r_scan_kernel<1, StopKth>}};
const LevelKernels<LongParams> kLevelsWhole[] = {{kth16r_hist_kernel<0>, kth16r_scan_kernel<0, StopNever16>},
                                                 {kth16r_hist_kernel<1>, kth16r_scan_kernel<1, StopKth>}};

int run_perrow(const uint16_t* keys, size_t rows, size_t cols, const uint32_t* ranks, const Key16Map& map, uint16_t* out_keys,
               uint32_t* out_idx, char* ws, const RowkLayout& L, hipStream_t stream)
{
    uint32_t* const ctl = reinterpret_cast<uint32_t*>(ws);
    const Outputs out{out_keys, out_idx, (uint32_t)rows, ctl};
    if (cols <= (size_t)kLocalSortCap) {
        const ShortParams sp{keys, ranks, (uint32_t)cols, map, out, nullptr, 0u};
        hipLaunchKernelGGL(kth16r_clear_kernel<false>, dim3(1), dim3(256), 0, stream, ctl, (uint32_t*)nullptr, 0u, (uint4*)nullptr, 0u,
                           (const uint32_t*)nullptr, 0u);
        if (cols <= (size_t)kWaveSegCap)
            hipLaunchKernelGGL(kth16r_short_kernel<1>, dim3(grid_for(rows, 8, 16384)), dim3(512), 0, stream, sp);
        else
            hipLaunchKernelGGL(kth16r_short_kernel<16>, dim3(grid_for(rows, 1, 4096)), dim3(1024), 0, stream, sp);
        LSD_HIP(hipGetLastError());
        return LSDSORT_OK;
    }
    LongParams lp{};
    lp.map = map;
    lp.out = out;
    if (!out_idx) {   // values only: both levels, then the prefix is the value
        LSD_TRY(select_long(lp, keys, rows, cols, ws, L, clear_from<false>(ranks, cols, stream), kLevelsWhole, stream));
        hipLaunchKernelGGL(kth16r_value_kernel, dim3(grid_for(rows, 256, 1024)), dim3(256), 0, stream, lp);
        LSD_HIP(hipGetLastError());
        return LSDSORT_OK;
    }
    LSD_TRY(select_long(lp, keys, rows, cols, ws, L, clear_from<false>(ranks, cols, stream), kLevelsKth, stream));
    const uint32_t grid = (uint32_t)(rows * lp.chunks), row_grid = (uint32_t)rows;
    hipLaunchKernelGGL(kth16r_count_kernel, dim3(grid), dim3(kLongThreads), 0, stream, lp);
    hipLaunchKernelGGL(kth16r_pick_kernel, dim3(row_grid), dim3(256), 0, stream, lp);
    hipLaunchKernelGGL(kth16r_locate_kernel, dim3(row_grid), dim3(kLongThreads), 0, stream, lp);
    LSD_HIP(hipGetLastError());
    return LSDSORT_OK;
}

int run_filter(const uint16_t* keys, size_t rows, size_t cols, const uint32_t* k, const Key16Map& map, uint32_t fill, uint16_t* dst,
               char* ws, const RowkLayout& L, hipStream_t stream)
{
    uint32_t* const ctl = reinterpret_cast<uint32_t*>(ws);
    const Outputs out{nullptr, nullptr, (uint32_t)rows, ctl};
    if (cols <= (size_t)kLocalSortCap) {
        const ShortParams sp{keys, k, (uint32_t)cols, map, out, dst, fill};
        hipLaunchKernelGGL(kth16r_clear_kernel<true>, dim3(1), dim3(256), 0, stream, ctl, (uint32_t*)nullptr, 0u, (uint4*)nullptr, 0u,
                           (const uint32_t*)nullptr, 0u);
        if (cols <= (size_t)kWaveSegCap)
            hipLaunchKernelGGL(topk16f_short_kernel<1>, dim3(grid_for(rows, 8, 16384)), dim3(512), 0, stream, sp);
        else
            hipLaunchKernelGGL(topk16f_short_kernel<16>, dim3(grid_for(rows, 1, 4096)), dim3(1024), 0, stream, sp);
        LSD_HIP(hipGetLastError());
        return LSDSORT_OK;
    }
    LongParams lp{};
    lp.map = map;
    lp.out = out;
    lp.dst = dst;
    lp.fill = fill;
    LSD_TRY(select_long(lp, keys, rows, cols, ws, L, clear_from<true>(k, cols, stream), kLevelsWhole, stream));
    hipLaunchKernelGGL(topk16f_apply_kernel, dim3((uint32_t)(rows * lp.chunks)), dim3(kLongThreads), 0, stream, lp);
    LSD_HIP(hipGetLastError());
    return LSDSORT_OK;
}

}  // namespace
}  // namespace lsd

extern "C" {

size_t lsdsort_kth16_perrow_workspace_bytes(size_t rows, size_t cols)
{
    if (cols > LSDSORT_MAX_KEYS || !lsd::sizes_ok(rows, cols)) return 0;
    return lsd::perrow_layout(rows, cols).end;
}

int lsdsort_kth16_perrow_device(const void* d_keys, size_t rows, size_t cols, const uint32_t* d_ranks, int key_type, int largest,
                                void* d_out_keys, uint32_t* d_out_idx, void* d_workspace, size_t workspace_bytes, void* hip_stream)
{
    Key16Map map;
    LSD_TRY(key16_map(key_type, largest, &map));
    if (!lsd::sizes_ok(rows, cols)) return LSDSORT_ERR_TOO_LARGE;
    if (rows == 0 || cols == 0) return LSDSORT_OK;
    if (!d_keys || !d_out_keys || (((uintptr_t)d_keys | (uintptr_t)d_out_keys) & 1)) return LSDSORT_ERR_INVALID_ARG;
    if (!d_ranks || ((uintptr_t)d_ranks & 3)) return LSDSORT_ERR_INVALID_ARG;   // their values are the device's to check
    const lsd::RowkLayout L = lsd::perrow_layout(rows, cols);
    if (!lsd::workspace_ok(d_workspace, workspace_bytes, L.end)) return LSDSORT_ERR_WORKSPACE;
    int rank_method = 0;   // asked for the device set-up alone: nothing here ranks with the returning add
    LSD_TRY(lsd::device_rank_method(8, &rank_method));
    return lsd::run_perrow(static_cast<const uint16_t*>(d_keys), rows, cols, d_ranks, map, static_cast<uint16_t*>(d_out_keys), d_out_idx,
                           static_cast<char*>(d_workspace), L, static_cast<hipStream_t>(hip_stream));
}

size_t lsdsort_topk16_filter_workspace_bytes(size_t rows, size_t cols)
{
    if (cols > LSDSORT_MAX_KEYS || !lsd::sizes_ok(rows, cols)) return 0;
    return lsd::filter_layout(rows, cols).end;
}

int lsdsort_topk16_filter_device(const void* d_keys, size_t rows, size_t cols, const uint32_t* d_k, int key_type, int largest,
                                 uint16_t fill_bits, void* d_out, void* d_workspace, size_t workspace_bytes, void* hip_stream)
{
    Key16Map map;
    LSD_TRY(key16_map(key_type, largest, &map));
    if (!lsd::sizes_ok(rows, cols)) return LSDSORT_ERR_TOO_LARGE;
    if (rows == 0 || cols == 0) return LSDSORT_OK;
    if (!d_keys || !d_out || (((uintptr_t)d_keys | (uintptr_t)d_out) & 1)) return LSDSORT_ERR_INVALID_ARG;
    if (!d_k || ((uintptr_t)d_k & 3)) return LSDSORT_ERR_INVALID_ARG;
    const lsd::RowkLayout L = lsd::filter_layout(rows, cols);
    if (!lsd::workspace_ok(d_workspace, workspace_bytes, L.end)) return LSDSORT_ERR_WORKSPACE;
    int rank_method = 0;   // asked for the device set-up alone: nothing here ranks with the returning add
    LSD_TRY(lsd::device_rank_method(8, &rank_method));
    return lsd::run_filter(static_cast<const uint16_t*>(d_keys), rows, cols, d_k, map, (uint32_t)fill_bits, static_cast<uint16_t*>(d_out),
                           static_cast<char*>(d_workspace), L, static_cast<hipStream_t>(hip_stream));
}

}  // extern "C"
