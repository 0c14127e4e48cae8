// kth16.hip -- the 16-bit key at ONE rank of every row of a [rows x cols] array, with its position (lsdsort_kth16_device; DESIGN.md
// section 6.9).  The 16-bit sibling of kth.hip: same contract, same size classes, and the same select skeleton, radix_select.hpp's,
// here with Levels16 (11 then 5 bits; two rounds of 8-bit digits for the short rows) under the stop rule StopKth.  The median, a
// percentile or a clipping threshold of float16 / bfloat16 rows, selected from the 2-byte keys as they lie in memory.
//
// No counterpart in the reference (it sorts one whole array of uint32, LSDRadixSort.cu:839-910).  Row r's result is item `rank` of
// the stable sort of the row in the requested order: the map of keys16_map.hpp (to_sortable16, with the complement for largest) is
// applied where a key is read, and the caller's 16-bit word is what is stored.
//
//   select   as in kth.hip, on 16 bits: it stops where the found bin holds ONE key, at the latest with all 16 bits in the prefix.
//   locate   every key under the final prefix has the same value, so the wanted item is the `need`-th of them in POSITION order:
//            per-lane match masks, a wave sum, per-wave counts through LDS (per-chunk counts through memory for long rows), and in
//            the one wave that holds it a wave scan per group of eight.  One lane stores the key, un-mapped, by a 2-byte store, and
//            its position.  No atomic-arrival order shows.
//   values only, long rows   a 16-bit value is fully known once both levels have run: without an index buffer the select runs under
//            StopNever16 (no early stop) and kth16_value_kernel stores from_sortable16(prefix) per row -- two reads of the row, six
//            launches, no count, pick or locate.
//
// Key reads, the loaders and locate_tile are select_tiles16.hpp's, shared with every 16-bit row select: a register without a key
// holds kNoKey, which no (prefix, shift) matches, so kth.hip's validity mask is not needed.  The long rows' count and locate kernels
// are that header's too, and the pick is radix_select.hpp's: kernel templates, shared with kth16_rowk.hip, that this unit names.
// Size classes (those of every select here, by cols):
//   cols <= kWaveSegCap (1024)      one wavefront per row, eight rows per workgroup, no workgroup barrier.  2 B/key read.
//   cols <= kLocalSortCap (16384)   one workgroup of 16 wavefronts per row: the same
//   longer                          many workgroups per row (chunks of body positions; chunk 0 owns the head): the two levels, then
//                                   one count pass (keys under the prefix, per chunk), a per-row pick of the chunk that holds the
//                                   `need`-th of them, and a locate that reads that ONE chunk up to the tile that holds the key.
//                                   At most three reads of the row plus one chunk (6 B/key); a row whose bin holds one key after
//                                   level 0 skips level 1.
// Every launch is sized from (rows, cols) and from whether an index buffer was given; phases are ordered by kernel boundaries; every
// store into the outputs is guarded by row < rows.  Counts that do not reach the rank, or a locate that finds no key, raise a fault
// bit instead -- never expected.  Nothing here ranks with the returning add: the result does not depend on lsdsort_set_rank_method.
#define LSDSORT_BUILD 1
#include "../../include/lsdsort.h"

#include "keys16_map.hpp"
#include "lsd_device.hpp"
#include "lsd_host.hpp"
#include "radix_select.hpp"
#include "select_tiles16.hpp"

namespace lsd {
namespace {

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
    uint32_t cols, rank;
    Key16Map map;
    Outputs out;
};

template <int WAVES>
__global__ void __launch_bounds__(WAVES == 1 ? 512 : 1024) kth16_short_kernel(const ShortParams p)
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
        const Row16 r = row_of(p.keys, row, p.cols);
        const uint32_t q0 = wave * kWaveTile;
        uint32_t t[kRegs];
        load_tile(r, q0, r.body, lane, p.map, t);
        const uint32_t h = wave == 0u ? load_head(r, lane, p.map) : kNoKey;
        // round 0: every key there is; round 1: those whose top byte is the prefix (kNoKey never is)
        auto count = [&](int round, uint32_t, uint32_t prefix, auto add) __attribute__((always_inline)) {
            auto one = [&](uint32_t key) __attribute__((always_inline)) {
                if (round == 0 ? key != kNoKey : (key >> 8) == prefix) add(key);
            };
#pragma unroll
            for (int i = 0; i < kRegs; i++) one(t[i]);
            one(h);
        };
        const Selected sel = select_short<WAVES, 2, StopKth>(s_cnt, s_found, wave, lane, p.rank + 1u, p.out.fault, kKthFaultCount, count);
        uint32_t base = 0u;
        const bool found = locate_tile<WAVES>(t, h, q0, r, sel.prefix, sel.shift, sel.need, base, s_wc, wave, lane, row, 0u, p.out, p.map);
        if (!found && sel.need != 0u && wave == 0u && lane == 0u) atomicOr(p.out.fault, kKthFaultLocate);
        group_sync<WAVES>();
    }
}

// ---- long rows ------------------------------------------------------------------------------------------------------------------
// Row state in the workspace (uint4).  During the select: x prefix, y shift (16: no level has run), z need, w done (the select
// stopped: later levels return at once).  After the pick: x prefix, y shift, z which of the chunk's keys under the prefix is the
// wanted one (1-based; 0: none), w the chunk that holds it.
struct LongParams {
    const uint16_t* keys;
    uint32_t cols;
    uint32_t chunk, chunks;       // body positions per chunk (a multiple of kLongTile), chunks per row
    uint32_t chunk_cap;           // row stride of `counts`
    uint4* state;
    uint32_t* hist;               // [rows][kBins], zero on entry to every level
    uint32_t* counts;             // [rows][chunk_cap]: keys under the prefix, per chunk
    Key16Map map;
    Outputs out;
};

// control block, counters and row states of a call (a kernel rather than memsets: one kind of node in a captured graph)
__global__ void __launch_bounds__(256) kth16_clear_kernel(uint32_t* ctl, uint32_t* hist, uint32_t hist_words, uint4* state, uint32_t rows,
                                                          uint32_t need)
{
    clear_select(blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x, ctl, hist, hist_words, state, rows, need, Levels16::kNoLevel);
}

// one chunk of one row per workgroup: the digit of every key under the row's prefix, counted in LDS (hist_level16)
template <int LEVEL>
__global__ void __launch_bounds__(kLongThreads) kth16_hist_kernel(const LongParams p)
{
    __shared__ uint32_t s_hist[kBins];
    hist_level16<LEVEL>(p, s_hist);
}

// One workgroup per row: walk the bins from the best end to the one that holds the wanted key; the counters go back to zero.
// The last level ends the select whatever the stop rule: both rules share its kernel.
template <int LEVEL, class Stop>
__global__ void __launch_bounds__(256) kth16_scan_kernel(const LongParams p)
{
    __shared__ uint32_t s_part[4];
    __shared__ uint32_t s_found[3];
    scan_level<Levels16, LEVEL, Stop>(p, s_part, s_found, kKthFaultCount);
}

// Count (the keys under the prefix, per chunk), pick (the chunk that holds the `need`-th of them) and locate (that ONE chunk, up to
// the tile that holds the key): the kernel templates of select_tiles16.hpp and radix_select.hpp, under this unit's name.
struct Kth16 {
    using Levels = Levels16;
    using Params = LongParams;
    static constexpr uint32_t kBadW = 0u;   // no row is refused from the start
};
constexpr auto kth16_count_kernel = count_rows16_kernel<Kth16>;
constexpr auto kth16_pick_kernel = pick_rows_kernel<Kth16>;
constexpr auto kth16_locate_kernel = locate_rows16_kernel<Kth16>;

// Values only: after both levels the prefix is the row's whole sortable value (shift 0, need not 0).  Anything else is a row whose
// counts fell short (its fault bit is set) or one no scan has visited -- never: nothing is stored for it.
__global__ void __launch_bounds__(256) kth16_value_kernel(const LongParams p)
{
    store_values16<0u>(blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x, p, kKthFaultLocate, 0u);
}

// Workspace: control | row states (16 B per row) | counters [rows][2048] | chunk counts (4 B per chunk) -- the last two for rows
// above kLocalSortCap keys only.  At most 256 + rows (16 + 8192 + 4 ceil(cols / 16384)) + 3 * 255 bytes; never O(rows * cols).
using Kth16Layout = SelectLayout;   // no offsets, and nothing behind the chunk counts: `end` is the figure
Kth16Layout kth16_layout(size_t rows, size_t cols) { return select_layout(rows, cols, false, 4); }

int run_kth16(const uint16_t* keys, size_t rows, size_t cols, size_t rank, const Key16Map& map, uint16_t* out_keys, uint32_t* out_idx,
              char* ws, const Kth16Layout& L, hipStream_t stream)
{
    uint32_t* const ctl = reinterpret_cast<uint32_t*>(ws);
    const Outputs out{out_keys, out_idx, (uint32_t)rows, ctl};
    if (cols <= (size_t)kLocalSortCap) {
        const ShortParams sp{keys, (uint32_t)cols, (uint32_t)rank, map, out};
        hipLaunchKernelGGL(kth16_clear_kernel, dim3(1), dim3(256), 0, stream, ctl, (uint32_t*)nullptr, 0u, (uint4*)nullptr, 0u, 0u);
        if (cols <= (size_t)kWaveSegCap)
            hipLaunchKernelGGL(kth16_short_kernel<1>, dim3(grid_for(rows, 8, 16384)), dim3(512), 0, stream, sp);
        else
            hipLaunchKernelGGL(kth16_short_kernel<16>, dim3(grid_for(rows, 1, 4096)), dim3(1024), 0, stream, sp);
        LSD_HIP(hipGetLastError());
        return LSDSORT_OK;
    }
    LongParams lp{};
    lp.map = map;
    lp.out = out;
    if (!out_idx) {   // values only: both levels, then the prefix is the value
        static const LevelKernels<LongParams> levels[] = {{kth16_hist_kernel<0>, kth16_scan_kernel<0, StopNever16>},
                                                          {kth16_hist_kernel<1>, kth16_scan_kernel<1, StopKth>}};
        LSD_TRY(select_long(lp, keys, rows, cols, (uint32_t)rank + 1u, ws, L, kth16_clear_kernel, levels, stream));
        hipLaunchKernelGGL(kth16_value_kernel, dim3(grid_for(rows, 256, 1024)), dim3(256), 0, stream, lp);
        LSD_HIP(hipGetLastError());
        return LSDSORT_OK;
    }
    static const LevelKernels<LongParams> levels[] = {{kth16_hist_kernel<0>, kth16_scan_kernel<0, StopKth>},
                                                      {kth16_hist_kernel<1>, kth16_scan_kernel<1, StopKth>}};
    LSD_TRY(select_long(lp, keys, rows, cols, (uint32_t)rank + 1u, ws, L, kth16_clear_kernel, levels, stream));
    const uint32_t grid = (uint32_t)(rows * lp.chunks), row_grid = (uint32_t)rows;
    hipLaunchKernelGGL(kth16_count_kernel, dim3(grid), dim3(kLongThreads), 0, stream, lp);
    hipLaunchKernelGGL(kth16_pick_kernel, dim3(row_grid), dim3(256), 0, stream, lp);
    hipLaunchKernelGGL(kth16_locate_kernel, dim3(row_grid), dim3(kLongThreads), 0, stream, lp);
    LSD_HIP(hipGetLastError());
    return LSDSORT_OK;
}

}  // namespace
}  // namespace lsd

extern "C" {

size_t lsdsort_kth16_workspace_bytes(size_t rows, size_t cols)
{
    if (rows > LSDSORT_MAX_KEYS || cols > LSDSORT_MAX_KEYS) return 0;
    if (rows != 0 && cols > LSDSORT_MAX_KEYS / rows) return 0;
    return lsd::kth16_layout(rows, cols).end;
}

int lsdsort_kth16_device(const void* d_keys, size_t rows, size_t cols, size_t rank, int key_type, int largest, void* d_out_keys,
                         uint32_t* d_out_idx, void* d_workspace, size_t workspace_bytes, void* hip_stream)
{
    Key16Map map;
    LSD_TRY(key16_map(key_type, largest, &map));
    if (rows > LSDSORT_MAX_KEYS || (rows != 0 && cols > LSDSORT_MAX_KEYS / rows)) return LSDSORT_ERR_TOO_LARGE;
    if (rows == 0 || cols == 0) return LSDSORT_OK;   // before the rank: an empty row has no valid rank
    if (rank >= cols) return LSDSORT_ERR_INVALID_ARG;
    if (!d_keys || !d_out_keys || (((uintptr_t)d_keys | (uintptr_t)d_out_keys) & 1)) return LSDSORT_ERR_INVALID_ARG;
    const lsd::Kth16Layout L = lsd::kth16_layout(rows, cols);
    if (!lsd::workspace_ok(d_workspace, workspace_bytes, L.end)) return LSDSORT_ERR_WORKSPACE;
    int rank_method = 0;   // asked for the device set-up alone: nothing here ranks with the returning add
    LSD_TRY(lsd::device_rank_method(8, &rank_method));
    return lsd::run_kth16(static_cast<const uint16_t*>(d_keys), rows, cols, rank, map, static_cast<uint16_t*>(d_out_keys), d_out_idx,
                          static_cast<char*>(d_workspace), L, static_cast<hipStream_t>(hip_stream));
}

}  // extern "C"
