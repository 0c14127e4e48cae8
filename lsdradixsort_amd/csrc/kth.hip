// kth.hip -- the key at ONE rank of every row of a [rows x cols] array, with its position (lsdsort_kth_device; DESIGN.md
// section 6.8).  The counterpart of torch.kthvalue / torch.median on rows and of the `lower` / `higher` / `nearest` quantiles.
//
// No counterpart in the reference (it sorts one whole array, LSDRadixSort.cu:839-910).  Row r's result is item `rank` of the stable
// sort of the row in the requested order: the key transform of lsd_kernels.hpp (to_sortable, with the complement for largest) is
// applied where a key is read, and the raw key is what is stored.
//
// A radix SELECT by counting only, as in topk.hip, and a LOCATE instead of top-k's compact + sort.  The select's skeleton is
// radix_select.hpp's, shared with topk.hip and topk16.hip, with the stop rule StopKth; the loads (Row<uint32_t> with a validity
// mask) and locate_tile are select_tiles32.hpp's, shared with kth_multi.hip; this unit adds the count and locate kernels, and
// names its instantiation of the pick kernel, a template of radix_select.hpp that every single-rank k-th value unit shares.
//   select   most significant digit first, count the digit of the keys that still match the prefix found so far, walk the counts
//            from the best end to the bin that holds the wanted key: that bin's digit joins the prefix and `need` (which of the
//            prefix's keys, in sorted order, is wanted; 1-based) shrinks by the number of keys in better bins.  Unlike top-k it
//            cannot stop where the bin holds exactly `need` keys (the wanted one is then the LAST of them by value, not yet
//            known): it stops where the bin holds ONE key, at the latest with all 32 bits in the prefix.
//   locate   every key under the final prefix has the same value (one key, or all 32 bits fixed), so the wanted item is the
//            `need`-th of them in POSITION order: per-lane counts, a wave scan, per-wave counts through LDS (and per-chunk counts
//            through memory for long rows).  One lane stores the key, un-mapped, and its position.  No atomic-arrival order shows.
//
// Key reads and the validity mask that stands for "no key": select_tiles32.hpp.
// Size classes (those of topk.hip, by cols):
//   cols <= kWaveSegCap (1024)      one wavefront per row, eight rows per workgroup, no workgroup barrier: the row in its registers,
//                                   8-bit digits counted in its own LDS slice.  4 B/key read, 8 B/row written.
//   cols <= kLocalSortCap (16384)   one workgroup per row: the same with 16 wavefronts
//   longer                          many workgroups per row (chunks of body positions; chunk 0 owns the head): digits of 11, 11 and
//                                   10 bits counted in LDS, flushed into [row][2048] by global atomics, one workgroup per row walks
//                                   the bins between the reads; a row whose bin holds one key skips the remaining levels.  Then one
//                                   count pass (keys equal to the prefix, per chunk), a per-row pick of the chunk that holds the
//                                   `need`-th of them, and a locate that reads that ONE chunk.  At most four reads of the row plus
//                                   one chunk (16 B/key); nothing written but the counters and 8 B per row.
// Every launch is sized from (rows, cols); phases are ordered by kernel boundaries; every store into the outputs is guarded by
// row < rows.  Counts that do not reach the rank, or a locate that finds no key, raise a fault bit instead -- never expected.
// Nothing here needs the returning-add rank form: the result does not depend on lsdsort_set_rank_method.
#define LSDSORT_BUILD 1
#include "../../include/lsdsort.h"

#include "lsd_device.hpp"
#include "lsd_host.hpp"
#include "radix_select.hpp"
#include "select_tiles32.hpp"

namespace lsd {
namespace {

struct Outputs {
    uint32_t* keys;       // [rows], raw keys
    uint32_t* idx;        // [rows] positions, may be null
    uint32_t rows;
    uint32_t* fault;
    __device__ __forceinline__ size_t at(uint32_t row, uint32_t) const { return row; }   // locate_tile's store: one slot per row
};

// ---- short rows: one wavefront (WAVES = 1, eight rows per workgroup) or one workgroup (WAVES = 16) per row ----------------------
struct ShortParams {
    const uint32_t* keys;
    uint32_t cols, rank;
    KeyTransform xf;
    Outputs out;
};

template <int WAVES>
__global__ void __launch_bounds__(WAVES == 1 ? 512 : 1024) kth_short_kernel(const ShortParams p)
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
        const Row32 r = row_of(p.keys, row, p.cols);
        const uint32_t q0 = wave * kWaveTile;
        uint32_t t[kRegs], h = 0u;
        uint32_t vm = load_tile(r, q0, r.body, lane, p.xf, t);
        if (wave == 0u) vm |= load_head(r, lane, p.xf, h);
        // round 0: every key there is; later: those whose bits above the digit are the prefix.  Always under the validity bit.
        auto count = [&](int round, uint32_t shift, uint32_t prefix, auto add) __attribute__((always_inline)) {
            auto one = [&](uint32_t key, bool valid) __attribute__((always_inline)) {
                const bool match = round == 0 || ((key >> shift) >> 8) == prefix;
                if (valid && match) add(key);
            };
#pragma unroll
            for (int i = 0; i < kRegs; i++) one(t[i], ((vm >> i) & 1u) != 0u);
            one(h, (vm & kHeadBit) != 0u);
        };
        const Selected sel = select_short<WAVES, 4, StopKth>(s_cnt, s_found, wave, lane, p.rank + 1u, p.out.fault, kKthFaultCount, count);
        uint32_t base = 0u;
        const bool found = locate_tile<WAVES>(t, h, vm, q0, r, sel.prefix, sel.shift, sel.need, base, s_wc, wave, lane, row, 0u, p.out, p.xf);
        if (!found && sel.need != 0u && wave == 0u && lane == 0u) atomicOr(p.out.fault, kKthFaultLocate);
        group_sync<WAVES>();
    }
}

// ---- long rows ------------------------------------------------------------------------------------------------------------------
// Row state in the workspace (uint4).  During the select: x prefix, y shift (32: no level has run), z need, w done (the select
// stopped: later levels return at once).  After the pick: x prefix, y shift, z which of the chunk's keys under the prefix is the
// wanted one (1-based; 0: none), w the chunk that holds it.
struct LongParams {
    const uint32_t* keys;
    uint32_t cols;
    uint32_t chunk, chunks;       // body positions per chunk (a multiple of kLongTile), chunks per row
    uint32_t chunk_cap;           // row stride of `counts`
    uint4* state;
    uint32_t* hist;               // [rows][kBins], zero on entry to every level
    uint32_t* counts;             // [rows][chunk_cap]: keys under the prefix, per chunk
    KeyTransform xf;
    Outputs out;
};

// control block, counters and row states of a call (a kernel rather than memsets: one kind of node in a captured graph)
__global__ void __launch_bounds__(256) kth_clear_kernel(uint32_t* ctl, uint32_t* hist, uint32_t hist_words, uint4* state, uint32_t rows,
                                                        uint32_t need)
{
    clear_select(blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x, ctl, hist, hist_words, state, rows, need, Levels32::kNoLevel);
}

// One chunk of one row per workgroup: the digit of every key under the row's prefix, counted in LDS.
template <int LEVEL>
__global__ void __launch_bounds__(kLongThreads) kth_hist_kernel(const LongParams p)
{
    __shared__ uint32_t s_hist[kBins];
    hist_level(p, s_hist, [&](uint32_t row, uint32_t c, const uint4& st, uint32_t lane, uint32_t wave) __attribute__((always_inline)) {
        const Row32 r = row_of(p.keys, row, p.cols);
        const ChunkRange g = chunk_of(r, p.chunk, c);
        const uint32_t shift = Levels32::shift(LEVEL), mask = (1u << Levels32::bits(LEVEL)) - 1u;
        auto count = [&](uint32_t key, bool valid) __attribute__((always_inline)) {
            const bool match = valid && (LEVEL == 0 || (key >> st.y) == st.x);
            count_digit(s_hist, match, (key >> shift) & mask, lane);
        };
        if (c == 0u && wave == 0u) {   // uniform
            uint32_t h;
            const uint32_t hv = load_head(r, lane, p.xf, h);
            count(h, hv != 0u);
        }
        for (uint32_t tile = g.lo; tile < g.hi; tile += kLongTile) {   // uniform
            uint32_t t[kRegs];
            const uint32_t vm = load_tile(r, tile + wave * kWaveTile, g.hi, lane, p.xf, t);
#pragma unroll
            for (int i = 0; i < kRegs; i++) count(t[i], ((vm >> i) & 1u) != 0u);
        }
    });
}

// One workgroup per row: walk the bins from the best end to the one that holds the wanted key; the counters go back to zero.
template <int LEVEL>
__global__ void __launch_bounds__(256) kth_scan_kernel(const LongParams p)
{
    __shared__ uint32_t s_part[4];
    __shared__ uint32_t s_found[3];
    scan_level<Levels32, LEVEL, StopKth>(p, s_part, s_found, kKthFaultCount);
}

// the keys under the prefix, per chunk
__global__ void __launch_bounds__(kLongThreads) kth_count_kernel(const LongParams p)
{
    __shared__ uint32_t s_part[kLongWaves];
    const uint32_t row = blockIdx.x / p.chunks, c = blockIdx.x % p.chunks;
    if (row >= p.out.rows) return;
    const uint4 st = p.state[row];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const Row32 r = row_of(p.keys, row, p.cols);
    const ChunkRange g = chunk_of(r, p.chunk, c);
    uint32_t ne = 0u;
    if (st.y < Levels32::kNoLevel && st.z != 0u) {   // (uniform) else: a row no scan has visited, or one whose counts fell short -- never
        if (c == 0u && wave == 0u) {   // uniform
            uint32_t h;
            const uint32_t hv = load_head(r, lane, p.xf, h);
            ne += (hv != 0u && (h >> st.y) == st.x) ? 1u : 0u;
        }
        for (uint32_t tile = g.lo; tile < g.hi; tile += kLongTile) {   // uniform
            uint32_t t[kRegs];
            const uint32_t vm = load_tile(r, tile + wave * kWaveTile, g.hi, lane, p.xf, t);
#pragma unroll
            for (int i = 0; i < kRegs; i++) ne += (((vm >> i) & 1u) != 0u && (t[i] >> st.y) == st.x) ? 1u : 0u;
        }
    }
    ne = wave_sum(ne);
    if (lane == 0u) s_part[wave] = ne;
    __syncthreads();
    if (tid == 0u) {
        uint32_t e = 0u;
        for (uint32_t w = 0; w < kLongWaves; w++) e += s_part[w];
        p.counts[(size_t)row * p.chunk_cap + c] = e;
    }
}

// One workgroup per row: the chunk that holds the `need`-th key under the prefix, and which of that chunk's such keys it is --
// radix_select.hpp's kernel template, under this unit's name.
struct Kth {
    using Levels = Levels32;
    using Params = LongParams;
    static constexpr uint32_t kBadW = 0u;   // no row is refused from the start
};
constexpr auto kth_pick_kernel = pick_rows_kernel<Kth>;

// One workgroup per row reads the picked chunk, and only up to the tile that holds the key.
__global__ void __launch_bounds__(kLongThreads) kth_locate_kernel(const LongParams p)
{
    __shared__ uint32_t s_wc_raw[kLongWaves];
    const uint32_t row = blockIdx.x;
    if (row >= p.out.rows) return;
    const uint4 st = p.state[row];
    if (st.z == 0u || st.w >= p.chunks) return;   // (uniform) nothing was picked: the fault bit is already set
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const Row32 r = row_of(p.keys, row, p.cols);
    const ChunkRange g = chunk_of(r, p.chunk, st.w);
    volatile lds_u32* const s_wc = (volatile lds_u32*)(lds_u32*)s_wc_raw;
    uint32_t base = 0u;
    bool found = false;
    // chunk 0 has at least one tile (a long row's body is longer than its head), and its first tile carries the head
    for (uint32_t tile = g.lo; tile < g.hi && !found; tile += kLongTile) {   // uniform
        const uint32_t q0 = tile + wave * kWaveTile;
        uint32_t t[kRegs], h = 0u;
        uint32_t vm = load_tile(r, q0, g.hi, lane, p.xf, t);
        if (st.w == 0u && tile == g.lo && wave == 0u) vm |= load_head(r, lane, p.xf, h);   // uniform
        found = locate_tile<(int)kLongWaves>(t, h, vm, q0, r, st.x, st.y, st.z, base, s_wc, wave, lane, row, 0u, p.out, p.xf);
    }
    if (!found && tid == 0u) atomicOr(p.out.fault, kKthFaultLocate);
}

// Workspace: control | row states (16 B per row) | counters [rows][2048] | chunk counts (4 B per chunk) -- the last two for rows
// above kLocalSortCap keys only.  At most 256 + rows (16 + 8192 + 4 ceil(cols / 16384)) + 3 * 255 bytes; never O(rows * cols).
using KthLayout = SelectLayout;   // no offsets, and nothing behind the chunk counts: `end` is the figure
KthLayout kth_layout(size_t rows, size_t cols) { return select_layout(rows, cols, false, 4); }

int run_kth(const uint32_t* keys, size_t rows, size_t cols, size_t rank, const KeyTransform& xf, uint32_t* out_keys, uint32_t* out_idx,
            char* ws, const KthLayout& L, hipStream_t stream)
{
    uint32_t* const ctl = reinterpret_cast<uint32_t*>(ws);
    const Outputs out{out_keys, out_idx, (uint32_t)rows, ctl};
    if (cols <= (size_t)kLocalSortCap) {
        const ShortParams sp{keys, (uint32_t)cols, (uint32_t)rank, xf, out};
        hipLaunchKernelGGL(kth_clear_kernel, dim3(1), dim3(256), 0, stream, ctl, (uint32_t*)nullptr, 0u, (uint4*)nullptr, 0u, 0u);
        if (cols <= (size_t)kWaveSegCap)
            hipLaunchKernelGGL(kth_short_kernel<1>, dim3(grid_for(rows, 8, 16384)), dim3(512), 0, stream, sp);
        else
            hipLaunchKernelGGL(kth_short_kernel<16>, dim3(grid_for(rows, 1, 4096)), dim3(1024), 0, stream, sp);
        LSD_HIP(hipGetLastError());
        return LSDSORT_OK;
    }
    static const LevelKernels<LongParams> levels[] = {{kth_hist_kernel<0>, kth_scan_kernel<0>},
                                                      {kth_hist_kernel<1>, kth_scan_kernel<1>},
                                                      {kth_hist_kernel<2>, kth_scan_kernel<2>}};
    LongParams lp{};
    lp.xf = xf;
    lp.out = out;
    LSD_TRY(select_long(lp, keys, rows, cols, (uint32_t)rank + 1u, ws, L, kth_clear_kernel, levels, stream));
    const uint32_t grid = (uint32_t)(rows * lp.chunks), row_grid = (uint32_t)rows;
    hipLaunchKernelGGL(kth_count_kernel, dim3(grid), dim3(kLongThreads), 0, stream, lp);
    hipLaunchKernelGGL(kth_pick_kernel, dim3(row_grid), dim3(256), 0, stream, lp);
    hipLaunchKernelGGL(kth_locate_kernel, dim3(row_grid), dim3(kLongThreads), 0, stream, lp);
    LSD_HIP(hipGetLastError());
    return LSDSORT_OK;
}

}  // namespace
}  // namespace lsd

extern "C" {

size_t lsdsort_kth_workspace_bytes(size_t rows, size_t cols)
{
    if (rows > LSDSORT_MAX_KEYS || cols > LSDSORT_MAX_KEYS) return 0;
    if (rows != 0 && cols > LSDSORT_MAX_KEYS / rows) return 0;
    return lsd::kth_layout(rows, cols).end;
}

int lsdsort_kth_device(const void* d_keys, size_t rows, size_t cols, size_t rank, int key_type, int largest, void* d_out_keys,
                       uint32_t* d_out_idx, void* d_workspace, size_t workspace_bytes, void* hip_stream)
{
    lsd::KeyTransform xf;
    LSD_TRY(lsd::key_transform(key_type, largest, &xf));
    if (rows > LSDSORT_MAX_KEYS || (rows != 0 && cols > LSDSORT_MAX_KEYS / rows)) return LSDSORT_ERR_TOO_LARGE;
    if (rows == 0 || cols == 0) return LSDSORT_OK;   // before the rank: an empty row has no valid rank
    if (rank >= cols) return LSDSORT_ERR_INVALID_ARG;
    if (!d_keys || !d_out_keys || (((uintptr_t)d_keys | (uintptr_t)d_out_keys) & 3)) return LSDSORT_ERR_INVALID_ARG;
    const lsd::KthLayout L = lsd::kth_layout(rows, cols);
    if (!lsd::workspace_ok(d_workspace, workspace_bytes, L.end)) return LSDSORT_ERR_WORKSPACE;
    int rank_method = 0;   // asked for the device set-up alone: nothing here ranks with the returning add
    LSD_TRY(lsd::device_rank_method(8, &rank_method));
    return lsd::run_kth(static_cast<const uint32_t*>(d_keys), rows, cols, rank, xf, static_cast<uint32_t*>(d_out_keys), d_out_idx,
                        static_cast<char*>(d_workspace), L, static_cast<hipStream_t>(hip_stream));
}

}  // extern "C"
