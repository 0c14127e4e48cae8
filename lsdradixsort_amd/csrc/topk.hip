// topk.hip -- the k best keys of every row of a [rows x cols] array, with their positions (lsdsort_topk_device).
//
// No counterpart in the reference (it sorts one whole array, LSDRadixSort.cu:839-910).  Row r's result is the first k items of the
// stable sort of the row in the requested order.  "Best" is always "smallest sortable key": the key transform of lsd_kernels.hpp
// (to_sortable, with the complement for largest) is applied where a key is read, and the raw key is what is stored.
//
// A radix SELECT by counting only, then a sort of the k winners alone.  The select's skeleton -- the short rows' rounds, the long
// rows' clear / hist / scan levels, chunking, the select's workspace and the sort route's threshold -- is radix_select.hpp's, shared
// with topk16.hip and kth.hip; this unit adds the loads (strided, validity by position), compact_tile, the count and write kernels
// and the sort route's copy and take.
//   select   most significant digit first, count the digit of the keys that still match the prefix found so far, walk the counts
//            from the best end to the bin that holds the k-th key: that bin's digit joins the prefix, the keys in better bins are
//            certain winners and `need` (how many the prefix's keys still have to supply) shrinks by their number.  It stops as soon
//            as the bin holds exactly `need` keys (the remainder is decided), at the latest with all 32 bits in the prefix: then
//            the prefix is the k-th VALUE and the ties are taken in position order.
//            State per row: (prefix, shift, need).  Key t wins if (t >> shift) < prefix, or if (t >> shift) == prefix and fewer
//            than `need` such keys stand before it in the row.
//   compact  the winners are written to the outputs IN POSITION ORDER, slot = winners before it in the row: counts per wave (and
//            per chunk of a long row), a small scan, one ordered write.  No atomic-arrival order shows anywhere.
//   sort     the rows x k winners are sorted in place by the segmented sort (segmented.hip), rows as segments, positions as the
//            payload: it is stable, so equal keys keep their position order.  That is a sort of k items per row, never of the row.
// Size classes (those of segmented.hip):
//   cols <= kWaveSegCap (1024)      one wavefront per row: the row in its registers, 8-bit digits counted in its own LDS slice
//   cols <= kLocalSortCap (16384)   one workgroup per row: the same with 16 wavefronts
//   longer                          many workgroups per row (chunks): digits of 11, 11 and 10 bits counted in LDS, flushed into
//                                   [row][2048] by global atomics, one workgroup per row walks the bins between the reads; then
//                                   per-chunk counts of "better" and "equal" and the ordered write.  Up to five reads of the row
//                                   (20 B/key), two fewer for every level the select stops early; nothing written but the winners.
//                                   A chunk without winners is not read by the write pass.
//   k above kLargeKNum / kLargeKDen of cols: the select cannot save much; the rows are copied into the workspace with their
//                                   positions, sorted whole by the segmented sort, and the first k of each are stored.
// Every launch is sized from (rows, cols, k); phases are ordered by kernel boundaries; every store into the outputs is guarded by
// slot < k (counts that do not describe the keys raise a fault bit instead -- never expected).
#define LSDSORT_BUILD 1
#include "../../include/lsdsort.h"

#include "lsd_device.hpp"
#include "lsd_host.hpp"
#include "radix_select.hpp"

namespace lsd {
namespace {

struct Outputs {
    uint32_t* keys;       // [rows][k], raw keys
    uint32_t* idx;        // [rows][k] positions, may be null
    uint32_t rows, k;
    uint32_t* fault;
};

// Ordered write of one tile held in registers: lane l's register i of wave `wave` is position first + 64 i + l of the row, valid
// below `end`.  base_b / base_e: the better / equal keys of the row before this tile; both move on past it.  s_wc: 2 WAVES words.
template <int WAVES>
__device__ __forceinline__ void compact_tile(const uint32_t (&t)[kRegs], uint32_t first, uint32_t end, uint32_t prefix, uint32_t shift,
                                             uint32_t need, uint32_t& base_b, uint32_t& base_e, volatile lds_u32* s_wc, uint32_t wave,
                                             uint32_t lane, uint32_t row, const Outputs& o, const KeyTransform& xf)
{
    uint32_t nb = 0, ne = 0;
#pragma unroll
    for (int i = 0; i < kRegs; i++) {
        const bool valid = first + (uint32_t)i * 64u + lane < end;
        const uint32_t top = t[i] >> shift;
        nb += popc64(__ballot(valid && top < prefix));
        ne += popc64(__ballot(valid && top == prefix));
    }
    uint32_t my_b = base_b, my_e = base_e, all_b = nb, all_e = ne;
    if (WAVES > 1) {
        if (lane == 0u) {
            s_wc[2u * wave] = nb;
            s_wc[2u * wave + 1u] = ne;
        }
        __syncthreads();
        all_b = 0u;
        all_e = 0u;
        for (uint32_t w = 0; w < (uint32_t)WAVES; w++) {
            const uint32_t b = s_wc[2u * w], e = s_wc[2u * w + 1u];
            if (w < wave) {
                my_b += b;
                my_e += e;
            }
            all_b += b;
            all_e += e;
        }
        __syncthreads();   // the next tile writes s_wc again
    }
    // (uniform) a tile without winners writes nothing
    if (all_b != 0u || (all_e != 0u && base_e < need)) {
#pragma unroll
        for (int i = 0; i < kRegs; i++) {
            const uint32_t pos = first + (uint32_t)i * 64u + lane;
            const bool valid = pos < end;
            const uint32_t top = t[i] >> shift;
            const bool better = valid && top < prefix, equal = valid && top == prefix;
            const uint64_t mb = __ballot(better), me = __ballot(equal);
            const uint32_t b_before = mbcnt_add(mb, my_b), e_before = mbcnt_add(me, my_e);
            const bool wins = better || (equal && e_before < need);
            if (wins) {
                const uint32_t slot = b_before + (e_before < need ? e_before : need);
                if (slot < o.k && row < o.rows) {
                    const size_t at = (size_t)row * o.k + slot;
                    o.keys[at] = from_sortable(t[i], xf);
                    if (o.idx) o.idx[at] = pos;
                } else {
                    atomicOr(o.fault, kTopkFaultDest);
                }
            }
            my_b += popc64(mb);
            my_e += popc64(me);
        }
    }
    base_b += all_b;
    base_e += all_e;
}

// ---- short rows: one wavefront (WAVES = 1, eight rows per workgroup) or one workgroup (WAVES = 16) per row ----------------------
struct ShortParams {
    const uint32_t* keys;
    uint32_t cols;
    KeyTransform xf;
    Outputs out;
};

template <int WAVES>
__global__ void __launch_bounds__(WAVES == 1 ? 512 : 1024) topk_short_kernel(const ShortParams p)
{
    constexpr int kGroups = WAVES == 1 ? 8 : 1;          // rows in flight per workgroup
    constexpr int kSlice = 256 + 8 + 2 * WAVES;          // per row: digit counters, the found bin, per-wave counts
    __shared__ uint32_t smem[kGroups * kSlice];
    const uint32_t lane = threadIdx.x & 63u, wave_of_block = threadIdx.x >> 6;
    const uint32_t group = WAVES == 1 ? wave_of_block : 0u, wave = WAVES == 1 ? 0u : wave_of_block;
    volatile lds_u32* const s_cnt = (volatile lds_u32*)((lds_u32*)smem + group * kSlice);
    volatile lds_u32* const s_found = s_cnt + 256;
    volatile lds_u32* const s_wc = s_cnt + 264;
    // `row` is the same for every thread of a group (a wave, or the whole workgroup): its barriers are reached together
    for (uint32_t row = blockIdx.x * kGroups + group; row < p.out.rows; row += gridDim.x * kGroups) {
        const uint32_t* const in = p.keys + (size_t)row * p.cols;
        const uint32_t first = wave * 1024u;
        uint32_t t[kRegs];
#pragma unroll
        for (int i = 0; i < kRegs; i++) {
            const uint32_t pos = first + (uint32_t)i * 64u + lane;
            t[i] = 0xFFFFFFFFu;
            if (first + (uint32_t)i * 64u < p.cols && pos < p.cols) t[i] = to_sortable(in[pos], p.xf);
        }
        // round 0: every key matches; later: those whose bits above the digit are the prefix
        auto count = [&](int round, uint32_t shift, uint32_t prefix, auto add) __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < kRegs; i++) {
                const bool valid = first + (uint32_t)i * 64u + lane < p.cols;
                const bool match = round == 0 || ((t[i] >> shift) >> 8) == prefix;
                if (valid && match) add(t[i]);
            }
        };
        const Selected sel = select_short<WAVES, 4, StopTopk>(s_cnt, s_found, wave, lane, p.out.k, p.out.fault, kTopkFaultCount, count);
        uint32_t base_b = 0u, base_e = 0u;
        compact_tile<WAVES>(t, first, p.cols, sel.prefix, sel.shift, sel.need, base_b, base_e, s_wc, wave, lane, row, p.out, p.xf);
        group_sync<WAVES>();
    }
}

// ---- long rows ------------------------------------------------------------------------------------------------------------------
// Row state in the workspace (uint4): x prefix, y shift, z need, w done (the select stopped: later levels return at once).
struct LongParams {
    const uint32_t* keys;
    uint32_t cols;
    uint32_t chunk, chunks;       // keys per chunk (a multiple of kLongTile), chunks per row
    uint32_t chunk_cap;           // row stride of `counts`
    uint4* state;
    uint32_t* hist;               // [rows][kBins], zero on entry to every level
    uint2* counts;                // [rows][chunk_cap]: better, equal per chunk
    KeyTransform xf;
    Outputs out;
};

// control block, counters and row states of a call (a kernel rather than memsets: one kind of node in a captured graph)
__global__ void __launch_bounds__(256) topk_clear_kernel(uint32_t* ctl, uint32_t* hist, uint32_t hist_words, uint4* state, uint32_t rows,
                                                         uint32_t k)
{
    clear_select(blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x, ctl, hist, hist_words, state, rows, k, Levels32::kNoLevel);
}

__device__ __forceinline__ void load_tile(const uint32_t* in, uint32_t first, uint32_t end, uint32_t lane, const KeyTransform& xf,
                                          uint32_t (&t)[kRegs])
{
#pragma unroll
    for (int i = 0; i < kRegs; i++) {
        const uint32_t pos = first + (uint32_t)i * 64u + lane;
        t[i] = 0xFFFFFFFFu;
        if (pos < end) t[i] = to_sortable(in[pos], xf);
    }
}

// One chunk of one row per workgroup: the digit of every key under the row's prefix, counted in LDS.
template <int LEVEL>
__global__ void __launch_bounds__(kLongThreads) topk_hist_kernel(const LongParams p)
{
    __shared__ uint32_t s_hist[kBins];
    hist_level(p, s_hist, [&](uint32_t row, uint32_t c, const uint4& st, uint32_t lane, uint32_t wave) __attribute__((always_inline)) {
        const uint32_t* const in = p.keys + (size_t)row * p.cols;
        const uint32_t lo = c * p.chunk, hi = p.cols - lo < p.chunk ? p.cols : lo + p.chunk;
        const uint32_t shift = Levels32::shift(LEVEL), mask = (1u << Levels32::bits(LEVEL)) - 1u;
        for (uint32_t tile = lo; tile < hi; tile += kLongTile) {   // uniform
            const uint32_t first = tile + wave * 1024u;
            uint32_t t[kRegs];
            load_tile(in, first, hi, lane, p.xf, t);
#pragma unroll
            for (int i = 0; i < kRegs; i++) {
                const bool valid = first + (uint32_t)i * 64u + lane < hi;
                const bool match = valid && (LEVEL == 0 || (t[i] >> st.y) == st.x);
                count_digit(s_hist, match, (t[i] >> shift) & mask, lane);
            }
        }
    });
}

// One workgroup per row: walk the bins from the best end to the one that holds the k-th key; the counters go back to zero.
template <int LEVEL>
__global__ void __launch_bounds__(256) topk_scan_kernel(const LongParams p)
{
    __shared__ uint32_t s_part[4];
    __shared__ uint32_t s_found[3];
    scan_level<Levels32, LEVEL, StopTopk>(p, s_part, s_found, kTopkFaultCount);
}

// better / equal keys of every chunk
__global__ void __launch_bounds__(kLongThreads) topk_count_kernel(const LongParams p)
{
    __shared__ uint32_t s_part[2 * kLongWaves];
    const uint32_t row = blockIdx.x / p.chunks, c = blockIdx.x % p.chunks;
    if (row >= p.out.rows) return;
    const uint4 st = p.state[row];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t* const in = p.keys + (size_t)row * p.cols;
    const uint32_t lo = c * p.chunk, hi = p.cols - lo < p.chunk ? p.cols : lo + p.chunk;
    uint32_t nb = 0u, ne = 0u;
    if (st.y < Levels32::kNoLevel) {
        for (uint32_t tile = lo; tile < hi; tile += kLongTile) {   // uniform
            const uint32_t first = tile + wave * 1024u;
            uint32_t t[kRegs];
            load_tile(in, first, hi, lane, p.xf, t);
#pragma unroll
            for (int i = 0; i < kRegs; i++) {
                const bool valid = first + (uint32_t)i * 64u + lane < hi;
                const uint32_t top = t[i] >> st.y;
                nb += (valid && top < st.x) ? 1u : 0u;
                ne += (valid && top == st.x) ? 1u : 0u;
            }
        }
    }
    nb = wave_sum(nb);
    ne = wave_sum(ne);
    if (lane == 0u) {
        s_part[2u * wave] = nb;
        s_part[2u * wave + 1u] = ne;
    }
    __syncthreads();
    if (tid == 0u) {
        uint32_t b = 0u, e = 0u;
        for (uint32_t w = 0; w < kLongWaves; w++) {
            b += s_part[2u * w];
            e += s_part[2u * w + 1u];
        }
        p.counts[(size_t)row * p.chunk_cap + c] = make_uint2(b, e);
    }
}

// the ordered write: the chunk's winners go to slots that follow those of the chunks before it
__global__ void __launch_bounds__(kLongThreads) topk_write_kernel(const LongParams p)
{
    __shared__ uint32_t s_part[2 * kLongWaves];
    __shared__ uint32_t s_wc_raw[2 * kLongWaves];
    const uint32_t row = blockIdx.x / p.chunks, c = blockIdx.x % p.chunks;
    if (row >= p.out.rows) return;
    const uint4 st = p.state[row];
    if (st.y >= Levels32::kNoLevel) return;   // (uniform) a row no scan has visited: never
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint2* const counts = p.counts + (size_t)row * p.chunk_cap;
    uint32_t base_b = 0u, base_e = 0u;
    for (uint32_t q = tid; q < c; q += kLongThreads) {
        const uint2 v = counts[q];
        base_b += v.x;
        base_e += v.y;
    }
    base_b = wave_sum(base_b);
    base_e = wave_sum(base_e);
    if (lane == 0u) {
        s_part[2u * wave] = base_b;
        s_part[2u * wave + 1u] = base_e;
    }
    __syncthreads();
    base_b = 0u;
    base_e = 0u;
    for (uint32_t w = 0; w < kLongWaves; w++) {
        base_b += s_part[2u * w];
        base_e += s_part[2u * w + 1u];
    }
    const uint2 mine = counts[c];
    if (mine.x == 0u && (mine.y == 0u || base_e >= st.z)) return;   // (uniform) no winner in this chunk: it is not read again
    const uint32_t* const in = p.keys + (size_t)row * p.cols;
    const uint32_t lo = c * p.chunk, hi = p.cols - lo < p.chunk ? p.cols : lo + p.chunk;
    volatile lds_u32* const s_wc = (volatile lds_u32*)(lds_u32*)s_wc_raw;
    for (uint32_t tile = lo; tile < hi; tile += kLongTile) {   // uniform
        const uint32_t first = tile + wave * 1024u;
        uint32_t t[kRegs];
        load_tile(in, first, hi, lane, p.xf, t);
        compact_tile<(int)kLongWaves>(t, first, hi, st.x, st.y, st.z, base_b, base_e, s_wc, wave, lane, row, p.out, p.xf);
    }
}

// ---- plumbing -------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) topk_offsets_kernel(uint32_t* off, uint32_t rows, uint32_t stride)
{
    row_offsets(blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x, off, rows, stride);
}

// the sort route: the rows and their positions into the workspace ...
__global__ void __launch_bounds__(256) topk_copy_kernel(const uint32_t* keys, uint32_t* copy, uint32_t* idx, uint32_t n, uint32_t cols)
{
    for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < n; q += gridDim.x * blockDim.x) {
        copy[q] = keys[q];
        if (idx) idx[q] = q % cols;
    }
}

// ... and the first k of every sorted row out of it
__global__ void __launch_bounds__(256) topk_take_kernel(const uint32_t* sorted, const uint32_t* idx, uint32_t cols, const Outputs o)
{
    const uint32_t total = o.rows * o.k;
    for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < total; q += gridDim.x * blockDim.x) {
        const uint32_t row = q / o.k, slot = q - row * o.k;
        const size_t from = (size_t)row * cols + slot;
        o.keys[q] = sorted[from];
        if (o.idx) o.idx[q] = idx[from];
    }
}

// Workspace.  Select route: the select's part (with offsets) | segmented sort of rows x k pairs.  Sort route: control | offsets |
// copy of the keys | their positions | segmented sort of rows x cols pairs.  The size is the larger of the two, the sort route's
// taken at the most keys a sort-route call with this (rows, k) can have: monotonic in each argument.
struct TopkLayout {
    SelectLayout sel;
    size_t seg, seg_bytes, total;   // select route
    SortRouteLayout sort;           // sort route, for `sort_keys` keys
    size_t bytes() const { return max_sz(total, sort.total); }
};
TopkLayout topk_layout(size_t rows, size_t cols, size_t k)
{
    TopkLayout L{};
    L.sel = select_layout(rows, cols, true, 8);
    L.seg = L.sel.end;
    L.seg_bytes = lsdsort_segmented_workspace_bytes(min_sz(rows * k, LSDSORT_MAX_KEYS), rows, 1);
    L.total = align_up(L.seg + L.seg_bytes);
    L.sort = sort_route_layout(rows, sort_route_keys(rows, cols, k));
    return L;
}

int run_topk(const uint32_t* keys, size_t rows, size_t cols, size_t k, int key_type, int largest, const KeyTransform& xf,
             uint32_t* out_keys, uint32_t* out_idx, char* ws, const TopkLayout& L, hipStream_t stream)
{
    uint32_t* const ctl = reinterpret_cast<uint32_t*>(ws);
    Outputs out{out_keys, out_idx, (uint32_t)rows, (uint32_t)k, ctl};
    const size_t n = rows * cols;

    if (sort_route(cols, k)) {
        uint32_t* const offsets = reinterpret_cast<uint32_t*>(ws + L.sort.offsets);
        uint32_t* const copy = reinterpret_cast<uint32_t*>(ws + L.sort.keys);
        uint32_t* const idx = out_idx ? reinterpret_cast<uint32_t*>(ws + L.sort.idx) : nullptr;
        hipLaunchKernelGGL(topk_clear_kernel, dim3(1), dim3(256), 0, stream, ctl, (uint32_t*)nullptr, 0u, (uint4*)nullptr, 0u, 0u);
        hipLaunchKernelGGL(topk_offsets_kernel, dim3(grid_for(rows + 1, 256, 1024)), dim3(256), 0, stream, offsets, (uint32_t)rows,
                           (uint32_t)cols);
        hipLaunchKernelGGL(topk_copy_kernel, dim3(grid_for(n, 1024, 8192)), dim3(256), 0, stream, keys, copy, idx, (uint32_t)n,
                           (uint32_t)cols);
        LSD_HIP(hipGetLastError());
        LSD_TRY(lsdsort_segmented_device(copy, idx, offsets, rows, n, key_type, largest, ws + L.sort.seg, L.sort.seg_bytes, stream));
        hipLaunchKernelGGL(topk_take_kernel, dim3(grid_for(rows * k, 1024, 8192)), dim3(256), 0, stream, copy, idx, (uint32_t)cols, out);
        LSD_HIP(hipGetLastError());
        LSD_HIP(launch_keep_fault(ctl, reinterpret_cast<const uint32_t*>(ws + L.sort.seg), stream));
        return LSDSORT_OK;
    }

    uint32_t* const offsets = reinterpret_cast<uint32_t*>(ws + L.sel.offsets);
    if (cols <= (size_t)kLocalSortCap) {
        ShortParams sp{keys, (uint32_t)cols, xf, out};
        hipLaunchKernelGGL(topk_clear_kernel, dim3(1), dim3(256), 0, stream, ctl, (uint32_t*)nullptr, 0u, (uint4*)nullptr, 0u, 0u);
        if (cols <= (size_t)kWaveSegCap)
            hipLaunchKernelGGL(topk_short_kernel<1>, dim3(grid_for(rows, 8, 16384)), dim3(512), 0, stream, sp);
        else
            hipLaunchKernelGGL(topk_short_kernel<16>, dim3(grid_for(rows, 1, 4096)), dim3(1024), 0, stream, sp);
        LSD_HIP(hipGetLastError());
    } else {
        static const LevelKernels<LongParams> levels[] = {{topk_hist_kernel<0>, topk_scan_kernel<0>},
                                                          {topk_hist_kernel<1>, topk_scan_kernel<1>},
                                                          {topk_hist_kernel<2>, topk_scan_kernel<2>}};
        LongParams lp{};
        lp.xf = xf;
        lp.out = out;
        LSD_TRY(select_long(lp, keys, rows, cols, (uint32_t)k, ws, L.sel, topk_clear_kernel, levels, stream));
        const uint32_t grid = (uint32_t)(rows * lp.chunks);
        hipLaunchKernelGGL(topk_count_kernel, dim3(grid), dim3(kLongThreads), 0, stream, lp);
        hipLaunchKernelGGL(topk_write_kernel, dim3(grid), dim3(kLongThreads), 0, stream, lp);
        LSD_HIP(hipGetLastError());
    }
    if (k < 2) return LSDSORT_OK;   // one winner per row is in order as it stands
    hipLaunchKernelGGL(topk_offsets_kernel, dim3(grid_for(rows + 1, 256, 1024)), dim3(256), 0, stream, offsets, (uint32_t)rows, (uint32_t)k);
    LSD_HIP(hipGetLastError());
    LSD_TRY(lsdsort_segmented_device(out_keys, out_idx, offsets, rows, rows * k, key_type, largest, ws + L.seg, L.seg_bytes, stream));
    LSD_HIP(launch_keep_fault(ctl, reinterpret_cast<const uint32_t*>(ws + L.seg), stream));
    return LSDSORT_OK;
}

}  // namespace
}  // namespace lsd

extern "C" {

size_t lsdsort_topk_workspace_bytes(size_t rows, size_t cols, size_t k)
{
    if (rows > LSDSORT_MAX_KEYS || cols > LSDSORT_MAX_KEYS || k > LSDSORT_MAX_KEYS) return 0;
    if (rows != 0 && cols > LSDSORT_MAX_KEYS / rows) return 0;
    if (rows != 0 && k > LSDSORT_MAX_KEYS / rows) return 0;
    return lsd::topk_layout(rows, cols, k).bytes();
}

int lsdsort_topk_device(const void* d_keys, size_t rows, size_t cols, size_t k, int key_type, int largest, void* d_out_keys,
                        uint32_t* d_out_idx, void* d_workspace, size_t workspace_bytes, void* hip_stream)
{
    lsd::KeyTransform xf;
    LSD_TRY(lsd::key_transform(key_type, largest, &xf));
    if (rows > LSDSORT_MAX_KEYS || (rows != 0 && cols > LSDSORT_MAX_KEYS / rows)) return LSDSORT_ERR_TOO_LARGE;
    if (k > cols) return LSDSORT_ERR_INVALID_ARG;
    if (rows == 0 || cols == 0 || k == 0) return LSDSORT_OK;
    if (!d_keys || !d_out_keys) return LSDSORT_ERR_INVALID_ARG;
    const lsd::TopkLayout L = lsd::topk_layout(rows, cols, k);
    if (!lsd::workspace_ok(d_workspace, workspace_bytes, L.bytes())) return LSDSORT_ERR_WORKSPACE;
    int rank_method = 0;
    LSD_TRY(lsd::device_rank_method(8, &rank_method));
    return lsd::run_topk(static_cast<const uint32_t*>(d_keys), rows, cols, k, key_type, largest ? 1 : 0, xf,
                         static_cast<uint32_t*>(d_out_keys), d_out_idx, static_cast<char*>(d_workspace), L,
                         static_cast<hipStream_t>(hip_stream));
}

}  // extern "C"
