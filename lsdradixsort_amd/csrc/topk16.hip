// topk16.hip -- the k best 16-bit keys of every row of a [rows x cols] array, with their positions (lsdsort_topk16_device;
// DESIGN.md section 6.6).  The 16-bit sibling of topk.hip: same contract, same three steps, same size classes, and the same select
// skeleton, radix_select.hpp's (two rounds, or the levels of 11 and 5 bits).  The loads are select_tiles16.hpp's (Row<uint16_t>,
// kNoKey for a key that does not exist), shared with every 16-bit row select; this unit adds compact_tile into the workspace, the
// count and write kernels, and the widen and finish kernels.
//
// No counterpart in the reference (it sorts one whole array of uint32, LSDRadixSort.cu:839-910).  Row r's result is the first k
// items of the stable sort of the row in the requested order.  "Best" is always "smallest sortable value": the map of
// keys16_map.hpp (to_sortable16, with the complement for largest) is applied where a key is read.
//
//   select   as in topk.hip, on 16 bits: state per row (prefix, shift, need); key t wins if (t >> shift) < prefix, or if
//            (t >> shift) == prefix and fewer than `need` such keys stand before it in the row.  At most TWO digit levels.
//   compact  the winners go to the WORKSPACE in position order, as uint32 words (the sortable value in the low half-word, the high
//            half-word zero) with their positions beside them: slot = winners before it in the row.
//   sort     those rows x k words are sorted by the segmented sort as uint32 ascending, rows as segments, positions as payload:
//            stable, and its tiers of up to 16384 keys skip the two dead high digits on their own.  k = 1 needs no sort.
//   finish   one small kernel un-maps, narrows into d_out_keys and copies the positions into d_out_idx.
//
// Key reads: select_tiles16.hpp (head keys one by one, the body in 16-byte groups of eight, two groups per lane and tile).
// Size classes (those of topk.hip, by cols):
//   cols <= kWaveSegCap (1024)      one wavefront per row: the row in its registers, two rounds of 8-bit digits in its LDS slice
//   cols <= kLocalSortCap (16384)   one workgroup per row: the same with 16 wavefronts
//   longer                          many workgroups per row (chunks of body positions): digits of 11 then 5 bits counted in LDS,
//                                   flushed into [row][2048] by global atomics, one workgroup per row walks the bins between the
//                                   reads; then per-chunk counts of "better" and "equal" and the ordered write.  At most four
//                                   reads of the row (8 B/key), one fewer where the select stops after the first level.  A chunk
//                                   without winners is not read by the write pass.  Chunk 0 also owns the row's head.
//   k above kLargeKNum / kLargeKDen of cols: the rows are widened into the workspace with their positions, sorted whole by the
//                                   segmented sort, and the first k of each are taken (the threshold is topk.hip's).
// Every launch is sized from (rows, cols, k); phases are ordered by kernel boundaries; every store of a winner is guarded by
// slot < k (counts that do not describe the keys raise a fault bit instead -- never expected).
#define LSDSORT_BUILD 1
#include "../../include/lsdsort.h"

#include "keys16_map.hpp"
#include "lsd_device.hpp"
#include "lsd_host.hpp"
#include "radix_select.hpp"
#include "select_tiles16.hpp"

namespace lsd {
namespace {

constexpr int kPlainThreads = 256;

struct Winners {
    uint32_t* keys;       // [rows][k] in the workspace: sortable values as uint32
    uint32_t* pos;        // [rows][k] positions, null where the caller wants none
    uint32_t rows, k;
    uint32_t* fault;
};

// Ordered write of one tile held in registers (load_tile at q0), and with `has_head` (uniform; the first tile of wave 0 of the
// row) of the head keys `h` in front of it.  base_b / base_e: the better / equal keys of the row before this tile; both move on
// past it.  s_wc: 2 WAVES words.  A lane's counts travel packed: better in the low half-word, equal in the high one.
template <int WAVES>
__device__ __forceinline__ void compact_tile(const uint32_t (&t)[kRegs], uint32_t h, bool has_head, uint32_t q0, const Row16& r,
                                             uint32_t prefix, uint32_t shift, uint32_t need, uint32_t& base_b, uint32_t& base_e,
                                             volatile lds_u32* s_wc, uint32_t wave, uint32_t lane, uint32_t row, const Winners& o)
{
    auto packed = [&](uint32_t key) {
        const uint32_t top = key >> shift;
        return (top < prefix ? 1u : 0u) | (top == prefix ? 0x10000u : 0u);
    };
    uint32_t c[kRegs / 8];
    const uint32_t ch = has_head ? packed(h) : 0u;
    uint32_t sum = ch;
#pragma unroll
    for (int j = 0; j < kRegs / 8; j++) {
        c[j] = 0u;
#pragma unroll
        for (int e = 0; e < 8; e++) c[j] += packed(t[8 * j + e]);
        sum += c[j];
    }
    sum = wave_sum(sum);
    const uint32_t nb = sum & 0xFFFFu, ne = sum >> 16;
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
        auto emit = [&](uint32_t key, uint32_t pos, uint32_t& b_before, uint32_t& e_before) {
            const uint32_t top = key >> shift;
            const bool better = top < prefix, equal = top == prefix;
            if (better || (equal && e_before < need)) {
                const uint32_t slot = b_before + (e_before < need ? e_before : need);
                if (slot < o.k && row < o.rows) {
                    const size_t at = (size_t)row * o.k + slot;
                    o.keys[at] = key;
                    if (o.pos) o.pos[at] = pos;
                } else {
                    atomicOr(o.fault, kTopkFaultDest);
                }
            }
            b_before += better ? 1u : 0u;
            e_before += equal ? 1u : 0u;
        };
        if (has_head) {   // uniform
            const uint32_t incl = wave_inclusive_scan(ch), excl = incl - ch;
            uint32_t b_before = my_b + (excl & 0xFFFFu), e_before = my_e + (excl >> 16);
            emit(h, lane, b_before, e_before);
            const uint32_t all = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            my_b += all & 0xFFFFu;
            my_e += all >> 16;
        }
#pragma unroll
        for (int j = 0; j < kRegs / 8; j++) {
            const uint32_t incl = wave_inclusive_scan(c[j]), excl = incl - c[j];
            uint32_t b_before = my_b + (excl & 0xFFFFu), e_before = my_e + (excl >> 16);
            const uint32_t pos = r.head + q0 + ((uint32_t)j * 64u + lane) * kGroupKeys;
#pragma unroll
            for (int e = 0; e < 8; e++) emit(t[8 * j + e], pos + (uint32_t)e, b_before, e_before);
            const uint32_t all = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            my_b += all & 0xFFFFu;
            my_e += all >> 16;
        }
    }
    base_b += all_b;
    base_e += all_e;
}

// ---- short rows: one wavefront (WAVES = 1, eight rows per workgroup) or one workgroup (WAVES = 16) per row ----------------------
struct ShortParams {
    const uint16_t* keys;
    uint32_t cols;
    Key16Map map;
    Winners out;
};

template <int WAVES>
__global__ void __launch_bounds__(WAVES == 1 ? 512 : 1024) topk16_short_kernel(const ShortParams p)
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
        const Selected sel = select_short<WAVES, 2, StopTopk>(s_cnt, s_found, wave, lane, p.out.k, p.out.fault, kTopkFaultCount, count);
        uint32_t base_b = 0u, base_e = 0u;
        compact_tile<WAVES>(t, h, wave == 0u, q0, r, sel.prefix, sel.shift, sel.need, base_b, base_e, s_wc, wave, lane, row, p.out);
        group_sync<WAVES>();
    }
}

// ---- long rows ------------------------------------------------------------------------------------------------------------------
// Row state in the workspace (uint4): x prefix, y shift (16: no level has run), z need, w done (the select stopped).
struct LongParams {
    const uint16_t* keys;
    uint32_t cols;
    uint32_t chunk, chunks;       // body positions per chunk (a multiple of kLongTile), chunks per row
    uint32_t chunk_cap;           // row stride of `counts`
    uint4* state;
    uint32_t* hist;               // [rows][kBins], zero on entry to every level
    uint2* counts;                // [rows][chunk_cap]: better, equal per chunk
    Key16Map map;
    Winners out;
};

// control block, counters and row states of a call (a kernel rather than memsets: one kind of node in a captured graph)
__global__ void __launch_bounds__(kPlainThreads) topk16_clear_kernel(uint32_t* ctl, uint32_t* hist, uint32_t hist_words, uint4* state,
                                                                    uint32_t rows, uint32_t k)
{
    clear_select(blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x, ctl, hist, hist_words, state, rows, k, Levels16::kNoLevel);
}

// one chunk of one row per workgroup: the digit of every key under the row's prefix, counted in LDS (hist_level16)
template <int LEVEL>
__global__ void __launch_bounds__(kLongThreads) topk16_hist_kernel(const LongParams p)
{
    __shared__ uint32_t s_hist[kBins];
    hist_level16<LEVEL>(p, s_hist);
}

// One workgroup per row: walk the bins from the best end to the one that holds the k-th key; the counters go back to zero.
template <int LEVEL>
__global__ void __launch_bounds__(256) topk16_scan_kernel(const LongParams p)
{
    __shared__ uint32_t s_part[4];
    __shared__ uint32_t s_found[3];
    scan_level<Levels16, LEVEL, StopTopk>(p, s_part, s_found, kTopkFaultCount);
}

// better / equal keys of every chunk
__global__ void __launch_bounds__(kLongThreads) topk16_count_kernel(const LongParams p)
{
    __shared__ uint32_t s_part[2 * kLongWaves];
    const uint32_t row = blockIdx.x / p.chunks, c = blockIdx.x % p.chunks;
    if (row >= p.out.rows) return;
    const uint4 st = p.state[row];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const Row16 r = row_of(p.keys, row, p.cols);
    const ChunkRange g = chunk_of(r, p.chunk, c);
    uint32_t nb = 0u, ne = 0u;
    if (st.y < Levels16::kNoLevel) {
        auto count = [&](uint32_t key) {
            const uint32_t top = key >> st.y;
            nb += top < st.x ? 1u : 0u;
            ne += top == st.x ? 1u : 0u;
        };
        if (c == 0u && wave == 0u) count(load_head(r, lane, p.map));   // uniform
        for (uint32_t tile = g.lo; tile < g.hi; tile += kLongTile) {   // uniform
            uint32_t t[kRegs];
            load_tile(r, tile + wave * kWaveTile, g.hi, lane, p.map, t);
#pragma unroll
            for (int i = 0; i < kRegs; i++) count(t[i]);
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
__global__ void __launch_bounds__(kLongThreads) topk16_write_kernel(const LongParams p)
{
    __shared__ uint32_t s_part[2 * kLongWaves];
    __shared__ uint32_t s_wc_raw[2 * kLongWaves];
    const uint32_t row = blockIdx.x / p.chunks, c = blockIdx.x % p.chunks;
    if (row >= p.out.rows) return;
    const uint4 st = p.state[row];
    if (st.y >= Levels16::kNoLevel) return;   // (uniform) a row no scan has visited: never
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
    const Row16 r = row_of(p.keys, row, p.cols);
    const ChunkRange g = chunk_of(r, p.chunk, c);
    volatile lds_u32* const s_wc = (volatile lds_u32*)(lds_u32*)s_wc_raw;
    // chunk 0 has at least one tile (a long row's body is longer than its head), and its first tile carries the head
    for (uint32_t tile = g.lo; tile < g.hi; tile += kLongTile) {   // uniform
        const uint32_t q0 = tile + wave * kWaveTile;
        const bool has_head = c == 0u && tile == g.lo && wave == 0u;
        uint32_t t[kRegs];
        load_tile(r, q0, g.hi, lane, p.map, t);
        const uint32_t h = has_head ? load_head(r, lane, p.map) : kNoKey;
        compact_tile<(int)kLongWaves>(t, h, has_head, q0, r, st.x, st.y, st.z, base_b, base_e, s_wc, wave, lane, row, p.out);
    }
}

// ---- plumbing -------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kPlainThreads) topk16_offsets_kernel(uint32_t* off, uint32_t rows, uint32_t stride)
{
    row_offsets(blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x, off, rows, stride);
}

// The sort route: every key of the array widened to its sortable value, with its position in its row beside it.  The array as a
// whole is one Span here (the rows lie back to back); `wide` and `idx` are 256-byte aligned, so the eight words of a group lie on
// 16-byte lines where the head is a multiple of four keys (wide_vec).
__global__ void __launch_bounds__(kPlainThreads) topk16_widen_kernel(const uint16_t* __restrict__ keys, Span sp, uint32_t wide_vec, uint32_t cols,
                                                                    Key16Map m, uint32_t* __restrict__ wide, uint32_t* __restrict__ idx)
{
    const uint32_t tid = threadIdx.x;
    auto one = [&](uint32_t q) {
        wide[q] = to_sortable16(keys[q], m);
        if (idx) idx[q] = q % cols;
    };
    if (blockIdx.x == 0) {
        if (tid < sp.head) one(tid);
        if (tid < sp.tail) one(first_tail_key(sp) + tid);
    }
    const uint4* body = body_of(keys, sp);
    for (uint32_t g = blockIdx.x * kPlainThreads + tid; g < sp.groups; g += gridDim.x * kPlainThreads) {
        const uint4 v = body[g];
        const uint32_t in[4] = {v.x, v.y, v.z, v.w};
        uint32_t t[kGroupKeys], at[kGroupKeys];
        const uint32_t q = sp.head + g * kGroupKeys;
        uint32_t col = q % cols;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            t[2 * i] = to_sortable16(in[i] & 0xFFFFu, m);
            t[2 * i + 1] = to_sortable16(in[i] >> 16, m);
        }
#pragma unroll
        for (uint32_t i = 0; i < kGroupKeys; i++) {
            at[i] = col;
            col = col + 1u == cols ? 0u : col + 1u;
        }
        if (wide_vec) {
            reinterpret_cast<uint4*>(wide + q)[0] = make_uint4(t[0], t[1], t[2], t[3]);
            reinterpret_cast<uint4*>(wide + q)[1] = make_uint4(t[4], t[5], t[6], t[7]);
            if (idx) {
                reinterpret_cast<uint4*>(idx + q)[0] = make_uint4(at[0], at[1], at[2], at[3]);
                reinterpret_cast<uint4*>(idx + q)[1] = make_uint4(at[4], at[5], at[6], at[7]);
            }
        } else {
#pragma unroll
            for (uint32_t i = 0; i < kGroupKeys; i++) {
                wide[q + i] = t[i];
                if (idx) idx[q + i] = at[i];
            }
        }
    }
}

// Both routes end here: slot j of row r is word r * stride + j of `sorted` (stride k: the sorted winners; stride cols: the
// sorted rows).  Un-map, narrow, and the positions where the caller wants them.
__global__ void __launch_bounds__(kPlainThreads) topk16_finish_kernel(const uint32_t* __restrict__ sorted, const uint32_t* __restrict__ pos,
                                                                     uint32_t stride, Key16Map m, uint16_t* __restrict__ out_keys,
                                                                     uint32_t* __restrict__ out_idx, uint32_t rows, uint32_t k)
{
    const uint32_t total = rows * k;
    for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < total; q += gridDim.x * blockDim.x) {
        const uint32_t row = q / k, slot = q - row * k;
        const size_t from = (size_t)row * stride + slot;
        out_keys[q] = (uint16_t)from_sortable16(sorted[from] & 0xFFFFu, m);
        if (out_idx) out_idx[q] = pos[from];
    }
}

// Workspace.  Select route: the select's part (with offsets) | the winners as uint32 | their positions | segmented sort of rows x k
// pairs.  Sort route: control | offsets | the widened keys | their positions | segmented sort of rows x cols pairs.  The size is
// the larger of the two, the sort route's taken at the most keys a sort-route call with this (rows, k) can have: monotonic in each
// argument.  Sized for the call with indices.
struct Topk16Layout {
    SelectLayout sel;
    size_t win, win_pos, seg, seg_bytes, total;   // select route
    SortRouteLayout sort;                         // sort route, for `sort_keys` keys
    size_t bytes() const { return max_sz(total, sort.total); }
};
Topk16Layout topk16_layout(size_t rows, size_t cols, size_t k)
{
    Topk16Layout L{};
    const size_t winners = min_sz(rows * k, LSDSORT_MAX_KEYS);
    L.sel = select_layout(rows, cols, true, 8);
    size_t off = L.sel.end;
    L.win = off;      off = align_up(off + winners * 4);
    L.win_pos = off;  off = align_up(off + winners * 4);
    L.seg = off;
    L.seg_bytes = lsdsort_segmented_workspace_bytes(winners, rows, 1);
    L.total = align_up(off + L.seg_bytes);
    L.sort = sort_route_layout(rows, sort_route_keys(rows, cols, k));
    return L;
}

int run_topk16(const uint16_t* keys, size_t rows, size_t cols, size_t k, const Key16Map& map, uint16_t* out_keys, uint32_t* out_idx,
               char* ws, const Topk16Layout& L, hipStream_t stream)
{
    uint32_t* const ctl = reinterpret_cast<uint32_t*>(ws);
    const size_t n = rows * cols;
    const uint32_t finish_grid = grid_for(rows * k, 1024, 8192);

    if (sort_route(cols, k)) {
        uint32_t* const offsets = reinterpret_cast<uint32_t*>(ws + L.sort.offsets);
        uint32_t* const wide = reinterpret_cast<uint32_t*>(ws + L.sort.keys);
        uint32_t* const idx = out_idx ? reinterpret_cast<uint32_t*>(ws + L.sort.idx) : nullptr;
        const Span sp = span_of(keys, n);
        hipLaunchKernelGGL(topk16_clear_kernel, dim3(1), dim3(kPlainThreads), 0, stream, ctl, (uint32_t*)nullptr, 0u, (uint4*)nullptr, 0u, 0u);
        hipLaunchKernelGGL(topk16_offsets_kernel, dim3(grid_for(rows + 1, 256, 1024)), dim3(kPlainThreads), 0, stream, offsets,
                           (uint32_t)rows, (uint32_t)cols);
        hipLaunchKernelGGL(topk16_widen_kernel, dim3(grid_for(sp.groups, kPlainThreads, 2048)), dim3(kPlainThreads), 0, stream, keys, sp,
                           (sp.head & 3u) == 0 ? 1u : 0u, (uint32_t)cols, map, wide, idx);
        LSD_HIP(hipGetLastError());
        LSD_TRY(lsdsort_segmented_device(wide, idx, offsets, rows, n, LSDSORT_KEY_U32, 0, ws + L.sort.seg, L.sort.seg_bytes, stream));
        hipLaunchKernelGGL(topk16_finish_kernel, dim3(finish_grid), dim3(kPlainThreads), 0, stream, static_cast<const uint32_t*>(wide),
                           static_cast<const uint32_t*>(idx), (uint32_t)cols, map, out_keys, out_idx, (uint32_t)rows, (uint32_t)k);
        LSD_HIP(hipGetLastError());
        LSD_HIP(launch_keep_fault(ctl, reinterpret_cast<const uint32_t*>(ws + L.sort.seg), stream));
        return LSDSORT_OK;
    }

    uint32_t* const offsets = reinterpret_cast<uint32_t*>(ws + L.sel.offsets);
    uint32_t* const win = reinterpret_cast<uint32_t*>(ws + L.win);
    uint32_t* const win_pos = out_idx ? reinterpret_cast<uint32_t*>(ws + L.win_pos) : nullptr;
    const Winners out{win, win_pos, (uint32_t)rows, (uint32_t)k, ctl};
    if (cols <= (size_t)kLocalSortCap) {
        ShortParams sp{keys, (uint32_t)cols, map, out};
        hipLaunchKernelGGL(topk16_clear_kernel, dim3(1), dim3(kPlainThreads), 0, stream, ctl, (uint32_t*)nullptr, 0u, (uint4*)nullptr, 0u, 0u);
        if (cols <= (size_t)kWaveSegCap)
            hipLaunchKernelGGL(topk16_short_kernel<1>, dim3(grid_for(rows, 8, 16384)), dim3(512), 0, stream, sp);
        else
            hipLaunchKernelGGL(topk16_short_kernel<16>, dim3(grid_for(rows, 1, 4096)), dim3(1024), 0, stream, sp);
        LSD_HIP(hipGetLastError());
    } else {
        static const LevelKernels<LongParams> levels[] = {{topk16_hist_kernel<0>, topk16_scan_kernel<0>},
                                                          {topk16_hist_kernel<1>, topk16_scan_kernel<1>}};
        LongParams lp{};
        lp.map = map;
        lp.out = out;
        LSD_TRY(select_long(lp, keys, rows, cols, (uint32_t)k, ws, L.sel, topk16_clear_kernel, levels, stream));
        const uint32_t grid = (uint32_t)(rows * lp.chunks);
        hipLaunchKernelGGL(topk16_count_kernel, dim3(grid), dim3(kLongThreads), 0, stream, lp);
        hipLaunchKernelGGL(topk16_write_kernel, dim3(grid), dim3(kLongThreads), 0, stream, lp);
        LSD_HIP(hipGetLastError());
    }
    if (k >= 2) {   // one winner per row is in order as it stands
        hipLaunchKernelGGL(topk16_offsets_kernel, dim3(grid_for(rows + 1, 256, 1024)), dim3(kPlainThreads), 0, stream, offsets, (uint32_t)rows,
                           (uint32_t)k);
        LSD_HIP(hipGetLastError());
        LSD_TRY(lsdsort_segmented_device(win, win_pos, offsets, rows, rows * k, LSDSORT_KEY_U32, 0, ws + L.seg, L.seg_bytes, stream));
    }
    hipLaunchKernelGGL(topk16_finish_kernel, dim3(finish_grid), dim3(kPlainThreads), 0, stream, static_cast<const uint32_t*>(win),
                       static_cast<const uint32_t*>(win_pos), (uint32_t)k, map, out_keys, out_idx, (uint32_t)rows, (uint32_t)k);
    LSD_HIP(hipGetLastError());
    if (k >= 2) LSD_HIP(launch_keep_fault(ctl, reinterpret_cast<const uint32_t*>(ws + L.seg), stream));
    return LSDSORT_OK;
}

}  // namespace
}  // namespace lsd

extern "C" {

size_t lsdsort_topk16_workspace_bytes(size_t rows, size_t cols, size_t k)
{
    if (rows > LSDSORT_MAX_KEYS || cols > LSDSORT_MAX_KEYS || k > LSDSORT_MAX_KEYS) return 0;
    if (rows != 0 && cols > LSDSORT_MAX_KEYS / rows) return 0;
    if (rows != 0 && k > LSDSORT_MAX_KEYS / rows) return 0;
    return lsd::topk16_layout(rows, cols, k).bytes();
}

int lsdsort_topk16_device(const void* d_keys, size_t rows, size_t cols, size_t k, int key_type, int largest, void* d_out_keys,
                          uint32_t* d_out_idx, void* d_workspace, size_t workspace_bytes, void* hip_stream)
{
    Key16Map map;
    LSD_TRY(key16_map(key_type, largest, &map));
    if (rows > LSDSORT_MAX_KEYS || (rows != 0 && cols > LSDSORT_MAX_KEYS / rows)) return LSDSORT_ERR_TOO_LARGE;
    if (k > cols) return LSDSORT_ERR_INVALID_ARG;
    if (rows == 0 || cols == 0 || k == 0) return LSDSORT_OK;
    if (!d_keys || !d_out_keys || (((uintptr_t)d_keys | (uintptr_t)d_out_keys) & 1)) return LSDSORT_ERR_INVALID_ARG;
    const lsd::Topk16Layout L = lsd::topk16_layout(rows, cols, k);
    if (!lsd::workspace_ok(d_workspace, workspace_bytes, L.bytes())) return LSDSORT_ERR_WORKSPACE;
    int rank_method = 0;
    LSD_TRY(lsd::device_rank_method(8, &rank_method));
    return lsd::run_topk16(static_cast<const uint16_t*>(d_keys), rows, cols, k, map, static_cast<uint16_t*>(d_out_keys), d_out_idx,
                           static_cast<char*>(d_workspace), L, static_cast<hipStream_t>(hip_stream));
}

}  // extern "C"
