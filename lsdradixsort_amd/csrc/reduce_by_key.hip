// reduce_by_key.hip -- sum, min or max of 32-bit values per run and per distinct key, 32- and 64-bit keys.
//
// No reference counterpart: the reference sorts ascending uint32 keys and stops there (LSDRadixSort.cu:62).  unique.hip gives the
// distinct keys, their counts and the inverse map; what a caller does next is aggregate a value array per group.  This unit does it
// on the device, without atomics, in an order fixed by the positions alone: the same input gives the same bits on every call.
//
//   reduce runs (lsdsort_reduce_runs_device): COUNT | SCAN | EMIT, the shape of unique.hip -- ordered by kernel boundaries only, no
//       workgroup waits for another, so no kernel can hang.  A tile is 256 threads x 16 keys.  All three phases fold PARTS with one
//       associative join (below): a part is a stretch of positions, known by 1 + the position of its last run head (0: it has none)
//       and the aggregate of its values from that head on (or of all of them).  COUNT stores every tile's part and head count; SCAN
//       (one workgroup) turns the counts into exclusive offsets and the parts into the part IN FRONT of every tile -- the run still
//       open there and what it has gathered -- and stores the last run's aggregate and length; EMIT recomputes the flags, ranks them,
//       and folds the parts in position order in front of every key: every head stores the aggregate and the length of the run
//       BEFORE it at its rank - 1.  Two reads of keys and values, and the outputs.
//   reduce by key (lsdsort_reduce_by_key_device): copy keys and values into the workspace | the library's own stable pair sort on the
//       copies, through its public device entry and inside a sub-range of this call's workspace, the value bits as the 32-bit
//       payload | the three phases over the sorted copies.  The sort is stable, so the values of a group meet in input order.
//
// Values are 32-bit words throughout.  MIN and MAX of all three types are one unsigned minimum in a mapped domain (ValueMap: the
// sortable map of the library's float and int order, complemented for MAX), mapped back where a result is stored; integer sums wrap;
// float sums are IEEE additions and nothing but values is ever added: a part without values is skipped by the join, not replaced by
// an identity, so a run of one element keeps its bits.
//
// Stream-ordered, nothing allocated, never synchronises, every launch sized from n alone; for graph capture see include/lsdsort.h.
// Keys and values need the alignment of their word only: 16-byte loads are used where an array starts on a 16-byte line, single
// words otherwise and in the last, partial group.  The tile, its loaders and head flags, the workspace carve-up and the sort of the
// copies are run_tiles.hpp's, shared with unique.hip.
#define LSDSORT_BUILD 1
#include "../../include/lsdsort.h"

#include "lsd_device.hpp"
#include "lsd_host.hpp"
#include "run_tiles.hpp"

namespace {

using namespace lsd;   // run_tiles.hpp: the tile constants, Groups, the loaders, the head flags, the host plumbing

// ---- values and their three operations ----------------------------------------------------------------------------------------
// to_domain(x) = x ^ ((sign(x) ? a : 0) | b) ^ c, where the operation runs; from_domain is its inverse.  Sums: a = b = c = 0.
// MIN / MAX: the unsigned order of the mapped words is the order of the values -- uint32: a = b = 0; int32: b = the top bit; float32:
// a = the other 31 bits as well (the library's total order: -NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN); MAX: c = all ones.
struct ValueMap {
    uint32_t a, b, c;
};

__device__ __forceinline__ uint32_t to_domain(uint32_t x, ValueMap m)
{
    return x ^ (((uint32_t)((int32_t)x >> 31) & m.a) | m.b) ^ m.c;
}

__device__ __forceinline__ uint32_t from_domain(uint32_t t, ValueMap m)
{
    const uint32_t u = t ^ m.c;
    return u ^ (((uint32_t)(~(int32_t)u >> 31) & m.a) | m.b);
}

struct AddWords {   // uint32 and int32 sums: mod 2^32
    static __device__ __forceinline__ uint32_t apply(uint32_t a, uint32_t b) { return a + b; }
};
struct AddFloats {   // one IEEE float32 addition, a the earlier positions
    static __device__ __forceinline__ uint32_t apply(uint32_t a, uint32_t b) { return __float_as_uint(__uint_as_float(a) + __uint_as_float(b)); }
};
struct LeastWord {   // MIN and MAX of every type, in the mapped domain
    static __device__ __forceinline__ uint32_t apply(uint32_t a, uint32_t b) { return b < a ? b : a; }
};

// A stretch of positions.  s == 0: it holds no value (positions at or behind n).  Otherwise bit 0 is set and s >> 1 is 1 + the
// position of its last run head (0: it has none); v is the aggregate of its values from that head on, or of all of them.
struct Part {
    uint32_t s, v;
};

// a, then b behind it.  Associative; a part without values changes nothing, and nothing is ever combined with it.
template <class Op>
__device__ __forceinline__ Part join(Part a, Part b)
{
    if (!(b.s & 1u)) return a;
    if (b.s > 1u || a.s == 0u) return b;   // b holds a head: the run open behind b starts inside it; or there is no a
    return Part{a.s, Op::apply(a.v, b.v)};
}

// Inclusive scan of one part per lane across the wave, the lanes in position order.  All 64 lanes must be active.
template <class Op>
__device__ __forceinline__ Part wave_join_scan(Part x, uint32_t lane)
{
#pragma unroll
    for (int d = 1; d < lsd::kWave; d <<= 1) {
        Part up;
        up.s = __shfl_up(x.s, (unsigned)d, lsd::kWave);
        up.v = __shfl_up(x.v, (unsigned)d, lsd::kWave);
        const Part both = join<Op>(up, x);
        if ((int)lane >= d) x = both;
    }
    return x;
}

// the part of the lane below; nothing for lane 0
__device__ __forceinline__ Part part_below(Part x, uint32_t lane)
{
    Part up;
    up.s = __shfl_up(x.s, 1u, lsd::kWave);
    up.v = __shfl_up(x.v, 1u, lsd::kWave);
    if (lane == 0) up = Part{0u, 0u};
    return up;
}

// This thread's values of `tile`, in the domain of the operation.
template <class Word>
__device__ __forceinline__ void tile_values(const uint32_t* __restrict__ vals, uint32_t n, bool vec, uint32_t tile, uint32_t tid, ValueMap map,
                                            uint32_t (&v)[Groups<Word>::J][Groups<Word>::G])
{
    constexpr uint32_t G = Groups<Word>::G, J = Groups<Word>::J;
#pragma unroll
    for (uint32_t j = 0; j < J; j++) {
        load_words32<Word>(vals, group_start<Word>(tile, j, tid), n, vec, v[j]);
#pragma unroll
        for (uint32_t e = 0; e < G; e++) v[j][e] = to_domain(v[j][e], map);
    }
}

// the part that is position i alone (i < n)
__device__ __forceinline__ Part part_of(uint32_t i, bool head, uint32_t v)
{
    return Part{head ? ((i + 1u) << 1) | 1u : 1u, v};
}

// the part that is this thread's group j: its G positions in order, those at or behind n left out
template <class Word, class Op>
__device__ __forceinline__ Part group_part(uint32_t i0, uint32_t n, uint32_t flags_of_group, const uint32_t (&v)[Groups<Word>::G])
{
    Part t{0u, 0u};
#pragma unroll
    for (uint32_t e = 0; e < Groups<Word>::G; e++) {
        const Part one = i0 + e < n ? part_of(i0 + e, (flags_of_group >> e) & 1u, v[e]) : Part{0u, 0u};
        t = join<Op>(t, one);
    }
    return t;
}

// ------------------------------------------------------------------------------------------------ count
// tile_heads[tile] = number of run heads in the tile; (tile_state, tile_value)[tile] = the tile as a part: 1 + the position of its
// last head (0: none) and the aggregate of its values from that head on -- three plain stores per workgroup, every tile word on
// every call.  The first workgroup clears the unit's fault word, which the scan (behind this kernel's end) may set.
template <class Word, class Op>
__global__ void __launch_bounds__(kRunThreads) rbk_count_kernel(const Word* __restrict__ keys, const uint32_t* __restrict__ vals, uint32_t n,
                                                               uint32_t vec, uint32_t vec_vals, ValueMap map, uint32_t* __restrict__ tile_heads,
                                                               uint32_t* __restrict__ tile_state, uint32_t* __restrict__ tile_value,
                                                               uint32_t* __restrict__ fault)
{
    constexpr uint32_t G = Groups<Word>::G, J = Groups<Word>::J;
    __shared__ uint32_t part_heads[kRunWaves];
    __shared__ uint32_t part_s[J * kRunWaves];
    __shared__ uint32_t part_v[J * kRunWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, tile = blockIdx.x;
    Word k[J][G];
    const uint32_t flags = tile_keys_and_heads<Word>(keys, n, vec != 0, tile, tid, lane, k);
    uint32_t v[J][G];
    tile_values<Word>(vals, n, vec_vals != 0, tile, tid, map, v);
#pragma unroll
    for (uint32_t j = 0; j < J; j++) {
        const Part mine = group_part<Word, Op>(group_start<Word>(tile, j, tid), n, group_flags<Word>(flags, j), v[j]);
        const Part upto = wave_join_scan<Op>(mine, lane);
        if (lane == 63u) {
            part_s[j * kRunWaves + wave] = upto.s;
            part_v[j * kRunWaves + wave] = upto.v;
        }
    }
    const uint32_t heads = lsd::wave_sum((uint32_t)__builtin_popcount(flags));
    if (lane == 0) part_heads[wave] = heads;
    __syncthreads();
    if (tid == 0) {
        uint32_t all = 0;
#pragma unroll
        for (int w = 0; w < kRunWaves; w++) all += part_heads[w];
        Part whole{0u, 0u};   // groups follow each other in the tile as (j, wave)
#pragma unroll
        for (uint32_t x = 0; x < J * (uint32_t)kRunWaves; x++) whole = join<Op>(whole, Part{part_s[x], part_v[x]});
        tile_heads[tile] = all;
        tile_state[tile] = whole.s;
        tile_value[tile] = whole.v;
        if (tile == 0) *fault = 0u;
    }
}

// ------------------------------------------------------------------------------------------------ scan
// tile_heads[t] = heads in tile t  ->  heads in the tiles before t; (tile_state, tile_value)[t] = tile t as a part  ->  the tiles
// before t as one part: 1 + the position of the last head in front of tile t, and what the run open there has gathered (nothing for
// tile 0); *num_runs = the total.  One workgroup, in place, as many rounds of 1024 threads x 4 tiles as the tiles need, the running
// total and the running part carried from round to round.  The arrays are 256-byte aligned and padded, so the last quad is read and
// written whole; its words behind `tiles` count as nothing.  All tiles as one part are the last run: its aggregate and its length
// -- from the last head of all to n -- are stored here; every other run's are stored by the head BEHIND it (emit).
template <class Op>
__global__ void __launch_bounds__(kRunScanThreads) rbk_scan_kernel(uint32_t* __restrict__ tile_heads, uint32_t* __restrict__ tile_state,
                                                                  uint32_t* __restrict__ tile_value, uint32_t tiles, uint32_t n, ValueMap map,
                                                                  uint32_t* __restrict__ num_runs, uint32_t* __restrict__ out_vals,
                                                                  uint32_t* __restrict__ counts, uint32_t* __restrict__ fault)
{
    __shared__ uint32_t part[kRunScanWaves];
    __shared__ uint32_t part_s[kRunScanWaves];
    __shared__ uint32_t part_v[kRunScanWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint4* heads4 = reinterpret_cast<uint4*>(tile_heads);
    uint4* state4 = reinterpret_cast<uint4*>(tile_state);
    uint4* value4 = reinterpret_cast<uint4*>(tile_value);
    uint32_t carry = 0;
    Part carried{0u, 0u};
    for (uint32_t first = 0; first < tiles; first += kRunScanRound) {
        const uint32_t t = first + 4 * tid;
        uint4 h = make_uint4(0, 0, 0, 0), s = make_uint4(0, 0, 0, 0), v = make_uint4(0, 0, 0, 0);
        if (t < tiles) {
            h = heads4[t / 4];
            s = state4[t / 4];
            v = value4[t / 4];
        }
        if (t + 1 >= tiles) h.y = s.y = 0;
        if (t + 2 >= tiles) h.z = s.z = 0;
        if (t + 3 >= tiles) h.w = s.w = 0;
        const Part a0{s.x, v.x}, a1{s.y, v.y}, a2{s.z, v.z}, a3{s.w, v.w};
        const Part mine = join<Op>(join<Op>(join<Op>(a0, a1), a2), a3);
        const Part upto = wave_join_scan<Op>(mine, lane);
        const Part below = part_below(upto, lane);
        if (lane == 63u) {
            part_s[wave] = upto.s;
            part_v[wave] = upto.v;
        }
        uint32_t all = 0;
        const uint32_t excl = carry + lsd::group_exclusive_scan<kRunScanWaves>(h.x + h.y + h.z + h.w, lane, wave, part, &all);   // a barrier inside
        Part running = carried, front = carried;   // the waves of this round in order, behind what the rounds before left
#pragma unroll
        for (uint32_t w = 0; w < (uint32_t)kRunScanWaves; w++) {
            if (w == wave) front = running;
            running = join<Op>(running, Part{part_s[w], part_v[w]});
        }
        if (t < tiles) {
            const Part x0 = join<Op>(front, below), x1 = join<Op>(x0, a0), x2 = join<Op>(x1, a1), x3 = join<Op>(x2, a2);
            heads4[t / 4] = make_uint4(excl, excl + h.x, excl + h.x + h.y, excl + h.x + h.y + h.z);
            state4[t / 4] = make_uint4(x0.s, x1.s, x2.s, x3.s);
            value4[t / 4] = make_uint4(x0.v, x1.v, x2.v, x3.v);
        }
        carry += all;
        carried = running;
        __syncthreads();   // part, part_s and part_v are rewritten by the next round
    }
    if (tid == 0) {
        *num_runs = carry;
        const uint32_t last = carried.s >> 1;   // 1 + the position of the last head of all
        if (carry == 0 || carry > n || !(carried.s & 1u) || last == 0 || last > n) {
            atomicOr(fault, kRunFault);
        } else {
            out_vals[carry - 1] = from_domain(carried.v, map);
            if (counts) counts[carry - 1] = n - (last - 1u);
        }
    }
}

// ------------------------------------------------------------------------------------------------ emit
// The flags again, ranked as in unique.hip: per group the thread's head count, the wave's scan, the waves' totals of every group
// through LDS, one barrier.  Beside them the parts: per group the thread's part, the wave's inclusive scan of parts, the waves' last
// parts of every group through LDS behind the same barrier.  Groups follow each other in the tile as (j, wave, lane), so what lies in
// front of this thread's group j is the part in front of the tile (scanned), the groups below j, the waves below this one in group j
// and the lanes below this one -- joined in that order, then carried on word by word.  A head at position i with rank r: out_keys[r]
// = its word; and where a part `open` lies in front of it, out_vals[r - 1] = its aggregate -- the run that ends at i - 1, whatever
// tiles it began in -- and counts[r - 1] = i - (its last head).  counts may be null.  Every store is guarded by its rank and by
// i < n; nothing is stored where the scan set the fault word.
template <class Word, class Op>
__global__ void __launch_bounds__(kRunThreads) rbk_emit_kernel(const Word* __restrict__ keys, const uint32_t* __restrict__ vals, uint32_t n,
                                                              uint32_t vec, uint32_t vec_vals, ValueMap map,
                                                              const uint32_t* __restrict__ tile_heads, const uint32_t* __restrict__ tile_state,
                                                              const uint32_t* __restrict__ tile_value, const uint32_t* __restrict__ fault,
                                                              Word* __restrict__ out_keys, uint32_t* __restrict__ out_vals,
                                                              uint32_t* __restrict__ counts)
{
    constexpr uint32_t G = Groups<Word>::G, J = Groups<Word>::J;
    __shared__ uint32_t part[J * kRunWaves];
    __shared__ uint32_t part_s[J * kRunWaves];
    __shared__ uint32_t part_v[J * kRunWaves];
    if (*fault != 0u) return;   // uniform
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, tile = blockIdx.x;
    Word k[J][G];
    const uint32_t flags = tile_keys_and_heads<Word>(keys, n, vec != 0, tile, tid, lane, k);
    uint32_t v[J][G];
    tile_values<Word>(vals, n, vec_vals != 0, tile, tid, map, v);
    uint32_t count[J], incl[J];
    Part below[J];   // the lanes below this one in group j, as one part
#pragma unroll
    for (uint32_t j = 0; j < J; j++) {
        count[j] = (uint32_t)__builtin_popcount(group_flags<Word>(flags, j));
        incl[j] = lsd::wave_inclusive_scan(count[j]);
        const Part mine = group_part<Word, Op>(group_start<Word>(tile, j, tid), n, group_flags<Word>(flags, j), v[j]);
        const Part upto = wave_join_scan<Op>(mine, lane);
        below[j] = part_below(upto, lane);
        if (lane == 63u) {
            part[j * kRunWaves + wave] = incl[j];
            part_s[j * kRunWaves + wave] = upto.s;
            part_v[j * kRunWaves + wave] = upto.v;
        }
    }
    __syncthreads();
    const uint32_t base = tile_heads[tile];                    // heads in front of the tile
    Part running{tile_state[tile], tile_value[tile]};          // everything in front of group j of wave w, as one part
    uint32_t heads_below = 0;                                  // heads of the tile in front of group j of wave 0
#pragma unroll
    for (uint32_t j = 0; j < J; j++) {
        uint32_t mine = 0, all = 0;
        Part front = running;
#pragma unroll
        for (uint32_t w = 0; w < (uint32_t)kRunWaves; w++) {
            const uint32_t t = part[j * kRunWaves + w];
            mine += w < wave ? t : 0u;
            all += t;
            if (w == wave) front = running;
            running = join<Op>(running, Part{part_s[j * kRunWaves + w], part_v[j * kRunWaves + w]});
        }
        uint32_t q = heads_below + mine + incl[j] - count[j];   // heads of the tile in front of this thread's group j
        heads_below += all;
        Part open = join<Op>(front, below[j]);                 // everything in front of position i
        const uint32_t i0 = group_start<Word>(tile, j, tid);
#pragma unroll
        for (uint32_t e = 0; e < G; e++) {
            const uint32_t i = i0 + e;
            const bool head = (flags >> (j * G + e)) & 1u;      // a head: i < n
            if (head) {
                const uint32_t r = base + q;
                if (r < n) out_keys[r] = k[j][e];
                const uint32_t start = open.s >> 1;             // 1 + the head of the run that ends at i - 1
                if ((open.s & 1u) && r >= 1u && r <= n && start >= 1u && start <= i) {
                    out_vals[r - 1] = from_domain(open.v, map);
                    if (counts) counts[r - 1] = i - (start - 1u);
                }
                q++;
            }
            if (i < n) open = join<Op>(open, part_of(i, head, v[j][e]));
        }
    }
}

// ------------------------------------------------------------------------------------------------ reduce by key: copy
// key_copy[i] = keys[i], val_copy[i] = vals[i].  One 16-byte group of keys, and the values beside it, per thread and round; the copies
// are 256-byte aligned, the caller's arrays need not be (vec, vec_vals).
template <class Word>
__global__ void __launch_bounds__(kRunThreads) rbk_copy_kernel(const Word* __restrict__ keys, const uint32_t* __restrict__ vals, uint32_t n,
                                                              uint32_t vec, uint32_t vec_vals, Word* __restrict__ key_copy,
                                                              uint32_t* __restrict__ val_copy)
{
    constexpr uint32_t G = Groups<Word>::G;
    const uint32_t groups = (n + G - 1) / G;
    for (uint32_t g = blockIdx.x * kRunThreads + threadIdx.x; g < groups; g += gridDim.x * kRunThreads) {
        const uint32_t i0 = g * G;
        Word k[G];
        uint32_t v[G];
        load_group<Word>(keys, i0, n, vec != 0, k);
        load_words32<Word>(vals, i0, n, vec_vals != 0, v);
        if (i0 + G <= n) {
            store_group<Word>(key_copy, i0, k);
            if constexpr (G == 4) *reinterpret_cast<uint4*>(val_copy + i0) = make_uint4(v[0], v[1], v[2], v[3]);
            else *reinterpret_cast<uint2*>(val_copy + i0) = make_uint2(v[0], v[1]);
        } else {
#pragma unroll
            for (uint32_t e = 0; e < G; e++) {
                if (i0 + e < n) {
                    key_copy[i0 + e] = k[e];
                    val_copy[i0 + e] = v[e];
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ host side
// The tile arrays of the three phases (TileArrays::at): [0] tile_heads, [1] tile_state and [2] tile_value -- a part's s and v, per tile
// and then in front of each tile.  By key the companion of the key copy (RunLayout) is the value copy: always there.
constexpr int kTileArrays = 3;

enum OpKind { kAddWords, kAddFloats, kLeastWord };

// The operation the kernels are built for and the map into its domain; false for what is no (val_type, op).
bool plan_values(int val_type, int op, OpKind* kind, ValueMap* map)
{
    if (val_type != LSDSORT_VAL_U32 && val_type != LSDSORT_VAL_I32 && val_type != LSDSORT_VAL_F32) return false;
    if (op != LSDSORT_REDUCE_SUM && op != LSDSORT_REDUCE_MIN && op != LSDSORT_REDUCE_MAX) return false;
    *map = ValueMap{0u, 0u, 0u};
    if (op == LSDSORT_REDUCE_SUM) {
        *kind = val_type == LSDSORT_VAL_F32 ? kAddFloats : kAddWords;
        return true;
    }
    *kind = kLeastWord;
    if (val_type != LSDSORT_VAL_U32) map->b = 0x80000000u;
    if (val_type == LSDSORT_VAL_F32) map->a = 0x7FFFFFFFu;
    if (op == LSDSORT_REDUCE_MAX) map->c = 0xFFFFFFFFu;
    return true;
}

// count | scan | emit over keys[0 .. n) and vals[0 .. n), n >= 1
template <class Word, class Op>
int run_phases(const Word* keys, const uint32_t* vals, size_t n, ValueMap map, Word* out_keys, uint32_t* out_vals, uint32_t* counts,
               uint32_t* num_runs, uint32_t* fault, char* ws, const TileArrays& A, hipStream_t s)
{
    const uint32_t vec = aligned_to(keys, 16) ? 1u : 0u, vec_vals = aligned_to(vals, 16) ? 1u : 0u;
    uint32_t* tile_heads = reinterpret_cast<uint32_t*>(ws + A.at[0]);
    uint32_t* tile_state = reinterpret_cast<uint32_t*>(ws + A.at[1]);
    uint32_t* tile_value = reinterpret_cast<uint32_t*>(ws + A.at[2]);
    hipLaunchKernelGGL((rbk_count_kernel<Word, Op>), dim3(A.tiles), dim3(kRunThreads), 0, s, keys, vals, (uint32_t)n, vec, vec_vals, map,
                       tile_heads, tile_state, tile_value, fault);
    LSD_HIP(hipGetLastError());
    hipLaunchKernelGGL(rbk_scan_kernel<Op>, dim3(1), dim3(kRunScanThreads), 0, s, tile_heads, tile_state, tile_value, A.tiles, (uint32_t)n, map,
                       num_runs, out_vals, counts, fault);
    LSD_HIP(hipGetLastError());
    hipLaunchKernelGGL((rbk_emit_kernel<Word, Op>), dim3(A.tiles), dim3(kRunThreads), 0, s, keys, vals, (uint32_t)n, vec, vec_vals, map,
                       static_cast<const uint32_t*>(tile_heads), static_cast<const uint32_t*>(tile_state),
                       static_cast<const uint32_t*>(tile_value), static_cast<const uint32_t*>(fault), out_keys, out_vals, counts);
    LSD_HIP(hipGetLastError());
    return LSDSORT_OK;
}

template <class Word>
int run_phases_of(OpKind kind, const void* keys, const void* vals, size_t n, ValueMap map, void* out_keys, void* out_vals, uint32_t* counts,
                  uint32_t* num_runs, uint32_t* fault, char* ws, const TileArrays& A, hipStream_t s)
{
    const Word* k = static_cast<const Word*>(keys);
    const uint32_t* v = static_cast<const uint32_t*>(vals);
    Word* ok = static_cast<Word*>(out_keys);
    uint32_t* ov = static_cast<uint32_t*>(out_vals);
    switch (kind) {
        case kAddWords: return run_phases<Word, AddWords>(k, v, n, map, ok, ov, counts, num_runs, fault, ws, A, s);
        case kAddFloats: return run_phases<Word, AddFloats>(k, v, n, map, ok, ov, counts, num_runs, fault, ws, A, s);
        default: return run_phases<Word, LeastWord>(k, v, n, map, ok, ov, counts, num_runs, fault, ws, A, s);
    }
}

template <class Word>
hipError_t launch_copy(const void* keys, const void* vals, size_t n, void* key_copy, void* val_copy, hipStream_t s)
{
    const size_t groups = (n + Groups<Word>::G - 1) / Groups<Word>::G;
    hipLaunchKernelGGL(rbk_copy_kernel<Word>, dim3(lsd::grid_for(groups, kRunThreads, kRunMaxGrid)), dim3(kRunThreads), 0, s,
                       static_cast<const Word*>(keys), static_cast<const uint32_t*>(vals), (uint32_t)n, aligned_to(keys, 16) ? 1u : 0u,
                       aligned_to(vals, 16) ? 1u : 0u, static_cast<Word*>(key_copy), static_cast<uint32_t*>(val_copy));
    return hipGetLastError();
}

}  // namespace

extern "C" {

size_t lsdsort_reduce_runs_workspace_bytes(size_t n, int key_bits)
{
    if ((key_bits != 32 && key_bits != 64) || n > LSDSORT_MAX_KEYS) return 0;
    return make_tile_arrays(n, kTileArrays, lsd::kCtlBytes).end;
}

int lsdsort_reduce_runs_device(const void* d_keys, const void* d_vals, size_t n, int key_bits, int val_type, int op, void* d_out_keys,
                               void* d_out_vals, uint32_t* d_out_counts, uint32_t* d_num_runs, void* d_workspace, size_t workspace_bytes,
                               void* hip_stream)
{
    OpKind kind;
    ValueMap map;
    if ((key_bits != 32 && key_bits != 64) || !plan_values(val_type, op, &kind, &map)) return LSDSORT_ERR_INVALID_ARG;
    if (n > LSDSORT_MAX_KEYS) return LSDSORT_ERR_TOO_LARGE;
    if (n == 0) return store_zero_runs(d_num_runs, hip_stream);
    const size_t word = (size_t)key_bits / 8;
    if (!d_keys || !d_vals || !d_out_keys || !d_out_vals || !d_num_runs) return LSDSORT_ERR_INVALID_ARG;
    if (!aligned_to(d_keys, word) || !aligned_to(d_vals, 4) || !aligned_to(d_out_keys, word) || !aligned_to(d_out_vals, 4) ||
        !aligned_to(d_out_counts, 4) || !aligned_to(d_num_runs, 4))
        return LSDSORT_ERR_INVALID_ARG;
    if (d_out_keys == d_keys || d_out_vals == d_vals) return LSDSORT_ERR_INVALID_ARG;   // read while the runs are stored
    const TileArrays A = make_tile_arrays(n, kTileArrays, lsd::kCtlBytes);
    if (!lsd::workspace_ok(d_workspace, workspace_bytes, A.end)) return LSDSORT_ERR_WORKSPACE;
    LSD_TRY(lsdsort_prepare_device());
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    char* ws = static_cast<char*>(d_workspace);
    uint32_t* fault = reinterpret_cast<uint32_t*>(ws);
    if (key_bits == 32) return run_phases_of<uint32_t>(kind, d_keys, d_vals, n, map, d_out_keys, d_out_vals, d_out_counts, d_num_runs, fault, ws, A, s);
    return run_phases_of<uint64_t>(kind, d_keys, d_vals, n, map, d_out_keys, d_out_vals, d_out_counts, d_num_runs, fault, ws, A, s);
}

size_t lsdsort_reduce_by_key_workspace_bytes(size_t n, int key_type)
{
    const int key_bits = key_bits_of(key_type);
    if (!key_bits || n > LSDSORT_MAX_KEYS) return 0;
    return make_run_layout(n, key_bits, true, kTileArrays).total;
}

int lsdsort_reduce_by_key_device(const void* d_keys, const void* d_vals, size_t n, int key_type, int descending, int val_type, int op,
                                 void* d_out_keys, void* d_out_vals, uint32_t* d_out_counts, uint32_t* d_num_groups, void* d_workspace,
                                 size_t workspace_bytes, void* hip_stream)
{
    OpKind kind;
    ValueMap map;
    const int key_bits = key_bits_of(key_type);
    if (!key_bits || !plan_values(val_type, op, &kind, &map)) return LSDSORT_ERR_INVALID_ARG;
    if (n > LSDSORT_MAX_KEYS) return LSDSORT_ERR_TOO_LARGE;
    if (n == 0) return store_zero_runs(d_num_groups, hip_stream);
    const size_t word = (size_t)key_bits / 8;
    if (!d_keys || !d_vals || !d_out_keys || !d_out_vals || !d_num_groups) return LSDSORT_ERR_INVALID_ARG;
    if (!aligned_to(d_keys, word) || !aligned_to(d_vals, 4) || !aligned_to(d_out_keys, word) || !aligned_to(d_out_vals, 4) ||
        !aligned_to(d_out_counts, 4) || !aligned_to(d_num_groups, 4))
        return LSDSORT_ERR_INVALID_ARG;
    const RunLayout L = make_run_layout(n, key_bits, true, kTileArrays);
    if (!lsd::workspace_ok(d_workspace, workspace_bytes, L.total)) return LSDSORT_ERR_WORKSPACE;
    LSD_TRY(lsdsort_prepare_device());
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    char* ws = static_cast<char*>(d_workspace);
    uint32_t* fault = reinterpret_cast<uint32_t*>(ws + L.control);
    void* key_copy = ws + L.copy;
    uint32_t* val_copy = reinterpret_cast<uint32_t*>(ws + L.companion);
    // after this copy d_keys and d_vals are no longer read: the outputs may be the inputs themselves
    LSD_HIP(key_bits == 32 ? launch_copy<uint32_t>(d_keys, d_vals, n, key_copy, val_copy, s) : launch_copy<uint64_t>(d_keys, d_vals, n, key_copy, val_copy, s));
    // the sorts are stable in either direction: the values of a group stay in input order
    LSD_TRY(sort_copies(ws, L, n, key_type, descending, hip_stream));
    if (key_bits == 32) return run_phases_of<uint32_t>(kind, key_copy, val_copy, n, map, d_out_keys, d_out_vals, d_out_counts, d_num_groups, fault, ws, L.arrays, s);
    return run_phases_of<uint64_t>(kind, key_copy, val_copy, n, map, d_out_keys, d_out_vals, d_out_counts, d_num_groups, fault, ws, L.arrays, s);
}

int lsdsort_reduce_by_key_check_device(void* d_workspace, size_t n, int key_type, void* hip_stream)
{
    if (!d_workspace) return LSDSORT_ERR_WORKSPACE;
    const int key_bits = key_bits_of(key_type);
    if (!key_bits) return LSDSORT_ERR_INVALID_ARG;
    if (n > LSDSORT_MAX_KEYS) return LSDSORT_ERR_TOO_LARGE;
    if (n == 0) return LSDSORT_OK;   // an empty call touches no workspace
    return check_copies(static_cast<char*>(d_workspace), make_run_layout(n, key_bits, true, kTileArrays), n, hip_stream);
}

}  // extern "C"
