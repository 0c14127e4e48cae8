// unique.hip -- run-length encode and unique for 32- and 64-bit keys.
//
// No reference counterpart: the reference sorts ascending uint32 keys and stops there (LSDRadixSort.cu:62).  What a caller does
// next with sorted keys is find the distinct ones and how often each occurs; this unit does it without going back to torch.
//
//   run-length encode (lsdsort_rle_device): COUNT | SCAN | EMIT, ordered by kernel boundaries only -- no workgroup waits for
//       another, so no kernel can hang.  A tile is 256 threads x 16 keys.  COUNT flags the run heads of its tile
//       (head(i) = i == 0 || key[i] != key[i-1], whole words compared) and stores their number and the position of the last one;
//       SCAN (one workgroup) turns the tile counts into exclusive offsets, carries the last head forward and stores the total;
//       EMIT recomputes the flags, ranks them inside the tile and stores the word and the start of every run at its rank, and
//       every head stores the length of the run before it (the heads of a tile meet in LDS).  Two reads of the keys, and the
//       outputs: no array of starts is written and read again for the counts.
//   unique (lsdsort_unique_device): copy the keys (with their positions 0..n-1 beside them where `first` or `inverse` is asked
//       for) | the library's own sort on the copy, through its public device entry and inside a sub-range of this call's
//       workspace | the run-length kernels over the sorted copy.  The sorts are stable, so the head of every run carries the
//       lowest input position; EMIT stores inverse[pos[i]] = rank of i's run for every i, each position exactly once.
//
// Stream-ordered, nothing allocated, never synchronises, every launch sized from n alone (the number of runs is known on the
// device only and sizes nothing); for graph capture see include/lsdsort.h.  Keys need the alignment of their word only: 16-byte loads are used
// where the array starts on a 16-byte line, single words otherwise and in the last, partial group.
#define LSDSORT_BUILD 1
#include "../../include/lsdsort.h"

#include "lsd_device.hpp"
#include "lsd_host.hpp"
#include "run_tiles.hpp"

namespace {

using namespace lsd;   // run_tiles.hpp: the tile constants, Groups, the loaders, the head flags, the host plumbing

// ------------------------------------------------------------------------------------------------ count
// tile_heads[tile] = number of run heads in the tile, tile_last[tile] = 1 + the position of its last head (0: the tile has none): two
// plain stores per workgroup, every tile word on every call.  The first workgroup clears the unit's fault word, which the scan
// (behind this kernel's end) may set.
template <class Word>
__global__ void __launch_bounds__(kRunThreads) rle_count_kernel(const Word* __restrict__ keys, uint32_t n, uint32_t vec,
                                                               uint32_t* __restrict__ tile_heads, uint32_t* __restrict__ tile_last,
                                                               uint32_t* __restrict__ fault)
{
    constexpr uint32_t G = Groups<Word>::G, J = Groups<Word>::J;
    __shared__ uint32_t part[2 * kRunWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    Word k[J][G];
    const uint32_t flags = tile_keys_and_heads<Word>(keys, n, vec != 0, blockIdx.x, tid, lane, k);
    uint32_t last = 0;   // this thread's groups lie in ascending position order
#pragma unroll
    for (uint32_t j = 0; j < J; j++) {
        const uint32_t f = group_flags<Word>(flags, j);
        if (f) last = group_start<Word>(blockIdx.x, j, tid) + (31u - (uint32_t)__builtin_clz(f)) + 1u;
    }
    const uint32_t heads = lsd::wave_sum((uint32_t)__builtin_popcount(flags));
    last = lsd::wave_max(last);
    if (lane == 0) {
        part[wave] = heads;
        part[kRunWaves + wave] = last;
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t all = 0, top = 0;
#pragma unroll
        for (int w = 0; w < kRunWaves; w++) {
            all += part[w];
            top = part[kRunWaves + w] > top ? part[kRunWaves + w] : top;
        }
        tile_heads[blockIdx.x] = all;
        tile_last[blockIdx.x] = top;
        if (blockIdx.x == 0) *fault = 0u;
    }
}

// ------------------------------------------------------------------------------------------------ scan
// tile_heads[t] = heads in tile t  ->  heads in the tiles before t; tile_last[t]  ->  1 + the position of the last head in the tiles
// before t (0 for tile 0); *num_runs = the total.  One workgroup, in place, as many rounds of 1024 threads x 4 words as the tiles
// need, the running total and the running last head carried from round to round.  The arrays are 256-byte aligned and padded, so the
// last quad is read and written whole; its words behind `tiles` count as 0.  Where the caller wants counts, the last run's -- from
// the last head of all to n -- is stored here: every other run's count is stored by the head BEHIND it (emit).
__global__ void __launch_bounds__(kRunScanThreads) rle_scan_kernel(uint32_t* __restrict__ tile_heads, uint32_t* __restrict__ tile_last,
                                                                  uint32_t tiles, uint32_t n, uint32_t* __restrict__ num_runs,
                                                                  uint32_t* __restrict__ counts, uint32_t* __restrict__ fault)
{
    __shared__ uint32_t part[kRunScanWaves];
    __shared__ uint32_t part_last[kRunScanWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint4* heads4 = reinterpret_cast<uint4*>(tile_heads);
    uint4* last4 = reinterpret_cast<uint4*>(tile_last);
    uint32_t carry = 0, carry_last = 0;
    for (uint32_t first = 0; first < tiles; first += kRunScanRound) {
        const uint32_t t = first + 4 * tid;
        uint4 v = make_uint4(0, 0, 0, 0), l = make_uint4(0, 0, 0, 0);
        if (t < tiles) {
            v = heads4[t / 4];
            l = last4[t / 4];
        }
        if (t + 1 >= tiles) v.y = l.y = 0;
        if (t + 2 >= tiles) v.z = l.z = 0;
        if (t + 3 >= tiles) v.w = l.w = 0;
        // positions ascend with the tiles: the running maximum of "last head" is the last non-zero word
        const uint32_t mine = l.w ? l.w : l.z ? l.z : l.y ? l.y : l.x;
        uint32_t incl_last = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl_last, (unsigned)d, lsd::kWave);
            if ((int)lane >= d) incl_last = up > incl_last ? up : incl_last;
        }
        uint32_t before_last = __shfl_up(incl_last, 1u, lsd::kWave);
        if (lane == 0) before_last = 0;
        if (lane == 63u) part_last[wave] = incl_last;
        uint32_t all = 0;
        const uint32_t excl = carry + lsd::group_exclusive_scan<kRunScanWaves>(v.x + v.y + v.z + v.w, lane, wave, part, &all);   // a barrier inside
        uint32_t all_last = carry_last;
        before_last = before_last > carry_last ? before_last : carry_last;
#pragma unroll
        for (uint32_t w = 0; w < (uint32_t)kRunScanWaves; w++) {
            const uint32_t x = part_last[w];
            if (w < wave) before_last = x > before_last ? x : before_last;
            all_last = x > all_last ? x : all_last;
        }
        if (t < tiles) {
            heads4[t / 4] = make_uint4(excl, excl + v.x, excl + v.x + v.y, excl + v.x + v.y + v.z);
            const uint32_t b1 = l.x ? l.x : before_last, b2 = l.y ? l.y : b1, b3 = l.z ? l.z : b2;
            last4[t / 4] = make_uint4(before_last, b1, b2, b3);
        }
        carry += all;
        carry_last = all_last;
        __syncthreads();   // part and part_last are rewritten by the next round
    }
    if (tid == 0) {
        *num_runs = carry;
        if (carry == 0 || carry > n || carry_last == 0 || carry_last > n) atomicOr(fault, kRunFault);
        else if (counts) counts[carry - 1] = n - (carry_last - 1u);
    }
}

// ------------------------------------------------------------------------------------------------ emit
// The flags again, ranked: per group the thread's head count, the wave's scan, the waves' totals of every group through LDS, one
// barrier.  Groups follow each other in the tile as (j, wave, lane), so the heads in front of this thread's group j are those of
// the groups below j, and of the waves below this one in group j.  A head at position i with rank r = tile_heads[tile] + (heads of
// the tile in front of it): out_keys[r] = its word, starts[r] = i, first[r] = pos[i]; with positions every i stores the rank of its
// run at inverse[pos[i]].  With counts every head also leaves its position in LDS at its rank within the tile, and behind a second
// barrier stores the length of the run BEFORE it, counts[r - 1] = i - (the head before it): the tile's first head takes that head
// from tile_last[tile] (scanned).  No array of starts is written and read again for the counts.  counts, starts, first and inverse
// may each be null.  Nothing is stored where the scan set the fault word.
template <class Word, bool POSITIONS>
__global__ void __launch_bounds__(kRunThreads) rle_emit_kernel(const Word* __restrict__ keys, const uint32_t* __restrict__ pos, uint32_t n,
                                                              uint32_t vec, const uint32_t* __restrict__ tile_heads,
                                                              const uint32_t* __restrict__ tile_last, const uint32_t* __restrict__ fault,
                                                              Word* __restrict__ out_keys, uint32_t* __restrict__ counts,
                                                              uint32_t* __restrict__ starts, uint32_t* __restrict__ first,
                                                              uint32_t* __restrict__ inverse)
{
    constexpr uint32_t G = Groups<Word>::G, J = Groups<Word>::J;
    __shared__ uint32_t part[J * kRunWaves];
    __shared__ uint32_t head_at[kRunTile];   // position of the tile's q-th head
    if (*fault != 0u) return;   // uniform
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, tile = blockIdx.x;
    Word k[J][G];
    const uint32_t flags = tile_keys_and_heads<Word>(keys, n, vec != 0, tile, tid, lane, k);
    uint32_t p[J][G];
    if constexpr (POSITIONS) {
#pragma unroll
        for (uint32_t j = 0; j < J; j++) load_words32<Word>(pos, group_start<Word>(tile, j, tid), n, true, p[j]);
    }
    uint32_t count[J], incl[J];
#pragma unroll
    for (uint32_t j = 0; j < J; j++) {
        count[j] = (uint32_t)__builtin_popcount(group_flags<Word>(flags, j));
        incl[j] = lsd::wave_inclusive_scan(count[j]);
        if (lane == 63u) part[j * kRunWaves + wave] = incl[j];
    }
    __syncthreads();
    const uint32_t base = tile_heads[tile];   // heads in front of the tile
    uint32_t below = 0;                       // heads of the tile in front of group j of wave 0
    uint32_t q0[J];                           // heads of the tile in front of this thread's group j
#pragma unroll
    for (uint32_t j = 0; j < J; j++) {
        uint32_t mine = 0, all = 0;
#pragma unroll
        for (uint32_t w = 0; w < (uint32_t)kRunWaves; w++) {
            const uint32_t t = part[j * kRunWaves + w];
            mine += w < wave ? t : 0u;
            all += t;
        }
        q0[j] = below + mine + incl[j] - count[j];
        below += all;
        uint32_t q = q0[j];
        const uint32_t i0 = group_start<Word>(tile, j, tid);
#pragma unroll
        for (uint32_t e = 0; e < G; e++) {
            const uint32_t i = i0 + e;
            if ((flags >> (j * G + e)) & 1u) {   // a head: i < n
                const uint32_t r = base + q;
                if (r < n) {
                    out_keys[r] = k[j][e];
                    if (starts) starts[r] = i;
                    if constexpr (POSITIONS) {
                        if (first) first[r] = p[j][e];
                    }
                }
                if (counts && q < kRunTile) head_at[q] = i;
                q++;
            }
            if constexpr (POSITIONS) {   // base + q = heads at positions <= i, at least 1: position 0 is one
                if (inverse && i < n && p[j][e] < n) inverse[p[j][e]] = base + q - 1u;
            }
        }
    }
    if (!counts) return;   // uniform
    __syncthreads();
    const uint32_t front = tile_last[tile];   // 1 + the last head in front of the tile; 0 for tile 0 only
#pragma unroll
    for (uint32_t j = 0; j < J; j++) {
        uint32_t q = q0[j];
        const uint32_t i0 = group_start<Word>(tile, j, tid);
#pragma unroll
        for (uint32_t e = 0; e < G; e++) {
            if ((flags >> (j * G + e)) & 1u) {
                const uint32_t i = i0 + e, r = base + q;
                const uint32_t prev = q ? head_at[q - 1] + 1u : front;   // 1 + the head before this one; 0: there is none
                if (r >= 1u && r <= n && prev >= 1u && prev <= i) counts[r - 1] = i - (prev - 1u);
                q++;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ unique: copy
// copy[i] = keys[i], and with positions pos[i] = i.  One 16-byte group of keys per thread and round; copy and pos are 256-byte
// aligned, the caller's keys need not be (vec).
template <class Word, bool POSITIONS>
__global__ void __launch_bounds__(kRunThreads) unique_copy_kernel(const Word* __restrict__ keys, uint32_t n, uint32_t vec,
                                                                 Word* __restrict__ copy, uint32_t* __restrict__ pos)
{
    constexpr uint32_t G = Groups<Word>::G;
    const uint32_t groups = (n + G - 1) / G;
    for (uint32_t g = blockIdx.x * kRunThreads + threadIdx.x; g < groups; g += gridDim.x * kRunThreads) {
        const uint32_t i0 = g * G;
        Word k[G];
        load_group<Word>(keys, i0, n, vec != 0, k);
        if (i0 + G <= n) {
            store_group<Word>(copy, i0, k);
            if constexpr (POSITIONS) {
                if constexpr (G == 4) *reinterpret_cast<uint4*>(pos + i0) = make_uint4(i0, i0 + 1, i0 + 2, i0 + 3);
                else *reinterpret_cast<uint2*>(pos + i0) = make_uint2(i0, i0 + 1);
            }
        } else {
#pragma unroll
            for (uint32_t e = 0; e < G; e++) {
                if (i0 + e < n) {
                    copy[i0 + e] = k[e];
                    if constexpr (POSITIONS) pos[i0 + e] = i0 + e;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ host side
// The tile arrays of the run-length phases (TileArrays::at): [0] tile_heads, [1] tile_last -- 1 + the position of the last head, per
// tile and then in front of each tile.
constexpr int kTileArrays = 2;

// count | scan | emit over keys[0 .. n), n >= 1.  pos: the positions beside the keys, or null (then first and inverse are null too).
template <class Word>
int run_rle(const void* keys_in, const uint32_t* pos, size_t n, void* out, uint32_t* counts, uint32_t* starts, uint32_t* first,
            uint32_t* inverse, uint32_t* num_runs, uint32_t* fault, char* ws, const TileArrays& A, hipStream_t s)
{
    const Word* keys = static_cast<const Word*>(keys_in);
    Word* out_keys = static_cast<Word*>(out);
    const uint32_t vec = aligned_to(keys, 16) ? 1u : 0u;
    uint32_t* tile_heads = reinterpret_cast<uint32_t*>(ws + A.at[0]);
    uint32_t* tile_last = reinterpret_cast<uint32_t*>(ws + A.at[1]);
    hipLaunchKernelGGL(rle_count_kernel<Word>, dim3(A.tiles), dim3(kRunThreads), 0, s, keys, (uint32_t)n, vec, tile_heads, tile_last, fault);
    LSD_HIP(hipGetLastError());
    hipLaunchKernelGGL(rle_scan_kernel, dim3(1), dim3(kRunScanThreads), 0, s, tile_heads, tile_last, A.tiles, (uint32_t)n, num_runs, counts, fault);
    LSD_HIP(hipGetLastError());
    if (pos)
        hipLaunchKernelGGL((rle_emit_kernel<Word, true>), dim3(A.tiles), dim3(kRunThreads), 0, s, keys, pos, (uint32_t)n, vec,
                           static_cast<const uint32_t*>(tile_heads), static_cast<const uint32_t*>(tile_last),
                           static_cast<const uint32_t*>(fault), out_keys, counts, starts, first, inverse);
    else
        hipLaunchKernelGGL((rle_emit_kernel<Word, false>), dim3(A.tiles), dim3(kRunThreads), 0, s, keys, pos, (uint32_t)n, vec,
                           static_cast<const uint32_t*>(tile_heads), static_cast<const uint32_t*>(tile_last),
                           static_cast<const uint32_t*>(fault), out_keys, counts, starts, first, inverse);
    LSD_HIP(hipGetLastError());
    return LSDSORT_OK;
}

template <class Word, bool POSITIONS>
hipError_t launch_copy(const void* keys, size_t n, void* copy, uint32_t* pos, hipStream_t s)
{
    const size_t groups = (n + Groups<Word>::G - 1) / Groups<Word>::G;
    hipLaunchKernelGGL((unique_copy_kernel<Word, POSITIONS>), dim3(lsd::grid_for(groups, kRunThreads, kRunMaxGrid)), dim3(kRunThreads), 0, s,
                       static_cast<const Word*>(keys), (uint32_t)n, aligned_to(keys, 16) ? 1u : 0u, static_cast<Word*>(copy), pos);
    return hipGetLastError();
}

}  // namespace

extern "C" {

size_t lsdsort_rle_workspace_bytes(size_t n, int key_bits)
{
    if ((key_bits != 32 && key_bits != 64) || n > LSDSORT_MAX_KEYS) return 0;
    return make_tile_arrays(n, kTileArrays, lsd::kCtlBytes).end;
}

int lsdsort_rle_device(const void* d_keys, size_t n, int key_bits, void* d_out_keys, uint32_t* d_out_counts, uint32_t* d_out_starts,
                       uint32_t* d_num_runs, void* d_workspace, size_t workspace_bytes, void* hip_stream)
{
    if (key_bits != 32 && key_bits != 64) return LSDSORT_ERR_INVALID_ARG;
    if (n > LSDSORT_MAX_KEYS) return LSDSORT_ERR_TOO_LARGE;
    if (n == 0) return store_zero_runs(d_num_runs, hip_stream);
    const size_t word = (size_t)key_bits / 8;
    if (!d_keys || !d_out_keys || !d_num_runs || d_out_keys == d_keys) return LSDSORT_ERR_INVALID_ARG;
    if (!aligned_to(d_keys, word) || !aligned_to(d_out_keys, word) || !aligned_to(d_out_counts, 4) || !aligned_to(d_out_starts, 4) ||
        !aligned_to(d_num_runs, 4))
        return LSDSORT_ERR_INVALID_ARG;
    const TileArrays A = make_tile_arrays(n, kTileArrays, lsd::kCtlBytes);
    if (!lsd::workspace_ok(d_workspace, workspace_bytes, A.end)) return LSDSORT_ERR_WORKSPACE;
    LSD_TRY(lsdsort_prepare_device());
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    char* ws = static_cast<char*>(d_workspace);
    uint32_t* fault = reinterpret_cast<uint32_t*>(ws);
    if (key_bits == 32) return run_rle<uint32_t>(d_keys, nullptr, n, d_out_keys, d_out_counts, d_out_starts, nullptr, nullptr, d_num_runs, fault, ws, A, s);
    return run_rle<uint64_t>(d_keys, nullptr, n, d_out_keys, d_out_counts, d_out_starts, nullptr, nullptr, d_num_runs, fault, ws, A, s);
}

size_t lsdsort_unique_workspace_bytes(size_t n, int key_type, int with_positions)
{
    const int key_bits = key_bits_of(key_type);
    if (!key_bits || n > LSDSORT_MAX_KEYS) return 0;
    return make_run_layout(n, key_bits, with_positions != 0, kTileArrays).total;
}

int lsdsort_unique_device(const void* d_keys, size_t n, int key_type, int descending, void* d_out_keys, uint32_t* d_out_counts,
                          uint32_t* d_out_first, uint32_t* d_out_inverse, uint32_t* d_num_unique, void* d_workspace, size_t workspace_bytes,
                          void* hip_stream)
{
    const int key_bits = key_bits_of(key_type);
    if (!key_bits) return LSDSORT_ERR_INVALID_ARG;
    if (n > LSDSORT_MAX_KEYS) return LSDSORT_ERR_TOO_LARGE;
    if (n == 0) return store_zero_runs(d_num_unique, hip_stream);
    const size_t word = (size_t)key_bits / 8;
    if (!d_keys || !d_out_keys || !d_num_unique) return LSDSORT_ERR_INVALID_ARG;
    if (!aligned_to(d_keys, word) || !aligned_to(d_out_keys, word) || !aligned_to(d_out_counts, 4) || !aligned_to(d_out_first, 4) ||
        !aligned_to(d_out_inverse, 4) || !aligned_to(d_num_unique, 4))
        return LSDSORT_ERR_INVALID_ARG;
    const bool positions = d_out_first || d_out_inverse;
    const RunLayout L = make_run_layout(n, key_bits, positions, kTileArrays);   // the companion of the key copy: the positions
    if (!lsd::workspace_ok(d_workspace, workspace_bytes, L.total)) return LSDSORT_ERR_WORKSPACE;
    LSD_TRY(lsdsort_prepare_device());
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    char* ws = static_cast<char*>(d_workspace);
    uint32_t* fault = reinterpret_cast<uint32_t*>(ws + L.control);
    void* copy = ws + L.copy;
    uint32_t* pos = positions ? reinterpret_cast<uint32_t*>(ws + L.companion) : nullptr;
    // after this copy d_keys is no longer read: d_out_keys may be d_keys itself
    if (key_bits == 32) LSD_HIP(positions ? (launch_copy<uint32_t, true>(d_keys, n, copy, pos, s)) : (launch_copy<uint32_t, false>(d_keys, n, copy, pos, s)));
    else LSD_HIP(positions ? (launch_copy<uint64_t, true>(d_keys, n, copy, pos, s)) : (launch_copy<uint64_t, false>(d_keys, n, copy, pos, s)));
    // the sorts are stable in either direction: the head of every run carries the lowest input position
    LSD_TRY(sort_copies(ws, L, n, key_type, descending, hip_stream));
    if (key_bits == 32) return run_rle<uint32_t>(copy, pos, n, d_out_keys, d_out_counts, nullptr, d_out_first, d_out_inverse, d_num_unique, fault, ws, L.arrays, s);
    return run_rle<uint64_t>(copy, pos, n, d_out_keys, d_out_counts, nullptr, d_out_first, d_out_inverse, d_num_unique, fault, ws, L.arrays, s);
}

int lsdsort_unique_check_device(void* d_workspace, size_t n, int key_type, int with_positions, void* hip_stream)
{
    if (!d_workspace) return LSDSORT_ERR_WORKSPACE;
    const int key_bits = key_bits_of(key_type);
    if (!key_bits) return LSDSORT_ERR_INVALID_ARG;
    if (n > LSDSORT_MAX_KEYS) return LSDSORT_ERR_TOO_LARGE;
    if (n == 0) return LSDSORT_OK;   // an empty call touches no workspace
    return check_copies(static_cast<char*>(d_workspace), make_run_layout(n, key_bits, with_positions != 0, kTileArrays), n, hip_stream);
}

}  // extern "C"


