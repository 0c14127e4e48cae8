// run_tiles.hpp -- what the two run units share, once: unique.hip (run-length encode and unique) and reduce_by_key.hip are one shape,
// COUNT | SCAN | EMIT over tiles of 256 threads x 16 keys, with a copy kernel in front and the library's own sort in the middle for the
// "by key" entries (DESIGN.md sections 6.18 and 6.19).  Here: the tile constants, a thread's groups of a tile and their loaders and
// stores, the head flags of a tile, the one-word store of an empty call; and on the host side the workspace carve-up of both kinds of
// entry, the sort of the copies and the check entry's two reads.  One definition each, so that the units cannot drift apart: the head
// flags carry the lane-0 reload, the `i < n` guard and the whole-word compare of 64-bit keys, load_group the fallback for an array
// that starts on no 16-byte line.  Internal linkage, as mass_rows16.hpp: a unit's kernels stay in its own global anonymous namespace
// (behind `using namespace lsd;`) and keep their symbols, and they call these helpers DIRECTLY -- a per-unit wrapper around one of
// them is one more inlining level and changes the register allocation of the kernel.  What a kernel does
// between the helpers stays in the kernel for the same reason.
#pragma once

#include "lsd_device.hpp"
#include "lsd_host.hpp"

namespace lsd {
namespace {

constexpr int kRunThreads = 256;
constexpr int kRunWaves = kRunThreads / kWave;
constexpr uint32_t kRunThreadKeys = 16;
constexpr uint32_t kRunTile = kRunThreads * kRunThreadKeys;   // keys of a workgroup: 4096
constexpr int kRunScanThreads = 1024;
constexpr int kRunScanWaves = kRunScanThreads / kWave;
constexpr uint32_t kRunScanRound = 4 * kRunScanThreads;       // tiles the one-workgroup scan takes per round: 4096
constexpr uint32_t kRunMaxGrid = 2048;                        // workgroups of the grid-stride copy kernels
constexpr uint32_t kRunFault = 1u;                            // the scanned total or the last head is 0 or above n: never expected

// ---- a tile in registers --------------------------------------------------------------------------------------------------------
// A thread holds its 16 keys as J groups of G words, one 16-byte load each; group j of thread t is the G keys from
// tile * kRunTile + (j * 256 + t) * G, so that the lanes of a wave read consecutive 16-byte lines.  A tile's keys in position order
// are indexed (group, wave, lane, word).
template <class Word>
struct Groups {
    static constexpr uint32_t G = 16 / sizeof(Word);        // 4 | 2
    static constexpr uint32_t J = kRunThreadKeys / G;       // 4 | 8
};

template <class Word>
__device__ __forceinline__ uint32_t group_start(uint32_t tile, uint32_t j, uint32_t tid)
{
    return tile * kRunTile + (j * kRunThreads + tid) * Groups<Word>::G;   // below 2^30 + 4096
}

// the G flags of group j out of a thread's J * G (tile_keys_and_heads)
template <class Word>
__device__ __forceinline__ uint32_t group_flags(uint32_t flags, uint32_t j)
{
    return (flags >> (j * Groups<Word>::G)) & ((1u << Groups<Word>::G) - 1u);
}

// The G words from i0 (a multiple of G); words at or behind n read as 0.  vec: the array starts on a 16-byte line.
template <class Word>
__device__ __forceinline__ void load_group(const Word* __restrict__ keys, uint32_t i0, uint32_t n, bool vec, Word (&k)[Groups<Word>::G])
{
    constexpr uint32_t G = Groups<Word>::G;
    if (vec && i0 + G <= n) {
        const uint4 v = *reinterpret_cast<const uint4*>(keys + i0);
        if constexpr (sizeof(Word) == 4) {
            k[0] = v.x; k[1] = v.y; k[2] = v.z; k[3] = v.w;
        } else {
            k[0] = (Word)v.x | (Word)v.y << 32;
            k[1] = (Word)v.z | (Word)v.w << 32;
        }
    } else {
#pragma unroll
        for (uint32_t e = 0; e < G; e++) k[e] = i0 + e < n ? keys[i0 + e] : (Word)0;
    }
}

// The 32-bit words beside the keys -- unique's positions, reduce's values: the same groups of a uint32 array, 16 or 8 bytes each.
// vec: the array starts on a 16-byte line (the copies inside a workspace are 256-byte aligned: a literal true).
template <class Word>
__device__ __forceinline__ void load_words32(const uint32_t* __restrict__ words, uint32_t i0, uint32_t n, bool vec, uint32_t (&v)[Groups<Word>::G])
{
    constexpr uint32_t G = Groups<Word>::G;
    if (vec && i0 + G <= n) {
        if constexpr (G == 4) {
            const uint4 q = *reinterpret_cast<const uint4*>(words + i0);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
            const uint2 q = *reinterpret_cast<const uint2*>(words + i0);
            v[0] = q.x; v[1] = q.y;
        }
    } else {
#pragma unroll
        for (uint32_t e = 0; e < G; e++) v[e] = i0 + e < n ? words[i0 + e] : 0u;
    }
}

// One whole group of keys into a 256-byte aligned copy: one 16-byte store.
template <class Word>
__device__ __forceinline__ void store_group(Word* __restrict__ copy, uint32_t i0, const Word (&k)[Groups<Word>::G])
{
    if constexpr (sizeof(Word) == 4)
        *reinterpret_cast<uint4*>(copy + i0) = make_uint4(k[0], k[1], k[2], k[3]);
    else
        *reinterpret_cast<uint4*>(copy + i0) = make_uint4((uint32_t)k[0], (uint32_t)(k[0] >> 32), (uint32_t)k[1], (uint32_t)(k[1] >> 32));
}

// This thread's keys of `tile` and their head flags: bit j * G + e is set where key (j, e) lies below n and is position 0 or
// differs from the key in front of it.  That key is the one before it in the group, for a group's first key the last key of the
// lane below, and for lane 0 one more global load.  All 64 lanes of every wave must be active.
template <class Word>
__device__ __forceinline__ uint32_t tile_keys_and_heads(const Word* __restrict__ keys, uint32_t n, bool vec, uint32_t tile, uint32_t tid,
                                                        uint32_t lane, Word (&k)[Groups<Word>::J][Groups<Word>::G])
{
    constexpr uint32_t G = Groups<Word>::G, J = Groups<Word>::J;
#pragma unroll
    for (uint32_t j = 0; j < J; j++) load_group<Word>(keys, group_start<Word>(tile, j, tid), n, vec, k[j]);
    uint32_t flags = 0;
#pragma unroll
    for (uint32_t j = 0; j < J; j++) {
        const uint32_t i0 = group_start<Word>(tile, j, tid);
        Word before = __shfl_up(k[j][G - 1], 1u, kWave);
        if (lane == 0 && i0 > 0 && i0 < n) before = keys[i0 - 1];
#pragma unroll
        for (uint32_t e = 0; e < G; e++) {
            const uint32_t i = i0 + e;
            const bool head = i < n && (i == 0 || k[j][e] != (e ? k[j][e - 1] : before));
            flags |= (head ? 1u : 0u) << (j * G + e);
        }
    }
    return flags;
}

// one word: the count of an empty call
__global__ void __launch_bounds__(kWave) run_store_kernel(uint32_t* __restrict__ word, uint32_t value)
{
    if (threadIdx.x == 0) *word = value;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
// 32 | 64, or 0 for what is no lsdsort_key_type
int key_bits_of(int key_type)
{
    if (key_type >= LSDSORT_KEY_U32 && key_type <= LSDSORT_KEY_F32) return 32;
    if (key_type >= LSDSORT_KEY_U64 && key_type <= LSDSORT_KEY_F64) return 64;
    return 0;
}

bool aligned_to(const void* p, size_t bytes) { return ((uintptr_t)p & (bytes - 1)) == 0; }

// the count of an empty call: one stream-ordered 4-byte store, where the caller gave the word
int store_zero_runs(uint32_t* d_num, void* hip_stream)
{
    if (!d_num) return LSDSORT_OK;
    if (!aligned_to(d_num, 4)) return LSDSORT_ERR_INVALID_ARG;
    LSD_TRY(lsdsort_prepare_device());
    hipLaunchKernelGGL(run_store_kernel, dim3(1), dim3(kWave), 0, static_cast<hipStream_t>(hip_stream), d_num, 0u);
    LSD_HIP(hipGetLastError());
    return LSDSORT_OK;
}

// The per-tile arrays of the three phases, behind whatever the entry keeps in front of them: `count` arrays (2 for run lengths: heads
// and last head; 3 for reduce: heads and a part's two words) of uint32[tiles], each padded -- the scan reads and writes whole quads.
struct TileArrays {
    uint32_t tiles = 1;
    size_t at[3] = {0, 0, 0};
    size_t end = 0;
};

TileArrays make_tile_arrays(size_t n, int count, size_t off)
{
    TileArrays A;
    A.tiles = grid_for(n, kRunTile, (size_t)1 << 31);
    for (int a = 0; a < count; a++) {
        A.at[a] = off;
        off += align_up(A.tiles * sizeof(uint32_t));
    }
    A.end = off;
    return A;
}

// The carve-up of the entries that sort a copy: control block (fault word first) | key copy | its 32-bit companion (unique's
// positions where they are asked for, reduce's values) | the sort's workspace | the tile arrays.
struct RunLayout {
    int key_bits = 32;
    bool with_companion = false;
    size_t control = 0;
    size_t copy = 0;
    size_t companion = 0;
    size_t sort_ws = 0;
    size_t sort_ws_bytes = 0;
    TileArrays arrays;
    size_t total = 0;
};

RunLayout make_run_layout(size_t n, int key_bits, bool with_companion, int tile_arrays)
{
    RunLayout L;
    L.key_bits = key_bits;
    L.with_companion = with_companion;
    size_t off = 0;
    L.control = off; off += kCtlBytes;
    L.copy = off; off += align_up(n * (size_t)(key_bits / 8));
    L.companion = off; off += with_companion ? align_up(n * sizeof(uint32_t)) : 0;
    L.sort_ws = off;
    L.sort_ws_bytes = key_bits == 32 ? lsdsort_workspace_bytes(n, 8, with_companion ? 1 : 0)
                                     : lsdsort_wide_workspace_bytes(n, 8, 64, with_companion ? 32 : 0);
    off += align_up(L.sort_ws_bytes);
    L.arrays = make_tile_arrays(n, tile_arrays, off);
    L.total = L.arrays.end;
    return L;
}

// The library's own sort on the copies, through the public device entry of the keys' width, the companion as the 32-bit payload.
// The sorts are stable in either direction: equal keys stay in input order.
int sort_copies(char* ws, const RunLayout& L, size_t n, int key_type, int descending, void* hip_stream)
{
    uint32_t* companion = L.with_companion ? reinterpret_cast<uint32_t*>(ws + L.companion) : nullptr;
    if (L.key_bits == 32) return lsdsort_keys_device(ws + L.copy, companion, ws + L.sort_ws, L.sort_ws_bytes, n, 8, key_type, descending, hip_stream);
    return lsdsort_keys64_device(ws + L.copy, companion, L.with_companion ? 32 : 0, ws + L.sort_ws, L.sort_ws_bytes, n, 8, key_type, descending,
                                 hip_stream);
}

// The check entry's two reads: the unit's own word, then the sort's inside its sub-range.  The first synchronises the stream.
int check_copies(char* ws, const RunLayout& L, size_t n, void* hip_stream)
{
    auto word_at = [&](size_t off) { return lsdsort_check_device(ws + off, hip_stream); };
    LSD_TRY(word_at(L.control));
    if (L.key_bits == 32) return word_at(L.sort_ws);
    return lsdsort_wide_check_device(ws + L.sort_ws, n, 8, 64, L.with_companion ? 32 : 0, hip_stream);
}

}  // namespace
}  // namespace lsd
