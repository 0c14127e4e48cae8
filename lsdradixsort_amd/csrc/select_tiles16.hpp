// select_tiles16.hpp -- the tile helpers of the 16-bit row selects, once: what topk16.hip, kth16.hip, kth16_multi.hip,
// kth16_rowk.hip and topp16.hip do with one wave's tile of a Row<uint16_t>.  Internal linkage, as
// radix_select.hpp: every unit's kernels keep their own symbols, and a unit calls these helpers DIRECTLY from its kernels -- a
// per-unit wrapper around one of them is one more inlining level and changes the register allocation of the kernel.  The count and
// the locate kernel of the two single-rank k-th value units are kernel TEMPLATES here, instantiated under each unit's name.
//
// Key reads.  A row starts 2 r cols bytes past the keys, at any even offset within a 16-byte line.  Every kernel therefore splits
// EACH ROW by address (Row): `head` keys in front of the row's first 16-byte line (0..7), read one by one, and the `body` from that
// line on, read as 16-byte groups of eight keys; the last group of a row (or chunk) that is not whole is read one by one too.  A
// lane holds two groups of its wave's tile: register 8 j + e is body position q0 + 8 (64 j + lane) + e.  A register without a key
// holds kNoKey = 0xFFFFFFFF: a sortable value is below 65536, so no (prefix, shift) of a select matches it and the 32-bit
// loaders' validity mask (select_tiles32.hpp) is not needed.
#pragma once

#include "keys16_map.hpp"
#include "lsd_device.hpp"
#include "radix_select.hpp"

namespace lsd {
namespace {

constexpr uint32_t kNoKey = 0xFFFFFFFFu;     // a sortable value is below 65536
constexpr uint32_t kHeadBit = 1u << kRegs;   // match mask: the head register
using Row16 = Row<uint16_t>;   // a lane holds two 16-byte groups of eight keys of its wave's tile

// a select whose levels always all run, so that the prefix is the whole value (values only, and the filters)
struct StopNever16 {
    static __device__ __forceinline__ bool stops(uint32_t, uint32_t) { return false; }
};

// ---- loads ----------------------------------------------------------------------------------------------------------------------
// The wave's tile from body position q0 on, valid below `end`: a whole group by one 16-byte load, the others key by key.
__device__ __forceinline__ void load_tile(const Row16& r, uint32_t q0, uint32_t end, uint32_t lane, const Key16Map& m, uint32_t (&t)[kRegs])
{
#pragma unroll
    for (int j = 0; j < kRegs / 8; j++) {
        const uint32_t q = q0 + ((uint32_t)j * 64u + lane) * kGroupKeys;
        if (q < end && end - q >= kGroupKeys) {
            const uint4 v = *reinterpret_cast<const uint4*>(r.keys + r.head + q);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int i = 0; i < 4; i++) {
                t[8 * j + 2 * i] = to_sortable16(w[i] & 0xFFFFu, m);
                t[8 * j + 2 * i + 1] = to_sortable16(w[i] >> 16, m);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; e++) {
                t[8 * j + e] = kNoKey;
                if (q + (uint32_t)e < end) t[8 * j + e] = to_sortable16(r.keys[r.head + q + (uint32_t)e], m);
            }
        }
    }
}
// head key `lane` of the row, for the one wave that owns the head
__device__ __forceinline__ uint32_t load_head(const Row16& r, uint32_t lane, const Key16Map& m)
{
    return lane < r.head ? to_sortable16(r.keys[lane], m) : kNoKey;
}

// ---- locate ---------------------------------------------------------------------------------------------------------------------
// Locate within one tile held in registers (load_tile at q0; h: the head keys in front of it, kNoKey where there is none).  `base`:
// the keys under the prefix before this tile in the row; it moves on past the tile.  If the `need`-th (1-based) such key of the row
// lies in this tile, the lane that holds it stores it, un-mapped, and its position at o.at(row, slot) of o.keys and o.idx (may be
// null): `row` in a single-rank unit, row * slots + slot in the multi-rank one.  Returns whether it did (uniform over the group).
// s_wc: WAVES words.  The store stays a lambda inside `if (here)` and the index is computed in it: a store callable passed in, or
// an index computed by the caller, allocates the kernels' registers differently.
template <int WAVES, class Out>
__device__ __forceinline__ bool locate_tile(const uint32_t (&t)[kRegs], uint32_t h, uint32_t q0, const Row16& r, uint32_t prefix,
                                            uint32_t shift, uint32_t need, uint32_t& base, volatile lds_u32* s_wc, uint32_t wave,
                                            uint32_t lane, uint32_t row, uint32_t slot, const Out& o, const Key16Map& m)
{
    uint32_t em = (h >> shift) == prefix ? kHeadBit : 0u;   // the keys under the prefix (kNoKey never is)
#pragma unroll
    for (int i = 0; i < kRegs; i++) em |= (t[i] >> shift) == prefix ? 1u << i : 0u;
    const uint32_t mine = wave_sum((uint32_t)__builtin_popcount(em));
    uint32_t before = base, all = mine;
    if (WAVES > 1) {
        if (lane == 0u) s_wc[wave] = mine;
        __syncthreads();
        all = 0u;
        for (uint32_t w = 0; w < (uint32_t)WAVES; w++) {
            const uint32_t c = s_wc[w];
            if (w < wave) before += c;
            all += c;
        }
        __syncthreads();   // the next tile writes s_wc again
    }
    const bool here = base < need && need - base <= all;   // uniform
    if (here) {
        auto store = [&](uint32_t key, uint32_t pos) {
            if (row < o.rows) {
                const size_t at = o.at(row, slot);
                o.keys[at] = (uint16_t)from_sortable16(key, m);
                if (o.idx) o.idx[at] = pos;
            }
        };
        // position order: the head keys by lane, then group j of lane 0, 1, .. 63, j = 0, 1
        const uint32_t ch = em >> kRegs;
        const uint32_t hi = wave_inclusive_scan(ch);
        if (ch != 0u && before + hi == need) store(h, lane);
        before += (uint32_t)__builtin_amdgcn_readlane((int)hi, 63);
#pragma unroll
        for (int j = 0; j < kRegs / 8; j++) {
            const uint32_t g = (em >> (8 * j)) & 0xFFu, c = (uint32_t)__builtin_popcount(g);
            const uint32_t incl = wave_inclusive_scan(c), lo = before + incl - c;
            if (lo < need && need - lo <= c) {
                uint32_t left = need - lo;   // 1 .. c: which of this group's matching keys
                const uint32_t pos = r.head + q0 + ((uint32_t)j * 64u + lane) * kGroupKeys;
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    if (((g >> e) & 1u) != 0u && --left == 0u) store(t[8 * j + e], pos + (uint32_t)e);
                }
            }
            before += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        }
    }
    base += all;
    return here;
}

// ---- the filters' stores --------------------------------------------------------------------------------------------------------
// The store of one tile held in registers (load_tile at q0, valid below `end`) into the destination row `orow`: a key is kept where
// (key >> shift) <= prefix and becomes `fill` elsewhere -- the top-k filter's prefix and shift, or a whole threshold with shift 0
// (a literal 0 folds away).  `vec`: the destination row has the source row's 16-byte phase, so a whole group is one 16-byte store
// at the address the load had; otherwise, and behind the last whole group, key by key.  Every store is below `end`, that is inside
// the row.
__device__ __forceinline__ void store_tile(uint16_t* orow, bool vec, const Row16& r, uint32_t q0, uint32_t end, uint32_t lane,
                                           const uint32_t (&t)[kRegs], uint32_t prefix, uint32_t shift, uint32_t fill, const Key16Map& m)
{
#pragma unroll
    for (int j = 0; j < kRegs / 8; j++) {
        const uint32_t q = q0 + ((uint32_t)j * 64u + lane) * kGroupKeys;
        if (q >= end) continue;
        uint32_t w[8];
#pragma unroll
        for (int e = 0; e < 8; e++) w[e] = (t[8 * j + e] >> shift) <= prefix ? from_sortable16(t[8 * j + e], m) & 0xFFFFu : fill;
        if (vec && end - q >= kGroupKeys) {
            *reinterpret_cast<uint4*>(orow + r.head + q) = make_uint4(w[0] | (w[1] << 16), w[2] | (w[3] << 16), w[4] | (w[5] << 16), w[6] | (w[7] << 16));
        } else {
#pragma unroll
            for (int e = 0; e < 8; e++)
                if (q + (uint32_t)e < end) orow[r.head + q + (uint32_t)e] = (uint16_t)w[e];
        }
    }
}
// the head keys of the row, by the one wave that owns them
__device__ __forceinline__ void store_head(uint16_t* orow, const Row16& r, uint32_t lane, uint32_t h, uint32_t prefix, uint32_t shift,
                                           uint32_t fill, const Key16Map& m)
{
    if (lane < r.head) orow[lane] = (uint16_t)((h >> shift) <= prefix ? from_sortable16(h, m) : fill);
}
__device__ __forceinline__ bool same_phase(const void* a, const void* b) { return (((uintptr_t)a ^ (uintptr_t)b) & 15u) == 0u; }

// ---- long rows: kernel bodies that do not depend on the unit --------------------------------------------------------------------
// LP is the unit's LongParams: keys, cols, chunk, chunks, state, hist, map, out.rows (hist_level's needs and the loaders').

// One chunk of one row per workgroup: the digit of every key under the row's prefix, counted in LDS.  LEVEL 0: the top 11 bits
// of every key; LEVEL 1: the low 5 bits of the keys whose top 11 are the prefix.  A done row returns at once.
template <int LEVEL, class LP>
__device__ __forceinline__ void hist_level16(const LP& p, uint32_t* s_hist)
{
    hist_level(p, s_hist, [&](uint32_t row, uint32_t c, const uint4& st, uint32_t lane, uint32_t wave) __attribute__((always_inline)) {
        const Row16 r = row_of(p.keys, row, p.cols);
        const ChunkRange g = chunk_of(r, p.chunk, c);
        auto count = [&](uint32_t key) __attribute__((always_inline)) {
            const bool match = LEVEL == 0 ? key != kNoKey : (key >> Levels16::shift(0)) == st.x;
            count_digit(s_hist, match, (key >> Levels16::shift(LEVEL)) & ((1u << Levels16::bits(LEVEL)) - 1u), lane);
        };
        if (c == 0u && wave == 0u) count(load_head(r, lane, p.map));   // uniform
        for (uint32_t tile = g.lo; tile < g.hi; tile += kLongTile) {   // uniform
            uint32_t t[kRegs];
            load_tile(r, tile + wave * kWaveTile, g.hi, lane, p.map, t);
#pragma unroll
            for (int i = 0; i < kRegs; i++) count(t[i]);
        }
    });
}

// Values only (kth16.hip, kth16_rowk.hip), row `at` and on by `step` -- the kernel's own blockIdx.x * blockDim.x + threadIdx.x and
// gridDim.x * blockDim.x: read in here, blockDim is no longer the kernel's known workgroup size.  After both levels the prefix is
// the row's whole sortable value (shift 0, need not 0).  Anything else is a row the unit's clear kernel refused from the start
// (state w == BAD_W with no level run: reported by `fault_bad`; BAD_W 0: the unit has no such rows), a row whose counts fell short
// (its fault bit is set) or one no scan has visited -- never: nothing is stored for it.
template <uint32_t BAD_W, class LP>
__device__ __forceinline__ void store_values16(uint32_t at, uint32_t step, const LP& p, uint32_t fault_locate, uint32_t fault_bad)
{
    for (uint32_t row = at; row < p.out.rows; row += step) {
        const uint4 st = p.state[row];
        if (st.y == 0u && st.z != 0u) p.out.keys[row] = (uint16_t)from_sortable16(st.x & 0xFFFFu, p.map);
        else atomicOr(p.out.fault, (BAD_W != 0u && st.y == Levels16::kNoLevel && st.w == BAD_W) ? fault_bad : fault_locate);
    }
}

// ---- long rows: the count and the locate of the single-rank units (kth16.hip, kth16_rowk.hip) -----------------------------------
// Kernel templates, with radix_select.hpp's pick_rows_kernel between them; U is the unit's own struct (U::Params: its LongParams).
// The 32-bit pair reads keys under a validity mask and is kth.hip's own.

// the keys under the prefix, per chunk
template <class U>
__global__ void __launch_bounds__(kLongThreads) count_rows16_kernel(const typename U::Params p)
{
    __shared__ uint32_t s_part[kLongWaves];
    const uint32_t row = blockIdx.x / p.chunks, c = blockIdx.x % p.chunks;
    if (row >= p.out.rows) return;
    const uint4 st = p.state[row];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const Row16 r = row_of(p.keys, row, p.cols);
    const ChunkRange g = chunk_of(r, p.chunk, c);
    uint32_t ne = 0u;
    // (uniform) else: a row no scan has visited or that was refused from the start, or one whose counts fell short
    if (st.y < Levels16::kNoLevel && st.z != 0u) {
        if (c == 0u && wave == 0u) ne += (load_head(r, lane, p.map) >> st.y) == st.x ? 1u : 0u;   // uniform
        for (uint32_t tile = g.lo; tile < g.hi; tile += kLongTile) {   // uniform
            uint32_t t[kRegs];
            load_tile(r, tile + wave * kWaveTile, g.hi, lane, p.map, t);
#pragma unroll
            for (int i = 0; i < kRegs; i++) ne += (t[i] >> st.y) == st.x ? 1u : 0u;
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

// One workgroup per row reads the picked chunk, and only up to the tile that holds the key.
template <class U>
__global__ void __launch_bounds__(kLongThreads) locate_rows16_kernel(const typename U::Params p)
{
    __shared__ uint32_t s_wc_raw[kLongWaves];
    const uint32_t row = blockIdx.x;
    if (row >= p.out.rows) return;
    const uint4 st = p.state[row];
    if (st.z == 0u || st.w >= p.chunks) return;   // (uniform) nothing was picked: the pick has set the row's fault bit
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const Row16 r = row_of(p.keys, row, p.cols);
    const ChunkRange g = chunk_of(r, p.chunk, st.w);
    volatile lds_u32* const s_wc = (volatile lds_u32*)(lds_u32*)s_wc_raw;
    uint32_t base = 0u;
    bool found = false;
    // chunk 0 has at least one tile (a long row's body is longer than its head), and its first tile carries the head
    for (uint32_t tile = g.lo; tile < g.hi && !found; tile += kLongTile) {   // uniform
        const uint32_t q0 = tile + wave * kWaveTile;
        uint32_t t[kRegs];
        load_tile(r, q0, g.hi, lane, p.map, t);
        const uint32_t h = (st.w == 0u && tile == g.lo && wave == 0u) ? load_head(r, lane, p.map) : kNoKey;   // uniform
        found = locate_tile<(int)kLongWaves>(t, h, q0, r, st.x, st.y, st.z, base, s_wc, wave, lane, row, 0u, p.out, p.map);
    }
    if (!found && tid == 0u) atomicOr(p.out.fault, kKthFaultLocate);
}

}  // namespace
}  // namespace lsd
