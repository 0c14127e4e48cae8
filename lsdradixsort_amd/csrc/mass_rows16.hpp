// mass_rows16.hpp -- the row helpers of the three softmax-mass units, once: what topp16.hip (the filter), sample16.hip (the draw) and
// logprob16.hip (the log-probabilities of given tokens) do with a float16 / bfloat16 logit row beside the mass arithmetic itself,
// which is keys16_map.hpp's (DESIGN.md sections 6.13 to 6.17).  One definition each, so that the three units cannot drift apart: a
// key has ONE best number and ONE mass in the filter, in the draw and in the log-probability.  Internal linkage, as radix_select.hpp:
// every unit's kernels keep their own symbols, and a unit calls these helpers DIRECTLY from its kernels -- a per-unit wrapper around
// one of them is one more inlining level and changes the register allocation of the kernel.
//
// The row read (read_body / read_front) is the draw's and the log-probabilities': they only read a row.  This header does NOT include
// select_tiles16.hpp, which belongs to the seven selecting units (topp16.hip among them: it stores through that header and keeps its
// load_tile).  read_body is load_tile but for how the bound of a group that is not whole is written -- `q < end && end - q > e` here,
// `q + e < end` there -- and the two stay two: with load_tile in read_body's place 9 of the 13 kernels of the two reading units
// compile to other instructions, all four short kernels among them, with VGPR counts up to 3 higher or lower.  The kernels that were
// measured are the ones with this form; do not "fix" it.
//
// A lane holds two 16-byte groups of its wave's tile: register 8 j + e is body position q0 + 8 (64 j + lane) + e.  A register
// without a key holds kAbsent.
#pragma once

#include "keys16_map.hpp"
#include "lsd_device.hpp"
#include "radix_select.hpp"

namespace lsd {
namespace {

constexpr uint32_t kAbsent = 0xFFFFFFFFu;        // a register without a key: a sortable value is below 65536, and it is no number
using RowKeys = Row<uint16_t>;

// ---- the row read -------------------------------------------------------------------------------------------------------------------
// The wave's tile from body position q0 on, valid below `end`: a whole group by one 16-byte load, the others key by key.
__device__ __forceinline__ void read_body(const RowKeys& r, uint32_t q0, uint32_t end, uint32_t lane, const Key16Map& m, uint32_t (&t)[kRegs])
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
                t[8 * j + e] = kAbsent;
                if (q < end && end - q > (uint32_t)e) t[8 * j + e] = to_sortable16(r.keys[r.head + q + (uint32_t)e], m);
            }
        }
    }
}
// key `lane` of the keys in front of the row's first 16-byte line, for the one wave that owns them
__device__ __forceinline__ uint32_t read_front(const RowKeys& r, uint32_t lane, const Key16Map& m)
{
    return lane < r.head ? to_sortable16(r.keys[lane], m) : kAbsent;
}

// ---- wave arithmetic ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t wave_least(uint32_t v) { return wave_reduce(v, [](uint32_t a, uint32_t b) { return b < a ? b : a; }); }
__device__ __forceinline__ uint32_t best_number(uint32_t s, uint32_t lo, const Values16& v)
{
    const uint32_t n = is_number(s, v) ? s : kAbsent;
    return n < lo ? n : lo;
}
// the sum over the wave of any 64-bit value per lane (the chunk sums of the long rows): every lane ends with it
__device__ __forceinline__ uint64_t wave_add64(uint64_t v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, off, kWave);
    return v;
}
// ln(Z * 2^-32): the conversion rounds Z to 24 bits, the scaling is exact; -inf for Z == 0
__device__ __forceinline__ float log_total(uint64_t z) { return logf((float)z * 2.3283064365386963e-10f); }

// ---- the best number of a row -------------------------------------------------------------------------------------------------------
// Short rows: the best number of the row one wave (WAVES == 1) or one workgroup of WAVES waves holds in registers (read_body's t; h the
// head keys, kAbsent where there is none).  WAVES > 1: through s_min[WAVES] and ONE barrier, which every thread of the group reaches.
template <int WAVES>
__device__ __forceinline__ uint32_t row_best_number(const uint32_t (&t)[kRegs], uint32_t h, uint32_t* s_min, uint32_t wave, uint32_t lane,
                                                    const Values16& v)
{
    uint32_t lo_num = best_number(h, kAbsent, v);
#pragma unroll
    for (int i = 0; i < kRegs; i++) lo_num = best_number(t[i], lo_num, v);
    lo_num = wave_least(lo_num);
    if (WAVES > 1) {
        if (lane == 0u) s_min[wave] = lo_num;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < WAVES; w++) {
            const uint32_t o = s_min[w];
            lo_num = o < lo_num ? o : lo_num;
        }
    }
    return lo_num;
}
// Long rows, one chunk of one row per workgroup of kLongThreads: the best number of chunk c, chunk 0 with the head keys, into the row's
// `word` by integer atomicMin.  Params: a unit's LongParams (keys, cols, chunk, map, val).  s_part: kLongWaves words.  The atomicMin
// stays in here: returned to the kernel, the minimum compiles to other instructions.
template <class Params>
__device__ __forceinline__ void chunk_best_number(const Params& p, uint32_t row, uint32_t c, uint32_t* s_part, uint32_t* word)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const RowKeys r = row_of(p.keys, row, p.cols);
    const ChunkRange g = chunk_of(r, p.chunk, c);
    uint32_t lo_num = best_number((c == 0u && wave == 0u) ? read_front(r, lane, p.map) : kAbsent, kAbsent, p.val);   // uniform
    for (uint32_t tile = g.lo; tile < g.hi; tile += kLongTile) {   // uniform
        uint32_t t[kRegs];
        read_body(r, tile + wave * kWaveTile, g.hi, lane, p.map, t);
#pragma unroll
        for (int i = 0; i < kRegs; i++) lo_num = best_number(t[i], lo_num, p.val);
    }
    lo_num = wave_least(lo_num);
    if (lane == 0u) s_part[wave] = lo_num;
    __syncthreads();
    if (tid != 0u) return;
    for (uint32_t w = 1; w < kLongWaves; w++) lo_num = s_part[w] < lo_num ? s_part[w] : lo_num;
    if (lo_num != kAbsent) atomicMin(word, lo_num);
}

}  // namespace
}  // namespace lsd
