// keys16_map.hpp -- what the two translation units for 16-bit keys share (keys16.hip: the sort; topk16.hip: the select): the map
// from the caller's key type and order to the sortable 16-bit value, and the split of an array of 2-byte keys into the keys in
// front of its first 16-byte line, whole groups of eight from there on, and the keys behind the last whole group.  And the value
// side of a float16 / bfloat16 key: its float32, its softmax mass under the row's temperature and the min-p threshold, one definition
// for topp16.hip's filter, sample16.hip's draw and logprob16.hip (their row helpers: mass_rows16.hpp).
//
// Everything here has internal linkage (an unnamed namespace, as when it lived in keys16.hip): every unit compiles its own copy
// into its own kernels, and the kernels of keys16.hip keep their symbols.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lsdsort.h"
#include "lsd_host.hpp"

namespace {

constexpr uint32_t kGroupKeys = 8;           // keys of one 16-byte access

// The caller's key type and order as the map to the sortable 16-bit value: t = k ^ (k & a ? 0xFFFF : b) ^ c.  uint16 (0, 0),
// int16 (0, 0x8000), float16 and bfloat16 (0x8000, 0x8000): a negative key is complemented, a non-negative one gets its sign bit
// flipped (IEEE total order); c = 0xFFFF for descending.  The 16-bit form of lsd::KeyTransform.
struct Key16Map {
    uint32_t a, b, c;
};
__device__ __forceinline__ uint32_t to_sortable16(uint32_t k, const Key16Map& m) { return k ^ ((k & m.a) ? 0xFFFFu : m.b) ^ m.c; }
// the inverse: u = t ^ c has its top bit SET where the key was not negative
__device__ __forceinline__ uint32_t from_sortable16(uint32_t t, const Key16Map& m)
{
    const uint32_t u = t ^ m.c;
    return u ^ ((~u & m.a) ? 0xFFFFu : m.b);
}

inline int key16_map(int key_type, int descending, Key16Map* m)
{
    *m = Key16Map{0, 0, descending ? 0xFFFFu : 0u};
    switch (key_type) {
        case LSDSORT_KEY16_U16: break;
        case LSDSORT_KEY16_I16: m->b = 0x8000u; break;
        case LSDSORT_KEY16_F16:
        case LSDSORT_KEY16_BF16: m->a = 0x8000u; m->b = 0x8000u; break;
        default: return LSDSORT_ERR_INVALID_ARG;
    }
    return LSDSORT_OK;
}

// The keys by address: `head` keys in front of the first 16-byte line (0..7), `groups` whole groups of eight from there on, and
// `tail` keys behind them (0..7).  Key i of group g is key head + 8 g + i.
struct Span {
    uint32_t head, groups, tail;
};
inline Span span_of(const void* keys, size_t n)
{
    Span s;
    const size_t to_line = ((16 - ((uintptr_t)keys & 15)) & 15) / sizeof(uint16_t);
    s.head = (uint32_t)lsd::min_sz(to_line, n);
    s.groups = (uint32_t)((n - s.head) / kGroupKeys);
    s.tail = (uint32_t)(n - s.head - (size_t)s.groups * kGroupKeys);
    return s;
}
__device__ __forceinline__ const uint4* body_of(const uint16_t* keys, const Span& sp) { return reinterpret_cast<const uint4*>(keys + sp.head); }
__device__ __forceinline__ uint32_t first_tail_key(const Span& sp) { return sp.head + sp.groups * kGroupKeys; }

// ---- the value side of a float16 / bfloat16 key: softmax masses (topp16.hip: the filter; sample16.hip: the draw) -------------------
// One definition, so that a value has ONE mass in every kernel of both units (DESIGN.md sections 6.13 and 6.15).
constexpr int kMassShift = 32;                 // q = floor(w * 2^32)

// The value side of a key type: where the NaNs lie among the sortable values, and the float32 of a key.
struct Values16 {
    uint32_t nan_lo;    // sortable(+inf): the +NaNs lie below it, the -NaNs above 0xFFFF - nan_lo = sortable(-inf)
    uint32_t bf16;      // bfloat16 (else float16)
};
// The map (largest first) and the value side of a float key type, for the entries that weigh keys: float16 or bfloat16 only.
inline int float16_values(int key_type, Key16Map* m, Values16* v)
{
    if (key_type != LSDSORT_KEY16_F16 && key_type != LSDSORT_KEY16_BF16) return LSDSORT_ERR_INVALID_ARG;
    *v = Values16{key_type == LSDSORT_KEY16_BF16 ? 0x007Fu : 0x03FFu, key_type == LSDSORT_KEY16_BF16 ? 1u : 0u};
    return key16_map(key_type, 1, m);
}
__device__ __forceinline__ bool is_number(uint32_t s, const Values16& v) { return s - v.nan_lo <= 0xFFFFu - 2u * v.nan_lo; }   // kNoKey: never
__device__ __forceinline__ float value_of(uint32_t s, const Key16Map& m, const Values16& v)
{
    const uint32_t bits = from_sortable16(s, m) & 0xFFFFu;
    return v.bf16 ? __uint_as_float(bits << 16) : (float)__builtin_bit_cast(_Float16, (uint16_t)bits);
}
// The scale c of a row: the mass of a key is exp2((x - m) * c), c = log2(e) / T.  kLog2e is c of T = 1, the
// literal every mass was taken with before there was a temperature: a NULL temperature array, a T of 1 and the entries without a
// temperature give the same bits.  T above 2^64 (+inf) acts as 2^64, so that c is a positive normal number and -inf * c is no NaN.
// !(T > 0) -- zero, a negative T, a NaN -- and a T so small that c overflows give c = +inf: GREEDY, every key but the maximum's
// duplicates has mass exp2(-inf) = 0.  The division is float64, rounded once more to float32 (above FLT_MAX: to +inf).
constexpr float kLog2e = 1.44269504088896341f;
constexpr float kMaxTemperature = 18446744073709551616.0f;   // 2^64
__device__ __forceinline__ float uniform_f32(float v) { return __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(v))); }
__device__ __forceinline__ float scale_of(float t)
{
    if (!(t > 0.0f)) return __builtin_inff();
    return (float)(1.4426950408889634 / (double)(t < kMaxTemperature ? t : kMaxTemperature));
}
// c of row `row` from the device array (NULL: T = 1 for every row); `row` is the same for the whole wave, and so is c: one SGPR
__device__ __forceinline__ float row_scale(const float* temperature, uint32_t row)
{
    return temperature ? uniform_f32(scale_of(temperature[row])) : kLog2e;
}
__device__ __forceinline__ bool is_greedy(float c) { return c == __builtin_inff(); }
// ln w of a key from x - m: (x - m) * c * ln 2, two roundings; for T = 1 the factor is 1 and the product is x - m itself
__device__ __forceinline__ float log_factor(float c) { return c == kLog2e ? 1.0f : c * 0.693147180559945309f; }

// q of a key that is a number; `best`: value_of(m); c: the row's scale.  The == also defines rows whose best number is an infinity
// (inf - inf) and keeps 0 * inf out of a greedy row; x < best otherwise, so the product is negative or -inf and w <= 1.
__device__ __forceinline__ uint64_t mass_of(float x, float best, float c)
{
    if (x == best) return 1ull << kMassShift;
    const float w = __builtin_amdgcn_exp2f((x - best) * c);
    return w >= 1.0f ? 1ull << kMassShift : (uint64_t)(uint32_t)(w * 4294967296.0f);
}
__device__ __forceinline__ uint64_t mass_of_key(uint32_t s, float best, float c, const Key16Map& m, const Values16& v)
{
    return is_number(s, v) ? mass_of(value_of(s, m, v), best, c) : 0ull;
}

// ---- min-p (topp16.hip) ------------------------------------------------------------------------------------------------------------
// theta = value(m) + T ln(mp) for mp > 0, in float32: logf (1 ulp), then ONE fused multiply-add.  With L = |T ln mp| the logarithm
// contributes at most 2^-23 L and the final rounding at most 2^-24 (|value(m)| + L): the error is below
// B = 2^-22 (|value(m)| + |T ln mp|).  T is the row's temperature (`t`: 1 where there is none), above 2^64 taken as 2^64; a greedy
// row has theta = value(m).  mp >= 1 gives theta >= value(m); a NaN theta (-inf + inf) compares false everywhere: the maximum alone.
__device__ __forceinline__ float minp_theta(float best, float t, float c, float mp)
{
    return is_greedy(c) ? best : fmaf(t < kMaxTemperature ? t : kMaxTemperature, logf(mp), best);
}
// The min-p threshold: the worst sortable value that is a number with value >= theta, and never worse than best_s = sortable(m).
// The numbers lie in [nan_lo, 0xFFFF - nan_lo] and their values fall as s grows (-0.0 behind +0.0 with the same value: theta == 0
// keeps both): a bisection of at most 16 steps, exact given theta.
__device__ __forceinline__ uint32_t minp_threshold(uint32_t best_s, float theta, const Key16Map& m, const Values16& v)
{
    uint32_t lo = best_s, hi = 0xFFFFu - v.nan_lo;
#pragma unroll 1
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1u) >> 1;
        if (value_of(mid, m, v) >= theta) lo = mid;
        else hi = mid - 1u;
    }
    return lo;
}

}  // namespace
