// keys16_map.hpp -- what the two translation units for 16-bit keys share (keys16.hip: the sort; topk16.hip: the select): the map
// from the caller's key type and order to the sortable 16-bit value, and the split of an array of 2-byte keys into the keys in
// front of its first 16-byte line, whole groups of eight from there on, and the keys behind the last whole group.  And the value
// side of a float16 / bfloat16 key: its float32 and its softmax mass, one definition for topp16.hip's filter and sample16.hip's draw.
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
__device__ __forceinline__ bool is_number(uint32_t s, const Values16& v) { return s - v.nan_lo <= 0xFFFFu - 2u * v.nan_lo; }   // kNoKey: never
__device__ __forceinline__ float value_of(uint32_t s, const Key16Map& m, const Values16& v)
{
    const uint32_t bits = from_sortable16(s, m) & 0xFFFFu;
    return v.bf16 ? __uint_as_float(bits << 16) : (float)__builtin_bit_cast(_Float16, (uint16_t)bits);
}
// q of a key that is a number; `best`: value_of(m).  The == also defines rows whose best number is an infinity (inf - inf).
__device__ __forceinline__ uint64_t mass_of(float x, float best)
{
    if (x == best) return 1ull << kMassShift;
    const float w = __builtin_amdgcn_exp2f((x - best) * 1.44269504088896341f);   // x < best: w <= 1
    return w >= 1.0f ? 1ull << kMassShift : (uint64_t)(uint32_t)(w * 4294967296.0f);
}
__device__ __forceinline__ uint64_t mass_of_key(uint32_t s, float best, const Key16Map& m, const Values16& v)
{
    return is_number(s, v) ? mass_of(value_of(s, m, v), best) : 0ull;
}

}  // namespace
