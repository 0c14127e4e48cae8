// kth_slots.hpp -- the slots of the two multi-rank k-th value units, once: what kth_multi.hip and kth16_multi.hip do with the
// SEVERAL (prefix, shift, need) states of one row (DESIGN.md sections 6.10, 6.11 and 6.14).  Slot j of a row is the select for
// ranks[j]; the state of (row, slot) lies at state[row * slots + slot].  Internal linkage, as radix_select.hpp: every unit's kernels
// keep their own symbols, a unit calls these helpers DIRECTLY from its kernels, and none of them reads blockDim or gridDim.
// The kernels that test every key against the slots stay in the units: the count kernels differ in how a missing key is told
// (a validity mask, kNoKey), the level kernels in their structure (11 + 11 + 10 bits against 11 + 5).  So do the few lines with
// which they turn the leaders into what a key is compared with (test / owner, lo / span): as a function of this header those lines
// compile to other registers in all nine kernels that use them.
#pragma once

#include <stddef.h>

#include "lsd_device.hpp"
#include "lsd_host.hpp"
#include "radix_select.hpp"

namespace lsd {
namespace {

constexpr int kMaxSlots = LSDSORT_KTH_MAX_RANKS;

// need[j] = ranks[j] + 1: which key of the row slot j wants, 1-based.  A kernel argument; need_of() reads it by a chain of selects, so
// that no kernel indexes its arguments by a run-time value.
struct Needs {
    uint32_t v[kMaxSlots];
};
__device__ __forceinline__ uint32_t need_of(const Needs& n, uint32_t j)
{
    uint32_t v = n.v[0];
#pragma unroll
    for (int i = 1; i < kMaxSlots; i++) v = j == (uint32_t)i ? n.v[i] : v;
    return v;
}

template <class Key>
struct Outputs {
    Key* keys;            // [rows][slots], the caller's keys
    uint32_t* idx;        // [rows][slots] positions, may be null
    uint32_t rows, slots;
    uint32_t* fault;
    __device__ __forceinline__ size_t at(uint32_t row, uint32_t slot) const { return (size_t)row * slots + slot; }   // locate_tile's store
};

// ---- leaders ----------------------------------------------------------------------------------------------------------------------
// Slots that share a (prefix, shift) are counted once, in the counters of their LEADER: the lowest slot of the row that takes part
// and has the pair -- a pure function of the row's states on entry to a kernel, evaluated identically by the kernels that count
// (leaders()) and by the scans that walk the counts (leader_of()).

// The states of a row's slots, for the kernels that test every key against all of them: SLOTS registers each, uniform over the
// workgroup.  Slots from `slots` on are done and match nothing.  LP: the unit's LongParams (state, out.slots).
template <int SLOTS>
struct SlotStates {
    uint32_t prefix[SLOTS], shift[SLOTS];
    bool live[SLOTS];   // the select goes on (w == 0)
};
template <int SLOTS, class LP>
__device__ __forceinline__ SlotStates<SLOTS> slot_states(const LP& p, uint32_t row)
{
    SlotStates<SLOTS> s;
#pragma unroll
    for (int l = 0; l < SLOTS; l++) {
        uint4 st = make_uint4(0u, 0u, 0u, 1u);
        if ((uint32_t)l < p.out.slots) st = p.state[(size_t)row * p.out.slots + l];   // uniform
        s.prefix[l] = st.x;
        s.shift[l] = st.y;
        s.live[l] = st.w == 0u;
    }
    return s;
}
// Bit l: slot l is a leader -- it takes part (`in[l]`) and no lower slot that takes part has the same (prefix, shift).
template <int SLOTS>
__device__ __forceinline__ uint32_t leaders(const SlotStates<SLOTS>& s, const bool (&in)[SLOTS])
{
    uint32_t lead = 0u;
#pragma unroll
    for (int l = 0; l < SLOTS; l++) {
        bool first = in[l];
#pragma unroll
        for (int i = 0; i < l; i++) first = first && !(in[i] && s.prefix[i] == s.prefix[l] && s.shift[i] == s.shift[l]);
        lead |= first ? 1u << l : 0u;
    }
    return lead;
}
// the lowest live slot of the row with slot j's (prefix, shift): j itself, or the slot whose counters j's keys were counted into
// (the histogram kernel's leaders() on the same states: there a live slot also has to carry the previous level's shift, which every
// live slot does -- one that did not would find its counters empty in the scan and raise the count fault)
__device__ __forceinline__ uint32_t leader_of(const uint4* st, uint32_t j)
{
    for (uint32_t i = 0; i < j; i++)
        if (st[i].w == 0u && st[i].x == st[j].x && st[i].y == st[j].y) return i;
    return j;
}


// ---- the pick ---------------------------------------------------------------------------------------------------------------------
// One workgroup per (row, slot): the chunk that holds the `need`-th key under the slot's prefix, and which of that chunk's such
// keys it is.  The chunk counts are those of the lowest slot of the row with the same (prefix, shift).  The workgroups of a row read
// one another's (prefix, shift) while they run, so a pick stores z and w ALONE: no word is read by one workgroup and written by
// another.  A kernel template as radix_select.hpp's pick_rows_kernel: U is the unit's own struct (U::Levels, U::Params).
template <class U>
__global__ void __launch_bounds__(256) pick_slots_kernel(const typename U::Params p)
{
    __shared__ uint32_t s_part[4];
    __shared__ uint32_t s_found[2];
    const uint32_t slots = p.out.slots, row = blockIdx.x / slots, slot = blockIdx.x % slots;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (row >= p.out.rows) return;
    uint4* const state = p.state + (size_t)row * slots;
    const uint2 xy = *reinterpret_cast<const uint2*>(&state[slot].x);
    uint32_t lead = slot;
    for (uint32_t i = slot; i-- > 0u;) {   // uniform
        const uint2 o = *reinterpret_cast<const uint2*>(&state[i].x);
        if (o.x == xy.x && o.y == xy.y) lead = i;
    }
    const uint32_t* const counts = p.counts + ((size_t)row * slots + lead) * p.chunk_cap;
    constexpr uint32_t E = kMaxChunks / 256u;
    uint32_t c[E], sum = 0u;
    const uint32_t need = xy.y < U::Levels::kNoLevel ? state[slot].z : 0u;
#pragma unroll
    for (uint32_t e = 0; e < E; e++) {
        c[e] = (need != 0u && tid * E + e < p.chunks) ? counts[tid * E + e] : 0u;
        sum += c[e];
    }
    if (tid == 0u) s_found[0] = kNoChunk;
    uint32_t run = group_exclusive_scan<4>(sum, lane, wave, s_part);
#pragma unroll
    for (uint32_t e = 0; e < E; e++) {
        if (run < need && need - run <= c[e]) {   // at most one chunk of the row
            s_found[0] = tid * E + e;
            s_found[1] = need - run;
        }
        run += c[e];
    }
    __syncthreads();
    if (tid != 0u) return;
    const uint32_t chunk = s_found[0];
    uint2* const zw = reinterpret_cast<uint2*>(&state[slot].z);
    if (chunk == kNoChunk) {   // the keys under the prefix are fewer than `need`: nothing is located
        atomicOr(p.out.fault, kKthFaultLocate);
        *zw = make_uint2(0u, kNoChunk);
        return;
    }
    *zw = make_uint2(s_found[1], chunk);
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
// no more than LSDSORT_MAX_KEYS rows, keys in all and (row, slot) pairs in all (no product that can overflow)
bool multi_too_large(size_t rows, size_t cols, size_t slots)
{
    if (rows > LSDSORT_MAX_KEYS) return true;
    return rows != 0 && (cols > LSDSORT_MAX_KEYS / rows || slots > LSDSORT_MAX_KEYS / rows);
}

// the host array of ranks (num_ranks of them, not more than kMaxSlots: the entry has checked that) as the launches' argument
int needs_from_ranks(const size_t* ranks, size_t num_ranks, size_t cols, Needs* need)
{
    if (!ranks) return LSDSORT_ERR_INVALID_ARG;
    *need = Needs{};
    for (size_t j = 0; j < num_ranks; j++) {
        if (ranks[j] >= cols) return LSDSORT_ERR_INVALID_ARG;
        need->v[j] = (uint32_t)ranks[j] + 1u;
    }
    return LSDSORT_OK;
}

// The short rows' two launches: the unit's clear kernel on the control block alone, then the short kernel the unit chose for the
// row length, on the grid it sized.
using SlotClearKernel = void (*)(uint32_t*, uint32_t*, uint32_t, uint4*, uint32_t, uint32_t, const Needs);
template <class SP>
int launch_short_slots(SlotClearKernel clear, uint32_t* ctl, void (*kernel)(const SP), dim3 grid, dim3 block, const SP& sp, hipStream_t stream)
{
    hipLaunchKernelGGL(clear, dim3(1), dim3(256), 0, stream, ctl, (uint32_t*)nullptr, 0u, (uint4*)nullptr, 0u, 0u, sp.need);
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, sp);
    LSD_HIP(hipGetLastError());
    return LSDSORT_OK;
}

}  // namespace
}  // namespace lsd
