// kth16_multi.hip -- the 16-bit keys at SEVERAL ranks of every row of a [rows x cols] array, with their positions, in one call
// (lsdsort_kth16_multi_device).  Quartiles, a set of percentiles, the clipping thresholds of float16 /
// bfloat16 rows, and the two adjacent order statistics an interpolating quantile needs -- selected from the 2-byte keys as they lie
// in memory.  The 16-bit sibling of kth_multi.hip and the multi-rank sibling of kth16.hip.
//
// No counterpart in the reference.  Slot j of row r is exactly what lsdsort_kth16_device stores for rank ranks[j] (kth16.hip): item
// ranks[j] of the stable sort of the row in the requested order (the map of keys16_map.hpp, applied where a key is read), and the
// position of that very item.  The ranks are a host array of at most LSDSORT_KTH_MAX_RANKS entries, in any order, repeats allowed;
// they travel in the launches' arguments as `need` = rank + 1.
//
// The select and the locate are kth16.hip's (radix_select.hpp's skeleton with Levels16 -- 11 bits then 5 -- under the stop rule
// StopKth; Row<uint16_t> loads, where a register without a key holds kNoKey and matches no prefix, so no validity mask is needed);
// what this unit adds is that the reads of the row are SHARED by the slots.  Size classes by cols, as in kth16.hip:
//   cols <= kWaveSegCap, <= kLocalSortCap   one wavefront or one workgroup per row: the row is loaded into registers ONCE, then a loop
//                                   over the slots runs the select and the locate of kth16.hip on those registers.  One read of the
//                                   row and one launch after the clear, whatever the number of ranks.
//   longer                          one (prefix, shift, need, done) state per (row, slot).
//     level 0    ONE 2048-bin histogram of every key per row; the scan reads it once and finds every slot's bin in it.
//     level 1    5 bits: 32 counters per LEADER, in LDS and in memory.  The leader of slot j is the lowest live slot of the row with
//                the same (prefix, shift) -- a pure function of the row's states on entry to the level, evaluated identically by the
//                histogram kernel (leaders()) and the scan kernel (leader_of()).  One reject branch per register on the OR of the slot
//                tests, then one counter update on the leader's bin; a follower's scan walks its leader's counters with its own need.
//                A row whose slots are all done skips the level.
//     with positions   one count pass (per chunk and per leader of the FINAL pairs, the keys under the prefix), then a pick and a
//                locate per (row, slot): at most three reads of the row plus num_ranks chunks, in eight launches.
//     values only      a 16-bit value is fully known after the two levels: level 0 runs under a never-stop rule, level 1 for every
//                slot, and one small kernel stores from_sortable16(prefix) per (row, slot).  Two reads of the row in six launches,
//                whatever the number of ranks.
// The two histograms of a call are separate arrays, each used by one level and zeroed by the call's clear kernel: no scan writes a
// counter.  Every launch is sized from (rows, cols, num_ranks) and from whether an index buffer was given; phases are ordered by
// kernel boundaries; every store into the outputs is guarded by row < rows; positions come from position-ordered scans.  Counts that
// do not reach a rank, or a locate that finds no key, raise a fault bit instead -- never expected.  Nothing here ranks with the
// returning add: the result does not depend on lsdsort_set_rank_method.
//
// load_tile, load_head and locate_tile are select_tiles16.hpp's, shared with the other 16-bit row selects; Outputs::at gives
// locate_tile the slot's place in the outputs.  The slots themselves -- Needs, Outputs, SlotStates, leaders(), leader_of(), the pick
// kernel, the entry's checks of the ranks and the short rows' launches -- are kth_slots.hpp's, shared with kth_multi.hip.
#define LSDSORT_BUILD 1
#include "../../include/lsdsort.h"

#include "keys16_map.hpp"
#include "kth_slots.hpp"
#include "lsd_device.hpp"
#include "lsd_host.hpp"
#include "radix_select.hpp"
#include "select_tiles16.hpp"

namespace lsd {
namespace {

constexpr uint32_t kBins1 = 1u << Levels16::bits(1);   // level 1: 32 counters per leader

// ---- short rows: one wavefront (WAVES = 1, eight rows per workgroup) or one workgroup (WAVES = 16) per row ----------------------
struct ShortParams {
    const uint16_t* keys;
    uint32_t cols;
    Needs need;
    Key16Map map;
    Outputs<uint16_t> out;
};

// The slot loop keeps the row's registers live across the select AND the locate; as in kth_multi.hip the hint asks for that unit's
// occupancy class -- seven and six waves per SIMD -- which hipcc's resource remarks show is reached without scratch.
template <int WAVES>
__global__ void __launch_bounds__(WAVES == 1 ? 512 : 1024) __attribute__((amdgpu_waves_per_eu(WAVES == 1 ? 7 : 6, 8)))
kth16m_short_kernel(const ShortParams p)
{
    constexpr int kGroups = WAVES == 1 ? 8 : 1;      // rows in flight per workgroup
    constexpr int kSlice = 256 + 8 + WAVES;          // per row: digit counters, the found bin, per-wave counts
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
        // the row stays in its registers: every slot selects and locates on the same sixteen keys per lane
#pragma unroll 1
        for (uint32_t slot = 0; slot < p.out.slots; slot++) {   // uniform
            // An empty statement that names the keys as changed: nothing derived from them (top bytes, digits, the no-key tests) is
            // computed in front of the loop and kept across it.  Left to hoist them the kernel takes 127 VGPRs (four waves per SIMD);
            // held to seven waves with them hoisted it spills 33.  No instruction is emitted.
#pragma unroll
            for (int i = 0; i < kRegs; i++) asm volatile("" : "+v"(t[i]));
            const Selected sel =
                select_short<WAVES, 2, StopKth>(s_cnt, s_found, wave, lane, need_of(p.need, slot), p.out.fault, kKthFaultCount, count);
            uint32_t base = 0u;
            const bool found =
                locate_tile<WAVES>(t, h, q0, r, sel.prefix, sel.shift, sel.need, base, s_wc, wave, lane, row, slot, p.out, p.map);
            if (!found && sel.need != 0u && wave == 0u && lane == 0u) atomicOr(p.out.fault, kKthFaultLocate);
            group_sync<WAVES>();
        }
    }
}

// ---- long rows ------------------------------------------------------------------------------------------------------------------
// Slot state in the workspace (uint4), at state[row * slots + slot].  During the select: x prefix, y shift (16: no level has run),
// z need, w done (the select stopped: level 1 passes the slot by).  After the pick: x prefix, y shift, z which of the chunk's keys
// under the prefix is the wanted one (1-based; 0: none), w the chunk that holds it.
struct LongParams {
    const uint16_t* keys;
    uint32_t cols;
    uint32_t chunk, chunks;       // body positions per chunk (a multiple of kLongTile), chunks per row
    uint32_t chunk_cap;           // row stride of `counts`
    uint4* state;                 // [rows][slots]
    uint32_t* hist0;              // [rows][kBins]: the top 11 bits of every key; zero on entry
    uint32_t* hist1;              // [rows][slots][kBins1]: the low 5 bits under a leader's prefix; zero on entry
    uint32_t* counts;             // [rows][slots][chunk_cap]: keys under the prefix, per chunk; only the final leaders' are written
    Key16Map map;
    Outputs<uint16_t> out;
};

// control block, both histograms (one stretch of the workspace) and slot states of a call (a kernel rather than memsets: one kind of
// node in a captured graph)
__global__ void __launch_bounds__(256) kth16m_clear_kernel(uint32_t* ctl, uint32_t* hist, uint32_t hist_words, uint4* state, uint32_t rows,
                                                           uint32_t slots, const Needs need)
{
    const uint32_t at = blockIdx.x * blockDim.x + threadIdx.x, step = gridDim.x * blockDim.x;
    clear_select(at, step, ctl, hist, hist_words, (uint4*)nullptr, 0u, 0u, Levels16::kNoLevel);
    if (state)
        for (uint32_t s = at; s < rows * slots; s += step) state[s] = make_uint4(0u, Levels16::kNoLevel, need_of(need, s % slots), 0u);
}

// Level 0, one chunk of one row per workgroup: the top 11 bits of EVERY key, whatever the ranks -- one histogram per row, counted in
// LDS and flushed into the row's level-0 counters.
__global__ void __launch_bounds__(kLongThreads) kth16m_hist0_kernel(const LongParams p)
{
    __shared__ uint32_t s_hist[kBins];
    const uint32_t row = blockIdx.x / p.chunks, c = blockIdx.x % p.chunks;
    if (row >= p.out.rows) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for (uint32_t b = tid; b < kBins; b += kLongThreads) s_hist[b] = 0u;
    __syncthreads();
    const Row16 r = row_of(p.keys, row, p.cols);
    const ChunkRange g = chunk_of(r, p.chunk, c);
    auto count = [&](uint32_t key) __attribute__((always_inline)) {
        count_digit(s_hist, key != kNoKey, (key >> Levels16::shift(0)) & (kBins - 1u), lane);
    };
    if (c == 0u && wave == 0u) count(load_head(r, lane, p.map));   // uniform
    for (uint32_t tile = g.lo; tile < g.hi; tile += kLongTile) {   // uniform
        uint32_t t[kRegs];
        load_tile(r, tile + wave * kWaveTile, g.hi, lane, p.map, t);
#pragma unroll
        for (int i = 0; i < kRegs; i++) count(t[i]);
    }
    __syncthreads();
    uint32_t* const out = p.hist0 + (size_t)row * kBins;
    for (uint32_t b = tid; b < kBins; b += kLongThreads) {
        const uint32_t v = s_hist[b];
        if (v != 0u) atomicAdd(out + b, v);
    }
}

// Level 0, one workgroup per row: the row's counters are read ONCE and scanned once; every slot then finds, among the bins its
// thread holds, the one with its key.  Stop: StopKth, or StopNever16 for the values-only sequence.
template <class Stop>
__global__ void __launch_bounds__(256) kth16m_scan0_kernel(const LongParams p)
{
    __shared__ uint32_t s_part[4];
    __shared__ uint32_t s_found[kMaxSlots][3];
    __shared__ uint32_t s_need[kMaxSlots];
    const uint32_t row = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (row >= p.out.rows) return;
    const uint32_t slots = p.out.slots;
    uint4* const state = p.state + (size_t)row * slots;
    if (tid < slots) {
        s_need[tid] = state[tid].z;
        s_found[tid][0] = 0xFFFFFFFFu;
    }
    const uint32_t* const h = p.hist0 + (size_t)row * kBins;
    constexpr uint32_t E = kBins / 256u;
    uint32_t c[E], sum = 0u;
#pragma unroll
    for (uint32_t e = 0; e < E; e++) {
        c[e] = h[tid * E + e];
        sum += c[e];
    }
    const uint32_t first = group_exclusive_scan<4>(sum, lane, wave, s_part);   // its barrier: s_need and s_found are set
#pragma unroll 1
    for (uint32_t j = 0; j < slots; j++) {   // uniform
        const uint32_t need = s_need[j];
        uint32_t run = first;
#pragma unroll
        for (uint32_t e = 0; e < E; e++) {
            if (run < need && need - run <= c[e]) {   // at most one bin of the walk
                s_found[j][0] = tid * E + e;
                s_found[j][1] = run;
                s_found[j][2] = c[e];
            }
            run += c[e];
        }
    }
    __syncthreads();
    if (tid >= slots) return;
    const uint32_t bin = s_found[tid][0], before = s_found[tid][1], count = s_found[tid][2];
    if (bin >= kBins) {   // no bin of the walk: nothing is selected
        atomicOr(p.out.fault, kKthFaultCount);
        state[tid] = make_uint4(0u, 0u, 0u, 1u);
        return;
    }
    const uint32_t left = s_need[tid] - before;
    state[tid] = make_uint4(bin, Levels16::shift(0), left, Stop::stops(count, left) ? 1u : 0u);
}

// Level 1, one chunk of one row per workgroup: the low 5 bits of every key under the prefix of a live slot, counted in the 32 LDS
// counters of that prefix's leader.  Nearly every key is under NO slot's prefix, so the test that sends a key away is what the pass
// costs: one shift, one compare per slot into a wave mask, and ONE branch per register on the OR of the masks.  A register without a
// key holds kNoKey, whose top bits are no prefix.  A slot that is no leader repeats a leader's prefix in that test.
__global__ void __launch_bounds__(kLongThreads) kth16m_hist1_kernel(const LongParams p)
{
    constexpr uint32_t kUp = Levels16::shift(0);   // the shift of every slot that is live on entry to this level
    static_assert(kMaxSlots * kBins1 == kLongThreads, "the flush takes one counter per thread");
    __shared__ uint32_t s_hist[kMaxSlots * kBins1];
    const uint32_t row = blockIdx.x / p.chunks, c = blockIdx.x % p.chunks;
    if (row >= p.out.rows) return;
    const SlotStates<kMaxSlots> s = slot_states<kMaxSlots>(p, row);
    bool in[kMaxSlots];
#pragma unroll
    for (int l = 0; l < kMaxSlots; l++) in[l] = s.live[l] && s.shift[l] == kUp;
    const uint32_t lead = leaders(s, in);
    if (lead == 0u) return;   // (uniform) every slot of the row is done
    constexpr uint32_t kNoSlot = 0xFFFFu;
    uint32_t first = 0u, some = 0u, test[kMaxSlots], owner[kMaxSlots];   // what a key is compared with, and whose counters it goes to
#pragma unroll
    for (int l = kMaxSlots - 1; l >= 0; l--) {
        first = ((lead >> l) & 1u) != 0u ? (uint32_t)l : first;
        some = ((lead >> l) & 1u) != 0u ? s.prefix[l] : some;
    }
#pragma unroll
    for (int l = 0; l < kMaxSlots; l++) {
        test[l] = ((lead >> l) & 1u) != 0u ? s.prefix[l] : some;
        owner[l] = ((lead >> l) & 1u) != 0u ? (uint32_t)l : first;
    }
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    s_hist[tid] = 0u;
    __syncthreads();
    const Row16 r = row_of(p.keys, row, p.cols);
    const ChunkRange g = chunk_of(r, p.chunk, c);
    auto count = [&](uint32_t key) __attribute__((always_inline)) {
        const uint32_t up = key >> kUp;
        uint64_t any = 0ull;
#pragma unroll
        for (int l = 0; l < kMaxSlots; l++) any |= __ballot(up == test[l]);
        if (any == 0ull) return;   // (uniform) no lane's key is under a live prefix
        // the leaders' prefixes differ: a key is under one of them at the most, so ONE counter takes it
        uint32_t mine = kNoSlot;
#pragma unroll
        for (int l = 0; l < kMaxSlots; l++) mine = up == test[l] ? owner[l] : mine;
        count_digit(s_hist, mine != kNoSlot, (mine & (uint32_t)(kMaxSlots - 1)) * kBins1 + (key & (kBins1 - 1u)), lane);
    };
    if (c == 0u && wave == 0u) count(load_head(r, lane, p.map));   // uniform
    for (uint32_t tile = g.lo; tile < g.hi; tile += kLongTile) {   // uniform
        uint32_t t[kRegs];
        load_tile(r, tile + wave * kWaveTile, g.hi, lane, p.map, t);
#pragma unroll
        for (int i = 0; i < kRegs; i++) count(t[i]);
    }
    __syncthreads();
    const uint32_t l = tid / kBins1, v = s_hist[tid];   // counters of a slot that is no leader, or beyond `slots`, stay zero
    if (v != 0u && l < p.out.slots) atomicAdd(p.hist1 + ((size_t)row * p.out.slots + l) * kBins1 + (tid % kBins1), v);
}

// Level 1, one wavefront per row: for every live slot, lane b holds bin b of its leader's 32 counters; the lane whose bin holds the
// slot's key stores the state.  All states of the row are read before any is written.  The last level ends the select.
__global__ void __launch_bounds__(64) kth16m_scan1_kernel(const LongParams p)
{
    __shared__ uint4 s_st[kMaxSlots];
    const uint32_t row = blockIdx.x, lane = threadIdx.x;
    if (row >= p.out.rows) return;
    const uint32_t slots = p.out.slots;
    uint4* const state = p.state + (size_t)row * slots;
    if (lane < slots) s_st[lane] = state[lane];
    __syncthreads();
#pragma unroll 1
    for (uint32_t j = 0; j < slots; j++) {   // uniform
        const uint4 st = s_st[j];
        if (st.w != 0u) continue;   // uniform
        const uint32_t lead = leader_of(s_st, j);
        const uint32_t c = lane < kBins1 ? p.hist1[((size_t)row * slots + lead) * kBins1 + lane] : 0u;
        const uint32_t run = wave_inclusive_scan(c) - c, need = st.z;
        const bool hit = lane < kBins1 && run < need && need - run <= c;   // at most one bin of the walk
        if (hit) state[j] = make_uint4((st.x << Levels16::bits(1)) | lane, Levels16::shift(1), need - run, 1u);
        if (__ballot(hit) == 0ull && lane == 0u) {   // no bin of the walk: nothing is selected
            atomicOr(p.out.fault, kKthFaultCount);
            state[j] = make_uint4(0u, 0u, 0u, 1u);
        }
    }
}

// One chunk of one row per workgroup, one pass: the keys under each FINAL (prefix, shift) of the row, counted once per distinct
// pair -- into the chunk counts of the lowest slot that has it.
__global__ void __launch_bounds__(kLongThreads) kth16m_count_kernel(const LongParams p)
{
    __shared__ uint32_t s_part[kMaxSlots * kLongWaves];
    const uint32_t row = blockIdx.x / p.chunks, c = blockIdx.x % p.chunks;
    if (row >= p.out.rows) return;
    const SlotStates<kMaxSlots> s = slot_states<kMaxSlots>(p, row);
    bool in[kMaxSlots];   // a slot no scan has visited (never) is not counted: its shift is no shift
#pragma unroll
    for (int l = 0; l < kMaxSlots; l++) in[l] = (uint32_t)l < p.out.slots && s.shift[l] < Levels16::kNoLevel;
    const uint32_t lead = leaders(s, in);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const Row16 r = row_of(p.keys, row, p.cols);
    const ChunkRange g = chunk_of(r, p.chunk, c);
    // (key ^ lo) <= span: the key is under the prefix -- lo is the prefix in place, span the bits below it (kNoKey never is: lo is
    // below 65536).  As in the level-1 histogram the pass costs what sends a key away: two operations per slot into a wave mask and
    // ONE branch per register; a slot that is no leader repeats a leader's pair.
    uint32_t lo[kMaxSlots], span[kMaxSlots], some_lo = 0u, some_span = 0u;
#pragma unroll
    for (int l = kMaxSlots - 1; l >= 0; l--) {
        const bool mine = ((lead >> l) & 1u) != 0u;
        lo[l] = mine ? s.prefix[l] << s.shift[l] : 0u;
        span[l] = mine ? (1u << s.shift[l]) - 1u : 0u;
        some_lo = mine ? lo[l] : some_lo;
        some_span = mine ? span[l] : some_span;
    }
#pragma unroll
    for (int l = 0; l < kMaxSlots; l++) {
        if (((lead >> l) & 1u) == 0u) {
            lo[l] = some_lo;
            span[l] = some_span;
        }
    }
    uint32_t ne[kMaxSlots];
#pragma unroll
    for (int l = 0; l < kMaxSlots; l++) ne[l] = 0u;
    auto count = [&](uint32_t key) __attribute__((always_inline)) {
        uint64_t any = 0ull;
#pragma unroll
        for (int l = 0; l < kMaxSlots; l++) any |= __ballot((key ^ lo[l]) <= span[l]);
        if (any == 0ull) return;   // (uniform) no lane's key is under a final prefix
#pragma unroll
        for (int l = 0; l < kMaxSlots; l++) {
            if (((lead >> l) & 1u) != 0u)   // uniform
                ne[l] += (key ^ lo[l]) <= span[l] ? 1u : 0u;
        }
    };
    if (lead != 0u) {   // (uniform) else: a row no scan has visited -- never
        if (c == 0u && wave == 0u) count(load_head(r, lane, p.map));   // uniform
        for (uint32_t tile = g.lo; tile < g.hi; tile += kLongTile) {   // uniform
            uint32_t t[kRegs];
            load_tile(r, tile + wave * kWaveTile, g.hi, lane, p.map, t);
#pragma unroll
            for (int i = 0; i < kRegs; i++) count(t[i]);
        }
    }
#pragma unroll
    for (int l = 0; l < kMaxSlots; l++) {
        const uint32_t v = wave_sum(ne[l]);
        if (lane == 0u) s_part[l * kLongWaves + wave] = v;
    }
    __syncthreads();
    if (tid < (uint32_t)kMaxSlots && ((lead >> tid) & 1u) != 0u) {
        uint32_t e = 0u;
        for (uint32_t w = 0; w < kLongWaves; w++) e += s_part[tid * kLongWaves + w];
        p.counts[((size_t)row * p.out.slots + tid) * p.chunk_cap + c] = e;
    }
}

// One workgroup per (row, slot): the chunk that holds the slot's key -- kth_slots.hpp's kernel template, under this unit's name.
struct Kth16Multi {
    using Levels = Levels16;
    using Params = LongParams;
};
constexpr auto kth16m_pick_kernel = pick_slots_kernel<Kth16Multi>;

// One workgroup per (row, slot) reads the picked chunk, and only up to the tile that holds the key.
__global__ void __launch_bounds__(kLongThreads) kth16m_locate_kernel(const LongParams p)
{
    __shared__ uint32_t s_wc_raw[kLongWaves];
    const uint32_t slots = p.out.slots, row = blockIdx.x / slots, slot = blockIdx.x % slots;
    if (row >= p.out.rows) return;
    const uint4 st = p.state[(size_t)row * slots + slot];
    if (st.z == 0u || st.w >= p.chunks) return;   // (uniform) nothing was picked: the fault bit is already set
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
        found = locate_tile<(int)kLongWaves>(t, h, q0, r, st.x, st.y, st.z, base, s_wc, wave, lane, row, slot, p.out, p.map);
    }
    if (!found && tid == 0u) atomicOr(p.out.fault, kKthFaultLocate);
}

// Values only: after both levels the prefix is the slot's whole sortable value (shift 0, need not 0).  Anything else is a slot whose
// counts fell short (its fault bit is set) or one no scan has visited -- never: nothing is stored for it.
__global__ void __launch_bounds__(256) kth16m_value_kernel(const LongParams p)
{
    const uint32_t n = p.out.rows * p.out.slots;   // s / slots < rows: the store stays inside the rows
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < n; s += gridDim.x * blockDim.x) {
        const uint4 st = p.state[s];
        if (st.y == 0u && st.z != 0u) p.out.keys[s] = (uint16_t)from_sortable16(st.x & 0xFFFFu, p.map);
        else atomicOr(p.out.fault, kKthFaultLocate);
    }
}

// Workspace: control | slot states (16 B per row and slot) | level-0 counters [rows][2048] | level-1 counters [rows][slots][32] |
// chunk counts (4 B per chunk and slot) -- the last three for rows above kLocalSortCap keys only.  At most
// 256 + rows (8192 + slots (16 + 128 + 4 ceil(cols / 16384))) + 4 * 255 bytes; never O(rows * cols).
struct Kth16mLayout {
    size_t state, hist0, hist1, counts, end;
};
Kth16mLayout kth16m_layout(size_t rows, size_t cols, size_t slots)
{
    Kth16mLayout L{};
    const bool is_long = cols > (size_t)kLocalSortCap;
    size_t off = kCtlBytes;
    L.state = off;   off = align_up(off + rows * slots * 16);
    L.hist0 = off;   off = align_up(off + (is_long ? rows * kBins * 4 : 0));
    L.hist1 = off;   off = align_up(off + (is_long ? rows * slots * kBins1 * 4 : 0));
    L.counts = off;  off = align_up(off + (is_long ? rows * slots * chunk_cap_for(cols) * 4 : 0));
    L.end = off;
    return L;
}

int run_kth16_multi(const uint16_t* keys, size_t rows, size_t cols, const Needs& need, size_t slots, const Key16Map& map,
                    uint16_t* out_keys, uint32_t* out_idx, char* ws, const Kth16mLayout& L, hipStream_t stream)
{
    uint32_t* const ctl = reinterpret_cast<uint32_t*>(ws);
    const Outputs<uint16_t> out{out_keys, out_idx, (uint32_t)rows, (uint32_t)slots, ctl};
    if (cols <= (size_t)kLocalSortCap) {
        const ShortParams sp{keys, (uint32_t)cols, need, map, out};
        if (cols <= (size_t)kWaveSegCap)
            return launch_short_slots(kth16m_clear_kernel, ctl, kth16m_short_kernel<1>, dim3(grid_for(rows, 8, 16384)), dim3(512), sp, stream);
        return launch_short_slots(kth16m_clear_kernel, ctl, kth16m_short_kernel<16>, dim3(grid_for(rows, 1, 4096)), dim3(1024), sp, stream);
    }
    const Chunks ch = chunks_for(rows, cols);
    LongParams lp{};
    lp.keys = keys;
    lp.cols = (uint32_t)cols;
    lp.chunk = ch.chunk;
    lp.chunks = ch.per_row;
    lp.chunk_cap = (uint32_t)chunk_cap_for(cols);
    lp.state = reinterpret_cast<uint4*>(ws + L.state);
    lp.hist0 = reinterpret_cast<uint32_t*>(ws + L.hist0);
    lp.hist1 = reinterpret_cast<uint32_t*>(ws + L.hist1);
    lp.counts = reinterpret_cast<uint32_t*>(ws + L.counts);
    lp.map = map;
    lp.out = out;
    if (lp.chunks > lp.chunk_cap) return LSDSORT_ERR_INVALID_ARG;   // never: chunks are at least kMinChunk keys
    const size_t hist_words = (L.counts - L.hist0) / 4;   // both histograms and the padding between them
    const uint32_t grid = (uint32_t)(rows * lp.chunks), row_grid = (uint32_t)rows, slot_grid = (uint32_t)(rows * slots);
    hipLaunchKernelGGL(kth16m_clear_kernel, dim3(grid_for(hist_words, 1024, 4096)), dim3(256), 0, stream, ctl, lp.hist0,
                       (uint32_t)hist_words, lp.state, (uint32_t)rows, (uint32_t)slots, need);
    hipLaunchKernelGGL(kth16m_hist0_kernel, dim3(grid), dim3(kLongThreads), 0, stream, lp);
    if (!out_idx) {   // values only: both levels for every slot, then the prefix is the value
        hipLaunchKernelGGL(kth16m_scan0_kernel<StopNever16>, dim3(row_grid), dim3(256), 0, stream, lp);
        hipLaunchKernelGGL(kth16m_hist1_kernel, dim3(grid), dim3(kLongThreads), 0, stream, lp);
        hipLaunchKernelGGL(kth16m_scan1_kernel, dim3(row_grid), dim3(64), 0, stream, lp);
        // 2048 workgroups hold every (row, slot) a call can have -- fewer than 65536 long rows, eight slots -- so the loop is one round
        hipLaunchKernelGGL(kth16m_value_kernel, dim3(grid_for(rows * slots, 256, 2048)), dim3(256), 0, stream, lp);
        LSD_HIP(hipGetLastError());
        return LSDSORT_OK;
    }
    hipLaunchKernelGGL(kth16m_scan0_kernel<StopKth>, dim3(row_grid), dim3(256), 0, stream, lp);
    hipLaunchKernelGGL(kth16m_hist1_kernel, dim3(grid), dim3(kLongThreads), 0, stream, lp);
    hipLaunchKernelGGL(kth16m_scan1_kernel, dim3(row_grid), dim3(64), 0, stream, lp);
    hipLaunchKernelGGL(kth16m_count_kernel, dim3(grid), dim3(kLongThreads), 0, stream, lp);
    hipLaunchKernelGGL(kth16m_pick_kernel, dim3(slot_grid), dim3(256), 0, stream, lp);
    hipLaunchKernelGGL(kth16m_locate_kernel, dim3(slot_grid), dim3(kLongThreads), 0, stream, lp);
    LSD_HIP(hipGetLastError());
    return LSDSORT_OK;
}

}  // namespace
}  // namespace lsd

extern "C" {

size_t lsdsort_kth16_multi_workspace_bytes(size_t rows, size_t cols, size_t num_ranks)
{
    if (num_ranks > LSDSORT_KTH_MAX_RANKS || cols > LSDSORT_MAX_KEYS || lsd::multi_too_large(rows, cols, num_ranks)) return 0;
    return lsd::kth16m_layout(rows, cols, num_ranks).end;
}

int lsdsort_kth16_multi_device(const void* d_keys, size_t rows, size_t cols, const size_t* ranks, size_t num_ranks, int key_type,
                               int largest, void* d_out_keys, uint32_t* d_out_idx, void* d_workspace, size_t workspace_bytes,
                               void* hip_stream)
{
    Key16Map map;
    LSD_TRY(key16_map(key_type, largest, &map));
    if (num_ranks > LSDSORT_KTH_MAX_RANKS) return LSDSORT_ERR_INVALID_ARG;
    if (lsd::multi_too_large(rows, cols, num_ranks)) return LSDSORT_ERR_TOO_LARGE;
    if (rows == 0 || cols == 0 || num_ranks == 0) return LSDSORT_OK;   // before the ranks: an empty row has no valid rank
    lsd::Needs need;
    LSD_TRY(lsd::needs_from_ranks(ranks, num_ranks, cols, &need));
    if (!d_keys || !d_out_keys || (((uintptr_t)d_keys | (uintptr_t)d_out_keys) & 1)) return LSDSORT_ERR_INVALID_ARG;
    const lsd::Kth16mLayout L = lsd::kth16m_layout(rows, cols, num_ranks);
    if (!lsd::workspace_ok(d_workspace, workspace_bytes, L.end)) return LSDSORT_ERR_WORKSPACE;
    int rank_method = 0;   // asked for the device set-up alone: nothing here ranks with the returning add
    LSD_TRY(lsd::device_rank_method(8, &rank_method));
    return lsd::run_kth16_multi(static_cast<const uint16_t*>(d_keys), rows, cols, need, num_ranks, map, static_cast<uint16_t*>(d_out_keys),
                                d_out_idx, static_cast<char*>(d_workspace), L, static_cast<hipStream_t>(hip_stream));
}

}  // extern "C"
