// kth_multi.hip -- the keys at SEVERAL ranks of every row of a [rows x cols] array, with their positions, in one call
// (lsdsort_kth_multi_device).  Quartiles, a set of percentiles, the two clipping thresholds of a row, and the
// two adjacent order statistics an interpolating quantile needs.
//
// No counterpart in the reference.  Slot j of row r is exactly what lsdsort_kth_device stores for rank ranks[j] (kth.hip): item
// ranks[j] of the stable sort of the row in the requested order, and the position of that very item.  The ranks are a host array of
// at most LSDSORT_KTH_MAX_RANKS entries, in any order, repeats allowed; they travel in the launches' arguments as `need` = rank + 1.
//
// The select and the locate are kth.hip's (radix_select.hpp's skeleton with the stop rule StopKth; Row<uint32_t> loads with a
// validity mask, because every 32-bit pattern is a real key); what this unit adds is that the reads of the row are SHARED by the
// slots.  Size classes by cols, as in kth.hip:
//   cols <= kWaveSegCap, <= kLocalSortCap   one wavefront or one workgroup per row: the row is loaded into registers ONCE, then a loop
//                                   over the slots runs the select and the locate of kth.hip on those registers.  One read of the
//                                   row and one launch, whatever the number of ranks.
//   longer                          one (prefix, shift, need, done) state, kBins counters and one chunk-count row per (row, slot).
//     level 0    ONE histogram of every key per row, in slot 0's counters; the scan walks it once per slot.
//     level 1, 2 every key is tested against the prefixes of the row's live slots.  Slots that share a prefix are counted once: the
//                LEADER of slot j is the lowest live slot of the row with the same (prefix, shift) -- a pure function of the row's
//                states on entry to the level, evaluated identically by the histogram kernel (leaders()) and the scan kernel
//                (leader_of()).  Only leaders have counters, in LDS and in memory; a follower's scan walks its leader's counters with
//                its own need.  The scan reads all states of the row before it writes any and zeroes the counters after the last slot
//                has read them.  A row whose slots are all done leaves the later levels at once.
//     count      one pass over the row: per chunk and per leader of the FINAL (prefix, shift) pairs, the keys under the prefix.
//     pick, locate   one workgroup per (row, slot): the chunk that holds the slot's key, then that ONE chunk up to the tile with it.
//                At most four reads of the row plus one chunk per slot, in the ten launches of the single-rank call.
// Every launch is sized from (rows, cols, num_ranks); phases are ordered by kernel boundaries; every store into the outputs is guarded
// by row < rows; positions come from position-ordered scans.  Counts that do not reach a rank, or a locate that finds no key, raise
// a fault bit instead -- never expected.  Nothing here needs the returning-add rank form.
//
// load_tile, load_head and locate_tile are select_tiles32.hpp's, shared with kth.hip; Outputs::at gives locate_tile the slot's place
// in the outputs.  The slots themselves -- Needs, Outputs, SlotStates, leaders(), leader_of(), the pick kernel, the entry's checks of
// the ranks and the short rows' launches -- are kth_slots.hpp's, shared with kth16_multi.hip.
#define LSDSORT_BUILD 1
#include "../../include/lsdsort.h"

#include "kth_slots.hpp"
#include "lsd_device.hpp"
#include "lsd_host.hpp"
#include "radix_select.hpp"
#include "select_tiles32.hpp"

namespace lsd {
namespace {

// ---- short rows: one wavefront (WAVES = 1, eight rows per workgroup) or one workgroup (WAVES = 16) per row ----------------------
struct ShortParams {
    const uint32_t* keys;
    uint32_t cols;
    Needs need;
    KeyTransform xf;
    Outputs<uint32_t> out;
};

// The slot loop keeps the row's registers live across the select AND the locate, and left to itself the register allocator takes what
// the launch bounds allow (105 and 118 VGPRs: four waves per SIMD).  The hint asks for the single-rank kernels' occupancy class or
// better -- seven and six waves per SIMD -- which hipcc's resource remarks show it reaches without scratch.
template <int WAVES>
__global__ void __launch_bounds__(WAVES == 1 ? 512 : 1024) __attribute__((amdgpu_waves_per_eu(WAVES == 1 ? 7 : 6, 8)))
kthm_short_kernel(const ShortParams p)
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
        const Row32 r = row_of(p.keys, row, p.cols);
        const uint32_t q0 = wave * kWaveTile;
        uint32_t t[kRegs], h = 0u;
        uint32_t vm = load_tile(r, q0, r.body, lane, p.xf, t);
        if (wave == 0u) vm |= load_head(r, lane, p.xf, h);
        // round 0: every key there is; later: those whose bits above the digit are the prefix.  Always under the validity bit.
        auto count = [&](int round, uint32_t shift, uint32_t prefix, auto add) __attribute__((always_inline)) {
            auto one = [&](uint32_t key, bool valid) __attribute__((always_inline)) {
                const bool match = round == 0 || ((key >> shift) >> 8) == prefix;
                if (valid && match) add(key);
            };
#pragma unroll
            for (int i = 0; i < kRegs; i++) one(t[i], ((vm >> i) & 1u) != 0u);
            one(h, (vm & kHeadBit) != 0u);
        };
        // the row stays in its registers: every slot selects and locates on the same sixteen keys per lane
#pragma unroll 1
        for (uint32_t slot = 0; slot < p.out.slots; slot++) {   // uniform
            const Selected sel =
                select_short<WAVES, 4, StopKth>(s_cnt, s_found, wave, lane, need_of(p.need, slot), p.out.fault, kKthFaultCount, count);
            uint32_t base = 0u;
            const bool found =
                locate_tile<WAVES>(t, h, vm, q0, r, sel.prefix, sel.shift, sel.need, base, s_wc, wave, lane, row, slot, p.out, p.xf);
            if (!found && sel.need != 0u && wave == 0u && lane == 0u) atomicOr(p.out.fault, kKthFaultLocate);
            group_sync<WAVES>();
        }
    }
}

// ---- long rows ------------------------------------------------------------------------------------------------------------------
// Slot state in the workspace (uint4), at state[row * slots + slot].  During the select: x prefix, y shift (32: no level has run),
// z need, w done (the select stopped: later levels pass the slot by).  After the pick: x prefix, y shift, z which of the chunk's keys
// under the prefix is the wanted one (1-based; 0: none), w the chunk that holds it.
struct LongParams {
    const uint32_t* keys;
    uint32_t cols;
    uint32_t chunk, chunks;       // body positions per chunk (a multiple of kLongTile), chunks per row
    uint32_t chunk_cap;           // row stride of `counts`
    uint4* state;                 // [rows][slots]
    uint32_t* hist;               // [rows][slots][kBins], zero on entry to every level; only a level's leaders are counted into
    uint32_t* counts;             // [rows][slots][chunk_cap]: keys under the prefix, per chunk; only the final leaders' are written
    KeyTransform xf;
    Outputs<uint32_t> out;
};

// control block, counters and slot states of a call (a kernel rather than memsets: one kind of node in a captured graph)
__global__ void __launch_bounds__(256) kthm_clear_kernel(uint32_t* ctl, uint32_t* hist, uint32_t hist_words, uint4* state, uint32_t rows,
                                                         uint32_t slots, const Needs need)
{
    const uint32_t at = blockIdx.x * blockDim.x + threadIdx.x, step = gridDim.x * blockDim.x;
    clear_select(at, step, ctl, hist, hist_words, (uint4*)nullptr, 0u, 0u, Levels32::kNoLevel);
    if (state)
        for (uint32_t s = at; s < rows * slots; s += step) state[s] = make_uint4(0u, Levels32::kNoLevel, need_of(need, s % slots), 0u);
}

// Level 0, one chunk of one row per workgroup: the top digit of EVERY key, whatever the ranks -- one histogram per row, counted in
// LDS and flushed into slot 0's counters.
__global__ void __launch_bounds__(kLongThreads) kthm_hist0_kernel(const LongParams p)
{
    __shared__ uint32_t s_hist[kBins];
    const uint32_t row = blockIdx.x / p.chunks, c = blockIdx.x % p.chunks;
    if (row >= p.out.rows) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for (uint32_t b = tid; b < kBins; b += kLongThreads) s_hist[b] = 0u;
    __syncthreads();
    const Row32 r = row_of(p.keys, row, p.cols);
    const ChunkRange g = chunk_of(r, p.chunk, c);
    const uint32_t shift = Levels32::shift(0), mask = (1u << Levels32::bits(0)) - 1u;
    if (c == 0u && wave == 0u) {   // uniform
        uint32_t h;
        const uint32_t hv = load_head(r, lane, p.xf, h);
        count_digit(s_hist, hv != 0u, (h >> shift) & mask, lane);
    }
    for (uint32_t tile = g.lo; tile < g.hi; tile += kLongTile) {   // uniform
        uint32_t t[kRegs];
        const uint32_t vm = load_tile(r, tile + wave * kWaveTile, g.hi, lane, p.xf, t);
#pragma unroll
        for (int i = 0; i < kRegs; i++) count_digit(s_hist, ((vm >> i) & 1u) != 0u, (t[i] >> shift) & mask, lane);
    }
    __syncthreads();
    uint32_t* const out = p.hist + (size_t)row * p.out.slots * kBins;
    for (uint32_t b = tid; b < kBins; b += kLongThreads) {
        const uint32_t v = s_hist[b];
        if (v != 0u) atomicAdd(out + b, v);
    }
}

// Levels 1 and 2, one chunk of one row per workgroup: the digit of every key under the prefix of a live slot, counted in the LDS
// counters of that prefix's leader.  SLOTS * kBins counters: the smallest SLOTS that holds the call's ranks is launched.
// Nearly every key is under NO slot's prefix, so the test that sends a key away is what the pass costs: one shift (every live slot
// carries the shift of the level before -- the scan of that level wrote it), one compare per slot into a wave mask, and ONE branch
// per register on the OR of the masks.  Validity is left to the counting path: a register without a key holds zero, which at worst
// sends a wave there for nothing.  A slot that is no leader repeats a leader's prefix in that test.
// Threads per workgroup grow with the counters, so that the waves a CU holds do not shrink with them: 64 KiB of counters at 256
// threads leave two waves per SIMD and the pass does not stream (eight percentiles of [64 x 2^22]: 1.99 ms a call at 256 threads,
// 1.47 at 512, 1.27 at 1024; quartiles with 32 KiB: 1.27 ms at 256, 1.10 at 512 -- DESIGN.md section 6.10).  A workgroup's waves
// share the chunk tile by tile: wave w of W takes tile + w * kWaveTile and the loop steps by W tiles.
template <int SLOTS>
constexpr uint32_t hist_threads() { return SLOTS == 8 ? 1024u : SLOTS == 4 ? 512u : kLongThreads; }
template <int LEVEL, int SLOTS>
__global__ void __launch_bounds__(hist_threads<SLOTS>()) kthm_hist_kernel(const LongParams p)
{
    static_assert(LEVEL >= 1, "level 0 counts every key once: kthm_hist0_kernel");
    constexpr uint32_t kThreads = hist_threads<SLOTS>(), kTile = kThreads * kRegs;
    constexpr uint32_t kUp = Levels32::shift(LEVEL - 1);   // the shift of every slot that is live on entry to this level
    __shared__ uint32_t s_hist[SLOTS * kBins];
    const uint32_t row = blockIdx.x / p.chunks, c = blockIdx.x % p.chunks;
    if (row >= p.out.rows) return;
    const SlotStates<SLOTS> s = slot_states<SLOTS>(p, row);
    bool in[SLOTS];
#pragma unroll
    for (int l = 0; l < SLOTS; l++) in[l] = s.live[l] && s.shift[l] == kUp;
    const uint32_t lead = leaders(s, in);
    if (lead == 0u) return;   // (uniform) every slot of the row is done
    constexpr uint32_t kNoSlot = 0xFFFFu;
    uint32_t first = 0u, some = 0u, test[SLOTS], owner[SLOTS];   // what a key is compared with, and whose counters it then goes to
#pragma unroll
    for (int l = SLOTS - 1; l >= 0; l--) {
        first = ((lead >> l) & 1u) != 0u ? (uint32_t)l : first;
        some = ((lead >> l) & 1u) != 0u ? s.prefix[l] : some;
    }
#pragma unroll
    for (int l = 0; l < SLOTS; l++) {
        test[l] = ((lead >> l) & 1u) != 0u ? s.prefix[l] : some;
        owner[l] = ((lead >> l) & 1u) != 0u ? (uint32_t)l : first;
    }
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
#pragma unroll
    for (int l = 0; l < SLOTS; l++) {
        if (((lead >> l) & 1u) != 0u)   // uniform
            for (uint32_t b = tid; b < kBins; b += kThreads) s_hist[l * kBins + b] = 0u;
    }
    __syncthreads();
    const Row32 r = row_of(p.keys, row, p.cols);
    const ChunkRange g = chunk_of(r, p.chunk, c);
    const uint32_t shift = Levels32::shift(LEVEL), mask = (1u << Levels32::bits(LEVEL)) - 1u;
    auto count = [&](uint32_t key, bool valid) __attribute__((always_inline)) {
        const uint32_t up = key >> kUp;
        uint64_t any = 0ull;
#pragma unroll
        for (int l = 0; l < SLOTS; l++) any |= __ballot(up == test[l]);
        if (any == 0ull) return;   // (uniform) no lane's key is under a live prefix
        // the leaders' prefixes differ and their shift is one: a key is under one of them at the most, so ONE counter takes it
        uint32_t mine = kNoSlot;
#pragma unroll
        for (int l = 0; l < SLOTS; l++) mine = up == test[l] ? owner[l] : mine;
        count_digit(s_hist, valid && mine != kNoSlot, mine * kBins + ((key >> shift) & mask), lane);
    };
    if (c == 0u && wave == 0u) {   // uniform
        uint32_t h;
        const uint32_t hv = load_head(r, lane, p.xf, h);
        count(h, hv != 0u);
    }
    for (uint32_t tile = g.lo; tile < g.hi; tile += kTile) {   // uniform; a wave whose tile starts at or past g.hi loads nothing
        uint32_t t[kRegs];
        const uint32_t vm = load_tile(r, tile + wave * kWaveTile, g.hi, lane, p.xf, t);
#pragma unroll
        for (int i = 0; i < kRegs; i++) count(t[i], ((vm >> i) & 1u) != 0u);
    }
    __syncthreads();
#pragma unroll
    for (int l = 0; l < SLOTS; l++) {
        if (((lead >> l) & 1u) == 0u) continue;   // uniform
        uint32_t* const out = p.hist + ((size_t)row * p.out.slots + l) * kBins;
        for (uint32_t b = tid; b < kBins; b += kThreads) {
            const uint32_t v = s_hist[l * kBins + b];
            if (v != 0u) atomicAdd(out + b, v);
        }
    }
}

// One workgroup per row: for every live slot, walk its leader's bins from the best end to the one that holds the slot's key.  All
// states of the row are read before any is written; the leaders' counters go back to zero after the last slot has read them.
template <int LEVEL>
__global__ void __launch_bounds__(256) kthm_scan_kernel(const LongParams p)
{
    __shared__ uint32_t s_part[4];
    __shared__ uint32_t s_found[3];
    __shared__ uint4 s_st[kMaxSlots];
    const uint32_t row = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (row >= p.out.rows) return;
    const uint32_t slots = p.out.slots;
    uint4* const state = p.state + (size_t)row * slots;
    if (tid < slots) s_st[tid] = state[tid];
    __syncthreads();
    constexpr uint32_t E = kBins / 256u;
    uint32_t zero = 0u;   // the leaders whose counters were walked
#pragma unroll 1
    for (uint32_t j = 0; j < slots; j++) {   // uniform
        const uint4 st = s_st[j];
        if (st.w != 0u) continue;   // uniform
        const uint32_t lead = leader_of(s_st, j);
        zero |= 1u << lead;
        const uint32_t* const h = p.hist + ((size_t)row * slots + lead) * kBins;
        uint32_t c[E], sum = 0u;
#pragma unroll
        for (uint32_t e = 0; e < E; e++) {
            c[e] = h[tid * E + e];
            sum += c[e];
        }
        if (tid == 0u) s_found[0] = 0xFFFFFFFFu;
        uint32_t run = group_exclusive_scan<4>(sum, lane, wave, s_part);
        const uint32_t need = st.z;
#pragma unroll
        for (uint32_t e = 0; e < E; e++) {
            if (run < need && need - run <= c[e]) {   // at most one bin of the walk
                s_found[0] = tid * E + e;
                s_found[1] = run;
                s_found[2] = c[e];
            }
            run += c[e];
        }
        __syncthreads();
        if (tid == 0u) {
            const uint32_t bin = s_found[0], before = s_found[1], count = s_found[2];
            // found means below 1 << bits(LEVEL); otherwise s_found[0] is still 0xFFFFFFFF (radix_select.hpp, scan_level)
            if (bin >= kBins) {   // no bin of the walk: nothing is selected
                atomicOr(p.out.fault, kKthFaultCount);
                state[j] = make_uint4(0u, 0u, 0u, 1u);
            } else {
                const uint32_t prefix = LEVEL == 0 ? bin : ((st.x << Levels32::bits(LEVEL)) | bin);
                const uint32_t left = need - before;
                state[j] = make_uint4(prefix, Levels32::shift(LEVEL), left,
                                      (LEVEL == Levels32::kLevels - 1 || StopKth::stops(count, left)) ? 1u : 0u);
            }
        }
        __syncthreads();   // the next slot writes s_found and s_part again
    }
    for (uint32_t l = 0; l < slots; l++) {   // uniform; each thread zeroes the words it read
        if (((zero >> l) & 1u) == 0u) continue;
        uint32_t* const h = p.hist + ((size_t)row * slots + l) * kBins;
#pragma unroll
        for (uint32_t e = 0; e < E; e++) h[tid * E + e] = 0u;
    }
}

// One chunk of one row per workgroup, one pass: the keys under each FINAL (prefix, shift) of the row, counted once per distinct
// pair -- into the chunk counts of the lowest slot that has it.
__global__ void __launch_bounds__(kLongThreads) kthm_count_kernel(const LongParams p)
{
    __shared__ uint32_t s_part[kMaxSlots * kLongWaves];
    const uint32_t row = blockIdx.x / p.chunks, c = blockIdx.x % p.chunks;
    if (row >= p.out.rows) return;
    const SlotStates<kMaxSlots> s = slot_states<kMaxSlots>(p, row);
    bool in[kMaxSlots];   // a slot no scan has visited (never) is not counted: its shift is no shift
#pragma unroll
    for (int l = 0; l < kMaxSlots; l++) in[l] = (uint32_t)l < p.out.slots && s.shift[l] < Levels32::kNoLevel;
    const uint32_t lead = leaders(s, in);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const Row32 r = row_of(p.keys, row, p.cols);
    const ChunkRange g = chunk_of(r, p.chunk, c);
    // (key ^ lo) <= span: the key is under the prefix -- lo is the prefix in place, span the bits below it.  As in the histogram
    // kernels the pass costs what sends a key away: two operations per slot into a wave mask and ONE branch per register; a slot
    // that is no leader repeats a leader's pair, and validity is left to the counting path.
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
    auto count = [&](uint32_t key, bool valid) __attribute__((always_inline)) {
        uint64_t any = 0ull;
#pragma unroll
        for (int l = 0; l < kMaxSlots; l++) any |= __ballot((key ^ lo[l]) <= span[l]);
        if (any == 0ull) return;   // (uniform) no lane's key is under a final prefix
#pragma unroll
        for (int l = 0; l < kMaxSlots; l++) {
            if (((lead >> l) & 1u) != 0u)   // uniform
                ne[l] += (valid && (key ^ lo[l]) <= span[l]) ? 1u : 0u;
        }
    };
    if (c == 0u && wave == 0u) {   // uniform
        uint32_t h;
        const uint32_t hv = load_head(r, lane, p.xf, h);
        count(h, hv != 0u);
    }
    for (uint32_t tile = g.lo; tile < g.hi; tile += kLongTile) {   // uniform
        uint32_t t[kRegs];
        const uint32_t vm = load_tile(r, tile + wave * kWaveTile, g.hi, lane, p.xf, t);
#pragma unroll
        for (int i = 0; i < kRegs; i++) count(t[i], ((vm >> i) & 1u) != 0u);
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
struct KthMulti {
    using Levels = Levels32;
    using Params = LongParams;
};
constexpr auto kthm_pick_kernel = pick_slots_kernel<KthMulti>;

// One workgroup per (row, slot) reads the picked chunk, and only up to the tile that holds the key.
__global__ void __launch_bounds__(kLongThreads) kthm_locate_kernel(const LongParams p)
{
    __shared__ uint32_t s_wc_raw[kLongWaves];
    const uint32_t slots = p.out.slots, row = blockIdx.x / slots, slot = blockIdx.x % slots;
    if (row >= p.out.rows) return;
    const uint4 st = p.state[(size_t)row * slots + slot];
    if (st.z == 0u || st.w >= p.chunks) return;   // (uniform) nothing was picked: the fault bit is already set
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const Row32 r = row_of(p.keys, row, p.cols);
    const ChunkRange g = chunk_of(r, p.chunk, st.w);
    volatile lds_u32* const s_wc = (volatile lds_u32*)(lds_u32*)s_wc_raw;
    uint32_t base = 0u;
    bool found = false;
    // chunk 0 has at least one tile (a long row's body is longer than its head), and its first tile carries the head
    for (uint32_t tile = g.lo; tile < g.hi && !found; tile += kLongTile) {   // uniform
        const uint32_t q0 = tile + wave * kWaveTile;
        uint32_t t[kRegs], h = 0u;
        uint32_t vm = load_tile(r, q0, g.hi, lane, p.xf, t);
        if (st.w == 0u && tile == g.lo && wave == 0u) vm |= load_head(r, lane, p.xf, h);   // uniform
        found = locate_tile<(int)kLongWaves>(t, h, vm, q0, r, st.x, st.y, st.z, base, s_wc, wave, lane, row, slot, p.out, p.xf);
    }
    if (!found && tid == 0u) atomicOr(p.out.fault, kKthFaultLocate);
}

// Workspace: control | slot states (16 B per row and slot) | counters [rows][slots][2048] | chunk counts (4 B per chunk and slot) --
// the last two for rows above kLocalSortCap keys only: the single-rank layout with rows * slots rows.  At most
// 256 + rows slots (16 + 8192 + 4 ceil(cols / 16384)) + 3 * 255 bytes; never O(rows * cols).
using KthmLayout = SelectLayout;
KthmLayout kthm_layout(size_t rows, size_t cols, size_t slots) { return select_layout(rows * slots, cols, false, 4); }

template <int SLOTS>
void launch_levels(const LongParams& lp, uint32_t grid, uint32_t row_grid, hipStream_t stream)
{
    hipLaunchKernelGGL((kthm_hist_kernel<1, SLOTS>), dim3(grid), dim3(hist_threads<SLOTS>()), 0, stream, lp);
    hipLaunchKernelGGL(kthm_scan_kernel<1>, dim3(row_grid), dim3(256), 0, stream, lp);
    hipLaunchKernelGGL((kthm_hist_kernel<2, SLOTS>), dim3(grid), dim3(hist_threads<SLOTS>()), 0, stream, lp);
    hipLaunchKernelGGL(kthm_scan_kernel<2>, dim3(row_grid), dim3(256), 0, stream, lp);
}

int run_kth_multi(const uint32_t* keys, size_t rows, size_t cols, const Needs& need, size_t slots, const KeyTransform& xf,
                  uint32_t* out_keys, uint32_t* out_idx, char* ws, const KthmLayout& L, hipStream_t stream)
{
    uint32_t* const ctl = reinterpret_cast<uint32_t*>(ws);
    const Outputs<uint32_t> out{out_keys, out_idx, (uint32_t)rows, (uint32_t)slots, ctl};
    if (cols <= (size_t)kLocalSortCap) {
        const ShortParams sp{keys, (uint32_t)cols, need, xf, out};
        if (cols <= (size_t)kWaveSegCap)
            return launch_short_slots(kthm_clear_kernel, ctl, kthm_short_kernel<1>, dim3(grid_for(rows, 8, 16384)), dim3(512), sp, stream);
        return launch_short_slots(kthm_clear_kernel, ctl, kthm_short_kernel<16>, dim3(grid_for(rows, 1, 4096)), dim3(1024), sp, stream);
    }
    const Chunks ch = chunks_for(rows, cols);
    LongParams lp{};
    lp.keys = keys;
    lp.cols = (uint32_t)cols;
    lp.chunk = ch.chunk;
    lp.chunks = ch.per_row;
    lp.chunk_cap = (uint32_t)chunk_cap_for(cols);
    lp.state = reinterpret_cast<uint4*>(ws + L.state);
    lp.hist = reinterpret_cast<uint32_t*>(ws + L.hist);
    lp.counts = reinterpret_cast<uint32_t*>(ws + L.counts);
    lp.xf = xf;
    lp.out = out;
    if (lp.chunks > lp.chunk_cap) return LSDSORT_ERR_INVALID_ARG;   // never: chunks are at least kMinChunk keys
    const size_t hist_words = rows * slots * kBins;
    const uint32_t grid = (uint32_t)(rows * lp.chunks), row_grid = (uint32_t)rows, slot_grid = (uint32_t)(rows * slots);
    hipLaunchKernelGGL(kthm_clear_kernel, dim3(grid_for(hist_words, 1024, 4096)), dim3(256), 0, stream, ctl, lp.hist, (uint32_t)hist_words,
                       lp.state, (uint32_t)rows, (uint32_t)slots, need);
    hipLaunchKernelGGL(kthm_hist0_kernel, dim3(grid), dim3(kLongThreads), 0, stream, lp);
    hipLaunchKernelGGL(kthm_scan_kernel<0>, dim3(row_grid), dim3(256), 0, stream, lp);
    if (slots <= 2) launch_levels<2>(lp, grid, row_grid, stream);
    else if (slots <= 4) launch_levels<4>(lp, grid, row_grid, stream);
    else launch_levels<8>(lp, grid, row_grid, stream);
    hipLaunchKernelGGL(kthm_count_kernel, dim3(grid), dim3(kLongThreads), 0, stream, lp);
    hipLaunchKernelGGL(kthm_pick_kernel, dim3(slot_grid), dim3(256), 0, stream, lp);
    hipLaunchKernelGGL(kthm_locate_kernel, dim3(slot_grid), dim3(kLongThreads), 0, stream, lp);
    LSD_HIP(hipGetLastError());
    return LSDSORT_OK;
}

}  // namespace
}  // namespace lsd

extern "C" {

size_t lsdsort_kth_multi_workspace_bytes(size_t rows, size_t cols, size_t num_ranks)
{
    if (num_ranks > LSDSORT_KTH_MAX_RANKS || cols > LSDSORT_MAX_KEYS || lsd::multi_too_large(rows, cols, num_ranks)) return 0;
    return lsd::kthm_layout(rows, cols, num_ranks).end;
}

int lsdsort_kth_multi_device(const void* d_keys, size_t rows, size_t cols, const size_t* ranks, size_t num_ranks, int key_type,
                             int largest, void* d_out_keys, uint32_t* d_out_idx, void* d_workspace, size_t workspace_bytes,
                             void* hip_stream)
{
    lsd::KeyTransform xf;
    LSD_TRY(lsd::key_transform(key_type, largest, &xf));
    if (num_ranks > LSDSORT_KTH_MAX_RANKS) return LSDSORT_ERR_INVALID_ARG;
    if (lsd::multi_too_large(rows, cols, num_ranks)) return LSDSORT_ERR_TOO_LARGE;
    if (rows == 0 || cols == 0 || num_ranks == 0) return LSDSORT_OK;   // before the ranks: an empty row has no valid rank
    lsd::Needs need;
    LSD_TRY(lsd::needs_from_ranks(ranks, num_ranks, cols, &need));
    if (!d_keys || !d_out_keys || (((uintptr_t)d_keys | (uintptr_t)d_out_keys) & 3)) return LSDSORT_ERR_INVALID_ARG;
    const lsd::KthmLayout L = lsd::kthm_layout(rows, cols, num_ranks);
    if (!lsd::workspace_ok(d_workspace, workspace_bytes, L.end)) return LSDSORT_ERR_WORKSPACE;
    int rank_method = 0;   // asked for the device set-up alone: nothing here ranks with the returning add
    LSD_TRY(lsd::device_rank_method(8, &rank_method));
    return lsd::run_kth_multi(static_cast<const uint32_t*>(d_keys), rows, cols, need, num_ranks, xf, static_cast<uint32_t*>(d_out_keys),
                              d_out_idx, static_cast<char*>(d_workspace), L, static_cast<hipStream_t>(hip_stream));
}

}  // extern "C"
