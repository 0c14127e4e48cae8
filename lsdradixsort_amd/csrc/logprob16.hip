// logprob16.hip -- log-probabilities and ranks of GIVEN tokens of float16 / bfloat16 logit rows:
//   lsdsort_logprob16_device   row r, slot s: the log-probability of key d_ids[r][s] under the row's tempered softmax, optionally its
//                              rank (the keys of the row that are numbers and strictly greater by value) and the row's log-sum-exp
// What sample16.hip's draw stores for the token it drew, for tokens the caller names: the same best number, the same masses and the
// same integer Z, so that this entry called on the drawn index gives the bits of the draw's d_logprob.  The answer is O(rows * slots)
// floats; no float32 copy of a row exists anywhere.
//
// Arithmetic (keys16_map.hpp's device functions: a value has ONE mass in the filter, the draw and here):
//   m, c, q(x), Z   those of sample16.hip: the best number, the row's scale log2(e) / T, floor(w * 2^32), the integer sum of q
//   logprob  (x == m ? 0 : (x - m) * log_factor(c)) - ln(Z * 2^-32) in float32, the draw's expression in the draw's order; NaN for a NaN
//            key, for a padding id (below 0, or at or above cols) and in a row without a number (Z == 0)
//   rank     the number of keys s of the row with s - nan_lo < S - nan_lo (unsigned), S the sortable value of the queried key, of +0.0
//            where its value is zero: the numbers strictly greater by value; a NaN, an absent register (kAbsent) and a -NaN wrap or
//            lie above and count for nothing.  -1 for a NaN key and a padding id.
//   lse      value(m) * log_factor(c) + ln(Z * 2^-32), a rounded product and a rounded sum; NaN for a greedy row and for Z == 0
// Integer adds commute: Z and the counts do not depend on the chunks, on the waves or on the other rows.
//
// No counterpart in the reference (it sorts one whole array of uint32, LSDRadixSort.cu:839-910).  Three size classes, by cols:
//   cols <= kWaveSegCap (1024)      one wavefront per row, eight rows per workgroup: lane s loads id s and gathers its key in front of
//                                   the row's loads; the row in registers, m by a wave reduction, Z by a 64-bit wave sum; per slot the
//                                   queried key is broadcast and counted by ballot and popcount; lane s stores slot s
//   cols <= kLocalSortCap (16384)   one workgroup of 16 wavefronts per row: the same, the per-wave minima behind one barrier, the
//                                   per-wave sums and counts behind a second; wave 0 stores
//   longer                          launches sized from (rows, cols, slots, with ranks), chunks of 16384 keys: clear, best number per chunk (integer
//                                   atomicMin), sum of q per chunk (ONE plain 64-bit store per chunk, every chunk word on every call)
//                                   and the chunk's counts (integer atomicAdd), finish (one wavefront per row: Z, ln Z, the slots)
// Short rows: one read of the row (2 B/key by byte accounting); long rows two: 4 B/key.
//
// The row read (read_body / read_front), the best number of a row or chunk, wave_add64 and log_total are mass_rows16.hpp's, the ones
// sample16.hip's draw uses; select_tiles16.hpp belongs to the seven selecting units.  Register 8 j + e of a lane is body position
// q0 + 8 (64 j + lane) + e.
// Keys are only read; every store goes to d_logprob / d_rank [row][slot] and d_lse[row] under row < rows.  This unit raises no fault
// bit: the clear kernel zeroes the control block and lsdsort_check_device answers OK.
#define LSDSORT_BUILD 1
#include "../../include/lsdsort.h"

#include "keys16_map.hpp"
#include "lsd_device.hpp"
#include "lsd_host.hpp"
#include "mass_rows16.hpp"
#include "radix_select.hpp"

namespace lsd {
namespace {

constexpr uint32_t kSlots = LSDSORT_LOGPROB_MAX_SLOTS;
constexpr uint32_t kNaN = 0x7FC00000u;
static_assert(kSlots <= 64u, "lane s owns slot s");

// ---- the slots ----------------------------------------------------------------------------------------------------------------------
struct Outputs {
    float* logprob;      // [rows][slots]
    int32_t* rank;       // [rows][slots] or null
    float* lse;          // [rows] or null
    uint32_t rows;
};
// The queried key of lane s < slots: the id of slot s, then the key at it.  A lane without a slot repeats the last slot's, a padding
// id reads key 0: both loads are unconditional and inside the row.  The id depends on nothing of the row and is asked for in front
// of the row's loads; the key is asked for behind them, when the id has long arrived, and is first used behind the masses.
struct Query {
    uint32_t s;      // the sortable value of the key read
    bool pad;        // the id names no key
};
__device__ __forceinline__ int32_t read_id(const int32_t* ids, uint32_t row, uint32_t slots, uint32_t lane)
{
    return ids[(size_t)row * slots + (lane < slots ? lane : slots - 1u)];
}
__device__ __forceinline__ Query read_query(int32_t id, const uint16_t* row_keys, uint32_t cols, const Key16Map& m)
{
    Query q;
    q.pad = (uint32_t)id >= cols;   // a negative id is above every cols as unsigned
    q.s = to_sortable16(row_keys[q.pad ? 0u : (uint32_t)id], m);
    return q;
}
// What a key is compared with for the rank, less nan_lo: a key s is a number strictly greater by value iff s - nan_lo is below it.
// A zero of either sign (by its bits: no float compare, no denormal mode) takes +0.0's sortable value; -0.0 is the next one.
__device__ __forceinline__ uint32_t rank_bound(uint32_t s, const Key16Map& m, const Values16& v)
{
    const bool zero = (from_sortable16(s, m) & 0x7FFFu) == 0u;
    return (zero ? to_sortable16(0u, m) : s) - v.nan_lo;
}
// The keys of one wave's registers below each slot's bound: the bound of slot s is broadcast from lane s, the keys are counted by
// ballot and popcount, and lane s adds the count to `mine`.  `slots` is uniform.
__device__ __forceinline__ void count_slots(const uint32_t (&t)[kRegs], uint32_t h, bool with_head, uint32_t bound, uint32_t slots, uint32_t lane,
                                            const Values16& v, uint32_t& mine)
{
#pragma unroll 1
    for (uint32_t s = 0; s < slots; s++) {
        const uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)bound, (int)s);
        uint32_t n = with_head ? (uint32_t)__popcll(__ballot(h - v.nan_lo < b)) : 0u;
#pragma unroll
        for (int i = 0; i < kRegs; i++) n += (uint32_t)__popcll(__ballot(t[i] - v.nan_lo < b));
        if (lane == s) mine += n;
    }
}
// Slot `lane` of a row: z the row's Z, best_s its best number (kAbsent: none), count the keys below the lane's bound
__device__ __forceinline__ void store_slot(const Outputs& o, uint32_t row, uint32_t slots, uint32_t lane, const Query& q, uint64_t z, uint32_t best_s,
                                           float scale, uint32_t count, const Key16Map& m, const Values16& v)
{
    if (row >= o.rows) return;
    const float best = value_of(best_s & 0xFFFFu, m, v), factor = log_factor(scale), log_z = log_total(z);
    if (lane < slots) {
        const float x = value_of(q.s, m, v);
        const bool none = q.pad || !is_number(q.s, v);
        const float lp = (x == best ? 0.0f : (x - best) * factor) - log_z;
        o.logprob[(size_t)row * slots + lane] = (none || z == 0ull) ? __uint_as_float(kNaN) : lp;
        if (o.rank) o.rank[(size_t)row * slots + lane] = none ? -1 : (int32_t)count;
    }
    if (lane == 0u && o.lse) o.lse[row] = (z == 0ull || is_greedy(scale)) ? __uint_as_float(kNaN) : __fadd_rn(__fmul_rn(best, factor), log_z);
}

// ---- short rows: one wavefront (WAVES = 1, eight rows per workgroup) or one workgroup (WAVES = 16) per row ----------------------
struct ShortParams {
    const uint16_t* keys;
    const int32_t* ids;         // [rows][slots], device
    const float* temperature;   // [rows], device, ALWAYS readable: without has_temperature (1 for every row) the host puts the
    uint32_t has_temperature;   // workspace's row-state area here, which the short tiers do not use, and the value is dropped
    uint32_t cols, rows, slots;
    Key16Map map;
    Values16 val;
    Outputs out;
};

template <int WAVES>
__global__ void __launch_bounds__(WAVES == 1 ? 512 : 1024) logprob16_short_kernel(const ShortParams p)
{
    // WAVES > 1: every row passes both barriers, so a wave that writes s_min for the next row has passed the barrier behind which
    // every wave read this row's minima, and a wave that writes s_sum / s_cnt has passed the next row's first barrier, which wave 0
    // reaches behind its reads of this row's: no third barrier
    __shared__ uint32_t s_min[WAVES];
    __shared__ uint64_t s_sum[WAVES];
    __shared__ uint32_t s_cnt[WAVES * kSlots];
    const uint32_t lane = threadIdx.x & 63u, wave_of_block = threadIdx.x >> 6;
    const uint32_t group = WAVES == 1 ? wave_of_block : 0u, wave = WAVES == 1 ? 0u : wave_of_block;
    // `row` is the same for every thread of a group (a wave, or the whole workgroup): its barriers are reached together
    for (uint32_t row = blockIdx.x * (WAVES == 1 ? 8u : 1u) + group; row < p.rows; row += gridDim.x * (WAVES == 1 ? 8u : 1u)) {
        // the row's scalar and the lane's id: unconditional loads issued in front of the row's loads, no wait of their own
        const float t_load = p.temperature[row];
        const int32_t id = read_id(p.ids, row, p.slots, lane);
        const RowKeys r = row_of(p.keys, row, p.cols);
        const uint32_t q0 = wave * kWaveTile;
        uint32_t t[kRegs];
        read_body(r, q0, r.body, lane, p.map, t);
        const uint32_t h = wave == 0u ? read_front(r, lane, p.map) : kAbsent;
        const Query q = read_query(id, r.keys, p.cols, p.map);
        const float scale = p.has_temperature ? uniform_f32(scale_of(t_load)) : kLog2e;   // one scale per row
        const uint32_t lo_num = row_best_number<WAVES>(t, h, s_min, wave, lane, p.val);
        const float best = value_of(lo_num & 0xFFFFu, p.map, p.val);   // a row of NaNs: every q is 0
        uint64_t z = mass_of_key(h, best, scale, p.map, p.val);
#pragma unroll
        for (int i = 0; i < kRegs; i++) z += mass_of_key(t[i], best, scale, p.map, p.val);
        z = wave_add64(z);
        uint32_t count = 0u;
        if (p.out.rank)   // uniform
            count_slots(t, h, wave == 0u, rank_bound(q.s, p.map, p.val), p.slots, lane, p.val, count);
        if (WAVES > 1) {
            if (lane == 0u) s_sum[wave] = z;
            if (lane < kSlots) s_cnt[wave * kSlots + lane] = count;
            __syncthreads();
            if (wave != 0u) continue;   // uniform over the wave; the barriers of the next row are reached all the same
            uint64_t zs[WAVES];
            uint32_t cs[WAVES];
#pragma unroll
            for (int w = 0; w < WAVES; w++) {   // the reads as one batch, then the adds
                zs[w] = s_sum[w];
                cs[w] = s_cnt[w * kSlots + (lane & (kSlots - 1u))];
            }
            __builtin_amdgcn_sched_barrier(0);
            z = 0ull;
            count = 0u;
#pragma unroll
            for (int w = 0; w < WAVES; w++) {
                z += zs[w];
                count += cs[w];
            }
        }
        store_slot(p.out, row, p.slots, lane, q, z, lo_num, scale, count, p.map, p.val);
    }
}

// ---- long rows ------------------------------------------------------------------------------------------------------------------
struct LongParams {
    const uint16_t* keys;
    const int32_t* ids;           // [rows][slots], device
    const float* temperature;     // [rows], device; null: 1 for every row
    uint32_t cols, rows, slots;
    uint32_t chunk, chunks;       // body positions per chunk (a multiple of kLongTile), chunks per row
    uint32_t* state;              // [rows]: the best number of the row (kAbsent: none), by atomicMin
    uint64_t* sums;               // [rows][chunks]: every word is written on every call
    uint32_t* counts;             // [rows][slots]: cleared and added to in calls with ranks only
    Key16Map map;
    Values16 val;
    Outputs out;
};

// Control block, row words and counts of a call.  With state == nullptr (short rows) it is the control block alone.
__global__ void __launch_bounds__(256) logprob16_clear_kernel(uint32_t* ctl, uint32_t* state, uint32_t rows, uint32_t* counts, uint32_t count_words)
{
    const uint32_t at = blockIdx.x * blockDim.x + threadIdx.x, step = gridDim.x * blockDim.x;
    if (at < (uint32_t)(kCtlBytes / 4)) ctl[at] = 0u;
    if (!state) return;
    for (uint32_t r = at; r < rows; r += step) state[r] = kAbsent;
    for (uint32_t w = at; w < count_words; w += step) counts[w] = 0u;
}

// One chunk of one row per workgroup: the best number of the chunk into the row's word by integer atomicMin.
__global__ void __launch_bounds__(kLongThreads) logprob16_best_kernel(const LongParams p)
{
    __shared__ uint32_t s_part[kLongWaves];
    const uint32_t row = blockIdx.x / p.chunks, c = blockIdx.x % p.chunks;
    if (row >= p.rows) return;
    chunk_best_number(p, row, c, s_part, p.state + row);
}

// One chunk of one row per workgroup: the sum of q over the chunk, chunk 0 with the head keys, by ONE plain 64-bit store -- an empty
// last chunk stores 0, so a replay never reads a stale sum -- and, with ranks, the chunk's keys below each slot's bound added to the
// row's counts.
__global__ void __launch_bounds__(kLongThreads) logprob16_sum_kernel(const LongParams p)
{
    __shared__ uint64_t s_part[kLongWaves];
    __shared__ uint32_t s_cnt[kLongWaves * kSlots];
    const uint32_t row = blockIdx.x / p.chunks, c = blockIdx.x % p.chunks;
    if (row >= p.rows) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const bool ranks = p.out.rank != nullptr;   // uniform
    const RowKeys r = row_of(p.keys, row, p.cols);
    const Query q = read_query(read_id(p.ids, row, p.slots, lane), r.keys, p.cols, p.map);
    const float best = value_of(p.state[row] & 0xFFFFu, p.map, p.val);   // a row of NaNs: every q is 0
    const float scale = row_scale(p.temperature, row);
    const ChunkRange g = chunk_of(r, p.chunk, c);
    const bool front = c == 0u && wave == 0u;   // uniform over the wave
    const uint32_t h = front ? read_front(r, lane, p.map) : kAbsent;
    const uint32_t bound = rank_bound(q.s, p.map, p.val);
    uint64_t sum = mass_of_key(h, best, scale, p.map, p.val);
    uint32_t count = 0u;
    for (uint32_t tile = g.lo; tile < g.hi; tile += kLongTile) {   // uniform
        uint32_t t[kRegs];
        read_body(r, tile + wave * kWaveTile, g.hi, lane, p.map, t);
#pragma unroll
        for (int i = 0; i < kRegs; i++) sum += mass_of_key(t[i], best, scale, p.map, p.val);
        if (ranks) count_slots(t, h, front && tile == g.lo, bound, p.slots, lane, p.val, count);   // chunk 0 has a body: cols is above kLocalSortCap
    }
    sum = wave_add64(sum);
    if (lane == 0u) s_part[wave] = sum;
    if (lane < kSlots) s_cnt[wave * kSlots + lane] = count;
    __syncthreads();
    if (tid < p.slots && ranks) {
        uint32_t all = 0u;
#pragma unroll
        for (uint32_t w = 0; w < kLongWaves; w++) all += s_cnt[w * kSlots + tid];
        if (all != 0u) atomicAdd(p.counts + (size_t)row * p.slots + tid, all);
    }
    if (tid != 0u) return;
    for (uint32_t w = 1; w < kLongWaves; w++) sum += s_part[w];
    p.sums[(size_t)row * p.chunks + c] = sum;
}

// One wavefront per row: Z from the chunk sums, then lane s finishes slot s.
__global__ void __launch_bounds__(64) logprob16_finish_kernel(const LongParams p)
{
    const uint32_t row = blockIdx.x, lane = threadIdx.x;
    if (row >= p.rows) return;
    const RowKeys r = row_of(p.keys, row, p.cols);
    const Query q = read_query(read_id(p.ids, row, p.slots, lane), r.keys, p.cols, p.map);
    const uint64_t* const sums = p.sums + (size_t)row * p.chunks;
    uint64_t z = 0ull;
    for (uint32_t c = lane; c < p.chunks; c += 64u) z += sums[c];
    z = wave_add64(z);
    const uint32_t count = (p.out.rank && lane < p.slots) ? p.counts[(size_t)row * p.slots + lane] : 0u;
    store_slot(p.out, row, p.slots, lane, q, z, p.state[row], row_scale(p.temperature, row), count, p.map, p.val);
}

// This unit's chunks, by cols alone -- a row is cut the same way in every batch: kMinChunk keys each while that gives at most
// kMaxChunks of them (cols up to 2^25), beyond that kMaxChunks chunks of a whole number of tiles.  per_row <= chunk_cap_for(cols).
struct Plan {
    uint32_t chunk, per_row;
};
Plan plan_for(size_t cols)
{
    const size_t cap = chunk_cap_for(cols);
    size_t chunk = max_sz(kMinChunk, (cols + cap - 1) / cap);
    chunk = (chunk + kLongTile - 1) / kLongTile * kLongTile;
    return Plan{(uint32_t)chunk, (uint32_t)((cols + chunk - 1) / chunk)};
}

// Workspace: control | row words, 4 B per row | for rows above kLocalSortCap keys the chunk sums, 8 B per chunk, and the counts, 4 B
// per slot.  The same figure with and without ranks.
struct LogprobLayout {
    size_t state, sums, counts, end;
};
LogprobLayout logprob_layout(size_t rows, size_t cols, size_t slots)
{
    const bool is_long = cols > (size_t)kLocalSortCap;
    LogprobLayout L{};
    L.state = kCtlBytes;
    L.sums = align_up(L.state + rows * 4);
    L.counts = align_up(L.sums + (is_long ? rows * chunk_cap_for(cols) * 8 : 0));
    L.end = align_up(L.counts + (is_long ? rows * slots * 4 : 0));
    return L;
}

int run_logprob(const uint16_t* keys, size_t rows, size_t cols, const int32_t* d_ids, size_t slots, const float* d_temperature, const Key16Map& map,
                const Values16& val, const Outputs& out, char* ws, const LogprobLayout& L, hipStream_t stream)
{
    uint32_t* const ctl = reinterpret_cast<uint32_t*>(ws);
    if (cols <= (size_t)kLocalSortCap) {
        const float* const unused = reinterpret_cast<const float*>(ws + L.state);
        const ShortParams sp{keys, d_ids, d_temperature ? d_temperature : unused, d_temperature ? 1u : 0u, (uint32_t)cols, (uint32_t)rows, (uint32_t)slots,
                             map, val, out};
        hipLaunchKernelGGL(logprob16_clear_kernel, dim3(1), dim3(256), 0, stream, ctl, (uint32_t*)nullptr, 0u, (uint32_t*)nullptr, 0u);
        if (cols <= (size_t)kWaveSegCap)
            hipLaunchKernelGGL(logprob16_short_kernel<1>, dim3(grid_for(rows, 8, 16384)), dim3(512), 0, stream, sp);
        else
            hipLaunchKernelGGL(logprob16_short_kernel<16>, dim3(grid_for(rows, 1, 4096)), dim3(1024), 0, stream, sp);
        LSD_HIP(hipGetLastError());
        return LSDSORT_OK;
    }
    const Plan ch = plan_for(cols);
    LongParams lp{};
    lp.keys = keys;
    lp.ids = d_ids;
    lp.temperature = d_temperature;
    lp.cols = (uint32_t)cols;
    lp.rows = (uint32_t)rows;
    lp.slots = (uint32_t)slots;
    lp.chunk = ch.chunk;
    lp.chunks = ch.per_row;
    lp.state = reinterpret_cast<uint32_t*>(ws + L.state);
    lp.sums = reinterpret_cast<uint64_t*>(ws + L.sums);
    lp.counts = reinterpret_cast<uint32_t*>(ws + L.counts);
    lp.map = map;
    lp.val = val;
    lp.out = out;
    if (lp.chunks > chunk_cap_for(cols)) return LSDSORT_ERR_INVALID_ARG;   // never: chunks are at least kMinChunk keys
    const uint32_t grid = (uint32_t)(rows * lp.chunks), row_grid = (uint32_t)rows;
    const size_t count_words = out.rank ? rows * slots : 0;
    hipLaunchKernelGGL(logprob16_clear_kernel, dim3(grid_for(rows + count_words, 256, 1024)), dim3(256), 0, stream, ctl, lp.state, (uint32_t)rows,
                       lp.counts, (uint32_t)count_words);
    hipLaunchKernelGGL(logprob16_best_kernel, dim3(grid), dim3(kLongThreads), 0, stream, lp);
    hipLaunchKernelGGL(logprob16_sum_kernel, dim3(grid), dim3(kLongThreads), 0, stream, lp);
    hipLaunchKernelGGL(logprob16_finish_kernel, dim3(row_grid), dim3(64), 0, stream, lp);
    LSD_HIP(hipGetLastError());
    return LSDSORT_OK;
}

bool slots_ok(size_t slots) { return slots >= 1 && slots <= LSDSORT_LOGPROB_MAX_SLOTS; }

}  // namespace
}  // namespace lsd

extern "C" {

size_t lsdsort_logprob16_workspace_bytes(size_t rows, size_t cols, size_t slots)
{
    if (!lsd::slots_ok(slots) || cols > LSDSORT_MAX_KEYS || !lsd::sizes_ok(rows, cols)) return 0;
    return lsd::logprob_layout(rows, cols, slots).end;
}

int lsdsort_logprob16_device(const void* d_keys, size_t rows, size_t cols, const int32_t* d_ids, size_t slots, const float* d_temperature,
                             int key_type, float* d_logprob, int32_t* d_rank, float* d_lse, void* d_workspace, size_t workspace_bytes,
                             void* hip_stream)
{
    Key16Map map;
    Values16 val;
    LSD_TRY(float16_values(key_type, &map, &val));
    if (!lsd::slots_ok(slots)) return LSDSORT_ERR_INVALID_ARG;
    if (!lsd::sizes_ok(rows, cols)) return LSDSORT_ERR_TOO_LARGE;
    if (rows == 0 || cols == 0) return LSDSORT_OK;
    if (!d_keys || ((uintptr_t)d_keys & 1)) return LSDSORT_ERR_INVALID_ARG;
    if (!d_ids || !d_logprob || (((uintptr_t)d_ids | (uintptr_t)d_logprob) & 3)) return LSDSORT_ERR_INVALID_ARG;   // the ids are the device's to read
    if (((uintptr_t)d_rank | (uintptr_t)d_lse | (uintptr_t)d_temperature) & 3) return LSDSORT_ERR_INVALID_ARG;     // NULL: none; T = 1
    const lsd::LogprobLayout L = lsd::logprob_layout(rows, cols, slots);
    if (!lsd::workspace_ok(d_workspace, workspace_bytes, L.end)) return LSDSORT_ERR_WORKSPACE;
    int rank_method = 0;   // asked for the device set-up alone: nothing here ranks with the returning add
    LSD_TRY(lsd::device_rank_method(8, &rank_method));
    const lsd::Outputs out{d_logprob, d_rank, d_lse, (uint32_t)rows};
    return lsd::run_logprob(static_cast<const uint16_t*>(d_keys), rows, cols, d_ids, slots, d_temperature, map, val, out,
                            static_cast<char*>(d_workspace), L, static_cast<hipStream_t>(hip_stream));
}

}  // extern "C"
