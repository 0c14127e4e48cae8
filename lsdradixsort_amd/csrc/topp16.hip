// topp16.hip -- the top-p (nucleus) filter of a sampling step for float16 / bfloat16 rows, without a sort:
//   lsdsort_topp16_filter_device   row r keeps the smallest set of its best keys whose softmax mass reaches d_p[r], every duplicate of
//                                  a kept value included; the others become `fill_bits`
//   lsdsort_topp16_filter_ex_device   the same with a temperature T_r and a min-p mp_r per row, each array or NULL (DESIGN.md section
//                                  6.16): masses under T_r, and a second threshold -- the worst number with value >= m + T ln mp --
//                                  of which the stricter one goes into the store; a row whose select is off and whose min-p is
//                                  on needs its best number only
// Softmax weight is a function of the value, so the kept set is "every key at least as good as a threshold T_r" -- what the top-k
// filter (kth16_rowk.hip) stores.  New is the select: it walks MASSES instead of counts.
//
// Arithmetic (the same device functions in every kernel, so that every kernel gives a value the same mass; is_number, value_of, mass_of
// and mass_of_key live in keys16_map.hpp, where sample16.hip's draw takes them from too):
//   s      the sortable value of a key under the 16-bit map with largest: SMALLER is better; +NaN above +inf, -NaN below -inf
//   m      the best key of the row that is no NaN (an integer minimum of s)
//   c      the row's scale log2(e) / T (keys16_map.hpp: scale_of; kLog2e without a temperature, +inf for a greedy row), one SGPR
//   w(x)   float32: 0 for a NaN, 1 where value(x) == value(m), else v_exp_f32((x - m) * c)
//   q(x)   floor(w(x) * 2^32) as uint64 (kMassShift): a row of LSDSORT_MAX_KEYS < 2^30 copies of the maximum sums to < 2^62
//   Z      the sum of q over the row; F(t) the sum of q over the keys with s < t (the mass strictly better than the value t)
//   T      ceil(p * Z) in float64 for p > 0, 0 for p <= 0: for an integer F, F < p * Z is F < T
//   thr    the largest t with F(t) < T, and the row's best key where T == 0 (F is monotonic, so "kept" is s <= thr)
// Integer adds commute: the sums do not depend on the order of LDS or global atomics, on the chunks or on the other rows, and a
// level-0 bin's mass IS the sum of count * q over its 32 values.  The result is deterministic and independent of `rows`.
//
// No counterpart in the reference (it sorts one whole array of uint32, LSDRadixSort.cu:839-910).  Three size classes, by cols:
//   cols <= kWaveSegCap (1024)      one wavefront per row, eight rows per workgroup: the row in registers, the best key by a wave
//                                   reduction, q per register, thr by a 16-step bisection on t (compare, add, wave reduction: no LDS,
//                                   no atomics), then the same registers are compared and stored
//   cols <= kLocalSortCap (16384)   one workgroup of 16 wavefronts per row: the same, the reductions through 16 LDS words and one
//                                   barrier per step
//   longer                          many workgroups per row, launches sized from (rows, cols): clear (states from d_p), best keys
//                                   (integer atomicMin), level-0 MASS histogram (2048 uint64 bins per chunk in LDS, flushed by
//                                   64-bit global atomics), scan 0 (Z, T, the bin where F crosses T, F in front of it), level-1
//                                   COUNT histogram of the low 5 bits under that bin, scan 1 (the 32 values by count * q), apply
// Short rows: one read and one write of the row (4 B/key by byte accounting); long rows three reads for the select, then one read and
// one write: 10 B/key.  Rows with !(p < 1) are off: copied, or left alone in place.
//
// load_tile / load_head / store_tile / store_head are select_tiles16.hpp's, shared with kth16_rowk.hip's top-k filter: the stores
// keep (key >> shift) <= prefix, here the whole threshold with shift 0.  wave_least is mass_rows16.hpp's, shared with the draw and
// the log-probabilities.  Every launch is sized from (rows, cols); phases are ordered by kernel boundaries; every store into d_out
// is guarded by row < rows and stays within the row.  Nothing here ranks with the returning add: the result does not depend on
// lsdsort_set_rank_method.
#define LSDSORT_BUILD 1
#include "../../include/lsdsort.h"

#include "keys16_map.hpp"
#include "lsd_device.hpp"
#include "lsd_host.hpp"
#include "mass_rows16.hpp"
#include "radix_select.hpp"
#include "select_tiles16.hpp"

namespace lsd {
namespace {

constexpr uint32_t kToppFaultSelect = 1024u;   // fault word: no threshold was selected for a row (never expected; nothing stored)
constexpr uint32_t kFailedRow = 2u, kOffRow = 3u;   // row state w: 0 in the select, 1 the threshold is in x, these two from the start or on a fault
// T: an integer F is below p * Z iff it is below ceil(p * Z).  p < 1, Z < 2^62.
__device__ __forceinline__ uint64_t mass_target(float p, uint64_t z)
{
    return p > 0.0f ? (uint64_t)ceil((double)p * (double)z) : 0ull;
}
// The sum over the wave of one value below 2^42 per lane (a lane holds kRegs + 1 masses of at most 2^32): two limbs of 22 and 20 bits,
// each summed on the DPP network (no LDS round trips); all 64 lanes must be active.
__device__ __forceinline__ uint64_t wave_sum64(uint64_t v)
{
    const uint32_t lo = wave_inclusive_scan((uint32_t)v & 0x3FFFFFu), hi = wave_inclusive_scan((uint32_t)(v >> 22));
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)hi, 63) << 22) + (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)lo, 63);
}

// ---- short rows: one wavefront (WAVES = 1, eight rows per workgroup) or one workgroup (WAVES = 16) per row ----------------------
struct ShortParams {
    const uint16_t* keys;
    // The three per-row arrays, [rows] float32 on the device.  All three pointers can ALWAYS be read: where the caller gave none,
    // the host puts the row-state area of the workspace there (16 B per row, which the short tiers do not use) and leaves the
    // array's bit out of `given`, and the value loaded is replaced by the default behind the load.  So the loads are unconditional
    // and stand in front of the row's key loads with no branch and no wait of their own.
    const float* p;          // kGivenP; not given: the select is off for every row
    const float* min_p;      // kGivenMinP; not given: min-p is off for every row
    const float* temperature;   // kGivenT; not given: 1 for every row
    uint32_t given;
    uint32_t cols, rows;
    Key16Map map;
    Values16 val;
    uint32_t* fault;
    uint16_t* dst;           // [rows][cols], may be `keys`
    uint32_t fill;
};
constexpr uint32_t kGivenP = 1u, kGivenMinP = 2u, kGivenT = 4u;

// The sum of one value per thread over the group.  WAVES > 1: through s_sum[WAVES] and ONE barrier; the caller alternates between
// two such arrays from call to call, so that a wave two calls on writes only what every wave has read.
template <int WAVES>
__device__ __forceinline__ uint64_t group_sum64(uint64_t v, volatile lds_u64* s_sum, uint32_t wave, uint32_t lane)
{
    v = wave_sum64(v);
    if (WAVES == 1) return v;
    if (lane == 0u) s_sum[wave] = v;
    __syncthreads();
    // Eight reads in flight, then their adds: left to itself hipcc may issue the 16 reads of the bisection's loop one by one, each
    // behind a full wait for the one before (16 LDS round trips per step: 14 % of the filter at [2^14 x 2^14] when it did).
    uint64_t all = 0ull;
#pragma unroll
    for (int w0 = 0; w0 < WAVES; w0 += 8) {
        uint64_t o[8];
#pragma unroll
        for (int i = 0; i < 8; i++) o[i] = s_sum[w0 + i];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < 8; i++) all += o[i];
    }
    return all;
}
template <int WAVES>
__device__ __forceinline__ uint32_t group_min(uint32_t v, volatile lds_u32* s_min, uint32_t wave, uint32_t lane)
{
    v = wave_least(v);
    if (WAVES == 1) return v;
    if (lane == 0u) s_min[wave] = v;
    __syncthreads();
    uint32_t all = kNoKey;
#pragma unroll
    for (int w = 0; w < WAVES; w++) {
        const uint32_t o = s_min[w];
        all = o < all ? o : all;
    }
    return all;
}

template <int WAVES>
__global__ void __launch_bounds__(WAVES == 1 ? 512 : 1024) topp16_short_kernel(const ShortParams p)
{
    constexpr int kWords = WAVES == 1 ? 1 : WAVES;
    __shared__ uint64_t s_sum_raw[2 * kWords];   // two arrays of per-wave sums, taken in turn
    __shared__ uint32_t s_min_raw[2 * kWords];   // per-wave minima: the best number, the best key
    const uint32_t lane = threadIdx.x & 63u, wave_of_block = threadIdx.x >> 6;
    const uint32_t group = WAVES == 1 ? wave_of_block : 0u, wave = WAVES == 1 ? 0u : wave_of_block;
    volatile lds_u64* const s_sum = (volatile lds_u64*)(lds_u64*)s_sum_raw;
    volatile lds_u32* const s_min = (volatile lds_u32*)(lds_u32*)s_min_raw;
    const bool in_place = p.dst == p.keys;
    // `row` is the same for every thread of a group (a wave, or the whole workgroup): its barriers are reached together
    for (uint32_t row = blockIdx.x * (WAVES == 1 ? 8u : 1u) + group; row < p.rows; row += gridDim.x * (WAVES == 1 ? 8u : 1u)) {
        // the row's scalars: three unconditional loads issued in front of the row's loads and used behind them, no wait of their own
        const float p_load = p.p[row], mp_load = p.min_p[row], t_load = p.temperature[row];
        const Row16 r = row_of(p.keys, row, p.cols);
        const uint32_t q0 = wave * kWaveTile;
        uint32_t t[kRegs];
        load_tile(r, q0, r.body, lane, p.map, t);
        const uint32_t h = wave == 0u ? load_head(r, lane, p.map) : kNoKey;
        // one value each per row; the default where the array was not given (what was loaded in its place means nothing)
        const float pr = (p.given & kGivenP) ? uniform_f32(p_load) : 1.0f, mp = (p.given & kGivenMinP) ? uniform_f32(mp_load) : 0.0f;
        const float tr = (p.given & kGivenT) ? uniform_f32(t_load) : 1.0f;
        const bool off = !(pr < 1.0f);   // (uniform) p >= 1 or NaN: no select
        const bool mp_on = mp > 0.0f;    // (uniform) else min-p is off; both off: the row is copied
        if (off && !mp_on && in_place) continue;
        uint32_t thr = 0xFFFFu;   // every key there is
        bool selected = true;
        if (!off || mp_on) {
            uint32_t lo_key = h, lo_num = is_number(h, p.val) ? h : kNoKey;
#pragma unroll
            for (int i = 0; i < kRegs; i++) {
                lo_key = t[i] < lo_key ? t[i] : lo_key;
                const uint32_t n = is_number(t[i], p.val) ? t[i] : kNoKey;
                lo_num = n < lo_num ? n : lo_num;
            }
            lo_key = group_min<WAVES>(lo_key, s_min, wave, lane);
            lo_num = group_min<WAVES>(lo_num, s_min + kWords, wave, lane);
            const float best = value_of(lo_num & 0xFFFFu, p.map, p.val);   // a row of NaNs: every q is 0
            const float c = (p.given & kGivenT) ? uniform_f32(scale_of(tr)) : kLog2e;
            // The min-p threshold FIRST, one uniform word: best, lo_num, mp and T then end here, and the select's loop below keeps the
            // registers it had before there was a min-p (with them live across it hipcc serialised the loop's 16 LDS reads).
            // A row without a number keeps its best key value alone.
            uint32_t thr_mp = 0xFFFFu;
            if (mp_on) thr_mp = lo_num == kNoKey ? lo_key : minp_threshold(lo_num, minp_theta(best, tr, c, mp), p.map, p.val);
            thr_mp = (uint32_t)__builtin_amdgcn_readfirstlane((int)thr_mp);
            if (!off) {
                uint64_t q[kRegs], part = 0ull;
#pragma unroll
                for (int i = 0; i < kRegs; i++) {
                    q[i] = mass_of_key(t[i], best, c, p.map, p.val);
                    part += q[i];
                }
                const uint64_t qh = mass_of_key(h, best, c, p.map, p.val);
                const uint64_t z = group_sum64<WAVES>(part + qh, s_sum, wave, lane);
                const uint64_t target = mass_target(pr, z);
                thr = 0u;
                // (uniform over the wave) whether any lane's first / second group of eight registers holds a key: a short row, or
                // the last waves of a workgroup, skip the registers that are all kNoKey
                const bool has0 = q0 < r.body, has1 = q0 + 64u * kGroupKeys < r.body;
#pragma unroll 1
                for (int bit = 15; bit >= 0 && target != 0ull; bit--) {   // uniform
                    const uint32_t cand = thr | (1u << bit);
                    uint64_t f = h < cand ? qh : 0ull;
                    if (has0) {
#pragma unroll
                        for (int i = 0; i < kRegs / 2; i++) f += t[i] < cand ? q[i] : 0ull;
                    }
                    if (has1) {
#pragma unroll
                        for (int i = kRegs / 2; i < kRegs; i++) f += t[i] < cand ? q[i] : 0ull;
                    }
                    f = group_sum64<WAVES>(f, s_sum + ((bit & 1) ? kWords : 0), wave, lane);   // z went through the array bit 15 does not take
                    if (f < target) thr = cand;
                }
                if (target == 0ull) thr = lo_key;   // p <= 0, or a row of NaNs: the best value alone
            }
            thr = thr_mp < thr ? thr_mp : thr;   // the stricter of the two thresholds
            selected = thr >= lo_key && lo_key != kNoKey;   // else nothing was selected (never): nothing is stored
            if (!selected && wave == 0u && lane == 0u) atomicOr(p.fault, kToppFaultSelect);
        }
        if (selected) {
            uint16_t* const orow = p.dst + (size_t)row * p.cols;
            store_tile(orow, same_phase(orow, r.keys), r, q0, r.body, lane, t, thr, 0u, p.fill, p.map);
            if (wave == 0u) store_head(orow, r, lane, h, thr, 0u, p.fill, p.map);
        }
        group_sync<WAVES>();   // the next row writes s_min and s_sum again
    }
}

// ---- long rows ------------------------------------------------------------------------------------------------------------------
// Row state in the workspace (uint4): x the bin after scan 0, the threshold after scan 1; y shift (16: no level has run, 5, 0);
// z the bits of p; w 0 in the select, 1 the threshold is in x (y == 0), kFailedRow, kOffRow.  A row's further words live in its
// counter area cnt[row][kBins]: [0, 32) the level-1 counts, then the words below.
constexpr uint32_t kWordBestNum = 32, kWordBestKey = 33, kWordTarget = 34, kWordBefore = 36, kRowWords = 64;

struct LongParams {
    const uint16_t* keys;
    uint32_t cols, rows;
    uint32_t chunk, chunks;       // body positions per chunk (a multiple of kLongTile), chunks per row
    uint4* state;
    uint32_t* cnt;                // [rows][kBins]: the first kRowWords of a row are used
    uint64_t* mass;               // [rows][kBins], zero on entry to the level-0 histogram
    Key16Map map;
    Values16 val;
    uint32_t* fault;
    uint16_t* dst;                // [rows][cols], may be `keys`
    uint32_t fill;
    const float* min_p;           // [rows], device; null: min-p is off for every row
    const float* temperature;     // [rows], device; null: 1 for every row
    uint32_t p_null;              // there is no d_p: the select is off for every row, whatever the clear kernel made of the words it read
};

// What the kernels do with a row.  The clear kernel knows d_p alone: a row is "select off" with the state kOffRow, or in a call
// without d_p.  Such a row is LIVE through min-p where min_p[row] > 0: the best kernel finds its best number and scan 1 turns that
// into its threshold; the mass, scan 0 and count kernels skip it.  Scan 1 leaves every row with kOffRow, a threshold or kFailedRow.
__device__ __forceinline__ bool select_off(const LongParams& p, uint32_t w) { return p.p_null != 0u || w == kOffRow; }
__device__ __forceinline__ bool in_select(const LongParams& p, uint32_t w) { return p.p_null == 0u && w == 0u; }
__device__ __forceinline__ bool minp_on(const LongParams& p, uint32_t row) { return p.min_p && p.min_p[row] > 0.0f; }

// Control block, mass bins, row words and row states of a call, the states from the device array: !(p < 1) gives the "off" state.
// In a call without d_p (LongParams::p_null) `p` is the start of the KEYS and the states made of it mean nothing: every kernel that
// reads a state's w goes through select_off() / in_select(), and scan 1 rewrites every state.
// With state == nullptr (short rows) it is the control block alone.
__global__ void __launch_bounds__(256) topp16_clear_kernel(uint32_t* ctl, uint64_t* mass, uint32_t* cnt, uint4* state, uint32_t rows, const float* p)
{
    const uint32_t at = blockIdx.x * blockDim.x + threadIdx.x, step = gridDim.x * blockDim.x;
    if (at < (uint32_t)(kCtlBytes / 4)) ctl[at] = 0u;
    if (!state) return;
    for (uint32_t q = at; q < rows * kBins; q += step) mass[q] = 0ull;
    for (uint32_t q = at; q < rows * kRowWords; q += step) {
        const uint32_t w = q % kRowWords;
        cnt[(size_t)(q / kRowWords) * kBins + w] = (w == kWordBestNum || w == kWordBestKey) ? kNoKey : 0u;
    }
    for (uint32_t r = at; r < rows; r += step) {
        const float v = p[r];
        state[r] = v < 1.0f ? make_uint4(0u, 16u, __float_as_uint(v), 0u) : make_uint4(0u, 16u, 0u, kOffRow);
    }
}

// One chunk of one row per workgroup: the best key and the best number of the chunk into the row's words by integer atomicMin.
__global__ void __launch_bounds__(kLongThreads) topp16_best_kernel(const LongParams p)
{
    __shared__ uint32_t s_part[2 * kLongWaves];
    const uint32_t row = blockIdx.x / p.chunks, c = blockIdx.x % p.chunks;
    if (row >= p.rows) return;
    const uint32_t w = p.state[row].w;
    if (select_off(p, w) ? !minp_on(p, row) : w != 0u) return;   // uniform
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const Row16 r = row_of(p.keys, row, p.cols);
    const ChunkRange g = chunk_of(r, p.chunk, c);
    uint32_t lo_key = (c == 0u && wave == 0u) ? load_head(r, lane, p.map) : kNoKey;   // uniform
    uint32_t lo_num = is_number(lo_key, p.val) ? lo_key : kNoKey;
    for (uint32_t tile = g.lo; tile < g.hi; tile += kLongTile) {   // uniform
        uint32_t t[kRegs];
        load_tile(r, tile + wave * kWaveTile, g.hi, lane, p.map, t);
#pragma unroll
        for (int i = 0; i < kRegs; i++) {
            lo_key = t[i] < lo_key ? t[i] : lo_key;
            const uint32_t n = is_number(t[i], p.val) ? t[i] : kNoKey;
            lo_num = n < lo_num ? n : lo_num;
        }
    }
    lo_key = wave_least(lo_key);
    lo_num = wave_least(lo_num);
    if (lane == 0u) {
        s_part[wave] = lo_key;
        s_part[kLongWaves + wave] = lo_num;
    }
    __syncthreads();
    if (tid != 0u) return;
    for (uint32_t w = 1; w < kLongWaves; w++) {
        lo_key = s_part[w] < lo_key ? s_part[w] : lo_key;
        lo_num = s_part[kLongWaves + w] < lo_num ? s_part[kLongWaves + w] : lo_num;
    }
    uint32_t* const words = p.cnt + (size_t)row * kBins;
    if (lo_key != kNoKey) atomicMin(words + kWordBestKey, lo_key);
    if (lo_num != kNoKey) atomicMin(words + kWordBestNum, lo_num);
}

// Level 0, one chunk of one row per workgroup: q of every key into the bin of its top 11 bits, in LDS; the non-zero bins are
// flushed into mass[row] by 64-bit global atomics.
__global__ void __launch_bounds__(kLongThreads) topp16_mass_kernel(const LongParams p)
{
    __shared__ unsigned long long s_mass[kBins];
    const uint32_t row = blockIdx.x / p.chunks, c = blockIdx.x % p.chunks;
    if (row >= p.rows) return;
    if (!in_select(p, p.state[row].w)) return;   // uniform
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for (uint32_t b = tid; b < kBins; b += kLongThreads) s_mass[b] = 0ull;
    __syncthreads();
    const float best = value_of(p.cnt[(size_t)row * kBins + kWordBestNum] & 0xFFFFu, p.map, p.val);   // a row of NaNs: every q is 0
    const float scale = row_scale(p.temperature, row);
    const Row16 r = row_of(p.keys, row, p.cols);
    const ChunkRange g = chunk_of(r, p.chunk, c);
    auto add = [&](uint32_t key) __attribute__((always_inline)) {
        const uint64_t q = mass_of_key(key, best, scale, p.map, p.val);
        if (q != 0ull) atomicAdd(&s_mass[key >> 5], (unsigned long long)q);
    };
    if (c == 0u && wave == 0u) add(load_head(r, lane, p.map));   // uniform
    for (uint32_t tile = g.lo; tile < g.hi; tile += kLongTile) {   // uniform
        uint32_t t[kRegs];
        load_tile(r, tile + wave * kWaveTile, g.hi, lane, p.map, t);
#pragma unroll
        for (int i = 0; i < kRegs; i++) add(t[i]);
    }
    __syncthreads();
    unsigned long long* const out = reinterpret_cast<unsigned long long*>(p.mass + (size_t)row * kBins);
    for (uint32_t b = tid; b < kBins; b += kLongThreads) {
        const unsigned long long v = s_mass[b];
        if (v != 0ull) atomicAdd(out + b, v);
    }
}

// Scan 0, one workgroup of 256 per row: Z, T, then the walk from the best end to the bin b with F(32 b) < T <= F(32 b + 32).  T == 0
// (p <= 0, or a row of NaNs): the threshold is the row's best key, and the select is over.
__global__ void __launch_bounds__(256) topp16_scan0_kernel(const LongParams p)
{
    __shared__ uint64_t s_part[4];
    __shared__ uint32_t s_found[3];
    const uint32_t row = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (row >= p.rows) return;
    const uint4 st = p.state[row];
    if (!in_select(p, st.w)) return;   // uniform
    const uint64_t* const bins = p.mass + (size_t)row * kBins;
    constexpr uint32_t E = kBins / 256u;
    uint64_t c[E], sum = 0ull;
#pragma unroll
    for (uint32_t e = 0; e < E; e++) {
        c[e] = bins[tid * E + e];
        sum += c[e];
    }
    uint64_t incl = sum;   // the wave's inclusive scan
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint64_t o = (uint64_t)__shfl_up((unsigned long long)incl, off, kWave);
        if (lane >= (uint32_t)off) incl += o;
    }
    if (lane == 63u) s_part[wave] = incl;
    if (tid == 0u) s_found[0] = kNoKey;
    __syncthreads();
    uint64_t run = incl - sum, z = 0ull;
#pragma unroll
    for (uint32_t w = 0; w < 4; w++) {
        const uint64_t o = s_part[w];
        run += w < wave ? o : 0ull;
        z += o;
    }
    const uint64_t target = mass_target(__uint_as_float(st.z), z);
#pragma unroll
    for (uint32_t e = 0; e < E; e++) {
        if (run < target && target - run <= c[e]) {   // at most one bin of the row
            s_found[0] = tid * E + e;
            s_found[1] = (uint32_t)run;
            s_found[2] = (uint32_t)(run >> 32);
        }
        run += c[e];
    }
    __syncthreads();
    if (tid != 0u) return;
    uint32_t* const words = p.cnt + (size_t)row * kBins;
    const uint32_t bin = s_found[0], best_key = words[kWordBestKey];
    if (target == 0ull && best_key != kNoKey) {
        p.state[row] = make_uint4(best_key & 0xFFFFu, 0u, st.z, 1u);
    } else if (bin >= kBins) {   // no bin of the walk, or a row without keys: nothing is selected (never)
        atomicOr(p.fault, kToppFaultSelect);
        p.state[row] = make_uint4(0u, 0u, st.z, kFailedRow);
    } else {
        words[kWordTarget] = (uint32_t)target;
        words[kWordTarget + 1] = (uint32_t)(target >> 32);
        words[kWordBefore] = s_found[1];
        words[kWordBefore + 1] = s_found[2];
        p.state[row] = make_uint4(bin, 5u, st.z, 0u);
    }
}

// Level 1, one chunk of one row per workgroup: the low 5 bits of the keys whose top 11 are the row's bin, counted.
__global__ void __launch_bounds__(kLongThreads) topp16_count_kernel(const LongParams p)
{
    __shared__ uint32_t s_hist[32];
    const uint32_t row = blockIdx.x / p.chunks, c = blockIdx.x % p.chunks;
    if (row >= p.rows) return;
    const uint4 st = p.state[row];
    if (!in_select(p, st.w)) return;   // uniform
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (tid < 32u) s_hist[tid] = 0u;
    __syncthreads();
    const Row16 r = row_of(p.keys, row, p.cols);
    const ChunkRange g = chunk_of(r, p.chunk, c);
    auto count = [&](uint32_t key) __attribute__((always_inline)) { count_digit(s_hist, (key >> 5) == st.x, key & 31u, lane); };
    if (c == 0u && wave == 0u) count(load_head(r, lane, p.map));   // uniform
    for (uint32_t tile = g.lo; tile < g.hi; tile += kLongTile) {   // uniform
        uint32_t t[kRegs];
        load_tile(r, tile + wave * kWaveTile, g.hi, lane, p.map, t);
#pragma unroll
        for (int i = 0; i < kRegs; i++) count(t[i]);
    }
    __syncthreads();
    if (tid < 32u) {
        const uint32_t v = s_hist[tid];
        if (v != 0u) atomicAdd(p.cnt + (size_t)row * kBins + tid, v);
    }
}

// Scan 1, one thread per row: F moves on through the bin's 32 values by count * q; the threshold is the last value F stays below T at.
// Then the min-p threshold where min-p is on, and the stricter of the two; for a row whose select is off it is the threshold.  A row
// scan 0 ended (T == 0: the best key alone) stays: no min-p threshold is better than the best number.
__global__ void __launch_bounds__(256) topp16_scan1_kernel(const LongParams p)
{
    for (uint32_t row = blockIdx.x * blockDim.x + threadIdx.x; row < p.rows; row += gridDim.x * blockDim.x) {
        const uint4 st = p.state[row];
        const bool no_select = select_off(p, st.w), mp_on = minp_on(p, row);
        if (no_select && !mp_on) {
            if (p.p_null) p.state[row] = make_uint4(0u, 16u, 0u, kOffRow);   // whatever the clear kernel read
            continue;
        }
        if (!no_select && st.w != 0u) continue;
        const uint32_t* const words = p.cnt + (size_t)row * kBins;
        const uint32_t best_num = words[kWordBestNum], best_key = words[kWordBestKey];
        const float best = value_of(best_num & 0xFFFFu, p.map, p.val);
        const float t = p.temperature ? p.temperature[row] : 1.0f, scale = p.temperature ? scale_of(t) : kLog2e;
        uint32_t thr = 0xFFFFu;
        if (!no_select) {
            const uint64_t target = (uint64_t)words[kWordTarget] | ((uint64_t)words[kWordTarget + 1] << 32);
            uint64_t f = (uint64_t)words[kWordBefore] | ((uint64_t)words[kWordBefore + 1] << 32);   // F(32 bin) < T
            thr = st.x << 5;
#pragma unroll 1
            for (uint32_t d = 0; d < 31u; d++) {
                f += (uint64_t)words[d] * mass_of_key((st.x << 5) + d, best, scale, p.map, p.val);   // F(32 bin + d + 1)
                if (f >= target) break;
                thr = (st.x << 5) + d + 1u;
            }
        }
        if (mp_on) {   // a row without a number keeps its best key value alone
            const uint32_t thr_mp = best_num == kNoKey ? best_key : minp_threshold(best_num, minp_theta(best, t, scale, p.min_p[row]), p.map, p.val);
            thr = thr_mp < thr ? thr_mp : thr;
        }
        if (thr > 0xFFFFu) {   // a row without keys (never): nothing is stored
            atomicOr(p.fault, kToppFaultSelect);
            p.state[row] = make_uint4(0u, 0u, st.z, kFailedRow);
            continue;
        }
        p.state[row] = make_uint4(thr, 0u, st.z, 1u);
    }
}

// The filter over one chunk of one row per workgroup, the chunks of the select: the state holds the row's threshold; an "off" row is
// copied, or left alone in place.  Anything else is a row nothing was selected for (its fault bit is set) -- never: nothing is stored.
__global__ void __launch_bounds__(kLongThreads) topp16_apply_kernel(const LongParams p)
{
    const uint32_t row = blockIdx.x / p.chunks, c = blockIdx.x % p.chunks;
    if (row >= p.rows) return;
    const uint4 st = p.state[row];
    const bool off = st.w == kOffRow;   // uniform
    if (off ? p.dst == p.keys : !(st.w == 1u && st.y == 0u)) return;
    const uint32_t thr = off ? 0xFFFFu : (st.x & 0xFFFFu);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const Row16 r = row_of(p.keys, row, p.cols);
    const ChunkRange g = chunk_of(r, p.chunk, c);
    uint16_t* const orow = p.dst + (size_t)row * p.cols;
    const bool vec = same_phase(orow, r.keys);
    if (c == 0u && wave == 0u) store_head(orow, r, lane, load_head(r, lane, p.map), thr, 0u, p.fill, p.map);   // uniform
    for (uint32_t tile = g.lo; tile < g.hi; tile += kLongTile) {   // uniform
        const uint32_t q0 = tile + wave * kWaveTile;
        uint32_t t[kRegs];
        load_tile(r, q0, g.hi, lane, p.map, t);
        store_tile(orow, vec, r, q0, g.hi, lane, t, thr, 0u, p.fill, p.map);
    }
}

// Workspace: the top-k filter's (control | row states, 16 B per row | counters [rows][2048] uint32 for rows above kLocalSortCap keys)
// and behind it, for such rows, the mass bins [rows][2048] uint64.
struct ToppLayout {
    size_t state, cnt, mass, end;
};
ToppLayout topp_layout(size_t rows, size_t cols)
{
    const SelectLayout S = select_layout(rows, cols, false, 0);
    ToppLayout L{};
    L.state = S.state;
    L.cnt = S.hist;
    L.mass = S.end;
    L.end = align_up(S.end + (cols > (size_t)kLocalSortCap ? rows * kBins * 8 : 0));
    return L;
}

// The per-row arrays of a call, each of them null where the caller gave none.
struct RowScalars {
    const float* p;
    const float* min_p;
    const float* temperature;
};

int run_topp(const uint16_t* keys, size_t rows, size_t cols, const RowScalars& rs, const Key16Map& map, const Values16& val, uint32_t fill,
             uint16_t* dst, char* ws, const ToppLayout& L, hipStream_t stream)
{
    uint32_t* const ctl = reinterpret_cast<uint32_t*>(ws);
    if (cols <= (size_t)kLocalSortCap) {
        const float* const unused = reinterpret_cast<const float*>(ws + L.state);   // 16 B per row: readable, and no short tier's
        const uint32_t given = (rs.p ? kGivenP : 0u) | (rs.min_p ? kGivenMinP : 0u) | (rs.temperature ? kGivenT : 0u);
        const ShortParams sp{keys, rs.p ? rs.p : unused, rs.min_p ? rs.min_p : unused, rs.temperature ? rs.temperature : unused, given,
                             (uint32_t)cols, (uint32_t)rows, map, val, ctl, dst, fill};
        hipLaunchKernelGGL(topp16_clear_kernel, dim3(1), dim3(256), 0, stream, ctl, (uint64_t*)nullptr, (uint32_t*)nullptr, (uint4*)nullptr, 0u,
                           (const float*)nullptr);
        if (cols <= (size_t)kWaveSegCap)
            hipLaunchKernelGGL(topp16_short_kernel<1>, dim3(grid_for(rows, 8, 16384)), dim3(512), 0, stream, sp);
        else
            hipLaunchKernelGGL(topp16_short_kernel<16>, dim3(grid_for(rows, 1, 4096)), dim3(1024), 0, stream, sp);
        LSD_HIP(hipGetLastError());
        return LSDSORT_OK;
    }
    const Chunks ch = chunks_for(rows, cols);
    LongParams lp{};
    lp.keys = keys;
    lp.cols = (uint32_t)cols;
    lp.rows = (uint32_t)rows;
    lp.chunk = ch.chunk;
    lp.chunks = ch.per_row;
    lp.state = reinterpret_cast<uint4*>(ws + L.state);
    lp.cnt = reinterpret_cast<uint32_t*>(ws + L.cnt);
    lp.mass = reinterpret_cast<uint64_t*>(ws + L.mass);
    lp.map = map;
    lp.val = val;
    lp.fault = ctl;
    lp.dst = dst;
    lp.fill = fill;
    lp.min_p = rs.min_p;
    lp.temperature = rs.temperature;
    lp.p_null = rs.p ? 0u : 1u;
    // The clear kernel takes the row states from an array of `rows` float32 that exists.  Without d_p it reads the first 4 * rows
    // bytes of the keys from their first 4-byte boundary on (rows of more than 16384 keys: they are there), and p_null tells every
    // kernel that those states mean nothing.
    const float* const clear_p = rs.p ? rs.p : reinterpret_cast<const float*>(((uintptr_t)keys + 3) & ~(uintptr_t)3);
    if (lp.chunks > chunk_cap_for(cols)) return LSDSORT_ERR_INVALID_ARG;   // never: chunks are at least kMinChunk keys
    const uint32_t grid = (uint32_t)(rows * lp.chunks), row_grid = (uint32_t)rows;
    hipLaunchKernelGGL(topp16_clear_kernel, dim3(grid_for(rows * kBins, 1024, 4096)), dim3(256), 0, stream, ctl, lp.mass, lp.cnt, lp.state,
                       (uint32_t)rows, clear_p);
    hipLaunchKernelGGL(topp16_best_kernel, dim3(grid), dim3(kLongThreads), 0, stream, lp);
    hipLaunchKernelGGL(topp16_mass_kernel, dim3(grid), dim3(kLongThreads), 0, stream, lp);
    hipLaunchKernelGGL(topp16_scan0_kernel, dim3(row_grid), dim3(256), 0, stream, lp);
    hipLaunchKernelGGL(topp16_count_kernel, dim3(grid), dim3(kLongThreads), 0, stream, lp);
    hipLaunchKernelGGL(topp16_scan1_kernel, dim3(grid_for(rows, 256, 1024)), dim3(256), 0, stream, lp);
    hipLaunchKernelGGL(topp16_apply_kernel, dim3(grid), dim3(kLongThreads), 0, stream, lp);
    LSD_HIP(hipGetLastError());
    return LSDSORT_OK;
}

// Both entries.  need_p: the entry without min-p has no defined answer for a NULL d_p.
int filter_call(const void* d_keys, size_t rows, size_t cols, const RowScalars& rs, bool need_p, int key_type, uint16_t fill_bits, void* d_out,
                void* d_workspace, size_t workspace_bytes, void* hip_stream)
{
    Key16Map map;
    Values16 val;
    LSD_TRY(float16_values(key_type, &map, &val));
    if (!lsd::sizes_ok(rows, cols)) return LSDSORT_ERR_TOO_LARGE;
    if (rows == 0 || cols == 0) return LSDSORT_OK;
    if (!d_keys || !d_out || (((uintptr_t)d_keys | (uintptr_t)d_out) & 1)) return LSDSORT_ERR_INVALID_ARG;
    if ((need_p && !rs.p) || ((uintptr_t)rs.p & 3)) return LSDSORT_ERR_INVALID_ARG;   // their values are the device's to read
    if ((((uintptr_t)rs.min_p | (uintptr_t)rs.temperature) & 3)) return LSDSORT_ERR_INVALID_ARG;
    const lsd::ToppLayout L = lsd::topp_layout(rows, cols);
    if (!lsd::workspace_ok(d_workspace, workspace_bytes, L.end)) return LSDSORT_ERR_WORKSPACE;
    int rank_method = 0;   // asked for the device set-up alone: nothing here ranks with the returning add
    LSD_TRY(lsd::device_rank_method(8, &rank_method));
    return lsd::run_topp(static_cast<const uint16_t*>(d_keys), rows, cols, rs, map, val, (uint32_t)fill_bits, static_cast<uint16_t*>(d_out),
                         static_cast<char*>(d_workspace), L, static_cast<hipStream_t>(hip_stream));
}

}  // namespace
}  // namespace lsd

extern "C" {

size_t lsdsort_topp16_filter_workspace_bytes(size_t rows, size_t cols)
{
    if (cols > LSDSORT_MAX_KEYS || !lsd::sizes_ok(rows, cols)) return 0;
    return lsd::topp_layout(rows, cols).end;
}

int lsdsort_topp16_filter_device(const void* d_keys, size_t rows, size_t cols, const float* d_p, int key_type, uint16_t fill_bits, void* d_out,
                                 void* d_workspace, size_t workspace_bytes, void* hip_stream)
{
    return lsd::filter_call(d_keys, rows, cols, lsd::RowScalars{d_p, nullptr, nullptr}, true, key_type, fill_bits, d_out, d_workspace,
                            workspace_bytes, hip_stream);
}

int lsdsort_topp16_filter_ex_device(const void* d_keys, size_t rows, size_t cols, const float* d_p, const float* d_min_p,
                                    const float* d_temperature, int key_type, uint16_t fill_bits, void* d_out, void* d_workspace,
                                    size_t workspace_bytes, void* hip_stream)
{
    return lsd::filter_call(d_keys, rows, cols, lsd::RowScalars{d_p, d_min_p, d_temperature}, false, key_type, fill_bits, d_out, d_workspace,
                            workspace_bytes, hip_stream);
}

}  // extern "C"
