// sample16.hip -- the draw of a sampling step for float16 / bfloat16 rows:
//   lsdsort_sample16_device   row r stores the position i whose softmax mass interval holds u_r * Z_r, u_r read from DEVICE memory,
//                             and optionally that key's log-probability
//   lsdsort_sample16_ex_device   the same under a temperature T_r per row from DEVICE memory; the entry above
//                             is this one with NULL
// The inverse CDF in POSITION order: no select, no sort -- one maximum, one prefix sum, one crossing.  It follows the filters
// (kth16_rowk.hip, topp16.hip) in place: what they fill with -inf has no mass and is never drawn.
//
// Arithmetic (keys16_map.hpp's device functions, the ones topp16.hip uses, so that a value has ONE mass in the filter and the draw):
//   m      the best key of the row that is no NaN (an integer minimum of the sortable value under the 16-bit map with largest)
//   c      the row's scale log2(e) / T (keys16_map.hpp: scale_of; kLog2e without a temperature, +inf for a greedy row), one SGPR
//   q(x)   floor(w(x) * 2^32) as uint64: w = 0 for a NaN, 1 where value(x) == value(m), else v_exp_f32((x - m) * c)
//   Z      the sum of q over the row (< 2^62); C_i the sum of q over the positions in front of i
//   G      0 where !(u > 0); Z - 1 where u >= 1; else min(Z - 1, floor((double)u * (double)Z))
//   i      the position with C_i <= G < C_i + q_i: a key of zero mass is never drawn; Z == 0 (no number in the row) gives -1
//   logprob (x_i - m) * (c ln 2) - ln(Z * 2^-32) in float32, the factor taken as 1 for c == kLog2e and x_i - m as 0 where x_i == m (a
//          row whose best number is an infinity)
// Integer adds commute: C, Z and G do not depend on the chunks, on the waves or on the other rows.  The same (row, u) gives the same
// index on every call, in any batch, at any `rows`.
//
// No counterpart in the reference (it sorts one whole array of uint32, LSDRadixSort.cu:839-910).  Three size classes, by cols:
//   cols <= kWaveSegCap (1024)      one wavefront per row, eight rows per workgroup: the row in registers, m by a wave reduction, q per
//                                   register, a 64-bit exclusive scan over the wave in position order (head, then load group by load
//                                   group, limbs on the DPP network), and the one lane whose range holds G walks its eight keys
//   cols <= kLocalSortCap (16384)   one workgroup of 16 wavefronts per row: the same, the per-wave minima and the per-wave sums through
//                                   LDS behind one barrier each; the wave whose range holds G finishes
//   longer                          launches sized from (rows, cols): clear, best number per chunk (integer atomicMin), sum of q per chunk
//                                   (ONE plain 64-bit store per chunk, every chunk word on every call), pick (Z, G, the chunk that holds
//                                   G and the remainder), locate (one workgroup per row reads that ONE chunk up to the crossing)
// Short rows: one read of the row (2 B/key by byte accounting); long rows two reads plus one chunk: about 4 B/key.
//
// The row read (read_front / read_body), the best number of a row or chunk and the small wave helpers are mass_rows16.hpp's, shared
// with logprob16.hip and topp16.hip; select_tiles16.hpp belongs to the seven selecting units.  A lane holds two 16-byte groups of its
// wave's tile: register 8 j + e is body position q0 + 8 (64 j + lane) + e, so position order is "head keys by lane, then group
// j = 0, 1: lane by lane, key by key".  Keys are only read; every store goes to d_index[row] / d_logprob[row] under row < rows.  Every
// launch is sized from (rows, cols); phases are ordered by kernel boundaries.
#define LSDSORT_BUILD 1
#include "../../include/lsdsort.h"

#include "keys16_map.hpp"
#include "lsd_device.hpp"
#include "lsd_host.hpp"
#include "mass_rows16.hpp"
#include "radix_select.hpp"

namespace lsd {
namespace {

constexpr uint32_t kSampleFaultLocate = 1024u;   // fault word: no key was located for a row that has mass (never expected; nothing stored)
constexpr uint32_t kNoPick = 0xFFFFu;            // row state of the long rows: no chunk was picked (Z == 0, or a fault)

// ---- wave arithmetic (wave_least, best_number, wave_add64 and log_total: mass_rows16.hpp) -------------------------------------------
// The inclusive scan over the wave of one value below 2^42 per lane (eight masses of at most 2^32): two limbs of 22 and 20 bits, each
// scanned on the DPP network.  All 64 lanes must be active.
__device__ __forceinline__ uint64_t wave_scan64(uint64_t v)
{
    const uint32_t lo = wave_inclusive_scan((uint32_t)v & 0x3FFFFFu), hi = wave_inclusive_scan((uint32_t)(v >> 22));
    return ((uint64_t)hi << 22) + (uint64_t)lo;
}
__device__ __forceinline__ uint64_t of_lane63(uint64_t v)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 63), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 63);
    return ((uint64_t)hi << 32) | lo;
}

// G of a row with Z != 0
__device__ __forceinline__ uint64_t mass_point(float u, uint64_t z)
{
    if (!(u > 0.0f)) return 0ull;   // zero, a negative u, a NaN
    if (u >= 1.0f) return z - 1ull;
    const uint64_t g = (uint64_t)floor((double)u * (double)z);   // below 2^62
    return g < z - 1ull ? g : z - 1ull;
}

// One wave's tile in registers (read_body at q0; h the head keys in front of it, kAbsent where there is none) with its masses, scanned
// in position order: per lane the mass in front of its head key and in front of each of its two groups, within the wave, and the wave's
// total.  HAS1 (uniform): the second group of some lane holds a key.
struct Masses {
    uint64_t q[kRegs], qh;
    uint64_t at_h, at_g[kRegs / 8], sum_g[kRegs / 8];   // exclusive prefixes within the wave, and the lane's group sums
    uint64_t total;
};
__device__ __forceinline__ void scan_masses(const uint32_t (&t)[kRegs], uint32_t h, float best, float scale, bool has1, const Key16Map& m,
                                            const Values16& v, Masses& s)
{
    s.qh = mass_of_key(h, best, scale, m, v);
    const uint64_t incl_h = wave_scan64(s.qh);
    s.at_h = incl_h - s.qh;
    uint64_t run = of_lane63(incl_h);
#pragma unroll
    for (int j = 0; j < kRegs / 8; j++) {
        s.sum_g[j] = 0ull;
        s.at_g[j] = run;
        if (j == 0 || has1) {   // uniform
#pragma unroll
            for (int e = 0; e < 8; e++) {
                s.q[8 * j + e] = mass_of_key(t[8 * j + e], best, scale, m, v);
                s.sum_g[j] += s.q[8 * j + e];
            }
            const uint64_t incl = wave_scan64(s.sum_g[j]);
            s.at_g[j] = run + incl - s.sum_g[j];
            run += of_lane63(incl);
        } else {
#pragma unroll
            for (int e = 0; e < 8; e++) s.q[8 * j + e] = 0ull;
        }
    }
    s.total = run;
}

struct DrawOut {
    int32_t* index;      // [rows]
    float* logprob;      // [rows] or null
    uint32_t rows;
};
// The wave whose range [before, before + s.total) holds g: the one lane whose key's interval holds g stores the key's position and its
// log-probability.  Returns whether a lane did (uniform over the wave).  `pos0`: the row position of body position q0; `factor`:
// log_factor of the row's scale.
__device__ __forceinline__ bool draw_in_wave(const uint32_t (&t)[kRegs], uint32_t h, const Masses& s, uint64_t before, uint64_t g, uint32_t pos0,
                                             uint32_t lane, uint32_t row, float best, float factor, float log_z, const DrawOut& o,
                                             const Key16Map& m, const Values16& v)
{
    bool mine = false;
    auto store = [&](uint32_t key, uint32_t pos) {
        mine = true;
        if (row < o.rows) {
            o.index[row] = (int32_t)pos;
            if (o.logprob) {
                const float x = value_of(key & 0xFFFFu, m, v);
                o.logprob[row] = (x == best ? 0.0f : (x - best) * factor) - log_z;
            }
        }
    };
    const uint64_t ch = before + s.at_h;
    if (ch <= g && g - ch < s.qh) store(h, lane);
#pragma unroll
    for (int j = 0; j < kRegs / 8; j++) {
        uint64_t c = before + s.at_g[j];
        if (c <= g && g - c < s.sum_g[j]) {
            uint64_t left = g - c;   // below the group's sum: one key of the eight takes it
            bool done = false;
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const uint64_t qe = s.q[8 * j + e];
                if (!done && left < qe) {
                    store(t[8 * j + e], pos0 + ((uint32_t)j * 64u + lane) * kGroupKeys + (uint32_t)e);
                    done = true;
                }
                left -= done ? 0ull : qe;
            }
        }
    }
    return __ballot(mine) != 0ull;
}

// ---- short rows: one wavefront (WAVES = 1, eight rows per workgroup) or one workgroup (WAVES = 16) per row ----------------------
struct ShortParams {
    const uint16_t* keys;
    const float* u;          // [rows], device
    const float* temperature;   // [rows], device, ALWAYS readable: without has_temperature (1 for every row) the host puts the
    uint32_t has_temperature;   // workspace's row-state area here, 16 B per row the short tiers do not use, and the value is dropped
    uint32_t cols, rows;
    Key16Map map;
    Values16 val;
    uint32_t* fault;
    DrawOut out;
};

template <int WAVES>
__global__ void __launch_bounds__(WAVES == 1 ? 512 : 1024) sample16_short_kernel(const ShortParams p)
{
    // WAVES > 1: the minima and the sums have an array each and every row passes both barriers, so a wave that writes s_min for the
    // next row has passed the barrier behind which every wave read this row's minima, and likewise s_sum: no third barrier
    __shared__ uint32_t s_min[WAVES];
    __shared__ uint64_t s_sum[WAVES];
    const uint32_t lane = threadIdx.x & 63u, wave_of_block = threadIdx.x >> 6;
    const uint32_t group = WAVES == 1 ? wave_of_block : 0u, wave = WAVES == 1 ? 0u : wave_of_block;
    // `row` is the same for every thread of a group (a wave, or the whole workgroup): its barriers are reached together
    for (uint32_t row = blockIdx.x * (WAVES == 1 ? 8u : 1u) + group; row < p.rows; row += gridDim.x * (WAVES == 1 ? 8u : 1u)) {
        // the row's scalars: two unconditional loads issued in front of the row's loads and used behind them, no wait of their own
        const float u_load = p.u[row], t_load = p.temperature[row];
        const RowKeys r = row_of(p.keys, row, p.cols);
        const uint32_t q0 = wave * kWaveTile;
        uint32_t t[kRegs];
        read_body(r, q0, r.body, lane, p.map, t);
        const uint32_t h = wave == 0u ? read_front(r, lane, p.map) : kAbsent;
        const float u = uniform_f32(u_load);   // one value per row
        const float scale = p.has_temperature ? uniform_f32(scale_of(t_load)) : kLog2e;   // and one scale
        const uint32_t lo_num = row_best_number<WAVES>(t, h, s_min, wave, lane, p.val);
        const float best = value_of(lo_num & 0xFFFFu, p.map, p.val);   // a row of NaNs: every q is 0
        Masses s;
        scan_masses(t, h, best, scale, q0 + 64u * kGroupKeys < r.body, p.map, p.val, s);
        uint64_t before = 0ull, z = s.total;
        if (WAVES > 1) {
            if (lane == 0u) s_sum[wave] = s.total;
            __syncthreads();
            z = 0ull;
#pragma unroll
            for (int w = 0; w < WAVES; w++) {
                const uint64_t o = s_sum[w];
                before += (uint32_t)w < wave ? o : 0ull;
                z += o;
            }
        }
        if (z == 0ull) {   // (uniform) no number in the row: data, not a fault
            if (wave == 0u && lane == 0u) {
                p.out.index[row] = -1;
                if (p.out.logprob) p.out.logprob[row] = __uint_as_float(0x7FC00000u);
            }
            continue;
        }
        const uint64_t g = mass_point(u, z);
        if (g < before || g - before >= s.total) continue;   // (uniform over the wave) another wave's range holds g
        if (!draw_in_wave(t, h, s, before, g, r.head + q0, lane, row, best, log_factor(scale), log_total(z), p.out, p.map, p.val) && lane == 0u)
            atomicOr(p.fault, kSampleFaultLocate);
    }
}

// ---- long rows ------------------------------------------------------------------------------------------------------------------
// Row state in the workspace (uint4): x the best number of the row (kAbsent: none), from the best kernel's atomicMin; the pick kernel
// adds the picked chunk in the bits above it (x = chunk << 16 | best; chunk kNoPick: nothing to locate), y the bits of ln(Z * 2^-32),
// (z, w) the remainder G - S_c, the mass in front of the crossing within the chunk.
struct LongParams {
    const uint16_t* keys;
    const float* u;               // [rows], device
    const float* temperature;     // [rows], device; null: 1 for every row
    uint32_t cols, rows;
    uint32_t chunk, chunks;       // body positions per chunk (a multiple of kLongTile), chunks per row
    uint4* state;
    uint64_t* sums;               // [rows][chunks]: every word is written on every call
    Key16Map map;
    Values16 val;
    uint32_t* fault;
    DrawOut out;
};

// Control block and row words of a call.  With state == nullptr (short rows) it is the control block alone.
__global__ void __launch_bounds__(256) sample16_clear_kernel(uint32_t* ctl, uint4* state, uint32_t rows)
{
    const uint32_t at = blockIdx.x * blockDim.x + threadIdx.x, step = gridDim.x * blockDim.x;
    if (at < (uint32_t)(kCtlBytes / 4)) ctl[at] = 0u;
    if (!state) return;
    for (uint32_t r = at; r < rows; r += step) state[r] = make_uint4(kAbsent, 0u, 0u, 0u);
}

// One chunk of one row per workgroup: the best number of the chunk into the row's word by integer atomicMin.
__global__ void __launch_bounds__(kLongThreads) sample16_best_kernel(const LongParams p)
{
    __shared__ uint32_t s_part[kLongWaves];
    const uint32_t row = blockIdx.x / p.chunks, c = blockIdx.x % p.chunks;
    if (row >= p.rows) return;
    chunk_best_number(p, row, c, s_part, reinterpret_cast<uint32_t*>(p.state + row));   // the state's x
}

// One chunk of one row per workgroup: the sum of q over the chunk, chunk 0 with the head keys, by ONE plain 64-bit store.  An empty
// last chunk stores 0: every chunk word is written on every call, so a replay never reads a stale sum.
__global__ void __launch_bounds__(kLongThreads) sample16_sum_kernel(const LongParams p)
{
    __shared__ uint64_t s_part[kLongWaves];
    const uint32_t row = blockIdx.x / p.chunks, c = blockIdx.x % p.chunks;
    if (row >= p.rows) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const float best = value_of(p.state[row].x & 0xFFFFu, p.map, p.val);   // a row of NaNs: every q is 0
    const float scale = row_scale(p.temperature, row);
    const RowKeys r = row_of(p.keys, row, p.cols);
    const ChunkRange g = chunk_of(r, p.chunk, c);
    uint64_t sum = mass_of_key((c == 0u && wave == 0u) ? read_front(r, lane, p.map) : kAbsent, best, scale, p.map, p.val);   // uniform
    for (uint32_t tile = g.lo; tile < g.hi; tile += kLongTile) {   // uniform
        uint32_t t[kRegs];
        read_body(r, tile + wave * kWaveTile, g.hi, lane, p.map, t);
#pragma unroll
        for (int i = 0; i < kRegs; i++) sum += mass_of_key(t[i], best, scale, p.map, p.val);
    }
    sum = wave_add64(sum);
    if (lane == 0u) s_part[wave] = sum;
    __syncthreads();
    if (tid != 0u) return;
    for (uint32_t w = 1; w < kLongWaves; w++) sum += s_part[w];
    p.sums[(size_t)row * p.chunks + c] = sum;
}

// One wavefront per row: Z from the chunk sums, G, the chunk c with S_c <= G < S_c + sum_c and the remainder G - S_c into the row
// state.  Z == 0: index -1 and logprob NaN are stored here, and nothing is left to locate.
__global__ void __launch_bounds__(64) sample16_pick_kernel(const LongParams p)
{
    const uint32_t row = blockIdx.x, lane = threadIdx.x;
    if (row >= p.rows) return;
    const uint64_t* const sums = p.sums + (size_t)row * p.chunks;
    const uint32_t per = (p.chunks + 63u) / 64u;   // consecutive chunks of one lane
    const uint32_t c_lo = lane * per < p.chunks ? lane * per : p.chunks, c_hi = p.chunks - c_lo < per ? p.chunks : c_lo + per;
    uint64_t mine = 0ull;
    for (uint32_t c = c_lo; c < c_hi; c++) mine += sums[c];
    uint64_t incl = mine;   // the wave's inclusive scan: a lane's sum has no 42-bit bound here
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint64_t o = (uint64_t)__shfl_up((unsigned long long)incl, off, kWave);
        if (lane >= (uint32_t)off) incl += o;
    }
    const uint64_t z = (uint64_t)__shfl((unsigned long long)incl, 63, kWave);
    const uint32_t best = p.state[row].x & 0xFFFFu;
    if (z == 0ull) {   // uniform
        if (lane == 0u) {
            p.state[row] = make_uint4((kNoPick << 16) | best, 0u, 0u, 0u);
            p.out.index[row] = -1;
            if (p.out.logprob) p.out.logprob[row] = __uint_as_float(0x7FC00000u);
        }
        return;
    }
    const float u = p.u[row];
    const uint64_t g = mass_point(u, z);
    uint64_t run = incl - mine;
    bool found = false;
    if (run <= g && g - run < mine) {   // one lane of the wave
        for (uint32_t c = c_lo; c < c_hi; c++) {
            const uint64_t v = sums[c];
            if (g - run < v) {
                const uint64_t left = g - run;
                p.state[row] = make_uint4((c << 16) | best, __float_as_uint(log_total(z)), (uint32_t)left, (uint32_t)(left >> 32));
                found = true;
                break;
            }
            run += v;
        }
    }
    if (__ballot(found) == 0ull && lane == 0u) {   // never: nothing is stored for the row
        atomicOr(p.fault, kSampleFaultLocate);
        p.state[row] = make_uint4((kNoPick << 16) | best, 0u, 0u, 0u);
    }
}

// One workgroup per row: the picked chunk is read tile by tile up to the tile that holds the crossing; there the wave whose range
// holds the remainder stores the index and the logprob.  s_part: the waves' totals of a tile, two arrays taken in turn, so that one
// barrier per tile is enough -- a wave two tiles on writes only what every wave has read.
__global__ void __launch_bounds__(kLongThreads) sample16_locate_kernel(const LongParams p)
{
    __shared__ uint64_t s_part[2 * kLongWaves];
    const uint32_t row = blockIdx.x;
    if (row >= p.rows) return;
    const uint4 st = p.state[row];
    const uint32_t c = st.x >> 16;
    if (c >= p.chunks) return;   // (uniform) kNoPick: Z == 0, or a fault already raised
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const float best = value_of(st.x & 0xFFFFu, p.map, p.val);
    const float scale = row_scale(p.temperature, row);
    const uint64_t left = (uint64_t)st.z | ((uint64_t)st.w << 32);
    const RowKeys r = row_of(p.keys, row, p.cols);
    const ChunkRange g = chunk_of(r, p.chunk, c);
    uint64_t base = 0ull;   // the chunk's mass in front of the tile
    uint32_t turn = 0u;
    bool here = false;
    for (uint32_t tile = g.lo; tile < g.hi && !here; tile += kLongTile, turn ^= kLongWaves) {   // uniform
        const uint32_t q0 = tile + wave * kWaveTile;
        uint32_t t[kRegs];
        read_body(r, q0, g.hi, lane, p.map, t);
        const uint32_t h = (c == 0u && tile == 0u && wave == 0u) ? read_front(r, lane, p.map) : kAbsent;   // uniform
        Masses s;
        scan_masses(t, h, best, scale, q0 + 64u * kGroupKeys < g.hi, p.map, p.val, s);
        if (lane == 0u) s_part[turn + wave] = s.total;
        __syncthreads();
        uint64_t before = base, all = 0ull;
#pragma unroll
        for (uint32_t w = 0; w < kLongWaves; w++) {
            const uint64_t o = s_part[turn + w];
            before += w < wave ? o : 0ull;
            all += o;
        }
        here = base <= left && left - base < all;   // uniform over the workgroup
        if (here && before <= left && left - before < s.total &&
            !draw_in_wave(t, h, s, before, left, r.head + q0, lane, row, best, log_factor(scale), __uint_as_float(st.y), p.out, p.map, p.val) &&
            lane == 0u)
            atomicOr(p.fault, kSampleFaultLocate);
        base += all;
    }
    if (!here && tid == 0u) atomicOr(p.fault, kSampleFaultLocate);   // never: the chunk's sum was above the remainder
}

// Workspace: control | row states, 16 B per row | for rows above kLocalSortCap keys the chunk sums, 8 B per chunk.
struct SampleLayout {
    size_t state, sums, end;
};
SampleLayout sample_layout(size_t rows, size_t cols)
{
    SampleLayout L{};
    L.state = kCtlBytes;
    L.sums = align_up(L.state + rows * 16);
    L.end = align_up(L.sums + (cols > (size_t)kLocalSortCap ? rows * chunk_cap_for(cols) * 8 : 0));
    return L;
}

int run_sample(const uint16_t* keys, size_t rows, size_t cols, const float* d_u, const float* d_temperature, const Key16Map& map,
               const Values16& val, const DrawOut& out, char* ws, const SampleLayout& L, hipStream_t stream)
{
    uint32_t* const ctl = reinterpret_cast<uint32_t*>(ws);
    if (cols <= (size_t)kLocalSortCap) {
        const float* const unused = reinterpret_cast<const float*>(ws + L.state);
        const ShortParams sp{keys, d_u, d_temperature ? d_temperature : unused, d_temperature ? 1u : 0u, (uint32_t)cols, (uint32_t)rows, map, val, ctl, out};
        hipLaunchKernelGGL(sample16_clear_kernel, dim3(1), dim3(256), 0, stream, ctl, (uint4*)nullptr, 0u);
        if (cols <= (size_t)kWaveSegCap)
            hipLaunchKernelGGL(sample16_short_kernel<1>, dim3(grid_for(rows, 8, 16384)), dim3(512), 0, stream, sp);
        else
            hipLaunchKernelGGL(sample16_short_kernel<16>, dim3(grid_for(rows, 1, 4096)), dim3(1024), 0, stream, sp);
        LSD_HIP(hipGetLastError());
        return LSDSORT_OK;
    }
    const Chunks ch = chunks_for(rows, cols);
    LongParams lp{};
    lp.keys = keys;
    lp.u = d_u;
    lp.temperature = d_temperature;
    lp.cols = (uint32_t)cols;
    lp.rows = (uint32_t)rows;
    lp.chunk = ch.chunk;
    lp.chunks = ch.per_row;
    lp.state = reinterpret_cast<uint4*>(ws + L.state);
    lp.sums = reinterpret_cast<uint64_t*>(ws + L.sums);
    lp.map = map;
    lp.val = val;
    lp.fault = ctl;
    lp.out = out;
    if (lp.chunks > chunk_cap_for(cols)) return LSDSORT_ERR_INVALID_ARG;   // never: chunks are at least kMinChunk keys
    const uint32_t grid = (uint32_t)(rows * lp.chunks), row_grid = (uint32_t)rows;
    hipLaunchKernelGGL(sample16_clear_kernel, dim3(grid_for(rows, 256, 1024)), dim3(256), 0, stream, ctl, lp.state, (uint32_t)rows);
    hipLaunchKernelGGL(sample16_best_kernel, dim3(grid), dim3(kLongThreads), 0, stream, lp);
    hipLaunchKernelGGL(sample16_sum_kernel, dim3(grid), dim3(kLongThreads), 0, stream, lp);
    hipLaunchKernelGGL(sample16_pick_kernel, dim3(row_grid), dim3(64), 0, stream, lp);
    hipLaunchKernelGGL(sample16_locate_kernel, dim3(row_grid), dim3(kLongThreads), 0, stream, lp);
    LSD_HIP(hipGetLastError());
    return LSDSORT_OK;
}

}  // namespace
}  // namespace lsd

extern "C" {

size_t lsdsort_sample16_workspace_bytes(size_t rows, size_t cols)
{
    if (cols > LSDSORT_MAX_KEYS || !lsd::sizes_ok(rows, cols)) return 0;
    return lsd::sample_layout(rows, cols).end;
}

int lsdsort_sample16_ex_device(const void* d_keys, size_t rows, size_t cols, const float* d_u, const float* d_temperature, int key_type,
                               int32_t* d_index, float* d_logprob, void* d_workspace, size_t workspace_bytes, void* hip_stream)
{
    Key16Map map;
    Values16 val;
    LSD_TRY(float16_values(key_type, &map, &val));
    if (!lsd::sizes_ok(rows, cols)) return LSDSORT_ERR_TOO_LARGE;
    if (rows == 0 || cols == 0) return LSDSORT_OK;
    if (!d_keys || ((uintptr_t)d_keys & 1)) return LSDSORT_ERR_INVALID_ARG;
    if (!d_u || !d_index || (((uintptr_t)d_u | (uintptr_t)d_index) & 3)) return LSDSORT_ERR_INVALID_ARG;   // u's values are the device's to read
    if (((uintptr_t)d_logprob | (uintptr_t)d_temperature) & 3) return LSDSORT_ERR_INVALID_ARG;             // NULL: no logprob; T = 1
    const lsd::SampleLayout L = lsd::sample_layout(rows, cols);
    if (!lsd::workspace_ok(d_workspace, workspace_bytes, L.end)) return LSDSORT_ERR_WORKSPACE;
    int rank_method = 0;   // asked for the device set-up alone: nothing here ranks with the returning add
    LSD_TRY(lsd::device_rank_method(8, &rank_method));
    const lsd::DrawOut out{d_index, d_logprob, (uint32_t)rows};
    return lsd::run_sample(static_cast<const uint16_t*>(d_keys), rows, cols, d_u, d_temperature, map, val, out, static_cast<char*>(d_workspace),
                           L, static_cast<hipStream_t>(hip_stream));
}

int lsdsort_sample16_device(const void* d_keys, size_t rows, size_t cols, const float* d_u, int key_type, int32_t* d_index, float* d_logprob,
                            void* d_workspace, size_t workspace_bytes, void* hip_stream)
{
    return lsdsort_sample16_ex_device(d_keys, rows, cols, d_u, nullptr, key_type, d_index, d_logprob, d_workspace, workspace_bytes, hip_stream);
}

}  // extern "C"
