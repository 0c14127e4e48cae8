// scans.hip -- stage 2: offsets from the counts of stage 1.
//
// Stands in for the reference's offset construction (.cu:862-895: D2D copy, BlockPrefixSumKernel, two TransposeSMEMKernel
// launches, GPUPrefixSum + AddBlockSumsKernel).  The chained form: the exclusive scan of each digit histogram
// (scan_digit_counts_kernel) or every pass's region table and the pass plan (scan_regions_kernel, finish_plan_kernel); the
// staged form: local and global offset tables from the per-tile counts.  All of it is small next to stage 3.
#include "lsd_device.hpp"
#include "lsd_kernels.hpp"

namespace lsd {

// ------------------------------------------------------------------------------------------
// Stage 2 (onesweep): exclusive scan of each group's 2^R digit counts -- the inclusive scan
// of .cu:38-41 turned exclusive (PrefixSum, .cu:128-139).  One workgroup per group.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) scan_digit_counts_kernel(const uint32_t* __restrict__ hist,
                                                               uint32_t* __restrict__ base, int bins)
{
    __shared__ uint32_t s_wave[4];
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u, wave = tid >> 6;
    const uint32_t v = tid < (uint32_t)bins ? hist[blockIdx.x * bins + tid] : 0u;
    uint32_t incl = wave_inclusive_scan(v);
    if (lane == 63u) s_wave[wave] = incl;
    __syncthreads();
    for (uint32_t w = 0; w < wave; w++) incl += s_wave[w];
    if (tid < (uint32_t)bins) base[blockIdx.x * bins + tid] = incl - v;
}

hipError_t launch_scan_digit_counts(int radix_bits, int groups, const uint32_t* hist, uint32_t* base,
                                    hipStream_t stream)
{
    if (radix_bits < 1 || radix_bits > 8) return hipErrorInvalidValue;
    hipLaunchKernelGGL(scan_digit_counts_kernel, dim3(groups), dim3(256), 0, stream, hist, base, 1 << radix_bits);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// Stage 2 (onesweep): every pass's region table from the counts.  One workgroup per pass:
//   digit_base[d]      = exclusive scan over d of the digit totals          (.cu:38-41 / PrefixSum)
//   base[x][d]         = digit_base[d] + counts of digit d in regions before x
//   extents of pass p+1 = [digit_base[x*H/8], digit_base[(x+1)*H/8])   (regions = top bits of digit p)
//   extents of pass 0   = [x*R0, (x+1)*R0) clipped to n
// ------------------------------------------------------------------------------------------
template <int REG>
__global__ void __launch_bounds__(256) scan_regions_kernel(const uint32_t* __restrict__ counts, int bins, uint32_t n,
                                                          uint32_t tile_keys, uint32_t region0_keys, int passes,
                                                          uint32_t* __restrict__ tables, uint32_t table_words,
                                                          uint32_t* __restrict__ plan, uint32_t* __restrict__ fault,
                                                          const uint32_t* __restrict__ hybrid_ok, uint32_t skip_dead_passes)
{
    __shared__ uint32_t s_wave[4];
    __shared__ uint32_t s_base[257];
    __shared__ uint32_t s_const[kPlanWords];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const int pass = blockIdx.x;
    if (hybrid_ok && *hybrid_ok != 0u) {
        // uniform: the hybrid form runs.  The first launches serve either form: theirs are the hybrid form's pairs -- run; an odd pass
        // reads what the one before it wrote.  The other passes leave at once and touch nothing (2).
        if (plan && tid == 0) {
            const bool shared = pass < hybrid_global_passes(bins == 256 ? 8 : 4);
            plan[2 * pass] = shared ? 0u : 2u;
            plan[2 * pass + 1] = shared ? (uint32_t)(pass & 1) : 0u;
            if (pass + 1 == passes) plan[2 * passes] = 0u;   // the local stage leaves the keys in the caller's buffer
        }
        return;
    }
    // This kernel is latency, not work: a small sort spends 5 of its 50 us here (rocprofv3, 2^20 keys, round 3).  So every
    // global load it needs is requested up front, in one window: this pass's counts first ...
    const uint32_t* c = counts + (size_t)pass * bins * REG;
    uint32_t* table = tables + (size_t)pass * table_words;
    uint32_t per_region[REG];
    uint32_t total = 0;
    if (tid < (uint32_t)bins) {
#pragma unroll
        for (int x = 0; x < REG; x++) per_region[x] = c[tid * REG + x];
    }
    if (plan) {
        // ... then the pass plan (PassParams::plan): a digit that is the same for every key (one bin holds all n) makes its
        // pass the identity.  This workgroup looks at its own pass and at the ones before it, whose number of REAL passes says
        // which buffer its keys are in: (pass + 1) * bins (pass, digit) cells, dealt over the threads.
        if (tid < (uint32_t)kPlanWords) s_const[tid] = 0;
        __syncthreads();
        const uint32_t cells = (uint32_t)(pass + 1) * (uint32_t)bins;
#pragma unroll 4
        for (uint32_t cell = tid; cell < cells; cell += 256u) {
            uint32_t t = 0;
#pragma unroll
            for (int x = 0; x < REG; x++) t += counts[(size_t)cell * REG + x];
            if (t == n && skip_dead_passes) s_const[cell / (uint32_t)bins] = 1;
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t moved = 0;
            for (int q = 0; q < pass; q++) moved += s_const[q] ? 0u : 1u;
            plan[2 * pass] = s_const[pass];
            plan[2 * pass + 1] = moved & 1u;
            if (pass + 1 == passes) plan[2 * passes] = (moved + (s_const[pass] ? 0u : 1u)) & 1u;
        }
    }
    if (tid < (uint32_t)bins) {
#pragma unroll
        for (int x = 0; x < REG; x++) total += per_region[x];
    }
    uint32_t incl = wave_inclusive_scan(total);
    if (lane == 63u) s_wave[wave] = incl;
    __syncthreads();
    for (uint32_t w = 0; w < wave; w++) incl += s_wave[w];
    const uint32_t digit_base = incl - total;
    // Every key has exactly one digit: a pass's counts sum to n.  Counts that do not (a miscounting stage-1 variant:
    // DESIGN.md section 4.5.2) would give the pass bases and extents that do not describe its input; say so in the fault
    // word here, once, before any pass runs on them (the passes' destination guard keeps their stores in bounds).
    if (fault && tid == (uint32_t)bins - 1u && incl != n) atomicOr(fault, 4u);
    if (tid < (uint32_t)bins) {
        s_base[tid] = digit_base < n ? digit_base : n;   // extents below stay inside [0, n] whatever the counts say
        uint32_t run = digit_base;
#pragma unroll
        for (int x = 0; x < REG; x++) {
            table[kRegionHeaderWords + x * bins + tid] = run;
            run += per_region[x];
        }
    }
    if (tid == 0) s_base[bins] = n;
    __syncthreads();
    // Extents: lane x of the first wave owns region x; the regions' first status rows are an exclusive scan of their tile
    // counts across those lanes.
    if (wave == 0) {
        auto write_extents = [&](uint32_t* t, uint32_t lo, uint32_t hi) {
            lo = lo < n ? lo : n;
            hi = hi < n ? hi : n;
            const uint32_t len = hi > lo ? hi - lo : 0u;
            const uint32_t tiles = lane < (uint32_t)REG ? (len + tile_keys - 1) / tile_keys : 0u;
            const uint32_t upto = wave_inclusive_scan(tiles);
            if (lane < (uint32_t)REG) {
                t[lane] = lo;
                t[kMaxRegions + lane] = len;
                t[2 * kMaxRegions + lane] = tiles;
                t[3 * kMaxRegions + lane] = upto - tiles;
            } else if (lane < (uint32_t)kMaxRegions) {
                // a kernel compiled for more regions than this table has (the 4-bit kernels partitioning by one region for
                // the multi-GPU step) must find the others empty
                t[2 * kMaxRegions + lane] = 0;
            }
        };
        const uint32_t x = lane < (uint32_t)REG ? lane : 0u;
        if (pass == 0) {
            const unsigned long long e0 = (unsigned long long)x * region0_keys, e1 = e0 + region0_keys;
            if (REG == 1) write_extents(table, 0u, n);
            else write_extents(table, e0 < n ? (uint32_t)e0 : n, e1 < n ? (uint32_t)e1 : n);
        }
        if (pass + 1 < passes) {
            uint32_t* next = tables + (size_t)(pass + 1) * table_words;
            const int per = bins / REG;   // digits per region
            if (REG == 1) write_extents(next, 0u, n);
            else write_extents(next, s_base[x * per], s_base[(x + 1) * per]);
        }
    }
}

// The keys (and payloads) back into the caller's buffer when the plan left them in the other one.
__global__ void __launch_bounds__(1024) finish_plan_kernel(const uint32_t* __restrict__ plan_final, uint32_t* __restrict__ keys,
                                                           const uint32_t* __restrict__ alt_keys, uint32_t* __restrict__ vals,
                                                           const uint32_t* __restrict__ alt_vals, uint32_t n)
{
    if (*plan_final == 0) return;   // uniform: the usual case
    for (size_t i = (size_t)blockIdx.x * 1024 + threadIdx.x; i < n; i += (size_t)gridDim.x * 1024) {
        keys[i] = alt_keys[i];
        if (vals) vals[i] = alt_vals[i];
    }
}

hipError_t launch_finish_plan(const uint32_t* plan_final, uint32_t* keys, const uint32_t* alt_keys, uint32_t* vals,
                              const uint32_t* alt_vals, uint32_t n, hipStream_t stream)
{
    if (!plan_final || !keys || !alt_keys || (vals && !alt_vals)) return hipErrorInvalidValue;
    uint32_t blocks = (n + 4 * 1024 - 1) / (4 * 1024);
    if (blocks > 512) blocks = 512;   // two workgroups per CU copy at full rate; the usual launch returns at once
    if (blocks == 0) blocks = 1;
    hipLaunchKernelGGL(finish_plan_kernel, dim3(blocks), dim3(1024), 0, stream, plan_final, keys, alt_keys, vals, alt_vals, n);
    return hipGetLastError();
}

hipError_t launch_scan_regions(int radix_bits, int passes, int regions, const uint32_t* counts, uint32_t n,
                               uint32_t tile_keys, uint32_t region0_keys, uint32_t* tables, hipStream_t stream, uint32_t* plan,
                               uint32_t* fault, const uint32_t* hybrid_ok, bool skip_dead_passes)
{
    if (radix_bits < 1 || radix_bits > 8 || (regions != 1 && regions != regions_for_radix(radix_bits))) return hipErrorInvalidValue;
    const uint32_t sdp = skip_dead_passes ? 1u : 0u;
    if (plan && 2 * passes + 1 > kPlanWords) return hipErrorInvalidValue;
    const int bins = 1 << radix_bits;
    const uint32_t words = (uint32_t)region_table_words(radix_bits);
    if (regions == 1)
        hipLaunchKernelGGL((scan_regions_kernel<1>), dim3(passes), dim3(256), 0, stream, counts, bins, n, tile_keys,
                           region0_keys, passes, tables, words, plan, fault, hybrid_ok, sdp);
    else if (regions == 8)
        hipLaunchKernelGGL((scan_regions_kernel<8>), dim3(passes), dim3(256), 0, stream, counts, bins, n, tile_keys,
                           region0_keys, passes, tables, words, plan, fault, hybrid_ok, sdp);
    else   // 16
        hipLaunchKernelGGL((scan_regions_kernel<16>), dim3(passes), dim3(256), 0, stream, counts, bins, n, tile_keys,
                           region0_keys, passes, tables, words, plan, fault, hybrid_ok, sdp);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// Stage 2 (staged): offset tables from h[tile][digit].
//   local[t][d]  = exclusive scan over d within tile t                       (.cu:869)
//   global[t][d] = keys with digit < d anywhere + keys with digit d in tiles < t   (.cu:877-895)
// The reference reaches the second by transposing to digit-major and scanning flat; here the
// table stays block-major and the digit-major order is walked directly:
//   (1) column sums over strips of kStrip tiles        -> strip_sum[strip][d]
//   (2) one workgroup scans strip_sum in digit-major order (d outer, strip inner), exclusive
//   (3) each (strip, d) thread replays its strip from that base and writes global[t][d].
// Threads are laid out digit-fastest so every access to a [.][d] row is coalesced.
// ------------------------------------------------------------------------------------------
constexpr uint32_t kStrip = 64;

__global__ void __launch_bounds__(256) local_offsets_kernel(const uint32_t* __restrict__ hist,
                                                           uint32_t* __restrict__ local, uint32_t tiles, int bins_log2)
{
    // 256 / bins rows per workgroup; Hillis-Steele inside each row through LDS
    __shared__ uint32_t s[2][256];
    const uint32_t bins = 1u << bins_log2;
    const uint32_t rows_per_block = 256u >> bins_log2;
    const uint32_t tid = threadIdx.x;
    const uint32_t d = tid & (bins - 1);
    const uint32_t row = blockIdx.x * rows_per_block + (tid >> bins_log2);
    const bool live = row < tiles;
    const uint32_t v = live ? hist[(size_t)row * bins + d] : 0u;
    int cur = 0;
    s[0][tid] = v;
    __syncthreads();
    for (uint32_t off = 1; off < bins; off <<= 1) {
        uint32_t x = s[cur][tid];
        if (d >= off) x += s[cur][tid - off];
        s[cur ^ 1][tid] = x;
        cur ^= 1;
        __syncthreads();
    }
    if (live) local[(size_t)row * bins + d] = s[cur][tid] - v;
}

__global__ void __launch_bounds__(256) strip_sums_kernel(const uint32_t* __restrict__ hist,
                                                        uint32_t* __restrict__ strip_sum, uint32_t tiles,
                                                        uint32_t strips, int bins_log2)
{
    const uint32_t bins = 1u << bins_log2;
    const uint32_t gid = blockIdx.x * 256u + threadIdx.x;   // (strip, digit), digit fastest
    const uint32_t strip = gid >> bins_log2, d = gid & (bins - 1);
    if (strip >= strips) return;
    const uint32_t t0 = strip * kStrip;
    const uint32_t t1 = (tiles - t0 < kStrip) ? tiles : t0 + kStrip;
    uint32_t sum = 0;
    for (uint32_t t = t0; t < t1; t++) sum += hist[(size_t)t * bins + d];
    strip_sum[(size_t)strip * bins + d] = sum;
}

// One workgroup; walks bins*strips entries in digit-major order with a running carry.
__global__ void __launch_bounds__(1024) scan_strip_sums_kernel(uint32_t* __restrict__ strip_sum, uint32_t strips,
                                                              int bins_log2)
{
    __shared__ uint32_t s_wave[16];
    __shared__ uint32_t s_carry;
    const uint32_t bins = 1u << bins_log2;
    const uint32_t total = strips << bins_log2;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < total; base += 1024u) {
        const uint32_t e = base + tid;                 // digit-major linear index
        const uint32_t d = e / strips, strip = e - d * strips;
        const bool live = e < total;
        const uint32_t v = live ? strip_sum[(size_t)strip * bins + d] : 0u;
        uint32_t incl = wave_inclusive_scan(v);
        if (lane == 63u) s_wave[wave] = incl;
        __syncthreads();
        uint32_t carry = s_carry;
        for (uint32_t w = 0; w < wave; w++) carry += s_wave[w];
        incl += carry;
        if (live) strip_sum[(size_t)strip * bins + d] = incl - v;
        __syncthreads();
        if (tid == 1023u) s_carry = incl;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) global_offsets_kernel(const uint32_t* __restrict__ hist,
                                                            const uint32_t* __restrict__ strip_base,
                                                            uint32_t* __restrict__ global, uint32_t tiles,
                                                            uint32_t strips, int bins_log2)
{
    const uint32_t bins = 1u << bins_log2;
    const uint32_t gid = blockIdx.x * 256u + threadIdx.x;
    const uint32_t strip = gid >> bins_log2, d = gid & (bins - 1);
    if (strip >= strips) return;
    const uint32_t t0 = strip * kStrip;
    const uint32_t t1 = (tiles - t0 < kStrip) ? tiles : t0 + kStrip;
    uint32_t running = strip_base[(size_t)strip * bins + d];
    for (uint32_t t = t0; t < t1; t++) {
        const uint32_t c = hist[(size_t)t * bins + d];
        global[(size_t)t * bins + d] = running;
        running += c;
    }
}

size_t tile_offsets_scratch_words(size_t tiles, int radix_bits)
{
    const size_t strips = (tiles + kStrip - 1) / kStrip;
    return strips << radix_bits;
}

hipError_t launch_tile_offsets(int radix_bits, const uint32_t* hist, uint32_t* local, uint32_t* global,
                               uint32_t tiles, uint32_t* scratch, hipStream_t stream)
{
    if (radix_bits < 1 || radix_bits > 8) return hipErrorInvalidValue;
    if (tiles == 0) return hipSuccess;
    const uint32_t bins = 1u << radix_bits;
    if (global) {
        const uint32_t strips = (tiles + kStrip - 1) / kStrip;
        const uint32_t threads = strips * bins;
        const uint32_t blocks = (threads + 255u) / 256u;
        hipLaunchKernelGGL(strip_sums_kernel, dim3(blocks), dim3(256), 0, stream, hist, scratch, tiles, strips,
                           radix_bits);
        hipLaunchKernelGGL(scan_strip_sums_kernel, dim3(1), dim3(1024), 0, stream, scratch, strips, radix_bits);
        hipLaunchKernelGGL(global_offsets_kernel, dim3(blocks), dim3(256), 0, stream, hist, scratch, global, tiles,
                           strips, radix_bits);
    }
    if (local) {
        // after `global`: local may alias hist (in-place, like the reference's h[0,GH))
        const uint32_t rows_per_block = 256u >> radix_bits;
        const uint32_t blocks = (tiles + rows_per_block - 1) / rows_per_block;
        hipLaunchKernelGGL(local_offsets_kernel, dim3(blocks), dim3(256), 0, stream, hist, local, tiles, radix_bits);
    }
    return hipGetLastError();
}

}  // namespace lsd
