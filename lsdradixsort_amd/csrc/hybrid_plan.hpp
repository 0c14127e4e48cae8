// hybrid_plan.hpp -- the body of the hybrid form's planner, shared by its two kernels: hybrid_plan_kernel (hybrid.hip), which reads
// the bucket counts from memory, and half_plan_kernel (half_hop.hip), which folds them from the half variant's packed group counts
// in its registers.  One workgroup of 1024 threads; thread t holds the counts of buckets [PER t, PER t + PER), which
// load_counts(cnt) fetches for it behind the body's first barrier (where hybrid_plan_kernel has always read them).
#pragma once
#include "lsd_device.hpp"
#include "lsd_kernels.hpp"

namespace lsd {

// From the bucket counts: the verdict (largest bucket <= kLocalSortCap and the counts sum to n), the buckets' bases (exclusive scan,
// 2^bucket_bits + 1 words), the plan words the other kernels read, and the global passes' (digit, region) count fields that the
// upfront read has not written itself:
//   8-bit digits: the second pass's field B -- region = top three bits of the first pass's digit, i.e. PER / 2 consecutive buckets
//                 per cell;
//   4-bit digits: all four ([pass][digit][region], region = the previous pass's digit): D (bits 28-31 by 24-27) and C (bits 24-27
//                 by 20-23) are sums of buckets, B (bits 20-23 by 16-19) and A (bits 16-19 by position region) sums of the joint
//                 field [position region][bits 16-23] of the upfront read.
template <int R, int PER, class LoadCounts>   // PER = consecutive buckets per thread: 64 / 32 / 16 for 2^16 / 2^15 / 2^14 buckets (a thread = the top ten bits)
__device__ __forceinline__ void hybrid_plan_body(const LoadCounts& load_counts, uint32_t n, uint32_t* __restrict__ bases,
                                                 uint32_t* __restrict__ fields_out, const uint32_t* __restrict__ joint,
                                                 uint32_t* __restrict__ words, uint32_t* __restrict__ large_list, uint32_t small_cap)
{
    __shared__ uint32_t s_wave[16], s_max[16], s_large, s_c[256], s_d[256];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (tid == 0) s_large = 0;
    if (R == 4 && tid < 256) s_c[tid] = s_d[tid] = 0;
    __syncthreads();
    uint32_t cnt[PER];
    load_counts(cnt);
    uint32_t sum = 0, mx = 0, half0 = 0;
    uint32_t quarter[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < (int)PER; j++) {
        if (j == (int)PER / 2) half0 = sum;
        sum += cnt[j];
        quarter[j / (PER / 4)] += cnt[j];
        mx = cnt[j] > mx ? cnt[j] : mx;
        // the launch over all buckets takes those of up to small_cap keys (the three-per-CU variant's capacity); the others
        // go on a list that a second, small launch walks with the large variant
        if (cnt[j] > small_cap) large_list[atomicAdd(&s_large, 1u)] = tid * PER + (uint32_t)j;
    }
    if (R == 8) {
        fields_out[2 * tid] = half0;             // cell (digit, region) = buckets [PER t, PER t + PER / 2): the layout of a pass's count table
        fields_out[2 * tid + 1] = sum - half0;
    } else {
        // tid = bits 22-31 of the key, a thread's quarter q = bits 20-21: cell D = [bits 28-31][bits 24-27] = tid >> 2,
        // cell C = [bits 24-27][bits 20-23] = (tid & 63) << 2 | q
        atomicAdd(&s_d[tid >> 2], sum);
#pragma unroll
        for (int q = 0; q < 4; q++) atomicAdd(&s_c[((tid & 63u) << 2) | (uint32_t)q], quarter[q]);
        if (tid < 256) {          // A[digit d4][region x] = sum over d5 of joint[x][d5 << 4 | d4]
            const uint32_t d4 = tid >> 4, x = tid & 15u;
            uint32_t a = 0;
#pragma unroll
            for (uint32_t d5 = 0; d5 < 16; d5++) a += joint[x * 256u + ((d5 << 4) | d4)];
            fields_out[tid] = a;
        } else if (tid < 512) {   // B[digit d5][region d4] = sum over x of joint[x][d5 << 4 | d4]: index = bits 16-23 as they are
            const uint32_t byte = tid - 256u;
            uint32_t b = 0;
#pragma unroll
            for (uint32_t x = 0; x < 16; x++) b += joint[x * 256u + byte];
            fields_out[256u + byte] = b;
        }
    }
    mx = wave_max(mx);
    if (lane == 0u) s_max[wave] = mx;
    uint32_t total = 0;
    uint32_t run = group_exclusive_scan<16>(sum, lane, wave, s_wave, &total);
    if (R == 4 && tid < 256) {
        fields_out[512u + tid] = s_c[tid];
        fields_out[768u + tid] = s_d[tid];
    }
    uint32_t largest = 0;
#pragma unroll
    for (int w = 0; w < 16; w++) largest = s_max[w] > largest ? s_max[w] : largest;
#pragma unroll
    for (int j = 0; j < (int)PER; j++) {
        bases[(size_t)tid * PER + j] = run;
        run += cnt[j];
    }
    if (tid == 0) {
        bases[1024 * PER] = n;
        const uint32_t ok = (largest <= (uint32_t)kLocalSortCap && total == n && words[kHybridWordViolated] == 0u) ? 1u : 0u;
        // what follows from the key prefix (the upfront read counted below it; if it did not run, nothing here is used)
        uint32_t prefix = hybrid_prefix_of(words[kHybridWordDiffer]);
        if (prefix > kHybridMaxPrefix) prefix = 0;
        words[kHybridWordPrefix] = prefix;
#pragma unroll
        for (int g = 0; g < 4; g++) words[kHybridWordShift + g] = 16u - prefix + (uint32_t)(g * R);
        // the pass launches that serve either form read their shift here: the hybrid form's, or the ordinary form's first digits
#pragma unroll
        for (int g = 0; g < 4; g++) words[kSlotWordShift + g] = (ok ? 16u - prefix : 0u) + (uint32_t)(g * R);
        words[kHybridWordLowBits] = 32u - prefix - (PER == 64 ? 16u : PER == 32 ? 15u : 14u);
        words[kHybridWordOk] = ok;            // the ordinary form's kernels return at once when this is set
        words[kHybridWordSkipLocal] = ok ^ 1u;
        words[kHybridWordLargeCount] = s_large;
#pragma unroll
        for (int g = 0; g < 4; g++) {          // PassParams::plan of the g-th global pass: skip?, roles swapped?
            words[kHybridWordPlan + 2 * g] = ok ^ 1u;
            words[kHybridWordPlan + 2 * g + 1] = (uint32_t)(g & 1);   // an odd pass reads what the one before it wrote
        }
        words[kHybridWordLargest] = largest;
    }
}

}  // namespace lsd
