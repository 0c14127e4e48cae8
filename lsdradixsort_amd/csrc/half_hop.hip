// half_hop.hip -- the small kernels of the hybrid form's HALF variant: 24 B/key instead of 28.
//
// After pass B the array is sorted by the 16 bits below the key prefix, so those bits of a key follow from its position and the
// exact counts of the 2^16 groups of equal such bits.  Pass B then writes only the low 16 bits of every key (2 B/key, into a
// buffer of halves in the roomy workspace) and the local stage reads them and rebuilds the keys on its way into LDS.  The
// upfront read counts the 2^16 groups (its B16 form with the packed flush, hybrid.hip); here the groups are folded into the
// planner's 2^15 buckets, and, behind the planner, the device decides whether the variant runs.  Everything else is the hybrid
// form's own code: the half-writing pass is an instantiation of rank_scatter_kernel (rank_scatter_r8.hip), the half-reading
// local stage a uniform branch in local_sort_kernel<20, false, false> (local_sort.hip).
#include "lsd_device.hpp"
#include "lsd_kernels.hpp"
#include "hybrid_plan.hpp"

namespace lsd {

constexpr int kHalfFoldThreads = 256;

// Group g = the 16 bits below the prefix; bucket j = its upper 15: groups 2 j and 2 j + 1, whose counts arrive in the low and the
// high half of packed[j].  Inside a bucket the keys of group 2 j come first (the array is sorted by group), first[j] of them.
// (A group of 65536 keys or more has carried into its neighbour or out of the word: the counts then sum to less than n and the
// planner refuses the form, whatever this kernel made of them.)
__global__ void __launch_bounds__(kHalfFoldThreads) half_fold_kernel(const uint32_t* __restrict__ packed, uint32_t* __restrict__ bucket15,
                                                                     uint32_t* __restrict__ first)
{
    const uint32_t j = blockIdx.x * (uint32_t)kHalfFoldThreads + threadIdx.x;
    if (j >= (uint32_t)(kHalfGroups / 2)) return;
    const uint32_t two = packed[j];
    bucket15[j] = (two & 0xFFFFu) + (two >> 16);
    first[j] = two & 0xFFFFu;
}

hipError_t launch_half_fold(const uint32_t* packed, uint32_t* bucket15, uint32_t* first, hipStream_t stream)
{
    if (!packed || !bucket15 || !first) return hipErrorInvalidValue;
    hipLaunchKernelGGL(half_fold_kernel, dim3(kHalfGroups / 2 / kHalfFoldThreads), dim3(kHalfFoldThreads), 0, stream, packed, bucket15, first);
    return hipGetLastError();
}

// One thread.  The half-reading local stage is the 10240-key variant alone (no half-reading list kernel): any listed bucket
// sends the sort down the full-key path, which is then exactly the hybrid form as it was -- pass B's one launch and the local
// launch both look at words[kHalfWordOk]: the first then stores keys, the second reads them.  (kHalfWordPlan and the 2 in the full
// pass B's plan word are what the variant's own pass-B launch used to read; they are kept as the record of the decision.)
__device__ __forceinline__ void half_decide(const uint32_t* __restrict__ keys, uint32_t* __restrict__ words)
{
    const uint32_t ok = (words[kHybridWordOk] != 0u && words[kHybridWordLargeCount] == 0u) ? 1u : 0u;
    const uint32_t t = words[kHybridWordPrefix];   // 0 .. kHybridMaxPrefix, written by the planner
    words[kHalfWordOk] = ok;
    words[kHalfWordHigh] = (t != 0u && t < 32u) ? keys[0] & ~((1u << (32u - t)) - 1u) : 0u;
    words[kHalfWordPlan] = ok ? 0u : 2u;
    words[kHalfWordPlan + 1] = 1u;   // pass B reads what pass A wrote: the alternate buffer
    if (ok) words[kHybridWordPlan + 2] = 2u;   // the full pass B: "the other form runs"
}

__global__ void __launch_bounds__(64) half_decide_kernel(const uint32_t* __restrict__ keys, uint32_t* __restrict__ words)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    half_decide(keys, words);
}

hipError_t launch_half_decide(const uint32_t* keys, uint32_t* words, hipStream_t stream)
{
    if (!keys || !words) return hipErrorInvalidValue;
    hipLaunchKernelGGL(half_decide_kernel, dim3(1), dim3(64), 0, stream, keys, words);
    return hipGetLastError();
}

// The half variant's planning in ONE launch: fold, planner and decision (three launches of a few microseconds each, every one of
// them behind the one before it on the sort's stream).  One workgroup of 1024 threads: it writes bucket15[] and first[] as
// half_fold_kernel does; thread t then owns buckets [32 t, 32 t + 32), reads their 32 packed words and plans from the folded counts
// in its registers (hybrid_plan_body, the planner's own body); last, thread 0 -- which wrote the planner's words itself -- decides.
__global__ void __launch_bounds__(1024) half_plan_kernel(const uint32_t* __restrict__ packed, uint32_t* __restrict__ bucket15,
                                                         uint32_t* __restrict__ first, uint32_t n, uint32_t* __restrict__ bases,
                                                         uint32_t* __restrict__ fields_out, uint32_t* __restrict__ words,
                                                         uint32_t* __restrict__ large_list, uint32_t small_cap,
                                                         const uint32_t* __restrict__ keys)
{
    constexpr int PER = kHalfGroups / 2 / 1024;
    static_assert(PER == 32, "2^15 buckets over 1024 threads");
    // bucket15[] and first[] for the local stage and the tests, a vector of four per lane (coalesced: written from the planner's
    // own layout below -- 32 consecutive buckets a thread -- every store instruction of a wave touched 64 lines, +8 us) ...
    {
        const uint4* src = reinterpret_cast<const uint4*>(packed);
        uint4* const to_bucket = reinterpret_cast<uint4*>(bucket15);
        uint4* const to_first = reinterpret_cast<uint4*>(first);
#pragma unroll
        for (uint32_t j = threadIdx.x; j < (uint32_t)(kHalfGroups / 2 / 4); j += 1024u) {
            const uint4 two = src[j];
            const uint4 low = make_uint4(two.x & 0xFFFFu, two.y & 0xFFFFu, two.z & 0xFFFFu, two.w & 0xFFFFu);
            to_bucket[j] = make_uint4(low.x + (two.x >> 16), low.y + (two.y >> 16), low.z + (two.z >> 16), low.w + (two.w >> 16));
            to_first[j] = low;
        }
    }
    // ... and the planner's counts folded again from the packed words, in registers
    const size_t at = (size_t)threadIdx.x * PER;
    auto fold_counts = [&](uint32_t (&cnt)[PER]) {
        const uint4* src = reinterpret_cast<const uint4*>(packed + at);
#pragma unroll
        for (int j = 0; j < PER / 4; j++) {
            const uint4 two = src[j];
            cnt[4 * j] = (two.x & 0xFFFFu) + (two.x >> 16);
            cnt[4 * j + 1] = (two.y & 0xFFFFu) + (two.y >> 16);
            cnt[4 * j + 2] = (two.z & 0xFFFFu) + (two.z >> 16);
            cnt[4 * j + 3] = (two.w & 0xFFFFu) + (two.w >> 16);
        }
    };
    hybrid_plan_body<8, PER>(fold_counts, n, bases, fields_out, nullptr, words, large_list, small_cap);
    if (threadIdx.x == 0) half_decide(keys, words);
}

hipError_t launch_half_plan(const uint32_t* packed, uint32_t* bucket15, uint32_t* first, uint32_t n, uint32_t* bases, uint32_t* fields_out,
                            uint32_t* words, uint32_t* large_list, uint32_t small_cap, const uint32_t* keys, hipStream_t stream)
{
    if (!packed || !bucket15 || !first || !bases || !fields_out || !words || !large_list || !keys) return hipErrorInvalidValue;
    hipLaunchKernelGGL(half_plan_kernel, dim3(1), dim3(1024), 0, stream, packed, bucket15, first, n, bases, fields_out, words, large_list,
                       small_cap, keys);
    return hipGetLastError();
}

}  // namespace lsd
