// half_hop.hip -- the two small kernels of the hybrid form's HALF variant: 24 B/key instead of 28.
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
// sends the sort down the full-key path, which is then exactly the hybrid form as it was -- the half-writing pass is told "2"
// and touches nothing, and the local launch, which looks at words[kHalfWordOk], reads keys.
__global__ void __launch_bounds__(64) half_decide_kernel(const uint32_t* __restrict__ keys, uint32_t* __restrict__ words)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const uint32_t ok = (words[kHybridWordOk] != 0u && words[kHybridWordLargeCount] == 0u) ? 1u : 0u;
    const uint32_t t = words[kHybridWordPrefix];   // 0 .. kHybridMaxPrefix, written by the planner
    words[kHalfWordOk] = ok;
    words[kHalfWordHigh] = (t != 0u && t < 32u) ? keys[0] & ~((1u << (32u - t)) - 1u) : 0u;
    words[kHalfWordPlan] = ok ? 0u : 2u;
    words[kHalfWordPlan + 1] = 1u;   // pass B reads what pass A wrote: the alternate buffer
    if (ok) words[kHybridWordPlan + 2] = 2u;   // the full pass B: "the other form runs"
}

hipError_t launch_half_decide(const uint32_t* keys, uint32_t* words, hipStream_t stream)
{
    if (!keys || !words) return hipErrorInvalidValue;
    hipLaunchKernelGGL(half_decide_kernel, dim3(1), dim3(64), 0, stream, keys, words);
    return hipGetLastError();
}

}  // namespace lsd
