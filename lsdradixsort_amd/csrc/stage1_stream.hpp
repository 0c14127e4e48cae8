// stage1_stream.hpp -- what the two kernels that read the whole array before anything moves share
// (joint_histograms_kernel, histograms.hip; hybrid_histograms_kernel, hybrid.hip): the thresholds of their heavy-value paths and
// the rule for which chunks their pipelined loops take.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lsd {

// HEAVY values.  LDS atomics of one wave instruction that meet on one word are served a lane per clock
// (tools/ceiling/lds_atomic.hip: 63 clocks for a whole 16-lane group on one word against 7 for random words), so a value that a
// quarter, half or all of the keys carry -- zeros, a default value, constant or sorted input, dead digits -- would cost the
// upfront read several times its uniform-key time.  A value counts as heavy when kHeavyLanes of a wave's 64 first keys hold it;
// a second one next to it when kHeavySecondLanes do.  Its holders are then counted in scalar registers (a compare, a ballot and
// a population count: no LDS operation) and added once.  Every path counts every key exactly; the choice is speed only.
constexpr uint32_t kHeavyLanes = 16;
constexpr uint32_t kHeavySecondLanes = 8;

// The keys come in chunks of THREADS 16-byte vectors (stream_grid, lsd_kernels.hpp) and a workgroup takes them a GROUP of VPT
// chunks at a time.  The pipelined loop takes FULL groups only; the chunks past the last full group, the keys past the last
// chunk -- and every key when the base is not 16-byte aligned (vec_chunks == 0) -- go through the kernel's tail loop, which
// starts at key full_group_chunks * THREADS * 4.
template <int VPT>
__host__ __device__ constexpr uint32_t full_group_chunks(uint32_t vec_chunks)
{
    return vec_chunks / VPT * VPT;
}

}  // namespace lsd
