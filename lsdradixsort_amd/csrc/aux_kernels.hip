// aux_kernels.hip -- one-thread and one-workgroup utilities of the multi-GPU and wide-key paths (sharded.hip, wide.hip).
#include "lsd_device.hpp"
#include "lsd_kernels.hpp"

namespace lsd {

__global__ void widen_counts_kernel(const uint32_t* __restrict__ in, uint64_t* __restrict__ out, int bins)
{
    const int i = threadIdx.x;
    if (i < bins) out[i] = in[i];
}

hipError_t launch_widen_counts(const uint32_t* hist32, uint64_t* counts64, int bins, hipStream_t stream)
{
    hipLaunchKernelGGL(widen_counts_kernel, dim3(1), dim3(256), 0, stream, hist32, counts64, bins);
    return hipGetLastError();
}

__global__ void keep_fault_kernel(uint32_t* sticky, const uint32_t* fault)
{
    if (*fault) *sticky |= *fault;
}

hipError_t launch_keep_fault(uint32_t* sticky, const uint32_t* fault, hipStream_t stream)
{
    hipLaunchKernelGGL(keep_fault_kernel, dim3(1), dim3(1), 0, stream, sticky, fault);
    return hipGetLastError();
}

// The opening clear of a sort, a partition or a caller's table: 16-byte stores, the grid walking the range.
constexpr int kClearThreads = 256;
constexpr uint32_t kClearMaxGrid = 2048;   // eight workgroups per CU: 8 MiB (a 2^28-key sort's counts and status rows) is 1 KiB a thread

__global__ void __launch_bounds__(kClearThreads) clear_kernel(uint4* __restrict__ quads, uint32_t count)
{
    for (uint32_t i = blockIdx.x * kClearThreads + threadIdx.x; i < count; i += gridDim.x * kClearThreads) quads[i] = make_uint4(0, 0, 0, 0);
}

// the same by single words, for a caller's array that is promised 4-byte alignment only
__global__ void __launch_bounds__(kClearThreads) clear_words_kernel(uint32_t* __restrict__ words, uint32_t count)
{
    for (uint32_t i = blockIdx.x * kClearThreads + threadIdx.x; i < count; i += gridDim.x * kClearThreads) words[i] = 0u;
}

hipError_t launch_clear(void* at, size_t bytes, hipStream_t stream)
{
    if (!at || ((uintptr_t)at & 3u) || (bytes & 3u) || bytes / 4 > 0xFFFFFFFFull) return hipErrorInvalidValue;
    if (bytes == 0) return hipSuccess;
    if ((((uintptr_t)at | bytes) & 15u) == 0) {
        const size_t quads = bytes / 16;
        const uint32_t grid = (uint32_t)((quads + kClearThreads - 1) / kClearThreads);
        hipLaunchKernelGGL(clear_kernel, dim3(grid < kClearMaxGrid ? grid : kClearMaxGrid), dim3(kClearThreads), 0, stream, static_cast<uint4*>(at),
                           (uint32_t)quads);
    } else {
        const size_t words = bytes / 4;
        const uint32_t grid = (uint32_t)((words + kClearThreads - 1) / kClearThreads);
        hipLaunchKernelGGL(clear_words_kernel, dim3(grid < kClearMaxGrid ? grid : kClearMaxGrid), dim3(kClearThreads), 0, stream,
                           static_cast<uint32_t*>(at), (uint32_t)words);
    }
    return hipGetLastError();
}

__global__ void store_u64_kernel(uint64_t* out, uint64_t value) { *out = value; }

hipError_t launch_store_u64(uint64_t* out, uint64_t value, hipStream_t stream)
{
    hipLaunchKernelGGL(store_u64_kernel, dim3(1), dim3(1), 0, stream, out, value);
    return hipGetLastError();
}

// A regular sample of a shard for the splitter choice (sharded.hip): out[0] = m = min(samples, n),
// out[1 + i] = keys[i * n / m] for i < m; the slots behind stay as they are.
__global__ void __launch_bounds__(256) sample_keys_kernel(const uint32_t* __restrict__ keys, uint32_t n, uint32_t samples,
                                                          uint32_t* __restrict__ out)
{
    const uint32_t m = n < samples ? n : samples;
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) out[0] = m;
    if (i < m) out[1 + i] = keys[(size_t)(((uint64_t)i * n) / m)];
}

hipError_t launch_sample_keys(const uint32_t* keys, uint32_t n, uint32_t samples, uint32_t* out, hipStream_t stream)
{
    if (samples == 0 || !out || (n && !keys)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sample_keys_kernel, dim3((samples + 255) / 256), dim3(256), 0, stream, keys, n, samples, out);
    return hipGetLastError();
}

}  // namespace lsd
