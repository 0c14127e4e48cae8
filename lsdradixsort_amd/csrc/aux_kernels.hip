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
