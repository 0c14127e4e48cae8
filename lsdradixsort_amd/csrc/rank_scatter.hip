// rank_scatter.hip -- stage 3's host side: the tile-shape tables, the dispatch to the per-radix translation units that hold the
// instantiations of rank_scatter.hpp (rank_scatter_r8.hip / _r4.hip / _small.hip), and the device probe of the property the
// returning-LDS-add rank method relies on.
#include "lsd_device.hpp"
#include "lsd_kernels.hpp"

namespace lsd {

// ------------------------------------------------------------------------------------------
// Probe for kRankLdsAdd: does a returning LDS add, issued by the 64 lanes of one wave
// instruction onto colliding addresses, return its old values in lane order?  Each wave
// compares ds_add_rtn_u32 against the ballot-derived stable rank over collision patterns from
// "none" to "all 64 lanes on one word", with every CU busy.  Any disagreement clears *ok.
// ------------------------------------------------------------------------------------------
// Run in the occupancy shapes of the kernels that rely on the property: 1024-thread workgroups holding 128 KiB of LDS
// (one per CU, sixteen waves contending for the LDS pipe: the default 32768-key tile) and 512-thread workgroups
// holding 74 KiB (two per CU); the tables sit at the front of the dynamic allocation, the rest only claims the space.
__global__ void __launch_bounds__(1024) probe_lds_add_kernel(uint32_t iters, uint32_t* mismatches)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_probe_raw[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t waves = blockDim.x >> 6;
    volatile lds_u32* cnt = (volatile lds_u32*)s_probe_raw + wave * 256;
    volatile lds_u32* ref = (volatile lds_u32*)s_probe_raw + (waves + wave) * 256;
    for (uint32_t j = lane; j < 256; j += 64) {
        cnt[j] = 0;
        ref[j] = 0;
    }
    uint32_t bad = 0;
    for (uint32_t it = 0; it < iters; it++) {
        uint32_t h = (it * 0x9E3779B9u) ^ (blockIdx.x * 0x85EBCA6Bu) ^ (tid * 0xC2B2AE35u);
        h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16;
        uint32_t d;
        switch ((it + blockIdx.x) % 6u) {
            case 0: d = h & 0xFFu; break;
            case 1: d = h & 0x0Fu; break;
            case 2: d = h & 0x01u; break;
            case 3: d = 7u; break;
            case 4: d = (lane >> 2) & 0xFFu; break;
            default: d = (h & 0xFFu) * ((h >> 8) & 1u); break;
        }
        const uint64_t peers = match_ballot<8>(d);
        const uint32_t before = ref[d];
        const uint32_t expect = mbcnt_add(peers, before);
        const uint32_t old = __hip_atomic_fetch_add((lds_u32*)&cnt[d], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        if (old != expect) bad++;
        if (expect == before) ref[d] = popc64_add(peers, before);
    }
    if (bad) atomicAdd(mismatches, bad);
}

hipError_t probe_lds_add_lane_order(bool* ok, hipStream_t stream)
{
    *ok = false;
    uint32_t* d_bad = nullptr;
    hipError_t e = hipMalloc(&d_bad, sizeof(uint32_t));
    if (e != hipSuccess) return e;
    uint32_t h_bad = 1;
    e = hipMemsetAsync(d_bad, 0, sizeof(uint32_t), stream);
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(probe_lds_add_kernel),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(probe_lds_add_kernel, dim3(256 * 3), dim3(1024), 128 * 1024, stream, 600u, d_bad);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(probe_lds_add_kernel, dim3(256 * 3), dim3(512), 74 * 1024, stream, 600u, d_bad);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&h_bad, d_bad, sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    (void)hipFree(d_bad);
    if (e == hipSuccess) *ok = (h_bad == 0);
    return e;
}

// ------------------------------------------------------------------------------------------
// rank-and-scatter dispatch: per-radix translation units hold the instantiations.
// ------------------------------------------------------------------------------------------
hipError_t launch_rank_scatter_r8(int shape_id, int rank_method, bool chained, const PassParams& p, hipStream_t stream);
hipError_t launch_rank_scatter_r4(int shape_id, int rank_method, bool chained, const PassParams& p, hipStream_t stream);
hipError_t launch_rank_scatter_small(int radix_bits, int shape_id, int rank_method, bool chained, const PassParams& p, hipStream_t stream);

// Slot 0 is the default; the others stay compiled for tools/tune.py (DESIGN.md has the sweep).
static const TileShape kShapesR8[] = {{512, 32}, {1024, 16}, {1024, 32}, {512, 16}, {1024, 32}, {256, 16}};
static const TileShape kShapesR4[] = {{512, 32}, {512, 16}, {256, 16}, {1024, 32}, {1024, 32}, {1024, 16}};
static const TileShape kShapesSmall[] = {{256, 16}, {512, 32}, {1024, 32}};

bool single_round_shape(int radix_bits, int id)
{
    // the CAP arguments of rank_scatter_r8.hip / _r4.hip / _small.hip: r8 shapes 1 (1024 x 16, CAP 8192) and 2 (1024 x 32,
    // CAP 16384) and r4 shape 3 (1024 x 32, CAP 16384) reorder in two rounds
    if (radix_bits == 8) return id != 1 && id != 2;
    if (radix_bits == 4) return id != 3;
    return true;
}

int tile_shapes(int radix_bits, const TileShape** out)
{
    switch (radix_bits) {
        case 8: *out = kShapesR8; return (int)(sizeof(kShapesR8) / sizeof(TileShape));
        case 4: *out = kShapesR4; return (int)(sizeof(kShapesR4) / sizeof(TileShape));
        case 1: case 2: case 3: *out = kShapesSmall; return (int)(sizeof(kShapesSmall) / sizeof(TileShape));
        default: *out = nullptr; return 0;
    }
}

hipError_t launch_rank_scatter(int radix_bits, const TileShape& shape, int rank_method, bool chained,
                               const PassParams& p, hipStream_t stream)
{
    const TileShape* shapes = nullptr;
    const int count = tile_shapes(radix_bits, &shapes);
    const int id = (int)(&shape - shapes);   // shapes are identified by their table slot
    if (id < 0 || id >= count) return hipErrorInvalidValue;
    if (p.num_tiles == 0) return hipSuccess;
    switch (radix_bits) {
        case 8: return launch_rank_scatter_r8(id, rank_method, chained, p, stream);
        case 4: return launch_rank_scatter_r4(id, rank_method, chained, p, stream);
        default: return launch_rank_scatter_small(radix_bits, id, rank_method, chained, p, stream);
    }
}

}  // namespace lsd
