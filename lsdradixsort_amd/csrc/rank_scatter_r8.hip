// rank_scatter_r8.hip -- 8-bit-digit instantiations of the rank-and-scatter kernel
// (BASELINE.json configs[2] and configs[4]).  Shape ids index kShapesR8 in rank_scatter.hip.
#include "rank_scatter.hpp"

namespace lsd {

hipError_t launch_rank_scatter_r8(int shape_id, int rank_method, bool chained, const PassParams& p, hipStream_t stream)
{
    switch (shape_id) {
        case 0: return launch_rank_scatter_shape<8, 512, 32, 16384>(rank_method, chained, p, stream);   // keys default
        case 1: return launch_rank_scatter_shape<8, 1024, 16, 8192>(rank_method, chained, p, stream);
        case 2: return launch_rank_scatter_shape<8, 1024, 32, 16384>(rank_method, chained, p, stream);
        case 3: return launch_rank_scatter_shape<8, 512, 16, 8192>(rank_method, chained, p, stream);
        case 4: return launch_rank_scatter_shape<8, 1024, 32, 32768>(rank_method, chained, p, stream);  // key/value default
        case 5: return launch_rank_scatter_shape<8, 256, 16, 4096>(rank_method, chained, p, stream);
        default: return hipErrorInvalidValue;
    }
}

// Pass B of the hybrid form's half variant (lsd_kernels.hpp): shape 4 above, keys only, chained, returning-add rank, HALF.
static_assert(kHalfShapeR8 == 4, "the HALF instantiation is shape 4's: 1024 x 32, one LDS round of 32768 keys");
hipError_t launch_rank_scatter_half(const PassParams& p, hipStream_t stream)
{
    if (!p.half_out || !p.half_on || p.vals_in || p.xin.on || p.xout.on || !p.plan) return hipErrorInvalidValue;
    if (p.num_tiles == 0) return hipSuccess;
    return launch_rank_scatter_inst<8, 1024, 32, 32768, kRankLdsAdd, false, true, false, true>(p, stream);
}

}  // namespace lsd
