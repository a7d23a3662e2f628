// denoise_link.hip -- k_denoise_temporal_linked: the temporal mode's reprojection and blend (denoise_temporal_body.h) of the first call
// after hrt_denoise_temporal_rebind, whose history was made for another TLAS of the same scene (DESIGN.md section 3e "History across TLAS
// handles"; tests/denoise_handoff_ref.py).  Per hit pixel one more 4-byte gather than k_denoise_temporal: the index its instance had in
// the history's TLAS, which selects the previous object -> world transform and the id a history tap must hold.  Kernels and a
// translation unit of their own: k_denoise_temporal (denoise.hip), whose kernel count and registers the tests pin, does not know the table.
#include "denoise_temporal_body.h"

#pragma clang fp contract(off)

namespace hrt {

template <bool kMoments>
__global__ __launch_bounds__(256) void k_denoise_temporal_linked(DenoiseTemporalLinkedArgs args) {
    constexpr bool kLinked = true;
    constexpr bool kByPrim = false;
    const DenoiseTemporalArgs &a = args.t;
    const uint32_t *prev_index = args.prev_index;
    const float *const *prev_verts = nullptr;
#include "denoise_temporal_body.inc"
}

// a.prev_index: one entry per instance of the TLAS the frame was traced through, each below the instance count a.t.prev_xf was made
// for or kNoInstance (hrt_denoise_temporal_rebind checks them)
void launch_denoise_temporal_linked(const DenoiseTemporalLinkedArgs &a, hipStream_t s) {
    const uint32_t n = a.t.width * a.t.height;
    if (!n) return;
    const dim3 grid((n + 255u) / 256u), block(256);
    if (a.t.moments) hipLaunchKernelGGL(k_denoise_temporal_linked<true>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(k_denoise_temporal_linked<false>, grid, block, 0, s, a);
}

}  // namespace hrt
