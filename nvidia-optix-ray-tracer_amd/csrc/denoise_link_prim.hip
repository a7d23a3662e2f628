// denoise_link_prim.hip -- k_denoise_temporal_by_prim: the temporal mode's reprojection and blend (denoise_temporal_body.h) of the first
// call after hrt_denoise_temporal_rebind_geometry when the link carries instances whose BLAS was rebuilt (DESIGN.md section 3e "History
// across rebuilt BLASes"; tests/denoise_by_primitive_ref.py).  It is k_denoise_temporal_linked with one more table: per instance the
// vertices of the BLAS it had in the history's TLAS, or NULL.  Where there are vertices, the object-space point of a hit is the material
// point (primitive, u, v) of that BLAS -- three vertices and two barycentrics -- instead of X_inv(i) P; the rest of the step is shared.
// Per hit pixel one 8-byte gather next to the index, then three 12-byte loads of the triangle, requested with the ray's record and
// ahead of the arithmetic on them; rigid and barycentric positions are both formed and one is selected, since every frame that mixes
// shared and rebuilt BLASes has lanes of both kinds in a wave.  Kernels and a translation unit of their own, as denoise_link.hip's.
#include "denoise_temporal_body.h"

#pragma clang fp contract(off)

namespace hrt {

template <bool kMoments>
__global__ __launch_bounds__(256) void k_denoise_temporal_by_prim(DenoiseTemporalByPrimArgs args) {
    constexpr bool kLinked = true;
    constexpr bool kByPrim = true;
    const DenoiseTemporalArgs &a = args.t;
    const uint32_t *prev_index = args.prev_index;
    const float *const *prev_verts = args.prev_verts;
#include "denoise_temporal_body.inc"
}

// a.prev_index as launch_denoise_temporal_linked's; a.prev_verts: one entry per instance of the TLAS the frame was traced through, NULL
// or the 9-floats-per-triangle array of a BLAS with as many triangles as the instance's own (hrt_denoise_temporal_rebind_geometry
// checks the counts and keeps the BLASes alive)
void launch_denoise_temporal_by_prim(const DenoiseTemporalByPrimArgs &a, hipStream_t s) {
    const uint32_t n = a.t.width * a.t.height;
    if (!n) return;
    const dim3 grid((n + 255u) / 256u), block(256);
    if (a.t.moments) hipLaunchKernelGGL(k_denoise_temporal_by_prim<true>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(k_denoise_temporal_by_prim<false>, grid, block, 0, s, a);
}

}  // namespace hrt
