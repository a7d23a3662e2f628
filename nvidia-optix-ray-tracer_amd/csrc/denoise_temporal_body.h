// denoise_temporal_body.h -- the temporal mode's reprojection and blend as device code, for the translation units that make kernels of
// it: denoise.hip (k_denoise_temporal<kMoments>, the unlinked form), denoise_link.hip (k_denoise_temporal_linked<kMoments>: the first
// call after hrt_denoise_temporal_rebind, whose history was made for another TLAS of the same scene) and denoise_link_prim.hip
// (k_denoise_temporal_by_prim<kMoments>: ... after hrt_denoise_temporal_rebind_geometry, with rebuilt BLASes among the instances), as
// fused_body.h serves fused.hip and fused_capture.hip.  This header holds what stands at file scope; the statements are denoise_temporal_body.inc, which a kernel
// includes as its body with these names in scope:
//   a           const DenoiseTemporalArgs (or a reference to one)
//   kMoments    constexpr bool: the variance-guided mode's moments ride along
//   kLinked     constexpr bool: the history is another TLAS's; every use sits under `if constexpr`
//   prev_index  const uint32_t *: per instance of this frame's TLAS, its index in the history's (kNoInstance: none); read if kLinked only
//   kByPrim     constexpr bool: the link has instances whose BLAS was rebuilt (denoise_link_prim.hip); every use sits under `if constexpr`
//   prev_verts  const float *const *: per instance of this frame's TLAS, the vertices of its predecessor's BLAS or NULL; read if kByPrim only
// The statements stand in the kernels themselves rather than in a __device__ function the kernels call: through a function, by value or
// by reference, the unlinked kernels come out with commutative operands swapped in a few instructions, and they are to stay instruction
// for instruction what they were when the body stood in denoise.hip (profiles/r21_denoise_handoff.txt has the comparison).
//
// The definition (DESIGN.md 3e "Temporal mode"; tests/denoise_temporal_ref.py), one thread per pixel.  A hit pixel of instance i at
// distance t:
//   P = o + d t;  P' = X_prev(i) (X_inv(i) P)   (xf_point: ((m0 x + m1 y) + m2 z) + m3 per row)
//   r = P' - C';  s = dot(r, W') / dot(W', W')   (dot: (a.x b.x + a.y b.y) + a.z b.z);  no projection unless s > 0
//   ndcx = (dot(r, U') / dot(U', U')) / (s aspect),  ndcy = (dot(r, V') / dot(V', V')) / s,  aspect = width / height
//   x' = ((ndcx + 1) 0.5) width - 0.5,  y' = ((ndcy + 1) 0.5) height - 0.5,  z' = sqrt(dot(r, r))
// then the bilinear taps (x0, y0) (x0+1, y0) (x0, y0+1) (x0+1, y0+1), x0 = floor(x'), fx = x' - x0, weights (1-fx)(1-fy), fx(1-fy),
// (1-fx)fy, fx fy, each taken if it lies in the frame and holds the same (instance, primitive) at |z_prev - z'| <= tol z'.  With the sum
// of the taken weights sw > 0: H = (sum w A_prev) / sw, Lh = (sum w L_prev) / sw (sums in tap order), L = min(Lh + 1, max_history),
// alpha = max(1 / L, alpha_min), A = H + alpha (C - H) per colour channel, alpha the current pixel's; else A = C, L = 1.  Background:
// A = C, L = 0.  (x', y') goes to `motion` (NaN without a projection).  The four taps' ids and depths, which decide whether a tap counts,
// are loaded together from clamped addresses; A_prev, L_prev (and M_prev) are then read for the taps that count only.
// kMoments (the variance-guided mode): M = (m1, m2), the moments of the luminance l(C), go through the same taps, weights and alpha:
// with mc = (l(C), l(C) l(C)), M = Hm + alpha (mc - Hm), Hm = (sum w M_prev) / sw; without history M = mc; background M = (0, 0).
// kLinked (DESIGN.md 3e "History across TLAS handles"; tests/denoise_handoff_ref.py): pi = prev_index[i].  pi == kNoInstance: a body
// that was not there, so no history -- A = C, L = 1, M = mc, no motion.  Otherwise P' = X_prev(pi) (X_inv(i) P) and a tap counts if it
// holds (pi, primitive); everything else as above.  The id written for the next call is (i, primitive) in both forms.
// kByPrim (DESIGN.md 3e "History across rebuilt BLASes"; tests/denoise_by_primitive_ref.py): s = prev_verts[i], asked for next to
// prev_index[i].  s == NULL: the rigid path above.  Otherwise, with the hit's (u, v) and primitive k: a = s[9k .. 9k+2],
// b = s[9k+3 .. 9k+5], c = s[9k+6 .. 9k+8], w = (1 - u) - v, Po = (a w + b u) + c v per component (hit_normal's order, trav_common.h:
// u weighs the second vertex, v the third), P' = X_prev(pi) Po; X_inv(i) is not used.  Taps, id test (pi, k), depth test, blend and
// moments as above.  The triangle is loaded with the ray record, by every lane (a rigid lane's address is its own world -> object
// row), and Po is selected, not branched on.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "device_types.h"
#include "trav_common.h"
#include "bvh8_geom.h"

#pragma clang fp contract(off)

namespace hrt {
namespace {
// luminance of an sRGB-encoded colour (the variance-guided mode's edge stop and moments)
__device__ __forceinline__ float luminance(const float4 c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }
}  // namespace
}  // namespace hrt
