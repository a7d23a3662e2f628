// denoise.hip -- the denoiser that takes the OptiX denoiser's slot (denoiseOutput, src/Global/RendererImpl.cu:680-710; include/hrt.h):
//   k_denoise_rays    the primary ray of every pixel of a full frame, as k_generate makes it (Shader.cu:246-267)
//   k_denoise_guides  hit record -> HrtDenoiseGuide: normalised shading normal and albedo of the primary hit as IEEE halves, hit distance
//                     (the depth-1 AOV of Shader.cu:216-227 that quirk Q3 blanks in the reference); the traversal between the two is
//                     hrt_trace_rays' (hrt_api.cpp trace_records): the path kernel in the context's configuration
//   k_denoise_pass    one pass of the edge-avoiding a-trous wavelet filter (Dammertz et al. 2010): 5x5 B3-spline taps `step` pixels
//                     apart, weighted by colour, normal, albedo and depth distance to the centre pixel (<.., true>: the variance-guided
//                     mode's, whose colour edge stop is scaled by the local variance, which it filters along with the colour)
//   k_denoise_temporal the temporal mode's reprojection of every hit pixel into the previous frame and its blend with the history there
//                     (<true>: the variance-guided mode's, which carries the first two moments of the luminance through the same blend)
//   k_denoise_variance the variance-guided mode's per-pixel luminance variance, from the moments or, under a young history, from the 5x5 block
// The filter is defined with + - * / and max only, taps in row-major order, sums in float32, and compiled with -ffp-contract=off: its
// result is reproduced bit for bit by tests/denoise_ref.py (DESIGN.md "Denoiser").
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "device_types.h"
#include "trav_common.h"
#include "bvh8_geom.h"
#include "denoise_temporal_body.h"

#pragma clang fp contract(off)

namespace hrt {

namespace {
constexpr int kDenoiseTile = 16;          // 16 x 16 pixels per workgroup: a tap's 16 rows of 16 pixels are 4 cache lines of colour + 4 of guides

__device__ __forceinline__ uint32_t half_bits(float x) { return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)x); }     // RNE
__device__ __forceinline__ float half_value(uint32_t bits) { return (float)__builtin_bit_cast(_Float16, (uint16_t)bits); }
__device__ __forceinline__ bool guide_hit(float z) { return z > 0.0f && z < INFINITY; }
// (luminance(), the variance-guided mode's edge stop and moments: denoise_temporal_body.h)

// one HrtDenoiseGuide as 4 words: normal[0..2], albedo[0..2] (halves, little-endian), depth
struct Guide { V3 n, a; float z; };
__device__ __forceinline__ Guide guide_decode(const uint4 g) {
    Guide r;
    r.n = mk3(half_value(g.x & 0xffffu), half_value(g.x >> 16), half_value(g.y & 0xffffu));
    r.a = mk3(half_value(g.y >> 16), half_value(g.z & 0xffffu), half_value(g.z >> 16));
    r.z = __uint_as_float(g.w);
    return r;
}
}  // namespace

__global__ __launch_bounds__(256) void k_denoise_rays(DenoiseRayArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.width * a.height) return;
    const uint32_t iy = i / a.width, ix = i - iy * a.width;
    const V3 dir = primary_direction(ix, iy, a.width, a.height, a.U, a.V, a.W);
    RayRec r;
    r.o = make_float4(a.center[0], a.center[1], a.center[2], __uint_as_float(i));
    r.d = make_float4(dir.x, dir.y, dir.z, __uint_as_float(i));
    a.rays[i] = r;
}

__global__ __launch_bounds__(256) void k_denoise_guides(DenoiseGuideArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t inst = a.inst[i];
    uint4 g = make_uint4(0u, 0u, 0u, __float_as_uint(INFINITY));
    if (inst != kMissPrim) {
        const float4 h = a.tuvp[i];
        const RayRec r = a.rays[i];
        const V3 o = mk3(r.o.x, r.o.y, r.o.z), d = mk3(r.d.x, r.d.y, r.d.z);
        const HitGroup hg = a.hitgroups[inst];
        const bool sphere = a.inst_program[inst] < (uint32_t)kProgramTriangleRough;
        const V3 n = normalize3(hit_normal<true>(sphere, hg, hit_point(o, d, h.x), d, h.y, h.z, __float_as_uint(h.w)));   // Shader.cu:114, :224
        g.x = half_bits(n.x) | (half_bits(n.y) << 16);
        g.y = half_bits(n.z) | (half_bits(hg.albedo[0]) << 16);
        g.z = half_bits(hg.albedo[1]) | (half_bits(hg.albedo[2]) << 16);
        g.w = __float_as_uint(h.x);
    }
    a.guides[i] = g;
}

// out(p) = sum_q w(p,q) c(q) / sum_q w(p,q) over the 25 taps q = p + step * (dx, dy), dx, dy in -2..2, row-major (dy outer), where
//   w = ((h[dx] * h[dy]) * wn) / ((stop * (1 + |a_p - a_q|^2 k_albedo)) * (1 + ((z_p - z_q) / (sigma_depth step z_p))^2)),
//   stop = 1 + |c_p - c_q|^2 k_color,  wn = max(0, n_p . n_q) squared normal_squarings times;
//   taps outside the frame or on background are left out; background pixels and pixels without weight (sw = sum_q w = 0) keep their
//   colour; alpha is the centre's.  (The three edge stops share one division; the depth term's reciprocal is taken once per pixel.)
// A row's five taps are loaded together -- addresses clamped into the frame, the taps that do not count left out of the sums by a
// select -- so that ten loads are in flight instead of a dependent guide-then-colour pair per tap.
// kSquarings >= 0: normal_squarings fixed at compile time (the default's instantiation), -1: read from the arguments.
// kVariance (the variance-guided mode, var_src != NULL; tests/denoise_variance_ref.py): the same geometry, taps, normal, albedo and
// depth stops, exclusions and `sw > 0` rule; the colour stop is the luminance difference over the local variance,
//   stop = 1 + (dl dl) inv_v,  dl = l(c_q) - l(c_p),  inv_v = 1 / (k_luminance gv + variance_floor),
//   gv = (sum g var_q) / (sum g) over the 3x3 block of step 1 around p, the taps inside the frame that are hits,
//   g = {1/4, 1/2, 1/4} x {1/4, 1/2, 1/4}, row-major,
// and the variance goes through the filter as the variance of the weighted mean: var_out = (sum (w w) var_q) / (sw sw).  A pixel that
// keeps its colour keeps its variance.  The stop does not shrink with the pass: the variance does.
template <int kSquarings, bool kVariance>
__global__ __launch_bounds__(kDenoiseTile * kDenoiseTile) void k_denoise_pass(DenoisePassArgs a) {
    const int x = (int)(blockIdx.x * kDenoiseTile + threadIdx.x), y = (int)(blockIdx.y * kDenoiseTile + threadIdx.y);
    const int W = (int)a.width, H = (int)a.height, s = (int)a.step;
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * a.width + (size_t)x;
    const float4 cp = a.src[p];
    float vp = 0.0f;
    if constexpr (kVariance) vp = a.var_src[p];
    const Guide gp = guide_decode(a.guides[p]);
    if (!guide_hit(gp.z)) {
        a.dst[p] = cp;
        if constexpr (kVariance) a.var_dst[p] = vp;
        return;
    }
    const uint32_t squarings = kSquarings >= 0 ? (uint32_t)kSquarings : a.normal_squarings;
    const float inv_z = 1.0f / (a.sigma_depth_step * gp.z);
    float inv_v = 0.0f, lp = 0.0f;
    if constexpr (kVariance) {
        const float kG[3] = {0.25f, 0.5f, 0.25f};
        float sgv = 0.0f, sgw = 0.0f;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int qy = y + (j - 1);
            if (qy < 0 || qy >= H) continue;
            const size_t row = (size_t)qy * a.width;
            float vq[3], zq[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const int qx = min(max(x + (i - 1), 0), W - 1);
                vq[i] = a.var_src[row + (size_t)qx];
                zq[i] = __uint_as_float(a.guides[row + (size_t)qx].w);
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const int qx = x + (i - 1);
                const bool take = qx >= 0 && qx < W && guide_hit(zq[i]);
                const float g = kG[i] * kG[j];
                sgw = take ? sgw + g : sgw;
                sgv = take ? sgv + g * vq[i] : sgv;
            }
        }
        const float gv = sgv / sgw;
        inv_v = 1.0f / (a.k_luminance * gv + a.variance_floor);
        lp = luminance(cp);
    }
    const float kH[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const int qy = y + (j - 2) * s;
        if (qy < 0 || qy >= H) continue;
        const size_t row = (size_t)qy * a.width;
        uint4 graw[5]; float4 cq[5]; float vq[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const int qx = min(max(x + (i - 2) * s, 0), W - 1);
            graw[i] = a.guides[row + (size_t)qx];
            cq[i] = a.src[row + (size_t)qx];
            if constexpr (kVariance) vq[i] = a.var_src[row + (size_t)qx];
        }
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const int qx = x + (i - 2) * s;
            const Guide gq = guide_decode(graw[i]);
            const bool take = qx >= 0 && qx < W && guide_hit(gq.z);
            float dc2;                                        // the squared colour distance: of the luminances in the variance form
            if constexpr (kVariance) {
                const float dl = luminance(cq[i]) - lp;
                dc2 = dl * dl;
            } else {
                const float dr = cq[i].x - cp.x, dg = cq[i].y - cp.y, db = cq[i].z - cp.z;
                dc2 = dr * dr + dg * dg + db * db;
            }
            float wn = fmaxf(dot3(gp.n, gq.n), 0.0f);
            for (uint32_t k = 0; k < squarings; ++k) wn = wn * wn;
            const V3 da = sub3(gp.a, gq.a);
            const float da2 = len2_3(da);
            const float rz = (gp.z - gq.z) * inv_z;
            const float stop = 1.0f + dc2 * (kVariance ? inv_v : a.k_color);
            const float w = ((kH[i] * kH[j]) * wn) / ((stop * (1.0f + da2 * a.k_albedo)) * (1.0f + rz * rz));
            sw = take ? sw + w : sw;
            sr = take ? sr + w * cq[i].x : sr; sg = take ? sg + w * cq[i].y : sg; sb = take ? sb + w * cq[i].z : sb;
            if constexpr (kVariance) sv = take ? sv + (w * w) * vq[i] : sv;
        }
    }
    const bool filtered = sw > 0.0f;
    a.dst[p] = filtered ? make_float4(sr / sw, sg / sw, sb / sw, cp.w) : cp;
    if constexpr (kVariance) a.var_dst[p] = filtered ? sv / (sw * sw) : vp;
}

// The temporal mode's reprojection and blend, one thread per pixel: denoise_temporal_body.h has the definition and the code.  These are
// its unlinked instantiations; the linked one, for a history handed over from another TLAS, is denoise_link.hip's.
template <bool kMoments>
__global__ __launch_bounds__(256) void k_denoise_temporal(DenoiseTemporalArgs a) {
    constexpr bool kLinked = false;
    constexpr bool kByPrim = false;
    const uint32_t *prev_index = nullptr;
    const float *const *prev_verts = nullptr;
#include "denoise_temporal_body.inc"
}

// The variance-guided mode's variance of the luminance, one thread per pixel (DESIGN.md 3e "Variance-guided mode";
// tests/denoise_variance_ref.py).  Background: 0.  A hit pixel with L >= history_min: max(0, m2 - m1 m1).  Any other hit pixel (a young
// history): over the 5x5 block around it, row-major, the taps inside the frame that hold the centre's instance (the centre among
// them): n their count, s1 = sum m1_q, s2 = sum m2_q, mu = s1 / n, var = max(0, s2 / n - mu mu).  max(0, x) is fmaxf: NaN -> 0.
__global__ __launch_bounds__(256) void k_denoise_variance(DenoiseVarianceArgs a) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.width * a.height) return;
    const uint32_t inst = a.id[p].x;
    float var = 0.0f;
    if (inst != kMissPrim) {
        if (a.length[p] >= a.history_min) {                  // (a NaN length: the spatial estimate)
            const float2 m = a.moments[p];
            var = fmaxf(0.0f, m.y - m.x * m.x);
        } else {
            const int W = (int)a.width, H = (int)a.height;
            const int y = (int)(p / a.width), x = (int)(p - (uint32_t)y * a.width);
            float n = 0.0f, s1 = 0.0f, s2 = 0.0f;
            for (int j = -2; j <= 2; ++j) {
                const int qy = y + j;
                if (qy < 0 || qy >= H) continue;
#pragma unroll
                for (int i = -2; i <= 2; ++i) {
                    const int qx = x + i;
                    const size_t q = (size_t)qy * a.width + (size_t)min(max(qx, 0), W - 1);
                    const uint32_t qi = a.id[q].x;
                    const float2 m = a.moments[q];
                    const bool take = qx >= 0 && qx < W && qi == inst;
                    n = take ? n + 1.0f : n;
                    s1 = take ? s1 + m.x : s1;
                    s2 = take ? s2 + m.y : s2;
                }
            }
            const float mu = s1 / n;
            var = fmaxf(0.0f, s2 / n - mu * mu);
        }
    }
    a.variance[p] = var;
}

static inline uint32_t ceil_div_u(uint32_t a, uint32_t b) { return (a + b - 1u) / b; }

void launch_denoise_temporal(const DenoiseTemporalArgs &a, hipStream_t s) {
    const uint32_t n = a.width * a.height;
    if (!n) return;
    if (a.moments) hipLaunchKernelGGL(k_denoise_temporal<true>, dim3(ceil_div_u(n, 256)), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_denoise_temporal<false>, dim3(ceil_div_u(n, 256)), dim3(256), 0, s, a);
}
void launch_denoise_variance(const DenoiseVarianceArgs &a, hipStream_t s) {
    const uint32_t n = a.width * a.height;
    if (n) hipLaunchKernelGGL(k_denoise_variance, dim3(ceil_div_u(n, 256)), dim3(256), 0, s, a);
}

void launch_denoise_rays(const DenoiseRayArgs &a, hipStream_t s) {
    const uint32_t n = a.width * a.height;
    if (n) hipLaunchKernelGGL(k_denoise_rays, dim3(ceil_div_u(n, 256)), dim3(256), 0, s, a);
}
void launch_denoise_guides(const DenoiseGuideArgs &a, hipStream_t s) {
    if (a.n) hipLaunchKernelGGL(k_denoise_guides, dim3(ceil_div_u(a.n, 256)), dim3(256), 0, s, a);
}
void launch_denoise_pass(const DenoisePassArgs &a, hipStream_t s) {
    if (!a.width || !a.height) return;
    const dim3 grid(ceil_div_u(a.width, kDenoiseTile), ceil_div_u(a.height, kDenoiseTile)), block(kDenoiseTile, kDenoiseTile);
    const bool fixed = a.normal_squarings == 3u;                      // the default (HrtDenoiseParams)
    auto *kernel = a.var_src ? (fixed ? k_denoise_pass<3, true> : k_denoise_pass<-1, true>)
                             : (fixed ? k_denoise_pass<3, false> : k_denoise_pass<-1, false>);
    hipLaunchKernelGGL(kernel, grid, block, 0, s, a);
}

}  // namespace hrt
