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

#pragma clang fp contract(off)

namespace hrt {

namespace {
constexpr int kDenoiseTile = 16;          // 16 x 16 pixels per workgroup: a tap's 16 rows of 16 pixels are 4 cache lines of colour + 4 of guides

__device__ __forceinline__ uint32_t half_bits(float x) { return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)x); }     // RNE
__device__ __forceinline__ float half_value(uint32_t bits) { return (float)__builtin_bit_cast(_Float16, (uint16_t)bits); }
__device__ __forceinline__ bool guide_hit(float z) { return z > 0.0f && z < INFINITY; }
// luminance of an sRGB-encoded colour (the variance-guided mode's edge stop and moments)
__device__ __forceinline__ float luminance(const float4 c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }

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

// The temporal mode's reprojection and blend (DESIGN.md 3e "Temporal mode"; tests/denoise_temporal_ref.py), one thread per pixel.  A hit
// pixel of instance i at distance t:
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
template <bool kMoments>
__global__ __launch_bounds__(256) void k_denoise_temporal(DenoiseTemporalArgs a) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.width * a.height) return;
    const float4 c = a.color[p];
    const uint32_t inst = a.inst[p];
    const float nan = __builtin_nanf("");
    float4 acc = c;
    float len = 0.0f;
    float2 mom = make_float2(0.0f, 0.0f);
    float2 mo = make_float2(nan, nan);
    uint2 id = make_uint2(kMissPrim, 0u);
    if (inst != kMissPrim) {
        const float4 h = a.tuvp[p];
        const uint32_t prim = __float_as_uint(h.w);
        id = make_uint2(inst, prim);
        len = 1.0f;
        float lc = 0.0f;
        if (kMoments) { lc = luminance(c); mom = make_float2(lc, lc * lc); }
        if (a.has_history) {
            const RayRec ray = a.rays[p];
            const float hp[3] = {ray.o.x + ray.d.x * h.x, ray.o.y + ray.d.y * h.x, ray.o.z + ray.d.z * h.x};      // hit_point
            float po[3], pw[3];
            xf_point(a.inst_inv + 12 * (size_t)inst, hp, po);
            xf_point(a.prev_xf + 12 * (size_t)inst, po, pw);
            const V3 r = mk3(pw[0] - a.prev_center[0], pw[1] - a.prev_center[1], pw[2] - a.prev_center[2]);
            const V3 U = mk3(a.prev_U[0], a.prev_U[1], a.prev_U[2]), V = mk3(a.prev_V[0], a.prev_V[1], a.prev_V[2]);
            const V3 W = mk3(a.prev_W[0], a.prev_W[1], a.prev_W[2]);
            const float s = dot3(r, W) / dot3(W, W);
            if (s > 0.0f) {
                const float fw = (float)a.width, fh = (float)a.height;
                const float aspect = fw / fh;
                const float ndcx = (dot3(r, U) / dot3(U, U)) / (s * aspect);
                const float ndcy = (dot3(r, V) / dot3(V, V)) / s;
                const float xp = ((ndcx + 1.0f) * 0.5f) * fw - 0.5f, yp = ((ndcy + 1.0f) * 0.5f) * fh - 0.5f;
                const float zp = sqrtf(dot3(r, r));
                mo = make_float2(xp, yp);
                const float x0 = floorf(xp), y0 = floorf(yp);
                const float fx = xp - x0, fy = yp - y0, gx = 1.0f - fx, gy = 1.0f - fy;
                const float w[4] = {gx * gy, fx * gy, gx * fy, fx * fy};
                size_t q[4]; bool in[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float qx = x0 + (float)(k & 1), qy = y0 + (float)(k >> 1);
                    in[k] = qx >= 0.0f && qx <= fw - 1.0f && qy >= 0.0f && qy <= fh - 1.0f;
                    const float cx = fminf(fmaxf(qx, 0.0f), fw - 1.0f), cy = fminf(fmaxf(qy, 0.0f), fh - 1.0f);      // (NaN -> 0)
                    q[k] = (size_t)(uint32_t)cy * a.width + (size_t)(uint32_t)cx;
                }
                uint2 qid[4]; float qz[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) { qid[k] = a.prev_id[q[k]]; qz[k] = __uint_as_float(a.prev_guides[q[k]].w); }
                float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sl = 0.0f, sm1 = 0.0f, sm2 = 0.0f;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const bool take = in[k] && qid[k].x == inst && qid[k].y == prim && fabsf(qz[k] - zp) <= a.depth_tolerance * zp;
                    if (take) {
                        const float4 ha = a.prev_accum[q[k]];
                        const float hl = a.prev_length[q[k]];
                        sw = sw + w[k];
                        sr = sr + w[k] * ha.x; sg = sg + w[k] * ha.y; sb = sb + w[k] * ha.z;
                        sl = sl + w[k] * hl;
                        if (kMoments) { const float2 hm = a.prev_moments[q[k]]; sm1 = sm1 + w[k] * hm.x; sm2 = sm2 + w[k] * hm.y; }
                    }
                }
                if (sw > 0.0f) {
                    const float hr = sr / sw, hg = sg / sw, hb = sb / sw;
                    len = fminf(sl / sw + 1.0f, a.max_history);
                    const float alpha = fmaxf(1.0f / len, a.alpha_min);
                    acc = make_float4(hr + alpha * (c.x - hr), hg + alpha * (c.y - hg), hb + alpha * (c.z - hb), c.w);
                    if (kMoments) { const float h1 = sm1 / sw, h2 = sm2 / sw; mom = make_float2(h1 + alpha * (mom.x - h1), h2 + alpha * (mom.y - h2)); }
                }
            }
        }
    }
    a.accum[p] = acc;
    a.length[p] = len;
    a.id[p] = id;
    a.motion[p] = mo;
    if (kMoments) a.moments[p] = mom;
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
