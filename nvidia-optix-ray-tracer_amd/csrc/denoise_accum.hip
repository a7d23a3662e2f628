// denoise_accum.hip -- the denoiser's accumulated mode (include/hrt.h "Accumulated mode"; tests/denoise_accumulated_ref.py):
//   k_denoise_accumulated  what hrt_render_accumulate leaves with its caller -- per pixel the sum of the radiance, the sum of the squared
//                          luminances and the number of samples -- and the frame's guides -> the three frames the variance-guided filter
//                          (denoise.hip k_denoise_pass<.., true>) takes: the linear mean, the variance of that mean, and the guides with
//                          every pixel that holds no sample turned into background
// One thread per pixel, + - * / and fmaxf only, sums in float32 and in row-major order, compiled with -ffp-contract=off: reproduced bit for
// bit by the numpy specification.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "device_types.h"

#pragma clang fp contract(off)

namespace hrt {

namespace {
__device__ __forceinline__ bool guide_hit(float z) { return z > 0.0f && z < INFINITY; }
// luminance of a linear radiance (kernels.hip luminance_variance's)
__device__ __forceinline__ float luminance(float x, float y, float z) { return (0.2126f * x + 0.7152f * y) + 0.0722f * z; }
}  // namespace

// Per pixel p with n = taken[p] samples:
//   mean    n == 0: (0, 0, 0);  n == 1: sum.xyz;  else sum.xyz / (float)n   (k_finalize_counts' arithmetic), alpha 1
//   guides' guides[p], the depth +inf where n == 0: such a pixel is background to the filter -- never a tap, never filtered.
//           A hit below is 0 < depth' < +inf: a hit of the guides that holds a sample
//   var     the variance of the mean's luminance.  Background: 0.  A hit with n >= believed: fmaxf(0, m2 - m1 m1) / (float)n, m1 = l(sum.xyz) / n,
//           m2 = sum.w / n (hrt_sample_counts' estimator over n).  Any other hit (a young pixel): over the 5x5 block around it, row-major,
//           the taps inside the frame that are hits (the centre among them): k their count, s1 = sum l(mean_q), s2 = sum l(mean_q) l(mean_q),
//           mu = s1 / k, var = fmaxf(0, s2 / k - mu mu).  fmaxf drops a NaN operand.
// A young pixel's taps are made of the neighbours' sums, totals and depths as the caller gave them -- their means are computed again, not
// read from the frame other threads are writing -- so no thread waits for another.  A row's five taps are loaded together from
// addresses clamped into the frame, and the taps that do not count are left out of the sums by a select (as k_denoise_pass does).  The
// block sits behind a branch: a pixel with n >= believed, the common one, loads its own 36 B and nothing else.
__global__ __launch_bounds__(256) void k_denoise_accumulated(DenoiseAccumArgs a) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.width * a.height) return;
    const float4 sum = a.sum[p];
    const uint32_t n = a.taken[p];
    const uint4 g = a.guides[p];
    const float fn = (float)n;
    float mx = sum.x, my = sum.y, mz = sum.z;
    if (n > 1u) { mx /= fn; my /= fn; mz /= fn; }
    const float z = n == 0u ? INFINITY : __uint_as_float(g.w);
    float var = 0.0f;
    if (guide_hit(z)) {
        if (n >= a.believed) {
            const float m1 = luminance(sum.x, sum.y, sum.z) / fn, m2 = sum.w / fn;
            var = fmaxf(0.0f, m2 - m1 * m1) / fn;
        } else {
            const int W = (int)a.width, H = (int)a.height;
            const int y = (int)(p / a.width), x = (int)(p - (uint32_t)y * a.width);
            float k = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll
            for (int j = -2; j <= 2; ++j) {
                const int qy = y + j;
                if (qy < 0 || qy >= H) continue;
                const size_t row = (size_t)qy * a.width;
                float4 sq[5]; uint32_t nq[5]; float zq[5];
#pragma unroll
                for (int i = 0; i < 5; ++i) {
                    const size_t q = row + (size_t)min(max(x + (i - 2), 0), W - 1);
                    sq[i] = a.sum[q];
                    nq[i] = a.taken[q];
                    zq[i] = __uint_as_float(a.guides[q].w);
                }
#pragma unroll
                for (int i = 0; i < 5; ++i) {
                    const int qx = x + (i - 2);
                    const bool take = qx >= 0 && qx < W && nq[i] != 0u && guide_hit(zq[i]);
                    const float d = nq[i] > 1u ? (float)nq[i] : 1.0f;      // (x / 1 is x: one sample's mean is its sum)
                    const float l = luminance(sq[i].x / d, sq[i].y / d, sq[i].z / d);
                    k = take ? k + 1.0f : k;
                    s1 = take ? s1 + l : s1;
                    s2 = take ? s2 + l * l : s2;
                }
            }
            const float mu = s1 / k;
            var = fmaxf(0.0f, s2 / k - mu * mu);
        }
    }
    a.mean[p] = n == 0u ? make_float4(0.0f, 0.0f, 0.0f, 1.0f) : make_float4(mx, my, mz, 1.0f);
    a.variance[p] = var;
    a.guides_out[p] = make_uint4(g.x, g.y, g.z, __float_as_uint(z));
}

void launch_denoise_accumulated(const DenoiseAccumArgs &a, hipStream_t s) {
    const uint32_t n = a.width * a.height;
    if (n) hipLaunchKernelGGL(k_denoise_accumulated, dim3((n + 255u) / 256u), dim3(256), 0, s, a);
}

}  // namespace hrt
