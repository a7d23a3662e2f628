// blas_update.hip -- the device half of hrt_blas_update_triangles and hrt_blas_update_spheres (gfx950): the same primitives at new
// object-space positions.
//
// Replaces optixAccelBuild with OPTIX_BUILD_OPERATION_UPDATE on a triangle GAS.  ONE pass over the caller's vertices where the build makes
// two (a device-to-device copy, then k_blas_bounds over the copy): every triangle is stored into the BLAS's own copy and folded into the
// object-space bounds on the way -- by k_blas_bounds' rule, vertex by vertex (a vertex with a coordinate beyond 3e38 contributes nothing),
// so that an updated BLAS has bit for bit the bounds a BLAS built from the same vertices has.  Min and max are exact: the order of the
// reduction (thread, wave, workgroup, ordered-integer atomics) does not show in the result.
// HBM-bound: 36 B read + 36 B written per triangle.  A thread takes four triangles at a time, 144 B = nine 16-byte words; the first group
// starts where the DESTINATION is 16-byte aligned (`head` triangles in front of it go one by one, as does the tail), the loads are 16
// bytes wide too when the source is aligned there, single words otherwise -- neither pointer is promised more than a float's alignment.
//
// Spheres (k_blas_update_spheres) likewise: one pass over the caller's centres and radii where the build makes two (k_pack_spheres, then
// k_blas_bounds over the copy).  28 B read + 16 B written per sphere.  A thread takes four spheres at a time: 48 B of centres = three
// 16-byte words, 16 B of radii = one, four {cx, cy, cz, r} records = four 16-byte stores; either source array that is not 16-byte aligned
// is read in single words (chosen per array: four variants); the last up to three spheres go one by one.  The copy is hipMalloc's and a
// record is 16 B, so the destination has no head.  k_blas_bounds' sphere rule: rr = |r|, and a sphere whose centre or rr is beyond 3e38
// contributes nothing.
#include <algorithm>
#include "build_dev.h"

#pragma clang fp contract(off)

namespace hrt {
namespace {

constexpr uint32_t kGroupTriangles = 4, kGroupSpheres = 4, kUpdateMaxBlocks = 2048;

__device__ __forceinline__ void fold_vertices(const float *q, int n_vertices, float (&lo)[3], float (&hi)[3]) {
    for (int v = 0; v < n_vertices; ++v, q += 3)
        if (fabsf(q[0]) <= 3.0e38f && fabsf(q[1]) <= 3.0e38f && fabsf(q[2]) <= 3.0e38f)
            for (int d = 0; d < 3; ++d) { lo[d] = fminf(lo[d], q[d]); hi[d] = fmaxf(hi[d], q[d]); }
}

// one triangle, word by word
__device__ __forceinline__ void update_triangle(const float *src, float *dst, uint32_t k, float (&lo)[3], float (&hi)[3]) {
    float f[9];
    for (int q = 0; q < 9; ++q) f[q] = src[9 * (size_t)k + q];
    for (int q = 0; q < 9; ++q) dst[9 * (size_t)k + q] = f[q];
    fold_vertices(f, 3, lo, hi);
}

// n_tris triangles; head <= min(3, n_tris): dst + 9 * head is 16-byte aligned, and with kVecLoad so is src + 9 * head
template <bool kVecLoad>
__global__ __launch_bounds__(256) void k_blas_update_triangles(const float *__restrict__ src, float *__restrict__ dst, uint32_t n_tris, uint32_t head, BuildCounters *c) {
    const uint32_t tid = blockIdx.x * 256u + threadIdx.x, stride = gridDim.x * 256u;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (tid < head) update_triangle(src, dst, tid, lo, hi);
    const uint32_t n_groups = (n_tris - head + kGroupTriangles - 1u) / kGroupTriangles;
    for (uint32_t g = tid; g < n_groups; g += stride) {
        const uint32_t first = head + kGroupTriangles * g;
        if (first + kGroupTriangles <= n_tris) {
            float f[36];
            if (kVecLoad) {
                const float4 *p = reinterpret_cast<const float4 *>(src + 9 * (size_t)first);
                for (int j = 0; j < 9; ++j) { const float4 v = p[j]; f[4 * j] = v.x; f[4 * j + 1] = v.y; f[4 * j + 2] = v.z; f[4 * j + 3] = v.w; }
            } else {
                for (int q = 0; q < 36; ++q) f[q] = src[9 * (size_t)first + q];
            }
            float4 *o = reinterpret_cast<float4 *>(dst + 9 * (size_t)first);
            for (int j = 0; j < 9; ++j) o[j] = make_float4(f[4 * j], f[4 * j + 1], f[4 * j + 2], f[4 * j + 3]);
            fold_vertices(f, 12, lo, hi);
        } else {
            for (uint32_t k = first; k < n_tris; ++k) update_triangle(src, dst, k, lo, hi);      // (the tail: at most three)
        }
    }
    block_minmax<3>(lo, hi);
    if (threadIdx.x == 0u && lo[0] <= hi[0])
        for (int d = 0; d < 3; ++d) { atomicMin(&c->bmin[d], f2ord(lo[d])); atomicMax(&c->bmax[d], f2ord(hi[d])); }
}

// one sphere into its record (the radius verbatim, sign included: the traversal squares it) and into the box
__device__ __forceinline__ void update_sphere(float cx, float cy, float cz, float r, float *dst, size_t k, float (&lo)[3], float (&hi)[3]) {
    *reinterpret_cast<float4 *>(dst + 4 * k) = make_float4(cx, cy, cz, r);
    const float c[3] = {cx, cy, cz}, rr = fabsf(r);
    if (fabsf(cx) <= 3.0e38f && fabsf(cy) <= 3.0e38f && fabsf(cz) <= 3.0e38f && rr <= 3.0e38f)
        for (int d = 0; d < 3; ++d) { lo[d] = fminf(lo[d], c[d] - rr); hi[d] = fmaxf(hi[d], c[d] + rr); }
}

// n spheres; dst is 16-byte aligned; with kVecCenters so is `centers`, with kVecRadii so is `radii`
template <bool kVecCenters, bool kVecRadii>
__global__ __launch_bounds__(256) void k_blas_update_spheres(const float *__restrict__ centers, const float *__restrict__ radii, float *__restrict__ dst, uint32_t n, BuildCounters *c) {
    const uint32_t tid = blockIdx.x * 256u + threadIdx.x, stride = gridDim.x * 256u;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    const uint32_t n_groups = (n + kGroupSpheres - 1u) / kGroupSpheres;
    for (uint32_t g = tid; g < n_groups; g += stride) {
        const uint32_t first = kGroupSpheres * g;
        if (first + kGroupSpheres <= n) {
            float f[12], r[4];
            if (kVecCenters) {
                const float4 *p = reinterpret_cast<const float4 *>(centers + 3 * (size_t)first);
                for (int j = 0; j < 3; ++j) { const float4 v = p[j]; f[4 * j] = v.x; f[4 * j + 1] = v.y; f[4 * j + 2] = v.z; f[4 * j + 3] = v.w; }
            } else {
                for (int q = 0; q < 12; ++q) f[q] = centers[3 * (size_t)first + q];
            }
            if (kVecRadii) {
                const float4 v = *reinterpret_cast<const float4 *>(radii + first);
                r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w;
            } else {
                for (int q = 0; q < 4; ++q) r[q] = radii[first + q];
            }
            for (int j = 0; j < 4; ++j) update_sphere(f[3 * j], f[3 * j + 1], f[3 * j + 2], r[j], dst, (size_t)first + j, lo, hi);
        } else {
            for (uint32_t k = first; k < n; ++k)                                                   // (the tail: at most three)
                update_sphere(centers[3 * (size_t)k], centers[3 * (size_t)k + 1], centers[3 * (size_t)k + 2], radii[k], dst, k, lo, hi);
        }
    }
    block_minmax<3>(lo, hi);
    if (threadIdx.x == 0u && lo[0] <= hi[0])
        for (int d = 0; d < 3; ++d) { atomicMin(&c->bmin[d], f2ord(lo[d])); atomicMax(&c->bmax[d], f2ord(hi[d])); }
}

}  // namespace

// One pass that leaves bounds in the counters: they go to the device empty (the caller's scratch, or memory of its own), launch(c) runs over
// them, and lo[3] / hi[3] are what they hold afterwards -- as gpu_blas_bounds reads them (synchronises the stream).
template <class Launch>
static hipError_t update_bounds(float *lo, float *hi, void *d_scratch, hipStream_t s, Launch launch) {
    static_assert(sizeof(BuildCounters) <= kBoundsScratchBytes, "the counters are the only working memory");
    BuildCounters h{};
    for (int d = 0; d < 3; ++d) { h.bmin[d] = h.cmin[d] = 0xffffffffu; h.bmax[d] = h.cmax[d] = 0u; }
    BuildCounters *c = reinterpret_cast<BuildCounters *>(d_scratch);
    hipError_t e = c ? hipSuccess : hipMalloc((void **)&c, sizeof(BuildCounters));
    if (e != hipSuccess) return e;
    e = hipMemcpyAsync(c, &h, sizeof h, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) { launch(c); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipMemcpyAsync(&h, c, sizeof h, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (!d_scratch) (void)hipFree(c);
    if (e != hipSuccess) return e;
    if (h.bmin[0] <= h.bmax[0] && h.bmax[0] != 0u)
        for (int d = 0; d < 3; ++d) { lo[d] = ord2f(h.bmin[d]); hi[d] = ord2f(h.bmax[d]); }
    return hipSuccess;
}

// d_src's triangles into d_dst (n_prims of them, 9 floats each; the two do not overlap) and their object-space bounds into lo[3] / hi[3],
// as gpu_blas_bounds gives them for the same vertices (synchronises the stream for the counters).  d_scratch: kBoundsScratchBytes, or NULL.
hipError_t gpu_blas_update_triangles(const float *d_src, float *d_dst, uint32_t n_prims, float *lo, float *hi, void *d_scratch, hipStream_t s) {
    for (int d = 0; d < 3; ++d) { lo[d] = INFINITY; hi[d] = -INFINITY; }
    if (n_prims == 0) return hipSuccess;
    if ((reinterpret_cast<uintptr_t>(d_src) & 3u) || (reinterpret_cast<uintptr_t>(d_dst) & 3u)) return hipErrorInvalidValue;
    // triangle k of the copy begins 36 k bytes in: every fourth one on a 16-byte boundary
    const uint32_t head = std::min<uint32_t>((uint32_t)(((16u - (reinterpret_cast<uintptr_t>(d_dst) & 15u)) >> 2) & 3u), n_prims);
    const bool vec_load = (reinterpret_cast<uintptr_t>(d_src + 9 * (size_t)head) & 15u) == 0u;
    const uint32_t n_groups = (n_prims - head + kGroupTriangles - 1u) / kGroupTriangles;
    const uint32_t grid = std::min(std::max(blocks(std::max(n_groups, head), 256u), 1u), kUpdateMaxBlocks);
    return update_bounds(lo, hi, d_scratch, s, [&](BuildCounters *c) {
        if (vec_load) hipLaunchKernelGGL(k_blas_update_triangles<true>, dim3(grid), dim3(256), 0, s, d_src, d_dst, n_prims, head, c);
        else hipLaunchKernelGGL(k_blas_update_triangles<false>, dim3(grid), dim3(256), 0, s, d_src, d_dst, n_prims, head, c);
    });
}

// d_centers' and d_radii's spheres into d_dst as {cx, cy, cz, r} (n of them; d_dst overlaps neither and is 16-byte aligned, as hipMalloc
// gives it) and their object-space bounds into lo[3] / hi[3], as gpu_blas_bounds gives them for d_dst afterwards (synchronises the stream
// for the counters).  d_scratch: kBoundsScratchBytes, or NULL.
hipError_t gpu_blas_update_spheres(const float *d_centers, const float *d_radii, float *d_dst, uint32_t n, float *lo, float *hi, void *d_scratch, hipStream_t s) {
    for (int d = 0; d < 3; ++d) { lo[d] = INFINITY; hi[d] = -INFINITY; }
    if (n == 0) return hipSuccess;
    if ((reinterpret_cast<uintptr_t>(d_centers) & 3u) || (reinterpret_cast<uintptr_t>(d_radii) & 3u) || (reinterpret_cast<uintptr_t>(d_dst) & 15u)) return hipErrorInvalidValue;
    // group g's centres begin 48 g bytes in, its radii 16 g: each array is aligned for every group or for none
    const bool vec_c = (reinterpret_cast<uintptr_t>(d_centers) & 15u) == 0u, vec_r = (reinterpret_cast<uintptr_t>(d_radii) & 15u) == 0u;
    const uint32_t grid = std::min(std::max(blocks((n + kGroupSpheres - 1u) / kGroupSpheres, 256u), 1u), kUpdateMaxBlocks);
    return update_bounds(lo, hi, d_scratch, s, [&](BuildCounters *c) {
        if (vec_c && vec_r) hipLaunchKernelGGL((k_blas_update_spheres<true, true>), dim3(grid), dim3(256), 0, s, d_centers, d_radii, d_dst, n, c);
        else if (vec_c) hipLaunchKernelGGL((k_blas_update_spheres<true, false>), dim3(grid), dim3(256), 0, s, d_centers, d_radii, d_dst, n, c);
        else if (vec_r) hipLaunchKernelGGL((k_blas_update_spheres<false, true>), dim3(grid), dim3(256), 0, s, d_centers, d_radii, d_dst, n, c);
        else hipLaunchKernelGGL((k_blas_update_spheres<false, false>), dim3(grid), dim3(256), 0, s, d_centers, d_radii, d_dst, n, c);
    });
}

}  // namespace hrt
