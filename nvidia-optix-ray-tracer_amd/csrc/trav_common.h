// trav_common.h -- device code shared by the kernels of kernels.hip (wavefront pipeline, counting build, round-1 fused
// kernel), fused.hip and fused_queue.hip (the production path kernel and its queue form): vector helpers, XORWOW, the shading arithmetic of shader/Shader.cu,
// the wave's slice fetch, the ray queues' feed (queue_*), the start of a ray in a TravState (trav_start), the canonical primitive
// test, the node step (node_slab_test), the load / wait primitives of the traversal step and the instrumented build's LaneStats.
// One definition each, hence one rounding behaviour everywhere.  Device-only: include from .hip files compiled with -ffp-contract=off.
// (The regeneration phase of the two path kernels: path_lane.h; the loop of k_fused / k_trace_queue: trav_loop.h over trav_lean.h.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "device_types.h"

#pragma clang fp contract(off)

namespace hrt {

// ---- what a path kernel IS, as one type: the shared device code (here, path_lane.h, trav_loop.h, fused_body.h) is compiled once per kernel, and
//      every function of it that depends on the kernel takes that kernel's variant V and reads V::kBlocks, V::kOneGroup, ... where it is explained
//      what the flag means.  Each translation unit names the variant of its kernel and sets only what the kernel is. ----
struct PathVariant {      // every flag false
    static constexpr bool kSpheres = false, kInstanced = false;     // the tree: spheres as well as triangles; two levels (fused_body.h: InstLane)
    static constexpr bool kReuse = false, kSeed = false;            // repeat primary rays: not traversed (the primary-hit cache); bounded at their known hit (fused_body.h)
    static constexpr bool kBlocks = false, kCapture = false;        // pixels go round in sample blocks; every pixel's primary hit is kept (path_lane.h)
    static constexpr bool kOneGroup = false, kRestart = false;      // every hit is instance 0's; ... and repeat primary rays start at their known hit's node (path_lane.h)
    static constexpr bool kCounts = false;                          // every pixel takes a sample count of its own and continues a caller's sum (path_lane.h)
    static constexpr bool kMaskIdle = false;                        // the loop's primitive test and node step run with the lanes that have none switched off (trav_loop.h)
    static constexpr bool kDirect = false;                          // repeat primary rays test their known hit's record in the regeneration and never enter the loop (fused_body.h)
};
// a kernel that is none of these -- k_traverse (kernels.hip), k_trace_queue (fused_queue.hip): no pixels of its own or no seed, every block in its plain form
template <bool HAS_SPHERES>
struct PlainVariant : PathVariant { static constexpr bool kSpheres = HAS_SPHERES; };
// the persistent kernel (fused_body.h) seeds, unless it does not traverse a pixel's repeat primary rays at all
template <bool REUSE>
struct FusedBodyVariant : PathVariant { static constexpr bool kReuse = REUSE, kSeed = !REUSE; };
// The constraints between the flags, in one place: fused_body asserts this of its variant, once.
template <class V>
constexpr bool path_variant_checked() {
    static_assert(!V::kSeed || !V::kReuse, "the seed bounds the walk of a repeat primary ray, which the primary-hit cache does not traverse");
    static_assert(!V::kRestart || (V::kOneGroup && V::kSeed), "the restart: the one-group block render (the record rides in binst, which it leaves free), whose repeat primary rays have a window");
    static_assert(!V::kOneGroup || (V::kBlocks && !V::kSpheres && !V::kCapture), "one hit group: the block render of a one-level tree of triangles");
    static_assert(!V::kCapture || (!V::kReuse && !V::kBlocks), "the capture: plain launches only (no primary-hit cache, no sample blocks)");
    static_assert(!V::kBlocks || (!V::kInstanced && !V::kReuse), "sample blocks: one-level trees, no primary-hit cache (which wants a pixel's samples in one lane)");
    static_assert(!V::kCounts || (!V::kReuse && !V::kBlocks && !V::kCapture), "per-pixel counts: plain launches only (no primary-hit cache, no sample blocks, no capture)");
    static_assert(!V::kMaskIdle || (!V::kInstanced && !V::kSpheres), "idle lanes off: the loop copy whose primitive test and node step are straight-line arithmetic for the whole wave (one level, triangles)");
    static_assert(!V::kDirect || (V::kRestart && V::kOneGroup && V::kBlocks && V::kSeed), "the record tested where the ray is made: the record rides in binst (kRestart), the seed is the test's bound, and the regeneration is the one-group block render's");
    return true;
}

// ---------------------------------------------------------------------------------------
// small helpers
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t lane_prefix(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}
__device__ __forceinline__ uint32_t wave_first_u32(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// The wave's next slice [wbeg, wend) of `n` items (pixels, rays): slices of `fetch_chunk` items are handed out by kFetchShards
// counters on a line of their own each (chunk c of shard s is the (c * kFetchShards + s)-th slice handed out), and slice_of maps that
// number to the slice it stands for.  A wave starts at its home shard and goes round the others once that is drained; shards found
// drained are skipped for good (kstart).  Leaves wbeg >= wend when nothing is left.  Wave-uniform; lane 0 asks.
template <class SliceOf>
__device__ __forceinline__ void wave_next_slice(uint32_t &wbeg, uint32_t &wend, uint32_t &kstart, uint32_t home_shard, uint32_t *counters, uint32_t fetch_chunk,
                                                uint32_t n, uint32_t tx, SliceOf slice_of) {
    for (uint32_t k = kstart; k < kFetchShards && wbeg >= wend; ++k) {
        const uint32_t shard = (home_shard + k) & (kFetchShards - 1);
        uint32_t c = 0;
        if (tx == 0u) c = atomicAdd(counters + shard * kFetchShardStride, 1u);
        c = (uint32_t)__shfl((int)c, 0);
        const uint64_t q = (uint64_t)c * kFetchShards + shard;
        if (q * (uint64_t)fetch_chunk < (uint64_t)n) {
            const uint64_t beg = slice_of(q) * (uint64_t)fetch_chunk;
            wbeg = (uint32_t)beg;
            wend = (uint32_t)(beg + fetch_chunk < (uint64_t)n ? beg + fetch_chunk : (uint64_t)n);
        } else kstart = k + 1;
    }
}

// Ray queues (k_trace_queue, k_traverse's queue form): up to two segments per launch (e.g. the depth-4 rays of sample s and the primary
// rays of sample s + 1), their lengths read from device memory so that a render is a fixed sequence of launches.  Position q of the
// concatenated queue is ray q of segment 0 while q < n_a, else ray q - n_a of segment 1.
//   n_a = queue_length(a.seg[0]), n_b = a.seg[1].rays ? queue_length(a.seg[1]) : 0
__device__ __forceinline__ uint32_t queue_length(const TraverseSeg &g) { return g.n_ptr ? (g.n_ptr[0] + g.n_ptr[1] + g.n_ptr[2] + g.n_ptr[3]) : g.n; }
struct QueuePos { bool in_b; uint32_t k; };        // segment 1? / index within the segment
__device__ __forceinline__ QueuePos queue_pos(uint32_t q, uint32_t n_a) { QueuePos p; p.in_b = q >= n_a; p.k = p.in_b ? q - n_a : q; return p; }
__device__ __forceinline__ RayRec queue_ray(const TraverseArgs &a, QueuePos p) { return p.in_b ? a.seg[1].rays[p.k] : a.seg[0].rays[p.k]; }
__device__ __forceinline__ bool queue_any_hit(const TraverseArgs &a, QueuePos p) { return (p.in_b ? a.seg[1].any_hit : a.seg[0].any_hit) != 0u; }
__device__ __forceinline__ void queue_write_hit(const TraverseArgs &a, QueuePos p, float t, float u, float v, uint32_t prim, uint32_t inst) {
    (p.in_b ? a.seg[1].hit_tuvp : a.seg[0].hit_tuvp)[p.k] = make_float4(t, u, v, __uint_as_float(prim));
    (p.in_b ? a.seg[1].hit_inst : a.seg[0].hit_inst)[p.k] = inst;
}

struct V3 { float x, y, z; };
__device__ __forceinline__ V3 mk3(float x, float y, float z) { V3 r; r.x = x; r.y = y; r.z = z; return r; }
__device__ __forceinline__ V3 add3(V3 a, V3 b) { return mk3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ V3 sub3(V3 a, V3 b) { return mk3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ V3 muls3(V3 a, float s) { return mk3(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ V3 divs3(V3 a, float s) { return mk3(a.x / s, a.y / s, a.z / s); }
__device__ __forceinline__ V3 neg3(V3 a) { return mk3(-a.x, -a.y, -a.z); }
__device__ __forceinline__ float dot3(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ float len2_3(V3 a) { return a.x * a.x + a.y * a.y + a.z * a.z; }
__device__ __forceinline__ V3 cross3(V3 a, V3 b) {
    return mk3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
// normalize(), include/Global/DeviceFunctions.cuh:397-404; rsqrtf pinned as 1/sqrtf
__device__ __forceinline__ V3 normalize3(V3 a) {
    const float len2 = len2_3(a);
    if (len2 <= kFloatZero * kFloatZero) return mk3(0.0f, 0.0f, 1.0f);
    const float invLen = 1.0f / sqrtf(len2);
    return muls3(a, invLen);
}
__device__ __forceinline__ bool finite3(V3 a) { return isfinite(a.x) && isfinite(a.y) && isfinite(a.z); }

// ---------------------------------------------------------------------------------------
// XORWOW (cuRAND curandStateXORWOW_t)
// ---------------------------------------------------------------------------------------
struct Xorwow { uint32_t d, v0, v1, v2, v3, v4; };

__device__ __forceinline__ uint32_t xorwow_next(Xorwow &s) {
    const uint32_t t = s.v0 ^ (s.v0 >> 2);
    s.v0 = s.v1; s.v1 = s.v2; s.v2 = s.v3; s.v3 = s.v4;
    s.v4 = (s.v4 ^ (s.v4 << 4)) ^ (t ^ (t << 1));
    s.d += 362437u;
    return s.v4 + s.d;
}
// curand_uniform: (0, 1]
__device__ __forceinline__ float xorwow_uniform(Xorwow &s) {
    return (float)xorwow_next(s) * 2.3283064e-10f + (2.3283064e-10f / 2.0f);
}
__device__ __forceinline__ Xorwow rng_load(const RngState *st) {
    const uint2 *p = reinterpret_cast<const uint2 *>(st);
    const uint2 a = p[0], b = p[1], c = p[2];
    Xorwow s; s.d = a.x; s.v0 = a.y; s.v1 = b.x; s.v2 = b.y; s.v3 = c.x; s.v4 = c.y;
    return s;
}
__device__ __forceinline__ void rng_store(RngState *st, const Xorwow &s) {
    uint2 *p = reinterpret_cast<uint2 *>(st);
    p[0] = make_uint2(s.d, s.v0); p[1] = make_uint2(s.v1, s.v2); p[2] = make_uint2(s.v3, s.v4);
}

// ---------------------------------------------------------------------------------------
// shading arithmetic shared by the wavefront kernels (k_generate / k_shade / k_accumulate) and the
// fused path mode of k_traverse: one definition, hence one rounding behaviour
// ---------------------------------------------------------------------------------------
// pinhole ray through the centre of pixel (ix, iy): shader/Shader.cu:249-261
__device__ __forceinline__ V3 primary_direction(uint32_t ix, uint32_t iy, uint32_t width, uint32_t height,
                                                const float *Uc, const float *Vc, const float *Wc) {
    const float ndcx = (((float)ix + 0.5f) / (float)width) * 2.0f - 1.0f;          // :250
    const float ndcy = (((float)iy + 0.5f) / (float)height) * 2.0f - 1.0f;         // :251
    const V3 U = mk3(Uc[0], Uc[1], Uc[2]), V = mk3(Vc[0], Vc[1], Vc[2]), W = mk3(Wc[0], Wc[1], Wc[2]);
    const float aspect = (float)width / (float)height;                            // :260
    return normalize3(add3(add3(muls3(U, ndcx * aspect), muls3(V, ndcy)), W));    // :261
}

// randomSpaceVector, include/Global/DeviceFunctions.cuh:570-582 (length = 1)
__device__ __forceinline__ V3 random_space_vector(Xorwow &rng) {
    V3 ret; float lengthSquare;
    do {
        ret.x = -1.0f + 2.0f * xorwow_uniform(rng);      // randomDouble(state, -1, 1) :220-222
        ret.y = -1.0f + 2.0f * xorwow_uniform(rng);
        ret.z = -1.0f + 2.0f * xorwow_uniform(rng);
        lengthSquare = len2_3(ret);
    } while (lengthSquare < kFloatZero * kFloatZero);
    ret = normalize3(ret);
    return muls3(ret, 1.0f);
}

// closesthitImpl for one (geometry, material) program, shader/Shader.cu:111-213: hit point and the
// direction of the next ray.  rng is touched only when the program draws (rough, or metal with fuzz > 0).
// hit point of a ray, shader/Shader.cu:111-114
__device__ __forceinline__ V3 hit_point(V3 rayOrigin, V3 rayDirection, float t) { return add3(rayOrigin, muls3(rayDirection, t)); }

// the normal a closest-hit program scatters about, shader/Shader.cu:122-155: the sphere's (hitPoint - centre) / radius with the
// object-space centre (quirk Q1) or the interpolated vertex normal, neither transformed nor normalised (Q2), turned against the ray.
// One definition for the programs below and the denoiser's guide pass (denoise.hip), which normalises it as the depth-1 AOV does (:216-227).
typedef const __attribute__((address_space(1))) float *global_floats;      // floats known to lie in device (global) memory: global_load, not flat_load
template <bool HAS_SPHERES>
__device__ __forceinline__ V3 hit_normal(bool sphere, const HitGroup &hg, V3 hitPoint, V3 rayDirection, float u, float v, uint32_t primitiveIndex) {
    V3 _normal;
    if (HAS_SPHERES && sphere) {                                          // :122-136
        const global_floats cp = (global_floats)(reinterpret_cast<const float *>(hg.ptr0) + 3 * (size_t)primitiveIndex);
        const V3 sphereCenter = mk3(cp[0], cp[1], cp[2]);
        const float sphereRadius = ((global_floats)reinterpret_cast<const float *>(hg.ptr1))[primitiveIndex];
        _normal = divs3(sub3(hitPoint, sphereCenter), sphereRadius);
    } else {                                                              // :137-155
        // (the normals are device memory, and the load says so: through the generic pointer it is a flat_load, which counts in lgkmcnt as
        // well as in vmcnt and makes the regeneration's scalar loads wait for it)
        const global_floats np = (global_floats)(reinterpret_cast<const float *>(hg.ptr0) + 9 * (size_t)primitiveIndex);
        const V3 n1 = mk3(np[0], np[1], np[2]), n2 = mk3(np[3], np[4], np[5]), n3 = mk3(np[6], np[7], np[8]);
        const float w = 1.0f - u - v;
        _normal = add3(add3(muls3(n1, w), muls3(n2, u)), muls3(n3, v));
    }
    const bool hitFrontFace = dot3(rayDirection, _normal) < 0.0f;
    return hitFrontFace ? _normal : neg3(_normal);
}

template <bool kSphere, bool kRough>
__device__ __forceinline__ void scatter_at(const HitGroup &hg, V3 hitPoint, V3 rayDirection, float u, float v,
                                           uint32_t primitiveIndex, Xorwow &rng, V3 &reflectDirection) {
    const V3 normalVector = hit_normal<kSphere>(kSphere, hg, hitPoint, rayDirection, u, v, primitiveIndex);
    if (kRough) {                                                         // :169-179
        reflectDirection = add3(normalVector, random_space_vector(rng));
        if (fabsf(len2_3(reflectDirection) - kFloatZero * kFloatZero) < kFloatZero) reflectDirection = normalVector;
    } else {                                                              // :180-192
        const V3 vv = rayDirection, nn = normalVector;
        reflectDirection = normalize3(sub3(vv, muls3(nn, 2.0f * dot3(vv, nn))));
        if (hg.fuzz > 0.0f) reflectDirection = add3(reflectDirection, muls3(random_space_vector(rng), hg.fuzz));
    }
    // :202-213
    if (!finite3(reflectDirection) || len2_3(reflectDirection) <= kFloatZero * kFloatZero) {
        reflectDirection = normalVector;
        if (len2_3(reflectDirection) <= kFloatZero * kFloatZero || !finite3(reflectDirection))
            reflectDirection = mk3(0.0f, 0.0f, 1.0f);
    }
    // the depth-1 AOV write (:216-227) is overwritten by the terminating program (quirk Q3): nothing to keep
}
template <bool kSphere, bool kRough>
__device__ __forceinline__ void scatter(const HitGroup &hg, V3 rayOrigin, V3 rayDirection, float t, float u, float v,
                                        uint32_t primitiveIndex, Xorwow &rng, V3 &hitPoint, V3 &reflectDirection) {
    hitPoint = hit_point(rayOrigin, rayDirection, t);                     // :114
    scatter_at<kSphere, kRough>(hg, hitPoint, rayDirection, u, v, primitiveIndex, rng, reflectDirection);
}
// All four programs in ONE body, for kernels whose lanes run different programs side by side (fused.hip): the programs differ
// in where the normal comes from (sphere / triangle) and in what becomes of it (rough / metal); the random vector, its
// normalisation, the checks of the result and the hit point are the same instructions for every lane, executed once instead of
// once per program present in the wave.  Operation for operation what scatter<kSphere, kRough> computes.
template <bool HAS_SPHERES>
__device__ __forceinline__ void scatter_programs(uint32_t program, const HitGroup &hg, V3 rayOrigin, V3 rayDirection, float t, float u, float v,
                                                 uint32_t primitiveIndex, Xorwow &rng, V3 &hitPoint, V3 &reflectDirection) {
    hitPoint = hit_point(rayOrigin, rayDirection, t);                     // :114
    const bool rough = (program & 1u) == 0u;                              // kProgramSphereRough = 0, kProgramTriangleRough = 2
    const V3 normalVector = hit_normal<HAS_SPHERES>(program < (uint32_t)kProgramTriangleRough, hg, hitPoint, rayDirection, u, v, primitiveIndex);
    V3 rsv = mk3(0.0f, 0.0f, 0.0f);
    if (rough || hg.fuzz > 0.0f) rsv = random_space_vector(rng);
    if (rough) {                                                          // :169-179
        reflectDirection = add3(normalVector, rsv);
        if (fabsf(len2_3(reflectDirection) - kFloatZero * kFloatZero) < kFloatZero) reflectDirection = normalVector;
    } else {                                                              // :180-192
        const V3 vv = rayDirection, nn = normalVector;
        reflectDirection = normalize3(sub3(vv, muls3(nn, 2.0f * dot3(vv, nn))));
        if (hg.fuzz > 0.0f) reflectDirection = add3(reflectDirection, muls3(rsv, hg.fuzz));
    }
    if (!finite3(reflectDirection) || len2_3(reflectDirection) <= kFloatZero * kFloatZero) {     // :202-213
        reflectDirection = normalVector;
        if (len2_3(reflectDirection) <= kFloatZero * kFloatZero || !finite3(reflectDirection))
            reflectDirection = mk3(0.0f, 0.0f, 1.0f);
    }
}
__device__ __forceinline__ bool program_draws(int program, const HitGroup &hg) {
    return program == kProgramSphereRough || program == kProgramTriangleRough || hg.fuzz > 0.0f;
}

// a path that ends at `depth`: miss colour (Shader.cu:276-287) or black at the depth limit (:102-107),
// then the albedo products of the unwinding recursion (:236-238), innermost bounce first
__device__ __forceinline__ V3 fold_chain(bool miss, const float *bg, const uint32_t *chain, uint32_t depth,
                                         const HitGroup *__restrict__ hitgroups) {
    V3 r = miss ? mk3(bg[0], bg[1], bg[2]) : mk3(0.0f, 0.0f, 0.0f);
    for (int k = (int)depth - 2; k >= 0; --k) {
        const HitGroup hg = hitgroups[chain[k]];
        r.x *= hg.albedo[0]; r.y *= hg.albedo[1]; r.z *= hg.albedo[2];
    }
    return r;
}

// ---------------------------------------------------------------------------------------
// traverse: persistent waves over a ray queue, BVH8 with compressed child boxes
// ---------------------------------------------------------------------------------------
constexpr int kLdsStack = 8;          // entries per lane staged in LDS
constexpr int kSpillStack = 56;       // overflow entries per lane in scratch
static_assert(kLdsStack + kSpillStack == (int)kTraversalStackEntries, "the builds' depth limit (device_types.h) is this stack's capacity");
constexpr int kTraverseBlock = 64;         // one wave per workgroup

struct TravState {
    float ox, oy, oz, dx, dy, dz;
    float idx, idy, idz;
    float bt, bu, bv;
    float tlo;                    // the path kernels' node step culls below it (per lane: the launch's tmin, or a repeat primary ray's window -- kSeedWindow)
    uint32_t bprim, binst;
    uint32_t oct_inv4;
    uint2 cur;
    uint2 ptri;                   // leaf group being consumed, one primitive per iteration
    int sp, base;                 // stack = entries [base, sp): the bottom can be given away (tail splitting)
    uint32_t slot;
};

// 1 / d for the slab test.  The counting build divides exactly, so that its node / primitive counts equal the CPU walk of
// the same bytes (tests); the production build takes v_rcp_f32 (1 ULP, one instruction instead of the ~10 of the IEEE
// sequence, three times per ray): the slab test only culls, and its boxes are padded by far more than an ULP.
constexpr float kRcpDirFloor = 1e-20f;      // a direction component below it counts as it
template <bool EXACT>
__device__ __forceinline__ float safe_rcp_dir(float d) {
    const float lim = kRcpDirFloor;
    // (the sign is the one the slab test's near / far choice and the octant use, `d < 0`: a component of -0.0 -- a ray mirrored by an axis-aligned
    // wall -- counts as positive there, and with copysignf here its reciprocal was negative: near and far swapped, every box culled, the ray left
    // a closed room.  Found in round 4 by tools/stress_modes.py: one pixel of a Cornell box; tests/test_gpu_parity.py has the rays.)
    // (d + 0.0f: -0.0 becomes +0.0, everything else stays -- one instruction, no new constant in a kernel that has no register to spare)
    const float dd = fabsf(d) < lim ? copysignf(lim, d + 0.0f) : d;
    return EXACT ? 1.0f / dd : __builtin_amdgcn_rcpf(dd);
}

// a new ray in `s`: origin, direction, guarded reciprocals, octant word, empty best hit.  (What the ray's first node is and how the
// stacks are emptied is the kernels': lean_start, k_traverse's start_ray.)
template <bool EXACT>
__device__ __forceinline__ void trav_start(TravState &s, V3 o, V3 d, float tmax_ray) {
    s.ox = o.x; s.oy = o.y; s.oz = o.z; s.dx = d.x; s.dy = d.y; s.dz = d.z;
    s.idx = safe_rcp_dir<EXACT>(s.dx); s.idy = safe_rcp_dir<EXACT>(s.dy); s.idz = safe_rcp_dir<EXACT>(s.dz);
    const uint32_t oct = (s.dx < 0.0f ? 4u : 0u) | (s.dy < 0.0f ? 2u : 0u) | (s.dz < 0.0f ? 1u : 0u);
    s.oct_inv4 = (7u - oct) * 0x01010101u;
    s.bt = tmax_ray; s.bu = 0.0f; s.bv = 0.0f; s.bprim = kMissPrim; s.binst = kMissPrim;
}

// A condition of the primitive test as the WHOLE WAVE's: one bit per lane in a scalar register pair, where `bool` is one lane's.  Made
// from a bool it is that compare's ballot, and & and | are scalar instructions -- the very instructions the compiler makes of a chain of
// per-lane bools.  What differs is that the outcome is there as a mask: the path kernels' loop (trav_loop.h) does mask arithmetic with
// it, where the ballot of a per-lane bool that is no single compare costs a v_cndmask 0 / 1 and a v_cmp.  All lanes must be active.
struct WaveCond {
    uint64_t m;
    __device__ __forceinline__ WaveCond(bool c) : m(__ballot(c)) {}
    __device__ __forceinline__ explicit WaveCond(uint64_t mask) : m(mask) {}
    __device__ __forceinline__ WaveCond operator&(WaveCond o) const { return WaveCond(m & o.m); }
    __device__ __forceinline__ WaveCond operator|(WaveCond o) const { return WaveCond(m | o.m); }
};
__device__ __forceinline__ bool cond_lane(bool c) { return c; }                  // this lane's outcome of a condition of either kind
__device__ __forceinline__ bool cond_lane(WaveCond c) { return __builtin_amdgcn_inverse_ballot_w64(c.m); }

// canonical primitive test (DESIGN.md "canonical intersector"); updates the best hit.
// kInstanced (two-level trees, fused.hip): the record is a shared BLAS's, in object space, and so is the ray in `s` by now (the transform
// node did that for triangles and spheres alike); the record does not know who instances it: `inst_cur` does.
// (test_prim_ray: the ray given explicitly -- a lane of the instanced kernel that has left an instance with leaf tests still to make keeps that
// instance's object-space ray in LDS while its registers hold the world ray again)
// (live, triangles only: false rejects the record -- the caller's lane has none and A / B / C are whatever its registers held; the
// test still runs, so that the caller needs no per-lane branch round it)
// (Cond: bool, or WaveCond -- triangles only, every lane active -- for the outcome as a wave mask)
// kOneGroup (k_path_one, fused_one.hip: triangles of ONE instance): every record's instance is 0, so it is not read from the record, a
// tie at the same distance goes to the lower primitive id -- what the (instance, primitive) order says when both instances are 0; a
// ray that has no hit yet holds bprim == kMissPrim, above every id -- and TravState::binst is left alone: whoever reads it takes 0.
// kRestart (k_path_restart, fused_restart.hip: kOneGroup, whose TravState::binst is free): binst keeps the RECORD the best hit was accepted from
// (`rec`: the record's index, the lane's pidx) -- kMissPrim, which trav_start leaves there, where the lane has accepted none itself.  The
// regeneration looks up the node whose leaf slot holds that record, where the pixel's next primary ray starts (fused_body.h: s_restart).
// kLiveIsExec (k_path_idle's loop copy with idle lanes off, trav_loop.h: kIdleOff -- not its drained copy, which tests for the whole wave): the
// caller has switched the lanes without a record off, so `live` is implied -- a compare writes 0 for a lane that is off -- and is not
// and-ed in; the best hit is updated in place (a lane that is off keeps its own).
template <class V, class Cond = bool, bool kLiveIsExec = false>
__device__ __forceinline__ Cond test_prim_ray(const float4 A, const float4 B, const float4 C, TravState &s, const V3 o, const V3 d,
                                              float tmin, float tmax_ray,
                                              const float *__restrict__ inst_inv, const uint32_t *__restrict__ inst_identity, uint32_t inst_cur = 0u,
                                              Cond live = true, [[maybe_unused]] uint32_t rec = 0u) {
    static_assert(!V::kSpheres || sizeof(Cond) == sizeof(bool), "spheres are tested under per-lane control flow");
    float t, u = 0.0f, v = 0.0f;
    uint32_t prim = __float_as_uint(A.w), inst;
    if (V::kSpheres && __float_as_uint(C.w) == 1u) {
        inst = V::kInstanced ? inst_cur : __float_as_uint(B.w);
        V3 oo = o, dd = d;
        if (!V::kInstanced && !inst_identity[inst]) {
            const float *m = inst_inv + 12 * (size_t)inst;
            oo = mk3(((m[0] * o.x + m[1] * o.y) + m[2] * o.z) + m[3], ((m[4] * o.x + m[5] * o.y) + m[6] * o.z) + m[7],
                     ((m[8] * o.x + m[9] * o.y) + m[10] * o.z) + m[11]);
            dd = mk3((m[0] * d.x + m[1] * d.y) + m[2] * d.z, (m[4] * d.x + m[5] * d.y) + m[6] * d.z,
                     (m[8] * d.x + m[9] * d.y) + m[10] * d.z);
        }
        const V3 oc = sub3(oo, mk3(A.x, A.y, A.z));
        const float r = B.x;
        const float a = dot3(dd, dd);
        if (!(a != 0.0f)) return false;
        const float b = dot3(oc, dd);
        const float cc = dot3(oc, oc) - r * r;
        const float disc = b * b - a * cc;
        if (!(disc >= 0.0f)) return false;
        const float sq = sqrtf(disc);
        const float t0 = (-b - sq) / a;
        if (t0 > tmin && t0 < tmax_ray) t = t0;
        else {
            const float t1 = (-b + sq) / a;
            if (t1 > tmin && t1 < tmax_ray) t = t1; else return false;
        }
    } else {
        // Straight-line: every quantity is computed for every lane and ONE condition decides.  The early returns of the
        // textbook form save nothing on a wave (the instructions run as long as one lane is still in) and cost a mask save /
        // branch / restore each; the SIMD issues ~1 instruction of ANY kind per 2.4 cycles, scalar ones included
        // (profiles/r02_valu_issue_patterns_microbench.txt).  Same decisions, same values: a rejected lane's later
        // quantities are never used, det == 0 gives inv = inf and u = NaN or +-inf, which fails the u test like the
        // explicit one does.  (u <= 1 is not tested: v >= 0 and u + v <= 1 imply it, the rounded sum included.)
        inst = V::kInstanced ? inst_cur : __float_as_uint(B.w);
        const V3 e1 = mk3(B.x, B.y, B.z), e2 = mk3(C.x, C.y, C.z);
        const V3 pvec = cross3(d, e2);
        const float det = dot3(e1, pvec);
        const float inv = 1.0f / det;
        const V3 tvec = sub3(o, mk3(A.x, A.y, A.z));
        u = dot3(tvec, pvec) * inv;
        const V3 qvec = cross3(tvec, e1);
        v = dot3(d, qvec) * inv;
        t = dot3(e2, qvec) * inv;
        const Cond nonzero(det != 0.0f);
        const Cond ok = (kLiveIsExec ? nonzero : live & nonzero) & Cond(u >= 0.0f) & Cond(v >= 0.0f) & Cond(u + v <= 1.0f) & Cond(t > tmin) & Cond(t < tmax_ray);
        if constexpr (V::kOneGroup) {
            const Cond better = ok & (Cond(t < s.bt) | (Cond(t == s.bt) & Cond(prim < s.bprim)));
            const bool mine = cond_lane(better);
            s.bt = mine ? t : s.bt; s.bu = mine ? u : s.bu; s.bv = mine ? v : s.bv;
            s.bprim = mine ? prim : s.bprim;
            if constexpr (V::kRestart) s.binst = mine ? rec : s.binst;
            return better;
        }
        if (!V::kSpheres) {
            // closest hit: min t, ties -> lowest (instance, primitive); predicated update
            const Cond better = ok & (Cond(t < s.bt) | (Cond(t == s.bt) & (Cond(inst < s.binst) | (Cond(inst == s.binst) & Cond(prim < s.bprim)))));
            const bool mine = cond_lane(better);
            s.bt = mine ? t : s.bt; s.bu = mine ? u : s.bu; s.bv = mine ? v : s.bv;
            s.bprim = mine ? prim : s.bprim; s.binst = mine ? inst : s.binst;
            return better;
        }
        if (!cond_lane(ok)) return false;
    }
    // closest hit: min t, ties -> lowest (instance, primitive)
    bool better = t < s.bt;
    if (!better && t == s.bt) {
        const uint64_t id = ((uint64_t)inst << 32) | prim, bid = ((uint64_t)s.binst << 32) | s.bprim;
        better = id < bid;
    }
    if (better) { s.bt = t; s.bu = u; s.bv = v; s.bprim = prim; s.binst = inst; }
    return better;
}

template <class V, class Cond = bool, bool kLiveIsExec = false>
__device__ __forceinline__ Cond test_prim(const float4 A, const float4 B, const float4 C, TravState &s,
                                          float tmin, float tmax_ray,
                                          const float *__restrict__ inst_inv, const uint32_t *__restrict__ inst_identity, uint32_t inst_cur = 0u,
                                          Cond live = true, uint32_t rec = 0u) {
    return test_prim_ray<V, Cond, kLiveIsExec>(A, B, C, s, mk3(s.ox, s.oy, s.oz), mk3(s.dx, s.dy, s.dz), tmin, tmax_ray, inst_inv, inst_identity, inst_cur, live, rec);
}

#define HRT_BYTE_F(w, k) ((float)(((w) >> (8 * (k))) & 0xffu))

// ---- the loads of the traversal step ------------------------------------------------------------
// Every lane loads its own node (5 dwordx4) and primitive (3 dwordx4) into registers: primitive first, node second, so that
// the primitive needs vmcnt(5) and the node vmcnt(0).  The destinations are named "+v" in the wait statements so that no use
// is scheduled above the wait.  (A cooperative LDS-DMA gather of the wave's 64 nodes was measured and not adopted: DESIGN.md 4.)
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void issue_prim_loads(const void *p, f32x4 &a, f32x4 &b, f32x4 &c) {
    asm volatile("global_load_dwordx4 %0, %3, off\n\t"
                 "global_load_dwordx4 %1, %3, off offset:16\n\t"
                 "global_load_dwordx4 %2, %3, off offset:32"
                 : "=&v"(a), "=&v"(b), "=&v"(c) : "v"(p) : "memory");
}
__device__ __forceinline__ void issue_node_loads(const void *p, u32x4 &a, u32x4 &b, u32x4 &c, u32x4 &d, u32x4 &e) {
    asm volatile("global_load_dwordx4 %0, %5, off\n\t"
                 "global_load_dwordx4 %1, %5, off offset:16\n\t"
                 "global_load_dwordx4 %2, %5, off offset:32\n\t"
                 "global_load_dwordx4 %3, %5, off offset:48\n\t"
                 "global_load_dwordx4 %4, %5, off offset:64"
                 : "=&v"(a), "=&v"(b), "=&v"(c), "=&v"(d), "=&v"(e) : "v"(p) : "memory");
}
__device__ __forceinline__ void wait_prim_loads(f32x4 &a, f32x4 &b, f32x4 &c) {
    asm volatile("s_waitcnt vmcnt(5)" : "+v"(a), "+v"(b), "+v"(c) :: "memory");
}
__device__ __forceinline__ void wait_node_loads(u32x4 &a, u32x4 &b, u32x4 &c, u32x4 &d, u32x4 &e) {
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e) :: "memory");
}

// The slab test's two forms.  0: the planes' distances clamped to the ray's interval [tmin, bt] with a max and a min per child (the form
// k_traverse keeps: exact reciprocals in its counting build, no limits).  1, the path kernels' (trav_loop.h): the interval mapped onto
// [0, 1] once per node step, in essence t' = (t - tmin) k with k = 1 / (bt - tmin) folded into the six coefficients, so that the clamp rides on the
// z axis' FMAs as their `clamp` output modifier: max3(tnx', tny', clamp(tnz')) = max(N', 0), min3(tfx', tfy', clamp(tfz')) = min(F', 1).
// -DHRT_SLAB_INTERVAL01=0 builds form 0 everywhere (A/B of two libraries; DESIGN.md 4.1 has the ranges and the error budget).
#ifndef HRT_SLAB_INTERVAL01
#define HRT_SLAB_INTERVAL01 1
#endif
constexpr bool kSlabInterval01 = HRT_SLAB_INTERVAL01 != 0;
// Exactly: t' = (t (1 - 2^-20) - tmin) k with k = 1 / ((bt - tmin) + 2^-36).
//   * The factor makes the bt end conservative: bt maps to 1 - 2^-20 at most, 2^4 ulps below the clamp and far above the one ulp of
//     v_rcp_f32 (tmin maps to -2^-20 tmin k <= 0: conservative too).  It is folded into the ray's reciprocals where the ray starts, so the
//     loop does not pay for it.
//   * The floor keeps k finite (<= 2^36) when a hit has come within nothing of tmin -- a denormal bt - tmin would make k infinite,
//     0 * inf a NaN and the clamp a 0 on both sides: a cull.  It is a literal of the add; it only lowers k (bt maps lower still) and
//     vanishes in the rounding once bt - tmin > 2^-12.  (A ray whose hits all lie below 2^-36 -- a direction of length 1e30 with
//     tmin = 0 -- is culled at its bt end by nothing any more: slower, not wrong.)
constexpr float kSlabSpanSlack = 1.0f - 0x1p-20f, kSlabSpanFloor = 0x1p-36f;
// The products idx k, (p - o) idx k and the per-cell step 2^e idx k must neither underflow nor overflow.  That is settled where a ray
// starts (lean_start; slab_cap_rcp also where the instanced kernel's lane enters an instance), not in the loop:
//   * the culling bound starts at min(tmax, kSlabReach / max |d_c|), so |d_c| (bt - tmin) <= 2^64 and |idx k| >= 2^-65 for the largest
//     component, more for the others: the step 2^e idx k stays a normal float for cells down to 2^-60 (a scene of 2^-52);
//   * a reciprocal is at most kSlabRcpRatio times the smallest of the three, i.e. a component below 2^-40 of the largest counts as that
//     (safe_rcp_dir's 1e-20 is the same approximation with an absolute bound: over a scene of extent S the ray it stands for leaves the
//     true one by 2^-40 * 12 S, against a padding of 4e-6 S).  With k <= 2^36, |idx| <= 1e20 and |p - o| <= 2^25 every product is finite.
constexpr float kSlabReach = 0x1p64f, kSlabRcpRatio = 0x1p40f;
// The interval's lower end is the LANE's (TravState::tlo; the `tmin` operand of node_slab_test): the launch's tmin for every ray but a pixel's
// repeat primary ray, which has a known hit at t (HRT_SEED_PRIMARY=2; fused_body.h) and starts with bt = t and tlo = t (1 - kSeedWindow):
// the identical ray has proved that nothing lies before t, so a box whose far plane is before t need not be opened.  The window is far
// wider than everything that rounds -- the slack 2^-20, the ulp of v_rcp_f32, half an ulp of t in the offset's FMA -- so a box that
// holds the hit keeps F' > 0 (DESIGN.md 4.1 has the argument); below 2^-10 the CPU walks gain nothing more.
// seed_window_lo: the lower end for a ray (direction d) whose known hit is at `seed`.  The argument wants the slab test's distances to be the
// ray's own, which they are not when ALL of d is below safe_rcp_dir's floor (a direction of length 1e-30: every plane then seems 1e10 times
// nearer than it is -- harmless for a bound from above, not for one from below): such a ray keeps tmin.  A camera ray is normalised.
constexpr float kSeedWindow = 0x1p-10f;
__device__ __forceinline__ float seed_window_lo(V3 d, float seed, float tmin) {
    const bool plain = fmaxf(fmaxf(fabsf(d.x), fabsf(d.y)), fabsf(d.z)) >= kRcpDirFloor;
    return plain ? fmaxf(tmin, seed * (1.0f - kSeedWindow)) : tmin;
}
// caps idx / idy / idz and folds the slack into them; returns the smallest of their magnitudes before that, 1 / max |d_c|
__device__ __forceinline__ float slab_cap_rcp(float &idx, float &idy, float &idz) {
    const float m = fminf(fminf(fabsf(idx), fabsf(idy)), fabsf(idz)), cap = m * kSlabRcpRatio;
    idx = copysignf(fminf(fabsf(idx), cap) * kSlabSpanSlack, idx); idy = copysignf(fminf(fabsf(idy), cap) * kSlabSpanSlack, idy);
    idz = copysignf(fminf(fabsf(idz), cap) * kSlabSpanSlack, idz);
    return m;
}

// the node step: slab test of the eight quantised children of the node in rn0..rn4 against the ray in `s`; returns the children's
// sibling group (first child, hit bits 31..24 | inner mask; y <= 0xffffff: none) and leaf group (first primitive, bit per primitive that
// may be hit; y == 0: none)
template <bool kInterval01>
__device__ __forceinline__ void node_slab_test(const TravState &s, float tmin, const u32x4 rn0, const u32x4 rn1, const u32x4 rn2, const u32x4 rn3,
                                          const u32x4 rn4, uint2 &child, uint2 &tri) {
    const float px = __uint_as_float(rn0.x), py = __uint_as_float(rn0.y), pz = __uint_as_float(rn0.z);
    const uint32_t e_imask = rn0.w;
    float kx = s.idx, ky = s.idy, kz = s.idz, c0 = 0.0f;
    if (kInterval01) {
        // (k is made again in every node step: a value kept alive across the loop costs more here than these three instructions)
        const float k = __builtin_amdgcn_rcpf((s.bt - tmin) + kSlabSpanFloor);
        kx = s.idx * k; ky = s.idy * k; kz = s.idz * k; c0 = -(tmin * k);
    }
    const float aix = __uint_as_float((e_imask & 0xffu) << 23) * kx;
    const float aiy = __uint_as_float(((e_imask >> 8) & 0xffu) << 23) * ky;
    const float aiz = __uint_as_float(((e_imask >> 16) & 0xffu) << 23) * kz;
    const float aox = kInterval01 ? fmaf(px - s.ox, kx, c0) : (px - s.ox) * kx;
    const float aoy = kInterval01 ? fmaf(py - s.oy, ky, c0) : (py - s.oy) * ky;
    const float aoz = kInterval01 ? fmaf(pz - s.oz, kz, c0) : (pz - s.oz) * kz;
    const bool nx = s.dx < 0.0f, ny = s.dy < 0.0f, nz = s.dz < 0.0f;
    uint32_t hitmask = 0u;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const uint32_t meta4 = h ? rn1.w : rn1.z;
        const uint32_t is_inner4 = (meta4 & (meta4 << 1)) & 0x10101010u;
        const uint32_t inner_mask4 = (is_inner4 >> 4) * 0xffu;
        const uint32_t bit_index4 = (meta4 ^ (s.oct_inv4 & inner_mask4)) & 0x1f1f1f1fu;
        const uint32_t child_bits4 = (meta4 >> 5) & 0x07070707u;
        const uint32_t qlox = h ? rn2.y : rn2.x, qloy = h ? rn2.w : rn2.z, qloz = h ? rn3.y : rn3.x;
        const uint32_t qhix = h ? rn3.w : rn3.z, qhiy = h ? rn4.y : rn4.x, qhiz = h ? rn4.w : rn4.z;
        const uint32_t xn = nx ? qhix : qlox, xf = nx ? qlox : qhix;
        const uint32_t yn = ny ? qhiy : qloy, yf = ny ? qloy : qhiy;
        const uint32_t zn = nz ? qhiz : qloz, zf = nz ? qloz : qhiz;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float tnx = fmaf(HRT_BYTE_F(xn, j), aix, aox), tfx = fmaf(HRT_BYTE_F(xf, j), aix, aox);
            const float tny = fmaf(HRT_BYTE_F(yn, j), aiy, aoy), tfy = fmaf(HRT_BYTE_F(yf, j), aiy, aoy);
            const float tnz = fmaf(HRT_BYTE_F(zn, j), aiz, aoz), tfz = fmaf(HRT_BYTE_F(zf, j), aiz, aoz);
            const uint32_t cb = (child_bits4 >> (8 * j)) & 0xffu;
            const uint32_t bi = (bit_index4 >> (8 * j)) & 0xffu;
            // conservative: the builder pads and rounds the child boxes outwards
            if (kInterval01) {
                // med3(x, 0, 1) of an FMA's result is the FMA's clamp modifier (DX10 clamp: NaN -> 0).  Strict: with both ends clamped a box
                // wholly before tmin gives 0 against 0 and one wholly beyond bt 1 against 1; padded boxes have thickness.
                const float tlo = fmaxf(fmaxf(tnx, tny), __builtin_amdgcn_fmed3f(tnz, 0.0f, 1.0f));
                const float thi = fminf(fminf(tfx, tfy), __builtin_amdgcn_fmed3f(tfz, 0.0f, 1.0f));
                if (tlo < thi) hitmask |= cb << bi;
            } else {
                const float tlo = fmaxf(fmaxf(tnx, tny), fmaxf(tnz, tmin));
                const float thi = fminf(fminf(tfx, tfy), fminf(tfz, s.bt));
                if (tlo <= thi) hitmask |= cb << bi;
            }
        }
    }
    child = make_uint2(rn1.x, (hitmask & 0xff000000u) | (e_imask >> 24));
    tri = make_uint2(rn1.y, hitmask & 0x00ffffffu);
}

// Lane-utilisation counters of the instrumented build (`make stats`, tools/lane_stats.py); empty otherwise.
constexpr unsigned long long kWaveClockLow = 1600ull, kWaveClockStep = 16ull, kWaveClockBins = 56ull;      // MHz: 1600 .. 2496 (HrtStats.wave_clock, include/hrt.h)
struct LaneStats {
#ifdef HRT_LANE_STATS
    unsigned long long iter = 0, alive = 0, node = 0, prim = 0, ppass = 0, regen = 0, enter = 0;
    // the drained phase (tools/tail_profile.py): iterations and alive lanes of the kTail copy of the loop, the wave's clock
    // (s_memrealtime: one 100 MHz counter for the whole device) when it first found the work used up
    unsigned long long tail_iter = 0, tail_alive = 0, t_drained = 0, mark_iter = 0, mark_alive = 0;
    // the clock the wave ran at (tools/wave_clock.py): the shader clock's counter (s_memtime) beside the 100 MHz one, both read at the wave's
    // first regeneration and at its exit -- clock = cycles / ticks x 100 MHz.  To the statistics slots only, never into an output.
    unsigned long long c_first = 0, r_first = 0;
#ifdef HRT_LANE_STATS_PRIMARY
    // what a pixel's repeat primary rays cost (make stats EXTRA_HIPFLAGS=-DHRT_LANE_STATS_PRIMARY, tools/lane_stats.py primary):
    // primary rays that entered the loop, those of them that started at a node other than the root (`quick`: their lanes, a wave mask), the
    // iterations those were alive and the iterations they waited for their regeneration, and the rays decided in the regeneration
    // (kDirect).  They take the drained phase's slots (HrtStats.tail), which such a build does not fill.
    unsigned long long quick = 0, prim_rays = 0, quick_rays = 0, quick_alive = 0, quick_wait = 0, direct_rays = 0;
    // what a pixel's primary MISSES cost (k_path_direct's miss block; profiles/r33_primary_miss_block.txt section 0): `root` -- the lanes whose ray
    // is a primary ray that walks from the root, root_alive / root_wait -- PER LANE, the iterations the lane's such ray has been alive and has
    // waited; a ray that comes back a miss at depth 1 adds them to the wave's sums (miss_*).  ff_rays: the samples the miss block decided.
    // miss_alive and miss_wait take the last two of the drained phase's slots; miss_rays and ff_rays share the word in front of debug[]
    // (prim_tests - prim_tests_closest), 32 bits each: one launch of 2^32 rays at most between two resets.
    unsigned long long root = 0, miss_rays = 0, miss_alive = 0, miss_wait = 0, ff_rays = 0;
    uint32_t root_alive = 0, root_wait = 0;
#endif
#endif
#if defined(HRT_LANE_STATS) && defined(HRT_LANE_STATS_PRIMARY)
    // the wave's sum of a per-lane count below 2^24, bit by bit (no cross-lane instruction that an instrumented loop would have to schedule)
    static __device__ __forceinline__ unsigned long long wave_sum24(uint32_t v) {
        unsigned long long sum = 0ull;
        for (int b = 0; b < 24; ++b) sum += (unsigned long long)__popcll(__ballot((v >> b) & 1u)) << b;
        return sum;
    }
#endif
    // the regeneration looks at a finished ray: `primary_miss` -- the lane's is a primary ray (depth 1) that came back from the loop a miss
    __device__ __forceinline__ void finished_primary([[maybe_unused]] bool primary_miss) {
#if defined(HRT_LANE_STATS) && defined(HRT_LANE_STATS_PRIMARY)
        miss_rays += __popcll(__ballot(primary_miss));
        miss_alive += wave_sum24(primary_miss ? root_alive : 0u); miss_wait += wave_sum24(primary_miss ? root_wait : 0u);
#endif
    }
    // ... and the miss block has decided `n` further samples of the lane's pixel without a walk
    __device__ __forceinline__ void fast_forwarded([[maybe_unused]] uint32_t n) {
#if defined(HRT_LANE_STATS) && defined(HRT_LANE_STATS_PRIMARY)
        ff_rays += wave_sum24(n);
#endif
    }
    // the wave has found the tile used up (every regeneration from then on says so: the first one counts)
    __device__ __forceinline__ void drained([[maybe_unused]] bool exhausted) {
#ifdef HRT_LANE_STATS
        if (exhausted && t_drained == 0ull) t_drained = __builtin_amdgcn_s_memrealtime();
#endif
    }
    // round a call of the drained copy of the loop
    __device__ __forceinline__ void tail_begin() {
#ifdef HRT_LANE_STATS
        mark_iter = iter; mark_alive = alive;
#endif
    }
    __device__ __forceinline__ void tail_end() {
#ifdef HRT_LANE_STATS
        tail_iter += iter - mark_iter; tail_alive += alive - mark_alive;
#endif
    }
    __device__ __forceinline__ void regeneration() {
#ifdef HRT_LANE_STATS
        if (regen == 0ull) { r_first = __builtin_amdgcn_s_memrealtime(); c_first = __builtin_amdgcn_s_memtime(); }
        ++regen;
#endif
    }
    __device__ __forceinline__ void iteration([[maybe_unused]] bool lane_alive, [[maybe_unused]] uint64_t mask_n, [[maybe_unused]] uint64_t mask_p) {
#ifdef HRT_LANE_STATS
        ++iter; alive += __popcll(__ballot(lane_alive)); node += __popcll(mask_n); prim += __popcll(mask_p); ppass += mask_p != 0ull;
#endif
    }
    // a regeneration has started its rays: `primary` -- the lane's is its pixel's primary ray, `quick` -- ... which does not start at the root,
    // `direct` -- the lane's primary ray was decided here, by its record's test (counted as a primitive test), and `launched`: the wave's new rays
    __device__ __forceinline__ void started([[maybe_unused]] bool primary, [[maybe_unused]] bool quick_lane, [[maybe_unused]] bool direct, [[maybe_unused]] uint64_t launched) {
#if defined(HRT_LANE_STATS) && defined(HRT_LANE_STATS_PRIMARY)
        const unsigned long long q = __ballot(quick_lane);
        quick = (quick & ~launched) | q;
        prim_rays += __popcll(__ballot(primary)); quick_rays += __popcll(q);
        const unsigned long long n = __popcll(__ballot(direct));
        direct_rays += n; prim += n;
        const bool from_root = primary && !quick_lane;
        root = (root & ~launched) | __ballot(from_root);
        if (from_root) { root_alive = 0u; root_wait = 0u; }
#endif
    }
    __device__ __forceinline__ void primary_slots([[maybe_unused]] uint64_t alive_m, [[maybe_unused]] uint64_t waiting_m) {
#if defined(HRT_LANE_STATS) && defined(HRT_LANE_STATS_PRIMARY)
        quick_alive += __popcll(quick & alive_m); quick_wait += __popcll(quick & waiting_m);
        root_alive += __builtin_amdgcn_inverse_ballot_w64(root & alive_m) ? 1u : 0u; root_wait += __builtin_amdgcn_inverse_ballot_w64(root & waiting_m & ~alive_m) ? 1u : 0u;
#endif
    }
    // k_path_idle's loop copy with idle lanes off (trav_loop.h: kIdleOff) counts between two of these, where every lane is on: the counters
    // are per-lane registers to the compiler, which would otherwise be free to add where lane 0, which reports, may be off
    __device__ __forceinline__ void pin() {
#ifdef HRT_LANE_STATS
        asm volatile("" : "+v"(iter), "+v"(alive), "+v"(node), "+v"(prim), "+v"(ppass));
#ifdef HRT_LANE_STATS_PRIMARY
        asm volatile("" : "+v"(quick), "+v"(quick_alive), "+v"(quick_wait), "+v"(root), "+v"(root_alive), "+v"(root_wait));
#endif
#endif
    }
    __device__ __forceinline__ void entered([[maybe_unused]] bool lane_enters) {
#ifdef HRT_LANE_STATS
        enter += __popcll(__ballot(lane_enters));
#endif
    }
    // end of a path kernel: lane 0 adds the wave's counters to the slots tools/lane_stats.py reads, behind the ray counters
    __device__ __forceinline__ void report([[maybe_unused]] uint64_t *rays_closest, [[maybe_unused]] uint32_t tx) {
#ifdef HRT_LANE_STATS
        if (tx == 0u) {
            unsigned long long *d = reinterpret_cast<unsigned long long *>(rays_closest);
            atomicAdd(d + 6, iter); atomicAdd(d + 7, alive); atomicAdd(d + 8, node); atomicAdd(d + 9, prim); atomicAdd(d + 2, ppass); atomicAdd(d + 3, regen); atomicAdd(d + 4, enter);
            // DeviceStats::tail, behind debug[4].  Clocks are kept relative to the first reporting wave's (slot 2), plus 2^40 so that a
            // wave that drained before that one exited stays positive; the first drained clock as the maximum of its complement,
            // so that zeroed memory is the neutral element of every slot.
            unsigned long long *t = d + 10;
            const unsigned long long now = __builtin_amdgcn_s_memrealtime();
            unsigned long long base = atomicCAS(t + 2, 0ull, now);
            if (base == 0ull) base = now;
            if (t_drained == 0ull) t_drained = now;
            const unsigned long long bias = 1ull << 40, exit_rel = now - base + bias, lane_iters = 64ull * tail_iter;
#ifdef HRT_LANE_STATS_PRIMARY
            (void)bias; (void)lane_iters; (void)exit_rel;
            atomicAdd(t + 0, prim_rays); atomicAdd(t + 1, quick_rays); atomicAdd(t + 3, quick_alive); atomicAdd(t + 4, quick_wait); atomicAdd(t + 5, direct_rays);
            atomicAdd(t + 6, miss_alive); atomicAdd(t + 7, miss_wait); atomicAdd(d + 5, miss_rays | (ff_rays << 32));
#else
            atomicAdd(t + 0, tail_iter); atomicAdd(t + 1, tail_alive);
            atomicMax(t + 3, ~(t_drained - base + bias)); atomicMax(t + 4, exit_rel); atomicAdd(t + 5, exit_rel);
            // lane-ticks without a ray between draining and exit: the share of idle lanes over the drained iterations, times that span
            atomicAdd(t + 6, tail_iter ? (now - t_drained) * (lane_iters - tail_alive) / tail_iter : (now - t_drained) * 64ull);
            atomicAdd(t + 7, 1ull);
#endif
            // DeviceStats::wave_clock, behind `paths`: waves, their cycles, their ticks, and the histogram of their clocks -- kWaveClockBins bins of
            // kWaveClockStep MHz from kWaveClockLow (the ends take what lies beyond).  A wave that lived less than 10 us says nothing.
            unsigned long long *c = d + 19;
            const unsigned long long cycles = __builtin_amdgcn_s_memtime() - c_first, ticks = now - r_first;
            if (regen != 0ull && ticks >= 1000ull) {
                const unsigned long long mhz = cycles * 100ull / ticks;
                const unsigned long long bin = mhz < kWaveClockLow ? 0ull : (mhz - kWaveClockLow) / kWaveClockStep;
                atomicAdd(c + 0, 1ull); atomicAdd(c + 1, cycles); atomicAdd(c + 2, ticks);
                atomicAdd(c + 4 + (bin < kWaveClockBins ? bin : kWaveClockBins - 1ull), 1ull);
            }
        }
#endif
    }
};

}  // namespace hrt
