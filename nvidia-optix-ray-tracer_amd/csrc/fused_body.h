// fused_body.h -- the body of the persistent path kernel, ONCE, for the kernels that run it: k_fused (fused.hip), k_path_blocks
// (fused_blocks.hip: pixels handed out in sample blocks, path_lane.h), k_path_one (fused_one.hip: k_path_blocks for a scene with one hit group)
// k_path_capture (fused_capture.hip: primary hits kept per pixel) and k_path_counts (fused_counts.hip: a sample count per pixel, the caller's sums).
// What the body does is described at the top of fused.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "device_types.h"
#include "trav_common.h"
#include "trav_loop.h"
#include "path_lane.h"

#pragma clang fp contract(off)

namespace hrt {

#ifndef HRT_SPHERE_CULL
#define HRT_SPHERE_CULL 1     // kInstanced: a ray that misses an instance's bounding sphere does not enter it (0: enters every instance whose box it crosses)
#endif
// kInstanced: the tree has two levels (bvh8.h: transform nodes; the reference's IAS over shared GASes, RendererImpl.cu:174-206).  A lane
// whose next node turns out to be a transform node leaves its world ray in LDS, goes on with the ray in the instance's object space
// (row-major 3x4 inverse from the node; identity: copied) and the BLAS's root as the only child; its node stack continues ABOVE what it
// held (`base` = the frame's bottom), so the bookkeeping sequence is the one-level kernel's, unchanged.  When it reports the frame
// empty the lane takes its world ray back and pops what it had left in world space.  A separate instantiation: the one-level kernels
// and their register budget are untouched.
struct InstLane {
    // the instance whose BLAS this lane is in (kNoWork: none), and what its node stack looked like when it went in (base | entries << 8)
    uint32_t inst_cur = kNoWork, frame = 0u;
    // the rest of a world ray that waits in LDS while its lane is inside an instance (reciprocals, octant); origin and direction wait in
    // the mailboxes' memory: tail splitting is off for two-level trees
    float *park_idx, *park_idy, *park_idz;
    uint32_t *park_oct;

    // after the node loads: lanes whose node is a transform node (`enter`) go on in the instance's object space, with the BLAS's root as
    // the only child -- unless the ray misses the instance's bounding sphere (`enter` is withdrawn, the node has no children)
    __device__ __forceinline__ bool enter_instance(bool enter, TravState &ls, uint2 &child, const u32x4 rn0, const u32x4 rn1, const u32x4 rn2, const u32x4 rn3,
                                                   const u32x4 rn4, const Mailboxes &mb, uint32_t tx) {
        if (__ballot(enter) != 0ull) {
            float ox = ls.ox, oy = ls.oy, oz = ls.oz, dx = ls.dx, dy = ls.dy, dz = ls.dz;      // the ray in the instance's object space
            if (enter) {
                const TravState &s = ls;
                if (rn1.z == 0u) {          // not the identity: xf_point / xf_vector of the oracle, operation for operation
                    const float m0 = __uint_as_float(rn2.x), m1 = __uint_as_float(rn2.y), m2 = __uint_as_float(rn2.z), m3 = __uint_as_float(rn2.w);
                    const float m4 = __uint_as_float(rn3.x), m5 = __uint_as_float(rn3.y), m6 = __uint_as_float(rn3.z), m7 = __uint_as_float(rn3.w);
                    const float m8 = __uint_as_float(rn4.x), m9 = __uint_as_float(rn4.y), m10 = __uint_as_float(rn4.z), m11 = __uint_as_float(rn4.w);
                    ox = ((m0 * s.ox + m1 * s.oy) + m2 * s.oz) + m3; oy = ((m4 * s.ox + m5 * s.oy) + m6 * s.oz) + m7; oz = ((m8 * s.ox + m9 * s.oy) + m10 * s.oz) + m11;
                    dx = (m0 * s.dx + m1 * s.dy) + m2 * s.dz; dy = (m4 * s.dx + m5 * s.dy) + m6 * s.dz; dz = (m8 * s.dx + m9 * s.dy) + m10 * s.dz;
                }
                // The object-space ray against the BLAS's bounding sphere (words 0-2: centre, word 7: radius, negative: none) -- the
                // instance's box in the top level is the box of that sphere under a rotation nobody knows in advance, and half the rays
                // that cross such a box miss the sphere.  Culling only, with slack for the rounding of every term: misses the line of
                // the ray by more than the radius, or starts outside and points away.
                const float R = __uint_as_float(rn1.w);
                const float cx = ox - __uint_as_float(rn0.x), cy = oy - __uint_as_float(rn0.y), cz = oz - __uint_as_float(rn0.z);
                const float cc = fmaf(cx, cx, fmaf(cy, cy, cz * cz)), aa = fmaf(dx, dx, fmaf(dy, dy, dz * dz)), b = fmaf(cx, dx, fmaf(cy, dy, cz * dz));
                const float R2 = R * R * 1.0001f, ca = cc * aa;
                // (branch-free on purpose, & and | instead of && and ||: with a branch on R >= 0 inside this block hipcc 7.2 carries child.x and
                // inst_cur of the block below through the registers it also uses for cc and b here, and the lanes that took the branch
                // entered node 0 instead of their BLAS, for ever -- found in the ISA, tools/debug_two_level.py)
                const bool beside = fmaf(-b, b, ca) > fmaf(R2, aa, 4e-6f * ca), behind = (b > 0.0f) & (cc > fmaf(4e-6f, cc, R2));
                if (HRT_SPHERE_CULL && ((R >= 0.0f) & (beside | behind))) enter = false;
            }
            if (enter) {
                TravState &s = ls;
                mb.t[tx] = s.ox; mb.u[tx] = s.oy; mb.v[tx] = s.oz;
                mb.prim[tx] = __float_as_uint(s.dx); mb.inst[tx] = __float_as_uint(s.dy); mb.pending[tx] = __float_as_uint(s.dz);
                park_idx[tx] = s.idx; park_idy[tx] = s.idy; park_idz[tx] = s.idz; park_oct[tx] = s.oct_inv4;
                inst_cur = rn1.y;
                s.ox = ox; s.oy = oy; s.oz = oz; s.dx = dx; s.dy = dy; s.dz = dz;
                s.idx = safe_rcp_dir<false>(dx); s.idy = safe_rcp_dir<false>(dy); s.idz = safe_rcp_dir<false>(dz);
                if (kSlabInterval01) slab_cap_rcp(s.idx, s.idy, s.idz);      // (bt stays the world ray's: the parameter is shared)
                const uint32_t oct = (dx < 0.0f ? 4u : 0u) | (dy < 0.0f ? 2u : 0u) | (dz < 0.0f ? 1u : 0u);
                s.oct_inv4 = (7u - oct) * 0x01010101u;
                child = make_uint2(rn1.x, 0x01000000u);      // one child, no inner-mask bits: the pick below is child base + 0 = the BLAS's root
            }
        }
        return enter;
    }
    // after the bookkeeping: frames begin and end
    __device__ __forceinline__ bool switch_frames(bool enter, bool done, bool hit_any, LeanLane &L, const Mailboxes &mb, uint2 (*nodes)[kTraverseBlock], uint32_t tx, uint32_t lane) {
        // in: the frame starts above what the lane holds (siblings still in hand have just been pushed, step 2 of the sequence)
        if (enter) { frame = (uint32_t)L.base | ((uint32_t)L.nsp << 8); L.base = L.nsp; }
        // out: the frame is empty -- nothing in hand, on the node stack above `base`, or in the leaf stack -- but the ray is not done
        const bool leave = done && !hit_any && inst_cur != kNoWork;
        if (__ballot(leave) != 0ull) {
            if (leave) {
                TravState &s = L.s;
                s.ox = mb.t[tx]; s.oy = mb.u[tx]; s.oz = mb.v[tx];
                s.dx = __uint_as_float(mb.prim[tx]); s.dy = __uint_as_float(mb.inst[tx]); s.dz = __uint_as_float(mb.pending[tx]);
                s.idx = park_idx[tx]; s.idy = park_idy[tx]; s.idz = park_idz[tx]; s.oct_inv4 = park_oct[tx];
                inst_cur = kNoWork;
                L.base = (int)(frame & 0xffu); L.nsp = (int)(frame >> 8);
                if (L.nsp != L.base) { --L.nsp; s.cur = nodes[L.nsp][lane]; }      // (only groups with hits are ever pushed)
                if (s.cur.y > 0x00ffffffu) { lean_pick_node(L); done = false; }
            }
        }
        return done;
    }
};

// kReuse (HRT_CTX_REUSE_PRIMARY): the reference's raygen has no pixel jitter (Shader.cu:249-261), so the primary ray of a pixel -- and its
// hit -- is the same for every sample.  The first sample a launch takes of a pixel traces it and leaves the hit record in the lane's slot of
// `primary_cache`; the later ones are shaded from there (same record, same shading, same random numbers: the same bits) and only their
// bounces are traversed.  Rays that are not traversed are not counted.  A separate instantiation, like kInstanced.
#ifndef HRT_FUSED_WAVES_PER_SIMD
#define HRT_FUSED_WAVES_PER_SIMD 4      // 128 VGPRs, the probe launch's clock spilled; 5 waves (96 VGPRs, 95 spilled around the shading): 2560 against 3122 Mrays/s
#endif
#ifndef HRT_INST_WAVES_PER_SIMD
#define HRT_INST_WAVES_PER_SIMD 3       // the kInstanced instantiation: 160 VGPRs, nothing spilled, 12 waves per CU (at 4 waves per SIMD it spills 47 registers around
                                        // the shading: 2 % slower on both particle clouds, profiles/r04_two_level_sweep.txt)
#endif
// The kernel's arguments as the regeneration reads them: straight from the kernel-argument segment, with scalar loads (s_load_dword*, the
// scalar cache) where a value is used.  Read through the by-value parameter the 108 dwords are loaded at the kernel's entry and stay live
// across the traversal loop, which has no scalar register to spare: hipcc spilled them into VGPR lanes (69 SGPRs in k_path_blocks<false>)
// and the regeneration fetched them back with v_readlane_b32, 16 at a time to use two or three.  The empty asm hides from the compiler
// that this is the memory the parameter came from, so it neither merges these loads with the entry's nor hoists them over the loop.
// REQUIRES the TraverseArgs to be the kernel's only explicit argument, at offset 0 of the segment (k_fused, k_path_blocks).
__device__ __forceinline__ const TraverseArgs &kernarg_traverse_args() {
    auto p = __builtin_amdgcn_kernarg_segment_ptr();           // (a pointer into the constant address space, address_space(4))
    asm volatile("" : "+s"(p));
    return *(const TraverseArgs *)p;
}

// The kernel's body: k_fused below, and -- kBlocks -- k_path_blocks, which hands pixels out in sample blocks (path_lane.h).  A kernel of its own
// because the hand-over costs the regeneration spilled registers, which the launches without blocks need not pay.
// `a`: the kernel's only argument (see kernarg_traverse_args); what the traversal loop consumes comes from it, the regeneration's
// constants from the segment.
// kCapture: k_path_capture (fused_capture.hip) -- every pixel's primary hit is left in frame order as well (path_lane.h: path_finish).
// kOneGroup: k_path_one (fused_one.hip) -- a block render of triangles of ONE instance: every hit is instance 0's, so the regeneration reads
// entry 0 of the per-instance tables with scalar loads and keeps no albedo chain (path_lane.h: path_finish), and the loop's primitive test
// decides ties by the primitive id alone (trav_common.h: test_prim_ray).
// kRestart: k_path_restart (fused_restart.hip) -- k_path_one whose repeat primary rays, which already start inside a window under their known hit,
// also start at the NODE whose leaf slot holds that hit's record instead of at the root (path_lane.h: path_finish).
// kCounts: k_path_counts (fused_counts.hip) -- every pixel takes its own number of samples and continues a sum the caller keeps (path_lane.h).
// kDirect: k_path_direct (fused_direct.hip) -- k_path_idle whose repeat primary rays test their known hit's record in the regeneration that makes
// them and never enter the loop: the regeneration block in its five-step order (below, at `finished`); the loop is untouched.
template <class V>
__device__ __forceinline__ void fused_body(const TraverseArgs &a) {
    static_assert(kTraverseBlock == 64, "one wave per workgroup: the stacks are per wave");
    static_assert(path_variant_checked<V>(), "trav_common.h: the constraints between a variant's flags");
    // kSeed: the hit distance the lane's pixel last found along its primary ray (path_lane.h), read once per sample: a word of LDS, so that
    // its register is the ray's TravState::tlo.  (One-level kernels: 9984 + 256 = 10240 bytes, still 16 waves per CU.)
    __shared__ float s_seed[kTraverseBlock];
    __shared__ uint2 s_nodes[kNodeStackLds][kTraverseBlock];     // sibling groups: one per tree level (hrt_api.cpp sends deeper trees to k_traverse)
    __shared__ uint2 s_leaves[kLeafStackLds][kTraverseBlock];    // leaf groups
    // tail splitting: one mailbox per lane that owns a split ray (indexed by its home lane) collects the pieces' hits
    __shared__ float s_mb_t[kTraverseBlock], s_mb_u[kTraverseBlock], s_mb_v[kTraverseBlock];
    __shared__ uint32_t s_mb_prim[kTraverseBlock], s_mb_inst[kTraverseBlock], s_mb_pending[kTraverseBlock];
    __shared__ uint32_t s_pair[kTraverseBlock];
    // kInstanced: the rest of a world ray that waits while its lane is inside an instance (reciprocals, octant)
    __shared__ float s_park_idx[kTraverseBlock], s_park_idy[kTraverseBlock], s_park_idz[kTraverseBlock];
    __shared__ uint32_t s_park_oct[kTraverseBlock];

    const uint32_t n_pixels = a.path.n_tile_pixels;
    const char *__restrict__ node_bytes = reinterpret_cast<const char *>(a.nodes);
    const char *__restrict__ prim_bytes = reinterpret_cast<const char *>(a.prims);
    const float tmin = a.tmin, tmax_ray = a.tmax;
    const uint32_t leaf_hold = a.leaf_hold >= 1 && a.leaf_hold <= 4 ? (uint32_t)a.leaf_hold : 4u;      // (a lane that could never take a node would never finish)
    // the traversal loop ends once at least refill_threshold lanes are idle -- or all of them: at most max_alive lanes alive
    const uint32_t max_alive = (uint32_t)a.refill_threshold >= 64u ? 0u : 64u - (uint32_t)a.refill_threshold;
    const uint32_t tx = threadIdx.x;
    const uint32_t ldsn = (uint32_t)reinterpret_cast<uintptr_t>(&s_nodes[0][tx]), ldsl = (uint32_t)reinterpret_cast<uintptr_t>(&s_leaves[0][tx]);

    const Mailboxes mb{s_mb_t, s_mb_u, s_mb_v, s_mb_prim, s_mb_inst, s_mb_pending, s_pair};
    // kRestart: the node the lane's pixel's next primary ray starts at (0: the root), a word per lane like the seed.  It lives in the mailboxes'
    // `inst` array, which a one-group kernel only ever filled with zeros and which the kRestart forms of the tail-splitting blocks leave alone.
    [[maybe_unused]] uint32_t *const s_restart = s_mb_inst;

    std::conditional_t<V::kInstanced, InstLane, NoInstLane> I;
    if constexpr (V::kInstanced) { I.park_idx = s_park_idx; I.park_idy = s_park_idy; I.park_idz = s_park_idz; I.park_oct = s_park_oct; }

    LeanLane L;
    lean_idle(L, tmax_ray, tmin);
    LaneFlags F;                            // alive / waiting / any / shared: trav_loop.h
    F.home = tx;
    bool exhausted = false;                 // wave-uniform: no pixels left to start

    std::conditional_t<V::kCounts, CountsLane, PathLane> P;      // the lane's pixel: path_lane.h
    uint32_t chain[4] = {0u, 0u, 0u, 0u};   // ... and the albedo chain of its path (kOneGroup: never written, never read)
    LaneStats stats;

    // the wave's slice of the tile: [wbeg, wend); slices of fetch_chunk pixels are handed out by kFetchShards counters
    uint32_t wbeg = 0, wend = 0, kstart = 0;
    const uint32_t home_shard = blockIdx.x & (kFetchShards - 1);
    [[maybe_unused]] BlockSlice B;                  // (kBlocks) the item the wave holds

    [[maybe_unused]] bool force_regen = false;      // (kReuse, wave-uniform)
    [[maybe_unused]] bool cached = false;           // (kReuse) this lane waits to be shaded with its pixel's cached primary hit
    for (;;) {
        const uint64_t idle = ~F.alive;
        const uint32_t n_idle = (uint32_t)__popcll(idle);
        // ---- regenerate: shade finished rays in place, start the next sample / pixel ----
        // (once the tile is used up the lanes without a pixel stay idle and the render ends with the slowest pixels' sample chains:
        // what counts then is how soon a finished ray's successor starts, against what a regeneration costs the rays still under
        // way -- a dozen waiting rays, or nothing else left to do: 1/8 of the C4 frame 142 ms with 1, 129 ms with 8 to 16)
        if (force_regen || idle == ~0ull || (exhausted ? (uint32_t)__popcll(F.waiting) >= (uint32_t)a.tail_regen : n_idle >= (uint32_t)a.refill_threshold)) {
            stats.regeneration();
            __builtin_amdgcn_s_setprio(HRT_PRIO_REGEN);
            const TraverseArgs &a = kernarg_traverse_args();      // (hides the parameter on purpose: nothing in this block reads the entry's copy)
            // (Tried for kBlocks: the block's constants -- samples, tmax, the seed's level, the schedule, the tables' and the hand-over's bases --
            // made to exist here by an empty asm with them as inputs, so that their loads go out back to back behind one wait: 33 -> 16
            // s_waitcnt lgkmcnt(0) in the block, nothing spilled, and 0.1 % SLOWER in five of five alternating runs, profiles/r23_block_regen.txt.)
            PathStep st;                            // st.launch: this lane starts the ray (st.ro, st.rd) below
            [[maybe_unused]] bool reshade = false;
            [[maybe_unused]] const bool was_forced = force_regen;
            force_regen = false;
            const uint64_t finished = F.waiting & ~F.alive;
            F.waiting &= F.alive;
            // kDirect (k_path_direct; DESIGN.md section 2.1 "The record tested where the ray is made"): the block in the order
            //   (a) what ends a path  (b) path_take  (c) the primary rays, and their records' tests  (d) the scatter, once  (e) the launch
            // A lane whose path ends here and whose pixel goes on wants the pixel's primary ray again: the same ray, which a complete walk has
            // shown to end in the hit accepted from record R (s_restart: the lane's word holds R, path_lane.h) -- no primitive computes a
            // smaller (t, primitive id), and the canonical test of R with the identical ray recomputes the identical t, u, v.  So (c) tests R alone,
            // with the culling bound at the seed as the loop would have it, and an accepted test leaves the lane with px_depth == 1 and the hit
            // in L.s: it is shaded in (d), together with the lanes whose rays came back from the loop with a hit, and launches its bounce.  The
            // ray is counted (path_count_ray), fetches its primitive and is decided by the canonical test against the launch's tmin and tmax;
            // it never enters the loop and never waits.  A test that does not accept -- by the argument it cannot happen -- launches the ray
            // from the root, bounded by seed and window, as k_path_idle would.  R's 48 bytes are asked for here, at the top, by the lanes that may
            // come to test them -- a record, and a finished bounce that is a miss or at the depth limit -- and waited for in (c).
            [[maybe_unused]] bool shade = false, may_test = false;
            [[maybe_unused]] uint32_t rec = kNoWork;
            // (the record's words the one-group test reads: A with the primitive id, and three floats each of B and C -- a fourth word that nobody
            // reads is a register the compiler hands out again at once, and then waits for the load in front of whatever it put there)
            typedef float f32x3 __attribute__((ext_vector_type(3)));
            [[maybe_unused]] f32x4 ra;
            [[maybe_unused]] f32x3 rb, rc;
            if constexpr (V::kDirect) {
                asm volatile("" : "=v"(ra), "=v"(rb), "=v"(rc));        // ("defined" without an instruction, like the loop's landing registers)
                rec = s_restart[tx];
                const bool ends_path = lane_bit(finished) && (L.s.bprim == kMissPrim || P.px_depth >= kRayTraceDepth);
                shade = lane_bit(finished) && !ends_path;
                may_test = ends_path && P.px_depth > 1u && rec != kNoWork;      // (a primary ray that ends its path is a miss: it leaves no record)
                if (may_test) {
                    typedef const __attribute__((address_space(1))) f32x4 *global_f32x4;
                    typedef const __attribute__((address_space(1))) f32x3 *global_f32x3;
                    const global_f32x4 rp = (global_f32x4)reinterpret_cast<const f32x4 *>(prim_bytes + rec * a.prim_stride);       // (32-bit byte offsets, as in the loop)
                    ra = rp[0]; rb = *(global_f32x3)(rp + 1); rc = *(global_f32x3)(rp + 2);
                }
                stats.finished_primary(lane_bit(finished) && P.px_depth == 1u && L.s.bprim == kMissPrim);
                [[maybe_unused]] const uint32_t sample_was = P.px_sample;        // (the instrumented build's)
                if (lane_bit(finished)) {
                    // (s.tlo > tmin: the walk began inside a seed's window -- a miss from there does not take the block, path_lane.h)
                    const TravState &s = L.s;
                    st = path_finish<V, PathLane, 1>(P, chain, a, mk3(s.ox, s.oy, s.oz), mk3(s.dx, s.dy, s.dz), lean_miss_t(s.bt, s.bprim, a.tmax), s.bu, s.bv, s.bprim, 0u,
                                                     s_seed + tx, s.binst, s.tlo > tmin, s_restart + tx);
                }
                stats.fast_forwarded(ends_path && P.px_sample > sample_was ? P.px_sample - sample_was - 1u : 0u);
                may_test = may_test && st.want_primary;      // (the pixel goes on in this lane: a pixel that path_take hands out has no record)
            } else
            if (lane_bit(finished)) {
                const TravState &s = L.s;
                // the finished ray and what it hit
                V3 o = mk3(s.ox, s.oy, s.oz), d = mk3(s.dx, s.dy, s.dz);
                float bt = lean_miss_t(s.bt, s.bprim, a.tmax), bu = s.bu, bv = s.bv; uint32_t bprim = s.bprim, binst = V::kOneGroup ? 0u : s.binst;      // (a miss says tmax)
                if constexpr (V::kReuse) {
                    float4 *slot = a.path.primary_cache + 2u * (blockIdx.x * kTraverseBlock + tx);
                    if (cached) {                   // ... or, for a primary ray that was not traversed again, what the pixel's first sample found
                        const float4 c0 = slot[0]; const float4 c1 = slot[1];
                        o = mk3(a.path.center[0], a.path.center[1], a.path.center[2]); d = mk3(P.px_pdx, P.px_pdy, P.px_pdz);
                        bt = c0.x; bu = c0.y; bv = c0.z; bprim = __float_as_uint(c0.w); binst = __float_as_uint(c1.x);
                        cached = false;
                    } else if (!a.path.trace_rays && P.px_depth == 1u && P.px_sample == 0u) {      // the primary hit of the pixel's first sample in this launch
                        slot[0] = make_float4(bt, bu, bv, __uint_as_float(bprim)); slot[1] = make_float4(__uint_as_float(binst), 0.0f, 0.0f, 0.0f);
                    }
                }
                // (kRestart: s.binst is the record the hit was accepted from, and the walk had a window if it began above the launch's tmin)
                st = path_finish<V>(P, chain, a, o, d, bt, bu, bv, bprim, binst, s_seed + tx, s.binst, s.tlo > tmin, s_restart + tx);
            }
            exhausted = path_take<V>(P, st, a, n_pixels, !lane_bit(F.alive) && !P.have_pixel && !st.want_primary && !st.launch, wbeg, wend, kstart, exhausted, home_shard, tx, &B, s_seed + tx, s_restart + tx);
            stats.drained(exhausted);
            if (st.want_primary) {
                bool from_cache = false;
                if constexpr (V::kReuse) from_cache = !a.path.trace_rays && P.px_sample > 0u;
                if (from_cache) {
                    // a pixel's later primary rays are not traversed again: the lane waits for its shading as if the ray had just finished (the hit is in the cache)
                    P.px_depth = 1u; cached = true; reshade = true;      // (F.waiting: below)
                } else {
                    const PathRay r = path_primary<V, false>(P, a);
                    st.ro = r.o; st.rd = r.d; st.launch = true;
                }
            }
            [[maybe_unused]] bool stat_primary = false, stat_quick = false, stat_direct = false;        // (the instrumented build's: LaneStats::started)
            if constexpr (V::kDirect) {
                // (c) the record's test, in place: the loop's inline function under the loop's `fp contract(off)`, on the ray path_primary has
                // just made, with what lean_start would leave as the best hit -- the seed as the culling bound, no primitive
                if (may_test && a.seed_primary >= 2 && s_seed[tx] < tmax_ray) {
                    TravState &s = L.s;
                    s.bt = s_seed[tx]; s.bu = 0.0f; s.bv = 0.0f; s.bprim = kMissPrim; s.binst = kMissPrim;
                    const bool accepted = test_prim_ray<V>(make_float4(ra.x, ra.y, ra.z, ra.w), make_float4(rb.x, rb.y, rb.z, 0.0f), make_float4(rc.x, rc.y, rc.z, 0.0f), s, st.ro, st.rd,
                                                           tmin, tmax_ray, a.inst_inv, a.inst_identity, 0u, true, rec);
                    if (accepted) {
                        (void)path_count_ray(P);        // (px_depth == 1: a closest-hit ray)
                        s.ox = st.ro.x; s.oy = st.ro.y; s.oz = st.ro.z; s.dx = st.rd.x; s.dy = st.rd.y; s.dz = st.rd.z;
                        st.launch = false; shade = true; stat_direct = true;
                    }
                }
                // (d) the scatter, once: the finished lanes with a hit below the depth limit and the lanes whose test has just accepted
                if (shade) {
                    const TravState &s = L.s;
                    st = path_finish<V, PathLane, 2>(P, chain, a, mk3(s.ox, s.oy, s.oz), mk3(s.dx, s.dy, s.dz), s.bt, s.bu, s.bv, s.bprim, 0u);
                }
            }
            bool any_hit = false;
            if (st.launch) {
                any_hit = path_count_ray(P);
                // a primary ray of a pixel the lane already holds starts bounded at the hit its previous sample found (s_seed; tmax after
                // path_take -- or, kBlocks, what the pixel's previous block left for it, path_lane.h: handover_load):
                // counted and walked from the root like any other, the primitive test keeps the launch's tmin and tmax.  At level
                // 2 it is bounded from below as well: the same ray has found nothing before that hit, so the node step's interval begins a
                // window (trav_common.h: kSeedWindow) below it.  Every other ray -- a bounce, a first sample, after a miss (the seed says
                // tmax), a caller's ray -- begins at the launch's tmin.
                // kRestart: ... and a ray that got a window starts at the node its predecessor left for it (s_restart: the root unless that ray
                // accepted its hit itself, inside the same window) -- still launched, counted and decided by the canonical primitive test.
                float hi = tmax_ray, lo = tmin;
                [[maybe_unused]] uint32_t first_node = 0u;
                if constexpr (V::kSeed) {
                    if (st.want_primary) {
                        hi = s_seed[tx];
                        if (a.seed_primary >= 2 && hi < tmax_ray) lo = seed_window_lo(st.rd, hi, tmin);
                        // (kDirect: the word holds a record, and a primary ray that is launched at all walks from the root)
                        if constexpr (V::kRestart && !V::kDirect) { if (a.seed_primary >= 2 && hi < tmax_ray) first_node = s_restart[tx]; }
                    }
                }
                stat_primary = st.want_primary; stat_quick = st.want_primary && first_node != 0u;
                lean_start(L, st.ro, st.rd, hi, lo);
                if constexpr (V::kRestart) L.nidx = first_node;
                if constexpr (V::kInstanced) I.inst_cur = kNoWork;      // (an any-hit ray may have ended inside an instance)
            }
            // the flags are wave masks (trav_loop.h): the lanes that have started a ray, and those that wait with a cached hit
            const uint64_t launched = __ballot(st.launch);
            stats.started(stat_primary, stat_quick, stat_direct, launched);
            F.alive |= launched; F.any = (F.any & ~launched) | __ballot(any_hit);
            if constexpr (V::kReuse) F.waiting |= __ballot(reshade);
            // kReuse: lanes that have just taken their primary hit from the cache are shaded in a second regeneration, at once, so that
            // their bounces start together with the other lanes' rays (one extra round, not more: the others are waiting)
            if constexpr (V::kReuse) { if (!was_forced && __ballot(reshade) != 0ull) { force_regen = true; continue; } }
            // s_waitcnt lgkmcnt(0): no scalar load of this block is under way when the traversal loop is entered.  A load issued in front of a
            // branch that skips its wait counts as pending to the compiler, which then waits INSIDE the loop wherever the loop reuses the
            // load's register (two s_waitcnt in the sphere kernels' loops, as the registers happened to fall)
            // kBlocks: ... and no vector load either (vmcnt(0) as well).  The words of a hand-over (path_lane.h: handover_load) are not needed before
            // the lane's next regeneration, so with nothing else in the block waiting for them the compiler lets them fly into the loop
            // and waits at the loop's header, in every iteration; here they have had the pixel's set-up and the ray's start to arrive
            if constexpr (V::kBlocks) __builtin_amdgcn_s_waitcnt(0x0070);
            else __builtin_amdgcn_s_waitcnt(0xc07f);
        }
        // the tile is used up and every lane has finished (nothing waits after a full regeneration -- but, kReuse, a lane with a cached hit to shade:
        // an empty pass through the loop below brings it back here)
        if ((V::kReuse ? F.alive | F.waiting : F.alive) == 0ull) {
            bool leave = true;
            if constexpr (V::kBlocks) leave = B.need == 0u;
            if (leave) break;
            // Sample blocks: the wave holds an item whose predecessor is still under way and has nothing else to do.  It must not leave
            // (the item's pixels would never be rendered), so it looks again after a short sleep.  This cannot hang, PROVIDED every one of
            // the kFetchShards counters is the home of a wave (grid >= kFetchShards: render_fused hands out blocks on no smaller grid).  The
            // counters do not hand the items out in order of their numbers -- a wave stays with its home counter until that is drained --
            // so "the predecessor was fetched before" is NOT what the argument rests on.  Suppose all waves were stuck, and let i be the
            // lowest-numbered item whose pixels have not all ended their block; every item below i is done, i's predecessor among them.
            //   i has been fetched: the wave that holds it finds it ready at its next look and its free lanes take i's pixels.
            //   i has not: it is item c of counter s = i % kFetchShards; the items of s below it are done, hence fetched, so the counter
            //     stands at c exactly.  A wave whose home is s has never found s drained, so whatever it has fetched came from s, is
            //     numbered below i and is done: it holds nothing, its lanes are free, and its next regeneration fetches i.
            // Either way some wave is not stuck (the grid is sized to what is resident; were it not, workgroups 0 to kFetchShards - 1, one
            // home wave per counter, are the first to be).  (With fewer waves than counters the second case fails: the only wave of an 8 x 6 frame
            // takes item 0, then item 8 of its home counter -- pass 2 of a slice whose passes 0 and 1 are items of counters nobody
            // visits.)  None of this asks how many samples a pass has: the schedule (device_types.h: block_first -- uniform blocks, or
            // tapered ones that start large and end small) only says at which sample a lane's hold on its pixel begins and ends.  What the
            // argument uses is that every pixel of a slice ends exactly one block per pass -- at a boundary of the schedule, or, the last
            // pass, where the launch's samples end -- so that item (b, q) is done when the slice's word stands at (b + 1) x its pixels and
            // ready when it stands at b x its pixels; the numbering of the items, the home counters and the floor of 8 waves are as they
            // were.  An empty pass through the loop below brings the wave back to its regeneration: a `continue` here costs the
            // kernel a hundred spilled registers.
            __builtin_amdgcn_s_sleep(32);
        }

        // ---- traverse until enough lanes have finished to make a regeneration worthwhile: trav_loop.h; the copy with tail splitting
        //      and the drained phase's exit rule runs once the tile is used up ----
        if (exhausted) {
            stats.tail_begin();
            traverse_to_regen<V, true>(L, F, I, stats, mb, s_nodes, s_leaves, ldsn, ldsl, a, node_bytes, prim_bytes, tmin, tmax_ray, leaf_hold, max_alive, !P.have_pixel, tx);
            stats.tail_end();
            // kRestart: s_waitcnt lgkmcnt(0) -- the drained copy's last block (tail_retire) takes a merged hit out of the mailboxes, and as the
            // registers fall in this kernel the compiler lets those LDS reads fly out of that loop.  To the compiler `exhausted` may turn false
            // again, so it then waits for them INSIDE the other copy of the loop, which this path can never reach: two s_waitcnt per iteration.
            if constexpr (V::kRestart) __builtin_amdgcn_s_waitcnt(0xc07f);
        }
        else traverse_to_regen<V, false>(L, F, I, stats, mb, s_nodes, s_leaves, ldsn, ldsl, a, node_bytes, prim_bytes, tmin, tmax_ray, leaf_hold, max_alive, !P.have_pixel, tx);
    }
    const TraverseArgs &k = kernarg_traverse_args();          // (the counters' addresses need not live in registers until here)
    stats.report(k.path.rays_closest, tx);
    path_report_rays(P, k, tx);
}

}  // namespace hrt
