// path_lane.h -- the regeneration phase of a path kernel, ONCE, for k_fused (fused.hip) and k_traverse<.., FUSED> (kernels.hip): a lane
// OWNS a pixel and carries its path state in registers (PathLane); when its ray has finished it is shaded in place and the next
// ray -- the bounce, the next sample's primary ray, the next pixel's -- starts in the same lane.  Three steps, in the order a
// regeneration runs them:
//   path_finish    what becomes of a finished ray: the hrt_trace_rays record, the end of a path, or a bounce
//   path_take      lanes without a pixel take the next ones of the wave's slice of the tile
//   path_primary   the ray a lane that wants a primary ray starts
// and path_count_ray / path_report_rays for the ray counters.  The kernels keep what is theirs: WHEN a regeneration happens, how a
// ray is started in their traversal state, k_fused's primary-hit cache (kReuse) and its instance state.
// Everything is inlined; PathLane is a plain struct of scalars, passed by reference, results come back by value, so that the state
// stays in registers exactly as when the kernels spelled it out (k_fused has none to spare: check the ISA after any change here).
#pragma once
#include "trav_common.h"

namespace hrt {

// the lane's pixel (hrt_trace_rays on a path kernel: a caller's ray, px_local its index).  Scalars only: the albedo chain of the path, an
// array indexed by the depth, is a variable of its own in the kernels (`uint32_t chain[4]`, path_finish's px_chain) -- as a member it
// would keep the whole struct in scratch memory.
struct PathLane {
    bool have_pixel = false, px_first = true;
    uint32_t px_local = 0u, px_tid = 0u, px_sample = 0u, px_depth = 1u;
    float px_ax = 0.0f, px_ay = 0.0f, px_az = 0.0f;
    uint32_t px_t0 = 0u;                                    // probe launch: clock at the pixel's start
    float px_pdx = 0.0f, px_pdy = 0.0f, px_pdz = 1.0f;      // the pixel's primary direction: the same for every sample (no jitter, Shader.cu:249-261)
    Xorwow px_rng{};
    uint32_t px_rays_closest = 0u, px_rays_any = 0u;
    // (The seed -- the culling bound the pixel's next primary ray may start with: the hit distance its last one found, exactly as found, or
    // tmax (none: a miss, a pixel just taken, HRT_SEED_PRIMARY=0) -- is NOT here: it is read once per sample, so it waits in the lane's
    // word of the wave's LDS (`seed` of path_finish / path_take; fused_body.h: s_seed) and the register it had is the traversal's
    // TravState::tlo.  Every sample's primary ray is the same ray, so it ends in the same hit again: a complete closest-hit walk from the
    // root that never enters what lies behind that hit nor, with the window, what ends before it.  Reset by
    // path_take, so it never outlives the launch's hold on the pixel -- the lane's, or, in a render by sample blocks, that of the lanes
    // that hand the pixel on within one launch (handover_store / handover_load); kept by the kernels that seed (kSeed: fused_body.h) only.)
};

// kCounts (k_path_counts, fused_counts.hip): what the lane of that kernel carries besides.  A type of its own, which path_finish and path_take
// take as their lane's: one more member of PathLane, even one that no other kernel touches, lets the registers of all of them fall differently.
struct CountsLane : PathLane {
    float px_aw = 0.0f;         // the sum of the samples' squared luminances: the w of the pixel's 16-byte sum
    bool gave_up = false;       // path_take: the pixel this lane drew has count 0 and is given up already
};

// what a lane does next: `launch` the ray (ro, rd), or -- `want_primary` -- a primary ray that path_primary has yet to make
struct PathStep {
    bool launch = false, want_primary = false;
    V3 ro = {0.0f, 0.0f, 0.0f}, rd = {0.0f, 0.0f, 1.0f};
};

// Sample blocks (PathArgs::sample_block = K > 0): the work item is not a slice of pixels with all their samples but
// (pass b, slice q) = samples [first(b), first(b + 1)) of the slice's pixels, first(b) = b K or a tapered schedule that starts on large
// blocks and ends on small ones (device_types.h: block_first); the counters hand all items of pass 0 out, then pass 1's, ... so
// that only the last pass has an end-of-frame tail, its share of a whole pixel's -- while the large blocks keep the hand-overs few.  A lane that finishes a block leaves sum and RNG state
// where a finished pixel's go and the lane that takes the pixel's next block continues from there: the same additions in the same
// order from the same stream, the same bits.  What a wave knows about the item it holds (wave-uniform):
struct BlockSlice {
    uint32_t pass = 0u;         // b
    uint32_t slice = 0u;        // q
    uint32_t need = 0u;         // what block_progress[q] must have reached before the item's pixels may start (0: nothing to wait for)
};

// The hand-over between passes crosses CUs and XCDs (whose L2s are not coherent with one another) and must not cost the tree its place
// in the caches, so no fence writes back or invalidates anything:
//   the lane that ends a block   stores the 40 bytes write-through (relaxed agent-scope atomic stores: global_store_dwordx2 ... sc1), the wave
//                                waits for them (s_waitcnt vmcnt(0)), then the lane adds 1 to the slice's progress word (agent-scope atomic add:
//                                global_atomic_add_u32 ... sc1);
//   the wave that holds (b, q)   reads the progress word past L1 (relaxed agent-scope atomic load: global_load_dword ... sc1) and, once it says that all
//                                pixels of (b - 1, q) are stored, its lanes load their 40 bytes past L1 as well (global_load_dwordx2 ... sc1).
// In block mode no other load or store touches those bytes inside a launch.
// x / d for a divisor the host knows, m = min(2^32 / d, 2^32 - 1): the product's high word is short by one at most (every x, every d >= 1)
__device__ __forceinline__ uint32_t div_magic(uint32_t x, uint32_t d, uint32_t m) { const uint32_t q = __umulhi(x, m); return x - q * d >= d ? q + 1u : q; }
__device__ __forceinline__ unsigned long long pack_u64(uint32_t lo, uint32_t hi) { return (unsigned long long)lo | ((unsigned long long)hi << 32); }
// The second half of the sum's 16 bytes is nobody's: k_finalize, the non-block take of a continued render and k_sum read x, y, z only.  It
// carries the pixel's seed (`seed`: the lane's LDS word, PathLane above) to the lane that takes the pixel's next block, whose first
// primary ray is the same ray from the same camera in the same launch; handover_load hands it back for the caller to believe (a pass
// b > 0) or not (pass 0: whatever is there comes from an earlier launch).
__device__ __forceinline__ void handover_store(const PathArgs &pa, const PathLane &P, uint32_t fetch_chunk, float seed = 0.0f) {
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(pa.accum + P.px_local), *st = reinterpret_cast<unsigned long long *>(pa.states + P.px_tid);
    __hip_atomic_store(acc, pack_u64(__float_as_uint(P.px_ax), __float_as_uint(P.px_ay)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(acc + 1, pack_u64(__float_as_uint(P.px_az), __float_as_uint(seed)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(st, pack_u64(P.px_rng.d, P.px_rng.v0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(st + 1, pack_u64(P.px_rng.v1, P.px_rng.v2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(st + 2, pack_u64(P.px_rng.v3, P.px_rng.v4), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // every store of the wave has been written through before any lane says so
    __hip_atomic_fetch_add(pa.block_progress + div_magic(P.px_local, fetch_chunk, pa.block_chunk_magic), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// (returns the word next to the sum's z, `none` where the sum is not read)
__device__ __forceinline__ float handover_load(const PathArgs &pa, PathLane &P, bool with_sum, float none = 0.0f) {
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(pa.accum + P.px_local), *st = reinterpret_cast<unsigned long long *>(pa.states + P.px_tid);
    const unsigned long long r0 = __hip_atomic_load(st, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), r1 = __hip_atomic_load(st + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                             r2 = __hip_atomic_load(st + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    P.px_rng.d = (uint32_t)r0; P.px_rng.v0 = (uint32_t)(r0 >> 32); P.px_rng.v1 = (uint32_t)r1; P.px_rng.v2 = (uint32_t)(r1 >> 32); P.px_rng.v3 = (uint32_t)r2; P.px_rng.v4 = (uint32_t)(r2 >> 32);
    if (with_sum) {
        const unsigned long long a0 = __hip_atomic_load(acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), a1 = __hip_atomic_load(acc + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        P.px_ax = __uint_as_float((uint32_t)a0); P.px_ay = __uint_as_float((uint32_t)(a0 >> 32)); P.px_az = __uint_as_float((uint32_t)a1);
        none = __uint_as_float((uint32_t)(a1 >> 32));
    }
    return none;
}

// fold_chain (trav_common.h) for a kernel that keeps the chain in registers (kBlocks): the loop there loads hitgroups[chain[k]] and waits,
// level by level, up to four round trips one behind the other, although all four addresses are known at once.  Here the albedos of
// the levels below the depth are all asked for first, then multiplied in in the loop's order, innermost bounce first: the same
// products in the same order, the same bits.
__device__ __forceinline__ V3 fold_chain_together(bool miss, const float *bg, const uint32_t (&chain)[4], uint32_t depth, const HitGroup *__restrict__ hitgroups) {
    static_assert(kRayTraceDepth <= 5u, "a path's chain has four entries");
    V3 r = miss ? mk3(bg[0], bg[1], bg[2]) : mk3(0.0f, 0.0f, 0.0f);
    float al[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        al[k][0] = al[k][1] = al[k][2] = 0.0f;
        if ((uint32_t)k + 1u < depth) {
            const global_floats ap = (global_floats)hitgroups[chain[k]].albedo;
            al[k][0] = ap[0]; al[k][1] = ap[1]; al[k][2] = ap[2];
        }
    }
#pragma unroll
    for (int k = 3; k >= 0; --k) {
        if ((uint32_t)k + 1u < depth) { r.x *= al[k][0]; r.y *= al[k][1]; r.z *= al[k][2]; }
    }
    return r;
}

// kOneGroup (k_path_one, fused_one.hip: every hit is instance 0's): the per-instance tables have one entry, the same for every lane, and it
// is read as such -- through the constant address space, with scalar loads (s_load_dword*) into scalar registers, where it is used.  The
// tables are written by the host before the launch and by nobody during it.
typedef const __attribute__((address_space(4))) HitGroup *constant_hitgroup;
typedef const __attribute__((address_space(4))) uint32_t *constant_words;
// fold_chain for a path all of whose bounces hit the one group: the albedo is asked for once and no chain is kept.  The same products in
// the same order as fold_chain_together makes of chain = {0, 0, 0, 0} (0 x inf, NaN and negative albedos included).
__device__ __forceinline__ V3 fold_chain_one(bool miss, const float *bg, uint32_t depth, const HitGroup *hitgroups) {
    static_assert(kRayTraceDepth <= 5u, "a path's chain has four entries");
    const constant_hitgroup hg = (constant_hitgroup)hitgroups;
    const float a0 = hg->albedo[0], a1 = hg->albedo[1], a2 = hg->albedo[2];
    V3 r = miss ? mk3(bg[0], bg[1], bg[2]) : mk3(0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int k = 3; k >= 0; --k) {
        if ((uint32_t)k + 1u < depth) { r.x *= a0; r.y *= a1; r.z *= a2; }
    }
    return r;
}

// A ray (o, d) has finished with the hit record (bt, bu, bv, bprim, binst).  The lane gives its pixel up (have_pixel = false: record or
// sum written), wants the next sample's primary ray, or launches the bounce.
// kReuse (k_fused's primary-hit cache): a primary ray that leaves the scene does so in every sample of the pixel.
// kBlocks: the instantiation knows sample blocks -- the lane's hold on its pixel also ends where a block does.
// kSeed: the kernel starts repeat primary rays at the lane's seed (`seed`: its word in LDS), so a finished primary ray records it (and path_take resets it).
// kCapture (k_path_capture, fused_capture.hip; HRT_CTX_CAPTURE_PRIMARY): the primary ray of the first sample the launch takes of a pixel
// leaves its hit record in frame order, in hrt_trace_rays' form (a miss: tmax, kMissPrim), where the denoiser's guide pass and
// hrt_primary_hits_get find it.  PathArgs::trace_tuvp / trace_inst are free in a render (trace_rays == NULL) and carry the two arrays.
// kOneGroup: see above -- `binst` is 0, `px_chain` is neither written nor read.
// kRestart (k_path_restart, fused_restart.hip; DESIGN.md section 4.1 "The start under the known hit"): a primary ray that ends in a hit leaves, in
// the lane's word `restart` of LDS, the node the pixel's next primary ray starts at instead of the root: leaf_parent[brec], the node whose
// leaf slot holds the record the hit was accepted from (`brec`; the table rides in PathArgs::slice_order, which a block render does not
// have).  Only where `restartable` -- the lane accepted the hit itself (brec != kNoWork) in a walk that had the window the next one will
// have, so that the node step of that node passes the slot again, bit for bit; everything else leaves 0, the root.  The table's load goes
// out in front of the normals', on the same round trip.
// kCounts (k_path_counts, fused_counts.hip; hrt_render_accumulate): every pixel takes a sample count of its own and continues a sum the caller
// keeps, in FRAME order.  Fields that are free in such a launch carry the arrays: PathArgs::accum the sums (xyz: radiance, w: squared luminances),
// trace_inst how many samples each sum holds on entry (0: the first sample is assigned), slice_order the counts (NULL: spp everywhere).
// The lane of such a kernel is a CountsLane (above): px_aw, the fourth accumulator next to px_ax / px_ay / px_az, and gave_up.
// A pixel of count c = min(counts[p], spp) starts at px_sample = spp - c, so that it ends where every pixel does, at px_sample >= spp, and
// the count needs no register; c == 0 is given up in path_take, before anything of it is loaded or stored.
// kDirect (k_path_direct, fused_direct.hip; DESIGN.md section 2.1 "The record tested where the ray is made"): the lane's word `restart` holds the
// RECORD a primary ray accepted its hit from (kNoWork: none -- a miss, or a hit that came out of a mailbox), not a node, and no table is read:
// the regeneration tests that record against the pixel's next primary ray where it makes the ray (fused_body.h).  Its block runs this function
// in two parts, with path_take and the primary rays between them: kPart 1, for every finished lane -- the seed, the record, and what ends a
// path (a lane whose ray goes on to be shaded comes back with nothing to do) -- and kPart 2, the shading branch alone, for the lanes that
// have a hit to shade: the finished ones and those whose record's test accepted.  kPart 0: all of it, one call, every other kernel.
// kPart 1 takes in `restartable` whether the finished ray's walk began inside a seed's window, and reads the miss block's switch (HRT_MISS_BLOCK)
// from PathArgs::trace_any, which a block render does not have (hrt_api.cpp: render_fused puts it there): a primary miss that had the launch's whole
// interval takes the rest of the lane's hold on the pixel, below.
typedef const __attribute__((address_space(1))) uint32_t *global_words;
template <class V, class Lane, int kPart = 0>
__device__ __forceinline__ PathStep path_finish(Lane &P, uint32_t (&px_chain)[4], const TraverseArgs &a, V3 o, V3 d, float bt, float bu, float bv, uint32_t bprim, uint32_t binst,
                                            [[maybe_unused]] float *seed = nullptr, [[maybe_unused]] uint32_t brec = 0u, [[maybe_unused]] bool restartable = false,
                                            [[maybe_unused]] uint32_t *restart = nullptr) {
    static_assert((kPart == 0) == !V::kDirect, "path_finish in two parts: k_path_direct's regeneration, and only that");
    PathStep st;
    const bool miss = bprim == kMissPrim;
    constexpr bool kEnds = kPart != 2, kShades = kPart != 1;      // which of the branches below this call has
    if constexpr (V::kSeed && kEnds) { if (P.px_depth == 1u && a.seed_primary) *seed = bt; }    // the pixel's primary ray (a miss says tmax: none; a caller's ray: its lane takes anew)
    if constexpr (V::kDirect && kEnds) { if (P.px_depth == 1u) *restart = miss ? kMissPrim : brec; }      // (kMissPrim is the word's "none", trav_lean.h: kNoWork)
    if constexpr (V::kCapture) {
        if (!a.path.trace_rays && P.px_depth == 1u && P.px_sample == 0u) {      // (the primary-hit cache's condition, fused_body.h)
            a.path.trace_tuvp[P.px_tid] = make_float4(bt, bu, bv, __uint_as_float(bprim));
            a.path.trace_inst[P.px_tid] = binst;
        }
    }
    // (kBlocks: a block render has no callers' rays, no cost probe and no slice order, and its sample_block is not 0 -- facts of the
    // instantiation, which path_launch_admitted (device_types.h) holds every launch to, so its regeneration neither loads nor tests them)
    if (!V::kBlocks && a.path.trace_rays) {           // hrt_trace_rays on this kernel: the "pixel" is a caller's ray, its hit record the result
        a.path.trace_tuvp[P.px_local] = make_float4(bt, bu, bv, __uint_as_float(bprim));
        a.path.trace_inst[P.px_local] = binst;
        P.have_pixel = false;
    } else if (kEnds && (miss || P.px_depth >= kRayTraceDepth)) {
        // the path ends: miss colour or black at the depth limit, folded through the albedo chain (Shader.cu:102-107, :236-238, :276-287)
        V3 r;
        if constexpr (V::kOneGroup) r = fold_chain_one(miss, a.path.bg, P.px_depth, a.path.hitgroups);
        else if constexpr (V::kBlocks) r = fold_chain_together(miss, a.path.bg, px_chain, P.px_depth, a.path.hitgroups);
        else r = fold_chain(miss, a.path.bg, px_chain, P.px_depth, a.path.hitgroups);
        if constexpr (V::kCounts) {
            // the sample's luminance, squared, joins its own sum by the radiance's rule: the first sample of a frame is assigned
            const float l = (0.2126f * r.x + 0.7152f * r.y) + 0.0722f * r.z;
            if (P.px_first) P.px_aw = l * l; else P.px_aw += l * l;
        }
        if (P.px_first) { P.px_ax = r.x; P.px_ay = r.y; P.px_az = r.z; P.px_first = false; }
        else { P.px_ax += r.x; P.px_ay += r.y; P.px_az += r.z; }
        ++P.px_sample;
        if constexpr (V::kReuse) {
            // a primary ray that leaves the scene: every sample of the pixel is the background colour, added one by one
            if (miss && P.px_depth == 1u && !a.path.slice_cost)
                for (; P.px_sample < a.path.spp; ++P.px_sample) { P.px_ax += r.x; P.px_ay += r.y; P.px_az += r.z; }
        }
        if (!V::kBlocks && a.path.slice_cost)     // probe launch: how long this pixel's sample took, start of its primary ray to here
            atomicAdd(a.path.slice_cost + P.px_local / a.fetch_chunk, ((uint32_t)__builtin_amdgcn_s_memtime() - P.px_t0) >> 4);
        bool ends = P.px_sample >= a.path.spp;
        if constexpr (V::kBlocks) {
            if (a.path.block_magic != 0u) {
                // ... or, uniform blocks, px_sample is a multiple of K: with M = min(2^32 / K, 2^32 - 1) the quotient is short by one at most, so
                // the remainder comes out as 0 or K exactly then (every px_sample, every K >= 1)
                const uint32_t rem = P.px_sample - __umulhi(P.px_sample, a.path.block_magic) * a.path.sample_block;
                ends = ends || rem == 0u || rem == a.path.sample_block;
            } else {
                // ... or the tapered schedule has a boundary there (device_types.h; no blocks, all three 0: never)
                ends = ends || block_ends(a.path.sample_block, a.path.block_min, a.path.block_taper_end, P.px_sample);
            }
        }
        if constexpr (V::kDirect) {
            // The miss block (HRT_MISS_BLOCK; DESIGN.md section 2.1 "A primary miss takes the rest of its block"): the pixel's primary ray has
            // walked the launch's whole interval from the root -- no seed bounded it, no window (`restartable`: path_finish's head) -- and left
            // the scene.  Every further sample's primary ray is the same ray (no jitter), a miss at depth 1 draws no random number and folds
            // to the same `r`, so the samples up to the end of the lane's hold are decided here: the same addends in the same order (n * r is
            // another float), each one counted as the closest-hit ray it stands for, none of them launched.  Where the hold ends is the test
            // above, as one function for the loop (device_types.h: hold_ends; hrt_sample_schedule holds both to the schedule's passes), and
            // nothing is carried over it: the next block's first primary ray walks again.  (A ray that comes back a miss from inside a seed's
            // window "cannot happen" and proves nothing: it goes on sample by sample.)
            if (miss && P.px_depth == 1u && !restartable && a.seed_primary >= 2 && a.path.trace_any != 0u) {
                while (!ends) {
                    P.px_ax += r.x; P.px_ay += r.y; P.px_az += r.z;
                    ++P.px_sample; ++P.px_rays_closest;
                    ends = hold_ends(a.path.spp, a.path.sample_block, a.path.block_magic, a.path.block_min, a.path.block_taper_end, P.px_sample);
                }
            }
        }
        if (ends) {
            if constexpr (V::kBlocks) {
                // (the seed travels with the pixel: what its last primary ray found, tmax after a miss or with HRT_SEED_PRIMARY=0)
                float carried = 0.0f;
                if constexpr (V::kSeed) carried = *seed;
                handover_store(a.path, P, a.fetch_chunk, carried);
            }
            else if constexpr (V::kCounts) {
                // the caller's sum, in frame order; how many samples it now holds is the launch's finalize kernel's to add (k_finalize_counts)
                a.path.accum[P.px_tid] = make_float4(P.px_ax, P.px_ay, P.px_az, P.px_aw);
                rng_store(a.path.states + P.px_tid, P.px_rng);
            }
            else {
                a.path.accum[P.px_local] = make_float4(P.px_ax, P.px_ay, P.px_az, 0.0f);
                rng_store(a.path.states + P.px_tid, P.px_rng);
            }
            P.have_pixel = false;
        } else st.want_primary = true;
    } else if constexpr (V::kOneGroup && !kShades) {
        // (kPart 1: this lane's hit is shaded by the block's second call)
    } else if constexpr (V::kOneGroup) {
        // entry 0 of both tables, in scalar registers: the normals' loads go out as soon as the pointer is there, and what the program is --
        // rough or metal, fuzz or none -- is the same in every lane, so scatter_programs' choices are the wave's
        const constant_hitgroup hp0 = (constant_hitgroup)a.path.hitgroups;
        HitGroup hg;
        hg.ptr0 = hp0->ptr0; hg.ptr1 = nullptr; hg.albedo[0] = hg.albedo[1] = hg.albedo[2] = 0.0f; hg.fuzz = hp0->fuzz;      // (what a triangle program reads)
        const uint32_t program = *(constant_words)a.path.inst_program;
        [[maybe_unused]] uint32_t node = 0u;
        if constexpr (V::kRestart && !V::kDirect) {
            // (no branch: every lane here loads -- entry 0 where it has nothing to look up -- and keeps the word or 0)
            const bool look = P.px_depth == 1u && restartable && brec != kMissPrim;
            node = ((global_words)a.path.slice_order)[look ? brec : 0u];
            node = look ? node : 0u;
        }
        V3 hp, nd;
        scatter_programs<V::kSpheres>(program, hg, o, d, bt, bu, bv, bprim, P.px_rng, hp, nd);
        if constexpr (V::kRestart && !V::kDirect) { if (P.px_depth == 1u) *restart = node; }
        ++P.px_depth;
        st.ro = hp; st.rd = nd; st.launch = true;
    } else {
        const uint32_t inst = binst;
        const HitGroup hg = a.path.hitgroups[inst];
        const uint32_t program = a.path.inst_program[inst];
        // A primary hit on a SPHERE seeds nothing: the seed bounds the next walk at bt on the promise that the ray is inside the record's padded
        // box at bt, which the triangle test's bt keeps and the sphere test's does not -- its discriminant cancels (b^2 - a cc, each term
        // ~|o - c|^2 |d|^2), so a sphere of radius 0.008 seen from 6 units away is hit up to 2e-4 in front of its box, the bounded walk culls
        // the box and the repeat ray, the same ray, comes back a miss.  The next primary ray walks the launch's whole interval, like a first one.
        if constexpr (V::kSeed && V::kSpheres) { if (P.px_depth == 1u && program < (uint32_t)kProgramTriangleRough) *seed = a.tmax; }
        V3 hp, nd;
        scatter_programs<V::kSpheres>(program, hg, o, d, bt, bu, bv, bprim, P.px_rng, hp, nd);
        px_chain[P.px_depth - 1u] = inst;
        ++P.px_depth;
        st.ro = hp; st.rd = nd; st.launch = true;
    }
    return st;
}

// Lanes without a pixel (`free_lane`) take the next ones of the wave's slice [wbeg, wend) of the tile's n_pixels, in lane order, and
// initialise them; a lane that took one wants a primary ray (st.want_primary).  Returns `exhausted` (wave-uniform): the tile is used up
// (in and out by value on purpose: as a `bool &` it moved k_fused's sphere instantiations' loops by an instruction).
// kBlocks (B: the wave's item): in block mode the counters hand out block_items = passes x slices numbers, number i standing for pass
// i / slices of slice i % slices, and an item of a later pass waits for its predecessor: while the slice's progress word says that pixels of
// (b - 1, q) are still under way the wave keeps the item, starts none of its pixels and looks again at its next regeneration.  It never
// waits here: the lane that has the predecessor's pixel may be one of this wave's own, so the wave must go on traversing.
// kRestart (path_finish): a pixel just taken has no restart node -- the word in LDS is the lane's previous pixel's, while the seed (kBlocks, a
// pass b > 0) comes with the pixel and switches the window on: a block's first primary ray walks from the root, inside its window.
// kCounts (path_finish): one round of path_take below -- P.gave_up says that the pixel this lane took has count 0 and is given up already.
template <class V, class Lane>
__device__ __forceinline__ bool path_take_slice(Lane &P, PathStep &st, const TraverseArgs &a, uint32_t n_pixels, bool free_lane, uint32_t &wbeg, uint32_t &wend, uint32_t &kstart,
                                                bool exhausted, uint32_t home_shard, uint32_t tx, [[maybe_unused]] BlockSlice *B = nullptr,
                                                [[maybe_unused]] float *seed = nullptr, [[maybe_unused]] uint32_t *restart = nullptr) {
    const uint64_t need = __ballot(free_lane);
    if (need != 0ull && !exhausted) {
        constexpr bool by_blocks = V::kBlocks;      // (path_launch_admitted: sample_block != 0)
        if (by_blocks) {
            if constexpr (V::kBlocks) {
                if (wbeg >= wend) {
                    uint32_t item = 0u;
                    wave_next_slice(wbeg, wend, kstart, home_shard, a.fetch_counter, a.fetch_chunk, a.path.block_items * a.fetch_chunk, tx,
                                    [&](uint64_t q) { item = (uint32_t)q; return q; });
                    if (wbeg >= wend) exhausted = true;
                    else {
                        item = wave_first_u32(item);
                        B->pass = div_magic(item, a.path.block_slices, a.path.block_slices_magic);
                        B->slice = item - B->pass * a.path.block_slices;
                        wbeg = B->slice * a.fetch_chunk;
                        wend = wbeg + a.fetch_chunk < n_pixels ? wbeg + a.fetch_chunk : n_pixels;
                        B->need = B->pass * (wend - wbeg);         // every pixel of the slice adds 1 per block it ends
                    }
                }
                if (!exhausted && B->need != 0u) {
                    const uint32_t done = __hip_atomic_load(a.path.block_progress + B->slice, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (wave_first_u32(done) >= B->need) {
                        B->need = 0u;
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");      // (no instruction: the pixels' loads stay behind the poll)
                    }
                }
            }
        } else if (wbeg >= wend) {
            // the q-th slice handed out is slice slice_order[q] of the tile: the expensive slices first, so that the render
            // ends on cheap pixels (longest-processing-time-first; a pixel's samples run one after the other)
            wave_next_slice(wbeg, wend, kstart, home_shard, a.fetch_counter, a.fetch_chunk, n_pixels, tx,
                            [&](uint64_t q) {
                                if constexpr (V::kCounts) return q;      // (slice_order carries the counts: the slices go out as they lie)
                                else return a.path.slice_order ? (uint64_t)a.path.slice_order[q] : q;
                            });
            if (wbeg >= wend) exhausted = true;
        }
        bool ready = true;
        if constexpr (V::kBlocks) ready = B->need == 0u;
        if (!exhausted && ready) {
            const uint32_t n_need = (uint32_t)__popcll(need);
            const uint32_t take = n_need < wend - wbeg ? n_need : wend - wbeg;
            const uint32_t rank = lane_prefix(need);
            const uint32_t mine = wbeg + rank;
            wbeg += take;
            if (free_lane && rank < take) {
                const uint32_t j = a.path.first_pixel + mine;
                P.px_local = j;
                P.have_pixel = true; st.want_primary = true;
                if constexpr (V::kSeed && !V::kBlocks) *seed = a.tmax;
                if constexpr (V::kRestart) *restart = V::kDirect ? kMissPrim : 0u;      // (kDirect: no record -- record 0 is a record)
                [[maybe_unused]] float carried = 0.0f;      // (kBlocks) the seed the pixel brings along
                if (V::kBlocks || !a.path.trace_rays) {
                    const uint32_t row = j / a.path.width;
                    const uint32_t ix = j - row * a.path.width;
                    const uint32_t iy = a.path.rows[row];
                    P.px_tid = iy * a.path.width + ix;
                    P.px_first = a.path.continue_sum == 0u;         // later launches of a long render continue the pixel's sum
                    if constexpr (V::kCounts) {
                        // the pixel's count, then -- unless that is 0: no ray, no store, the lane is free again -- what the caller's arrays hold of it
                        uint32_t c = a.path.spp;
                        if (a.path.slice_order) { const uint32_t want = ((global_words)a.path.slice_order)[P.px_tid]; c = want < c ? want : c; }
                        if (c == 0u) { P.have_pixel = false; st.want_primary = false; P.gave_up = true; }
                        else {
                            P.px_sample = a.path.spp - c; P.px_rng = rng_load(a.path.states + P.px_tid);
                            P.px_first = ((global_words)a.path.trace_inst)[P.px_tid] == 0u;
                            if (!P.px_first) { const float4 acc = a.path.accum[P.px_tid]; P.px_ax = acc.x; P.px_ay = acc.y; P.px_az = acc.z; P.px_aw = acc.w; }
                        }
                    } else if (by_blocks) {
                        if constexpr (V::kBlocks) {                     // ... and so do later blocks of a launch
                            P.px_sample = block_first(a.path.sample_block, a.path.block_min, a.path.block_taper_end, a.path.block_magic == 0u, B->pass);
                            P.px_first = P.px_first && B->pass == 0u;
                            // The seed comes with the pixel from the lane that ended its previous block IN THIS LAUNCH (a pass b > 0: the
                            // same ray from the same camera, so what that lane's last primary ray found is what this lane's first will
                            // find; a miss left tmax).  Pass 0 believes nothing it finds in memory -- the word is an earlier launch's,
                            // perhaps another camera's -- and starts at tmax, whether or not the launch continues a sum.
                            // (Stored below, behind the camera arithmetic, which the loads then have to arrive under.)
                            carried = handover_load(a.path, P, !P.px_first, a.tmax);
                            if (B->pass == 0u) carried = a.tmax;
                        }
                    } else {
                        P.px_sample = 0u; P.px_rng = rng_load(a.path.states + P.px_tid);
                        if (!P.px_first) { const float4 acc = a.path.accum[P.px_local]; P.px_ax = acc.x; P.px_ay = acc.y; P.px_az = acc.z; }
                    }
                    if (!V::kBlocks && a.path.slice_cost) P.px_t0 = (uint32_t)__builtin_amdgcn_s_memtime();
                    const V3 pd = primary_direction(ix, iy, a.path.width, a.path.height, a.path.U, a.path.V, a.path.W);
                    P.px_pdx = pd.x; P.px_pdy = pd.y; P.px_pdz = pd.z;
                    if constexpr (V::kSeed && V::kBlocks) *seed = carried;
                }
            }
        }
    }
    return exhausted;
}
// kCounts: a lane that drew a pixel of count 0 takes again at once, until every free lane holds a pixel with samples to take, the slice ran out
// on pixels that have some, or the tile is used up.  Without this a wave whose whole slice has count 0 would start no ray, and a wave
// with no ray under way and none to start is taken for one that has finished the tile (fused_body.h).  Every round hands out at least
// one pixel or finds the tile used up, so runs of zeros of any length end; after the last round either the tile is used up or some
// lane of the wave wants a primary ray.
template <class V, class Lane>
__device__ __forceinline__ bool path_take(Lane &P, PathStep &st, const TraverseArgs &a, uint32_t n_pixels, bool free_lane, uint32_t &wbeg, uint32_t &wend, uint32_t &kstart,
                                          bool exhausted, uint32_t home_shard, uint32_t tx, [[maybe_unused]] BlockSlice *B = nullptr,
                                          [[maybe_unused]] float *seed = nullptr, [[maybe_unused]] uint32_t *restart = nullptr) {
    if constexpr (V::kCounts) {
        for (;;) {
            P.gave_up = false;
            exhausted = path_take_slice<V>(P, st, a, n_pixels, free_lane, wbeg, wend, kstart, exhausted, home_shard, tx, B, seed, restart);
            if (__ballot(P.gave_up) == 0ull) break;
            free_lane = free_lane && !P.have_pixel;
        }
        return exhausted;
    } else return path_take_slice<V>(P, st, a, n_pixels, free_lane, wbeg, wend, kstart, exhausted, home_shard, tx, B, seed, restart);
}

// The primary ray of a lane that wants one: the caller's ray (hrt_trace_rays) or the camera ray of the lane's pixel; sets the depth.
// RECOMPUTE_DIRECTION: make the pixel's direction again instead of keeping px_pd* alive across the traversal (a kernel at its
// register limit: k_traverse<.., kSpheres, FUSED>).
struct PathRay { V3 o, d; };
template <class V, bool RECOMPUTE_DIRECTION>
__device__ __forceinline__ PathRay path_primary(PathLane &P, const TraverseArgs &a) {
    PathRay r;
    if (!V::kBlocks && a.path.trace_rays) {
        // (read as device memory, which it is: through generic pointers hipcc merges these loads with the other branch's into loads through
        // a pointer that is either the caller's ray or the camera in the kernel-argument segment -- a flat_load of kernel arguments)
        const global_floats q = (global_floats)reinterpret_cast<const float *>(a.path.trace_rays + P.px_local);
        P.px_depth = a.path.trace_any ? kRayTraceDepth : 1u;      // any-hit queries take the depth-limit ray's early exit
        r.o = mk3(q[0], q[1], q[2]); r.d = mk3(q[4], q[5], q[6]);
    } else {
        P.px_depth = 1u;
        r.o = mk3(a.path.center[0], a.path.center[1], a.path.center[2]); r.d = mk3(P.px_pdx, P.px_pdy, P.px_pdz);
        if (RECOMPUTE_DIRECTION) {
            const uint32_t iy = P.px_tid / a.path.width, ix = P.px_tid - iy * a.path.width;
            r.d = primary_direction(ix, iy, a.path.width, a.path.height, a.path.U, a.path.V, a.path.W);
        }
    }
    return r;
}

// the lane launches a ray: counted; returns whether any hit will do -- a hit at the depth limit is black whatever it is (Shader.cu:102-107)
__device__ __forceinline__ bool path_count_ray(PathLane &P) {
    const bool any = P.px_depth >= kRayTraceDepth;
    if (any) ++P.px_rays_any; else ++P.px_rays_closest;
    return any;
}

// end of the kernel: the wave's ray counts, one atomic pair per wave
__device__ __forceinline__ void path_report_rays(PathLane &P, const TraverseArgs &a, uint32_t tx) {
    for (int off = 32; off > 0; off >>= 1) {
        P.px_rays_closest += (uint32_t)__shfl_down((int)P.px_rays_closest, off);
        P.px_rays_any += (uint32_t)__shfl_down((int)P.px_rays_any, off);
    }
    if (tx == 0u) {
        atomicAdd(reinterpret_cast<unsigned long long *>(a.path.rays_closest), (unsigned long long)P.px_rays_closest);
        atomicAdd(reinterpret_cast<unsigned long long *>(a.path.rays_any), (unsigned long long)P.px_rays_any);
    }
}

}  // namespace hrt
