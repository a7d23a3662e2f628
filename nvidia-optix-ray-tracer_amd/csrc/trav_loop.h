// trav_loop.h -- the traversal loop of the path kernels: everything a wave does between two regenerations, ONCE, for k_fused
// (fused.hip: pixels, path state in registers) and k_trace_queue (fused_queue.hip: ray queues).  Built from the blocks of
// trav_lean.h -- hand-issued loads, the wave-wide node step, the hand-written bookkeeping sequence with its masks as operands --
// plus what only the loop knows: the issue priority of each phase, the any-hit shortcut, the exit rules, and the tail-splitting
// protocol (tail_donate / tail_publish / tail_adopt / tail_retire below), which can be read on its own.
// Everything here is inlined into the two kernels; their LDS arrays stay declared there and are named through Mailboxes.
// (LaneStats, the instrumented build's counters, is trav_common.h's: k_traverse counts with it too.)
#pragma once
#include "trav_lean.h"

namespace hrt {

// Issue priority of a wave per phase of its loop (s_setprio: among the waves of a SIMD that are ready, the highest goes first).
// A wave that is about to fetch -- the bookkeeping that chooses its next node and primitive, the loads themselves -- and a wave
// in a regeneration go before a wave in its node step, and that before a wave in its primitive test: the fetches go out as
// early as possible and the waves drift apart instead of queueing for memory together.  C4: 3180 -> 3390 Mrays/s
// (profiles/r02_sweep_wave_priority.txt; every other assignment of the levels tried is within 3 % of this one, no priorities at
// all 6 % below).
#ifndef HRT_PRIO_BOOK
#define HRT_PRIO_BOOK 2      // bookkeeping + address arithmetic + load issue
#define HRT_PRIO_PRIM 0      // primitive wait + test
#define HRT_PRIO_NODE 1      // node wait + slab tests
#define HRT_PRIO_REGEN 2     // the kernels' own phase: shading or hit stores, next pixel or queue entry, new ray
#endif

// What a lane is doing with its ray.  `alive`, `waiting` and `any` are WAVE MASKS, one bit per lane, the same value in every lane (scalar
// registers): all the loop does with them is wave-level -- the lanes the bookkeeping runs for, the population counts of the exit rules --
// and as a per-lane bool each cost a conversion to a mask and back in every iteration.  A lane reads its bit with lane_bit(); a write
// under per-lane control flow is a mask update from a ballot of the condition, made where every lane of the wave is active.
struct LaneFlags {
    uint64_t alive = 0ull;      // a ray is being traversed in this lane
    uint64_t waiting = 0ull;    // ... has finished and waits for the next regeneration
    uint64_t any = 0ull;        // this lane's ray only needs to know whether anything is hit
    bool shared = false;        // this lane works on a piece of a ray that has been split across lanes (tail splitting)
    uint32_t home;              // ... whose owner is this lane (the lane itself while nothing is shared)
};

// a wave mask that the compiler holds per lane, in a scalar register pair again (it IS the same in every lane)
__device__ __forceinline__ uint64_t wave_first_u64(uint64_t v) { return ((uint64_t)wave_first_u32((uint32_t)(v >> 32)) << 32) | wave_first_u32((uint32_t)v); }
// this lane's bit of a wave mask (no instruction: the mask is used as the lane condition it is)
__device__ __forceinline__ bool lane_bit(uint64_t mask) { return __builtin_amdgcn_inverse_ballot_w64(mask); }

// The wave's tail-splitting mailboxes: __shared__ arrays of kTraverseBlock entries each, declared in the kernels.  One mailbox
// per lane that owns a split ray (indexed by its home lane) collects the pieces' hits; `pending` counts the pieces still under
// way, `pair` matches donors with free lanes for one hand-over.  (k_fused's kInstanced instantiation, where tail splitting is
// off, parks a lane's world ray in the same memory while the lane is inside an instance: fused.hip, InstLane.)
struct Mailboxes {
    float *t, *u, *v;
    uint32_t *prim, *inst, *pending, *pair;
};

// One-level trees: the lane is never inside an instance.  (The two-level kernel's counterpart, with the transform-node steps, is
// fused.hip's InstLane.)
struct NoInstLane { static constexpr uint32_t inst_cur = 0u; };

// ---- tail splitting: the work is used up (no pixels, no queue entries left) and a few rays remain, one after the other in k_fused's
//      sample chains.  A busy lane gives the BOTTOM entry of its node stack (the largest pending subtree) to a free lane of
//      the wave, which continues with a copy of the ray.  The pieces of a split ray share ONE best hit, the mailbox of
//      the lane that owns the ray: a piece publishes every improvement there (canonical order: the result does not
//      depend on who found what, or when) and adopts what the others found closer, so every piece culls with the
//      ray's best hit so far.  A piece that finishes signs off at the mailbox, and the owner takes the merged hit once the last
//      one has.  Four blocks, in the order a loop iteration runs them; all lanes of the wave call each (they hold wave barriers).
//      `is_free`: this lane has nothing of its own to do and may take a piece. ----

// (one donation per busy lane and iteration: more rounds of this change nothing, r02_sweep_tile_tail.txt)
// kOneGroup, here and in the three blocks below (k_path_one, fused_one.hip): every hit is instance 0's, so TravState::binst is not kept --
// a mailbox's `inst` is given 0, and nobody takes a lane's binst from there.
// kRestart (k_path_restart, fused_restart.hip: kOneGroup with the best hit's record in binst, trav_common.h: test_prim_ray): the mailboxes' `inst`
// array is not theirs any more -- it holds the lanes' restart nodes (fused_body.h: s_restart) -- so it is neither written nor read here, and a
// hit that comes out of a mailbox has no record: binst = kNoWork, the pixel's next primary ray walks from the root.
template <class V>
__device__ __forceinline__ void tail_donate(LeanLane &L, LaneFlags &F, const Mailboxes &mb, uint2 (*nodes)[kTraverseBlock], bool is_free, uint32_t tx, float tmin, float tmax_ray) {
    const uint64_t free_m = __ballot(is_free);
    const uint64_t donors = F.alive & __ballot(L.nsp > L.base);
    const uint32_t n_free = (uint32_t)__popcll(free_m), n_don = (uint32_t)__popcll(donors);
    const uint32_t n_pairs = n_free < n_don ? n_free : n_don;
    if (n_pairs) {
        const uint32_t drank = lane_prefix(donors), irank = lane_prefix(free_m);
        const bool is_donor = lane_bit(donors) && drank < n_pairs;
        const bool is_recv = is_free && irank < n_pairs;
        uint2 give = make_uint2(0u, 0u);
        if (is_donor) {
            give = nodes[L.base][tx];
            ++L.base;
            if (!F.shared) {
                F.shared = true; F.home = tx;
                mb.t[tx] = L.s.bt; mb.u[tx] = L.s.bu; mb.v[tx] = L.s.bv; mb.prim[tx] = L.s.bprim;
                if constexpr (!V::kRestart) mb.inst[tx] = V::kOneGroup ? 0u : L.s.binst;
                mb.pending[tx] = 2u;
            } else atomicAdd(&mb.pending[F.home], 1u);
            mb.pair[drank] = tx;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int src = is_recv ? (int)mb.pair[irank] : (int)tx;
        // every lane shuffles; only receivers keep what they read
        TravState &s = L.s;
        const float r_ox = __shfl(s.ox, src), r_oy = __shfl(s.oy, src), r_oz = __shfl(s.oz, src);
        const float r_dx = __shfl(s.dx, src), r_dy = __shfl(s.dy, src), r_dz = __shfl(s.dz, src);
        const uint32_t r_home = (uint32_t)__shfl((int)(F.home | (lane_bit(F.any) ? 0x100u : 0u)), src);
        const uint32_t r_gx = (uint32_t)__shfl((int)give.x, src), r_gy = (uint32_t)__shfl((int)give.y, src);
        if (is_recv) {
            lean_start(L, mk3(r_ox, r_oy, r_oz), mk3(r_dx, r_dy, r_dz), tmax_ray, tmin);     // the same reciprocals and octant as the owner's (a piece culls from the launch's tmin)
            F.home = r_home & 0xffu; F.shared = true;
            s.bt = mb.t[F.home]; s.bu = mb.u[F.home]; s.bv = mb.v[F.home]; s.bprim = mb.prim[F.home];
            if constexpr (!V::kOneGroup) s.binst = mb.inst[F.home];
            s.cur = make_uint2(r_gx, r_gy);           // a sibling group with hits: only those are pushed
            lean_pick_node(L);                        // (replaces the root lean_start chose)
        }
        const uint64_t recv = __ballot(is_recv);
        F.alive |= recv; F.any = (F.any & ~recv) | (recv & __ballot((r_home & 0x100u) != 0u));      // (a piece asks what its ray asks)
    }
}

// pieces of split rays publish their improvements one lane at a time (rare: a few per ray) ...
template <class V>
__device__ __forceinline__ void tail_publish(const LeanLane &L, const LaneFlags &F, const Mailboxes &mb, bool improved, uint32_t tx) {
    uint64_t pub = __ballot(improved && F.shared);
    while (pub) {
        const uint32_t l = (uint32_t)__ffsll((long long)pub) - 1u;
        pub &= pub - 1ull;
        if (tx == l) {
            const TravState &s = L.s;
            const float mt = mb.t[F.home];
            const uint64_t mid = ((uint64_t)(V::kRestart ? 0u : mb.inst[F.home]) << 32) | mb.prim[F.home];
            const uint64_t id = ((uint64_t)(V::kOneGroup ? 0u : s.binst) << 32) | s.bprim;
            if (lane_bit(F.any) ? mb.prim[F.home] == kMissPrim : (s.bt < mt || (s.bt == mt && id < mid))) {
                mb.t[F.home] = s.bt; mb.u[F.home] = s.bu; mb.v[F.home] = s.bv; mb.prim[F.home] = s.bprim;
                if constexpr (!V::kRestart) mb.inst[F.home] = V::kOneGroup ? 0u : s.binst;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

// ... and take over what another piece has found closer; an any-hit ray is done once any piece has hit.  Returns the lane's hit_any
// (by value on purpose: as a `bool &` it cost each one-level k_fused three more spilled registers)
template <class V>
__device__ __forceinline__ bool tail_adopt(LeanLane &L, const LaneFlags &F, const Mailboxes &mb, bool hit_any) {
    if (lane_bit(F.alive) && F.shared) {
        if (lane_bit(F.any)) hit_any = hit_any || mb.prim[F.home] != kMissPrim;
        else if (mb.t[F.home] < L.s.bt) {
            L.s.bt = mb.t[F.home]; L.s.bu = mb.u[F.home]; L.s.bv = mb.v[F.home]; L.s.bprim = mb.prim[F.home];
            if constexpr (!V::kOneGroup) L.s.binst = mb.inst[F.home];
            if constexpr (V::kRestart) L.s.binst = kNoWork;
        }
    }
    return hit_any;
}

// a piece whose lane reports `done` retires; the owner of the ray takes the merged hit once the last piece has
template <class V>
__device__ __forceinline__ void tail_retire(LeanLane &L, LaneFlags &F, const Mailboxes &mb, bool done, uint32_t tx) {
    // a piece that has finished has nothing left to merge: the mailbox holds the ray's best hit
    const bool retires = lane_bit(F.alive) && done && F.shared;
    if (retires) {
        atomicSub(&mb.pending[F.home], 1u);
        if (F.home != tx) { F.shared = false; F.home = tx; }        // a helper is free again; the owner waits for the last piece
    }
    F.alive &= ~__ballot(retires);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // the owner of a split ray picks the merged hit up once its last piece has finished
    const bool merged = F.shared && !lane_bit(F.alive) && F.home == tx && mb.pending[tx] == 0u;
    if (merged) {
        L.s.bt = mb.t[tx]; L.s.bu = mb.u[tx]; L.s.bv = mb.v[tx]; L.s.bprim = mb.prim[tx];
        if constexpr (!V::kOneGroup) L.s.binst = mb.inst[tx];
        if constexpr (V::kRestart) L.s.binst = kNoWork;
        F.shared = false;
    }
    F.waiting |= __ballot(merged);
}

// ---- traverse until enough lanes have finished to make a regeneration worthwhile ----
// The kernels instantiate the loop twice: kTail = true, with tail splitting and the drained phase's exit rule (at least
// a.tail_regen rays wait, or none is alive), runs once the work is used up -- the other copy pays nothing for either and ends
// once at most `max_alive` lanes are alive.
//   I: the lane's instance state (NoInstLane, or fused.hip's InstLane with the transform-node steps of a two-level tree)
//   nodes / leaves: the wave's LDS stacks; ldsn / ldsl: byte address in LDS of this lane's column of each
//   leaf_hold: lean_bookkeeping_masked's `hold`;  may_help: the lane has no work of its own outside the loop either (tail splitting)
// `a` is the kernel's argument block, by reference: only scalars are read from it, where they are used.
// V: the kernel's variant (trav_common.h: PathVariant).  kSeed: the node step's interval begins at the lane's TravState::tlo (the kernels
// that give repeat primary rays a window) instead of the wave-uniform tmin -- the same instructions, one operand a vector register, not a scalar one.
// kOneGroup (k_path_one): the primitive test and the tail-splitting blocks in their one-instance forms (trav_common.h: test_prim_ray).
// kRestart (k_path_restart): ... which also keep the record of the lane's best hit (the primitive test is told the record it tests: pidx).
// kMaskIdle (k_path_idle): the copy without tail splitting switches the lanes without a record / a node off for the primitive test / the node step (kIdleOff below).
template <class V, bool kTail, class Inst>
__device__ __forceinline__ void traverse_to_regen(LeanLane &L, LaneFlags &F, Inst &I, LaneStats &stats, const Mailboxes &mb,
                                                  uint2 (*nodes)[kTraverseBlock], uint2 (*leaves)[kTraverseBlock], uint32_t ldsn, uint32_t ldsl,
                                                  const TraverseArgs &a, const char *node_bytes, const char *prim_bytes,
                                                  float tmin, float tmax_ray, uint32_t leaf_hold, uint32_t max_alive, bool may_help, uint32_t tx) {
    constexpr bool kSplit = kTail && !V::kInstanced;        // (tail splitting is off for two-level trees)
    // the registers the loads land in: "defined" without an instruction (lanes that load nothing never look at theirs)
    f32x4 rpa, rpb, rpc;
    u32x4 rn0, rn1, rn2, rn3, rn4;
    asm volatile("" : "=v"(rpa), "=v"(rpb), "=v"(rpc), "=v"(rn0), "=v"(rn1), "=v"(rn2), "=v"(rn3), "=v"(rn4));
    // The lanes that want a primitive / a node.  The bookkeeping sequence has just had both in exec and hands them out, so the one-level
    // copy without tail splitting carries them round the loop; found by compare where something else writes pidx / nidx: a new ray (here,
    // at the entry), tail_donate (the kTail copy), switch_frames (kInstanced).
    constexpr bool kCarryWork = !kTail && !V::kInstanced;
    // The same copy uses the blocks' exec-is-full forms (trav_lean.h: nothing saved, exec set back to all ones).  Every lane IS active at the
    // top level of this loop's body: a workgroup is one wave of exactly kTraverseBlock = 64 lanes (static_assert and launch), and every
    // branch round the loop and round this call -- the regeneration's, the choice of the copy, the exits -- is taken on a value that is the
    // same in all lanes (counts of the flag masks, `exhausted`).  Nothing in this copy's body leaves a lane switched off: the primitive
    // test's `if` is on a mask's emptiness, and the blocks restore exec themselves.  The other copies keep the saving forms: their bodies
    // call helpers with per-lane control flow of their own (tail splitting, InstLane), which this argument does not cover.
    constexpr bool kFull = kCarryWork;
    // kMaskIdle (k_path_idle, fused_idle.hip): in that copy the primitive test runs with exec = mask_p and the node step with exec = mask_n0 -- the
    // lanes that loaded a record / a node; the others no longer compute on what their landing registers hold -- and exec is all ones again
    // in front of the bookkeeping sequence.  The load groups already set these masks, so the moves are shared with them (trav_lean.h:
    // issue_prim_loads_lanes, issue_node_loads_lanes, wait_node_loads_lanes, all_lanes): five moves to exec per iteration where the plain
    // forms have four, nothing saved, no branch.  The argument above, extended to those writes: each is made at the top level of the body,
    // on a wave-uniform mask; exec is all ones from all_lanes to the loads -- the bookkeeping sequence, the exit counts, the addresses -- and
    // the only branch between the loads and all_lanes is the skip of an empty primitive pass, which is taken with exec = mask_p = 0 and
    // rejoins in front of the node step's move with nothing but scalar instructions on the way.  What runs with lanes off is straight-line
    // arithmetic that only a lane's own registers enter and leave:
    //   C: a lane that is off writes 0 in every compare (so `live` is implied: test_prim_ray) and keeps its best hit, which is updated in place;
    //   A: a lane that is off keeps stale child / tri, which is what mask_n0 already covers in the bookkeeping -- what lanes without a node
    //      made of their registers is not filed;
    // and everything that reads across lanes or is filed for every lane -- the any-hit select on nidx / pidx, the bookkeeping sequence, the
    // exit counts, the next iteration's addresses -- runs behind all_lanes, as before.  tests/test_mask_idle_cpu.py reads the moves, their
    // order and what the masked stretches write from the assembly.
    constexpr bool kIdleOff = kFull && V::kMaskIdle;
    // The flag masks in scalar registers for the loop.  Between two calls the compiler keeps them in vector register pairs: the kernels
    // choose this copy or the other by `exhausted`, which is wave-uniform but a per-lane value to the compiler, and whatever is merged
    // behind such a branch is per-lane to it as well.  (Making those branches scalar instead keeps the masks where they are, and spills
    // 22 to 49 VGPRs round the regeneration of every one-level kernel: profiles/r17_wave_masks.txt.)
    F.alive = wave_first_u64(F.alive); F.waiting = wave_first_u64(F.waiting); F.any = wave_first_u64(F.any);
    uint64_t mask_p = __ballot(L.pidx != kNoWork), mask_n0 = __ballot(L.nidx != kNoWork);
    for (;;) {
        if (kSplit && a.tail_split) tail_donate<V>(L, F, mb, nodes, !lane_bit(F.alive | F.waiting) && may_help && !F.shared, tx, tmin, tmax_ray);

        // ---- G. fetch what the lanes need next: primitives first, nodes second -- for the lanes that need one only (the
        //      instruction slots of the loads are not saved, but their L1 / TA cycles are).  The node loads are issued even when
        //      no lane wants one: they are then ALWAYS the five youngest vector-memory operations at the primitives' wait,
        //      whose vmcnt(5) is counted by hand. ----
        if constexpr (!kCarryWork) { mask_p = __ballot(L.pidx != kNoWork); mask_n0 = __ballot(L.nidx != kNoWork); }
        {
            uint32_t po = L.pidx * a.prim_stride, no = L.nidx * a.node_stride;      // (garbage for kNoWork: masked out)
            asm volatile("" : "+v"(po), "+v"(no));          // both offsets before the first load
            if constexpr (kIdleOff) {
                stats.pin(); stats.iteration(lane_bit(F.alive), mask_n0, mask_p); stats.primary_slots(F.alive, F.waiting); stats.pin();      // (counted here, where every lane is still on)
                if (mask_p != 0ull) issue_prim_loads_lanes(mask_p, prim_bytes, po, rpa, rpb, rpc);
                issue_node_loads_lanes(mask_n0, mask_p, node_bytes, no, rn0, rn1, rn2, rn3, rn4);
            } else {
                if (mask_p != 0ull) issue_prim_loads_off<kFull>(mask_p, prim_bytes, po, rpa, rpb, rpc);
                issue_node_loads_off<kFull>(mask_n0, node_bytes, no, rn0, rn1, rn2, rn3, rn4);
            }
            __builtin_amdgcn_s_setprio(HRT_PRIO_PRIM);
        }
        if constexpr (!kIdleOff) { stats.iteration(lane_bit(F.alive), mask_n0, mask_p); stats.primary_slots(F.alive, F.waiting); }
        // ---- C. leaf test: waits for the primitive pieces only (the node loads issued behind them stay in flight).  Triangles:
        //      every lane tests (straight-line arithmetic, no loads) and a lane without a primitive rejects whatever its
        //      registers hold -- some lane nearly always has one, so a per-lane branch would save nothing but cost a mask
        //      save, a branch and a restore.  Spheres read the instance table: only lanes with a primitive test. ----
        uint64_t hit_m = 0ull, improved_m = 0ull;           // wave masks: a closer hit was found; ... by an any-hit ray
        // (the same test as at the loads, on a copy the compiler cannot see through: it would otherwise keep the first one's outcome in a
        // register pair across the loads and test that -- two scalar instructions more than comparing again)
        uint64_t any_p = mask_p;
        asm volatile("" : "+s"(any_p));
        if (any_p != 0ull) {
            wait_prim_loads(rpa, rpb, rpc);
            const float4 pa = make_float4(rpa.x, rpa.y, rpa.z, rpa.w), pb = make_float4(rpb.x, rpb.y, rpb.z, rpb.w),
                         pc = make_float4(rpc.x, rpc.y, rpc.z, rpc.w);
            if constexpr (!V::kSpheres)
                improved_m = test_prim<V, WaveCond, kIdleOff>(pa, pb, pc, L.s, tmin, tmax_ray, a.inst_inv, a.inst_identity, I.inst_cur, WaveCond(any_p), L.pidx).m;
            else {
                bool improved = false;
                if (L.pidx != kNoWork) improved = test_prim<V>(pa, pb, pc, L.s, tmin, tmax_ray, a.inst_inv, a.inst_identity, I.inst_cur);
                improved_m = __ballot(improved);
            }
            hit_m = F.any & improved_m;
        }
        if (kSplit && a.tail_split) {
            tail_publish<V>(L, F, mb, lane_bit(improved_m), tx);
            hit_m = __ballot(tail_adopt<V>(L, F, mb, lane_bit(hit_m)));
        }
        const bool hit_any = lane_bit(hit_m);
        // ---- A. node step: one-level trees, for the whole wave (arithmetic only; what lanes without a node made of their
        //      registers is not filed: mask_n0 below) ----
        uint2 child = make_uint2(0u, 0u), tri = make_uint2(0u, 0u);
        __builtin_amdgcn_s_setprio(HRT_PRIO_NODE);
        if constexpr (kIdleOff) wait_node_loads_lanes(mask_n0, rn0, rn1, rn2, rn3, rn4, L.s);
        else wait_node_loads(rn0, rn1, rn2, rn3, rn4);
        [[maybe_unused]] bool enter = false;
        if constexpr (!V::kInstanced) {
            node_slab_test<kSlabInterval01>(L.s, V::kSeed ? L.s.tlo : tmin, rn0, rn1, rn2, rn3, rn4, child, tri);
        } else {
            enter = L.nidx != kNoWork && !hit_any && rn0.w == 0u;          // a transform node: word 3 == 0
            if (L.nidx != kNoWork && !hit_any && !enter) node_slab_test<kSlabInterval01>(L.s, V::kSeed ? L.s.tlo : tmin, rn0, rn1, rn2, rn3, rn4, child, tri);
            enter = I.enter_instance(enter, L.s, child, rn0, rn1, rn2, rn3, rn4, mb, tx);
            stats.entered(enter);
        }
        // ---- B. bookkeeping (trav_lean.h: one hand-written sequence): file the new groups; the leaf pass (ONE per iteration, one
        //      primitive per lane, skipped while few lanes have leaf work and none depends on it); the primitive and the node of
        //      the next iteration; finished? ----
        __builtin_amdgcn_s_setprio(HRT_PRIO_BOOK);
        if constexpr (kIdleOff) all_lanes(child, tri, L.nidx, L.pidx);
        // an any-hit ray is done with its first accepted intersection: nothing more to fetch (what is left on its stacks is
        // dropped when the lane's next ray starts, lean_start)
        if (hit_any) { L.nidx = kNoWork; L.pidx = kNoWork; }
        // the sequence runs for the lanes that are alive and not finished by an any-hit, and files the groups of those that
        // made a node step (nidx is still what it was at the loads for them)
        const uint64_t book = F.alive & ~hit_m;
        uint64_t fin;
        [[maybe_unused]] uint32_t lane = 0u;
        if constexpr (!V::kInstanced) {
            fin = lean_bookkeeping_masked<kFull>(L, child, tri, ldsn, ldsl, (uint32_t)a.postpone_pct, (uint32_t)a.leaf_quorum, leaf_hold, book, mask_n0, mask_p);
        } else {
            // (this instantiation is two registers over its budget and the compiler's choice of what to keep in scratch is the two
            // stack addresses, reloaded here in every iteration: they are a constant plus eight times the lane number -- two
            // instructions to make again)
            asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
            const uint32_t ldsn_i = (uint32_t)reinterpret_cast<uintptr_t>(&nodes[0][0]) + 8u * lane, ldsl_i = (uint32_t)reinterpret_cast<uintptr_t>(&leaves[0][0]) + 8u * lane;
            mask_n0 = ~0ull;        // (every lane of `book` files: a lane without a node step has an empty child / tri, above)
            fin = lean_bookkeeping_masked(L, child, tri, ldsn_i, ldsl_i, (uint32_t)a.postpone_pct, (uint32_t)a.leaf_quorum, leaf_hold, book, mask_n0, mask_p);
        }
        // finished: by an any-hit, or with nothing left to do.  All of it is mask arithmetic (`fin` only has bits inside `book`)
        uint64_t done_m = hit_m | fin;
        if constexpr (V::kInstanced) done_m = __ballot(I.switch_frames(enter, lane_bit(done_m), hit_any, L, mb, nodes, tx, lane));
        // (a piece of a split ray does not wait for a regeneration: tail_retire signs it off.  Only tail_donate shares rays)
        const uint64_t rest = kSplit ? done_m & ~__ballot(F.shared) : done_m;
        F.alive &= ~rest; F.waiting |= rest;
        if (kSplit && a.tail_split) tail_retire<V>(L, F, mb, lane_bit(done_m), tx);
        if constexpr (kTail) {
            if (F.alive == 0ull || (uint32_t)__popcll(F.waiting) >= (uint32_t)a.tail_regen) break;
        } else if ((uint32_t)__popcll(F.alive) <= max_alive) break;      // (every lane finished included)
    }
}

}  // namespace hrt
