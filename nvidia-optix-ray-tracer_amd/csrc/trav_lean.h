// trav_lean.h -- the building blocks of the path kernels' traversal step (the loop itself: trav_loop.h), written for INSTRUCTION COUNT.
//
// What round 2 measured (profiles/r02_valu_issue_patterns_microbench.txt, r02_exp_bounds.txt): a gfx950 SIMD issues about one
// instruction of ANY kind per 2.4 cycles -- scalar instructions, mask saves / restores and branches count like vector ones --
// and the path kernel is bound by exactly that.  The traversal loop of k_traverse spends a third of its 580 instructions on
// scalar mask bookkeeping: every `if` on per-lane data is a mask save, a branch and a restore, every per-lane bool carried
// round the loop three scalar instructions to merge, the two-level stack (LDS, overflow in scratch) two branches per access and
// a FLAT load per pop.  This step does the same work -- same nodes, same primitives, same canonical hit -- with:
//   * two small LDS stacks instead of one mixed LDS + scratch stack: sibling groups (node work) and leaf groups (primitive
//     work) are popped independently, one pop each per iteration, no "what kind is the top entry" loop; the leaf stack needs no
//     overflow path at all (a lane whose leaf stack is full does not take a new node until a group has been consumed), the
//     node stack holds one group per tree level and trees deeper than that take round 1's kernel (hrt_api.cpp);
//   * the bookkeeping after the node step as one hand-written instruction sequence;
//   * "no work" encoded in the work index itself (nidx / pidx = kNoWork) instead of separate bools;
//   * the straight-line primitive test and the node step (node_slab_test) of trav_common.h, the same as k_traverse's;
//   * lazy pushes: the sibling group in hand goes to the stack only when a child group arrives while siblings remain.
#pragma once
#include "trav_common.h"

namespace hrt {

constexpr uint32_t kNoWork = 0xffffffffu;
static_assert(kFusedMaxDepth == 12, "the node stack below is sized for it");
constexpr int kNodeStackLds = kFusedMaxDepth;      // sibling groups per lane in LDS: one per tree level above the current node (deeper trees: another kernel)
constexpr int kLeafStackLds = 4;       // leaf groups per lane in LDS (never more: see lean_select)

struct LeanLane {
    TravState s;                 // ray, reciprocal direction, octant, best hit; s.cur = sibling group in hand, s.ptri = leaf group in hand
    int nsp, lsp;                // top of the node stack / entries on the leaf stack
    int base;                    // bottom of the node stack: entries below have been given away (tail splitting, trav_loop.h)
    uint32_t nidx, pidx;         // node / primitive to fetch next (kNoWork: none)
};

__device__ __forceinline__ void lean_reset(LeanLane &L) {
    L.s.cur = make_uint2(0u, 0u); L.s.ptri = make_uint2(0u, 0u);
    L.nsp = 0; L.base = 0; L.lsp = 0; L.nidx = kNoWork; L.pidx = kNoWork;
}

// a lane without a ray: nothing to fetch, a ray and a best hit that are harmless to compute with (the wave-wide steps run for every lane)
__device__ __forceinline__ void lean_idle(LeanLane &L, float tmax_ray, float tlo) {
    lean_reset(L);
    L.s.bt = tmax_ray; L.s.tlo = tlo; L.s.bu = 0.0f; L.s.bv = 0.0f; L.s.bprim = kMissPrim; L.s.binst = kMissPrim;
    L.s.ox = L.s.oy = L.s.oz = 0.0f; L.s.dx = L.s.dy = 0.0f; L.s.dz = 1.0f; L.s.idx = L.s.idy = L.s.idz = 1.0f; L.s.oct_inv4 = 0u;
}

// a new ray: the root is its first node.  The node step's interval form (trav_common.h: kSlabInterval01) wants the ray's range settled
// here: slab_cap_rcp caps the reciprocals, and the culling bound starts at min(tmax, 2^64 / max |d_c|) -- a reach of 2^64 world units
// that no scene comes near; a normalised ray's 1e16 is untouched.  A ray that misses therefore may end with bt below tmax: lean_miss_t
// is what its record says.
// `tlo`: where the node step's interval begins for this ray (TravState::tlo) -- the launch's tmin, or the window of a repeat primary ray.
__device__ __forceinline__ void lean_start(LeanLane &L, V3 o, V3 d, float tmax_ray, float tlo) {
    trav_start<false>(L.s, o, d, tmax_ray);
    L.s.tlo = tlo;
    if (kSlabInterval01) L.s.bt = fminf(tmax_ray, kSlabReach * slab_cap_rcp(L.s.idx, L.s.idy, L.s.idz));
    lean_reset(L);
    L.nidx = 0u;
}

// the t of a finished ray's hit record: tmax for a miss, whatever lean_start made of the culling bound
__device__ __forceinline__ float lean_miss_t(float bt, uint32_t bprim, float tmax_ray) { return kSlabInterval01 && bprim == kMissPrim ? tmax_ray : bt; }

// the next node of a lane that has just been handed a sibling group (tail splitting): its nearest child -- step (7) of
// lean_bookkeeping_masked in C++
__device__ __forceinline__ void lean_pick_node(LeanLane &L) {
    TravState &s = L.s;
    const uint32_t hits_imask = s.cur.y;
    const uint32_t bit = 31u - (uint32_t)__clz((int)hits_imask);
    s.cur.y &= ~(1u << bit);
    const uint32_t slot_index = (bit - 24u) ^ (s.oct_inv4 & 0xffu);
    L.nidx = s.cur.x + (uint32_t)__popc(hits_imask & ~(0xffffffffu << slot_index));
}

// Hand-issued loads like issue_*_loads (trav_common.h) for a subset of the lanes (`mask`: a subset of the lanes that are active
// here; wave-uniform): the vector memory pipeline returns 16 bytes per ACTIVE lane and instruction whatever the address -- 64 B per
// clock and CU in all, the resource that bounds the path kernel (profiles/r02_exp_bounds.txt) -- so lanes that have no primitive /
// node to fetch are switched off for the loads instead of fetching record 0.  Lanes outside `mask` keep their registers (the
// operands are in/out: declare the registers once, outside the loop); an empty mask is fine: the loads still count in vmcnt, in
// order.  Addressed as uniform base + 32-bit byte offset per lane (one v_mul_lo_u32 per record instead of a 64-bit multiply-add and
// its operand moves).
// kExecFull: the caller vouches that EVERY lane of the wave is active at the call -- exec is all ones, so there is nothing to save: it is
// set back with a literal (one scalar instruction and one register pair less per group).  Say at the call why that holds.
template <bool kExecFull = false>
__device__ __forceinline__ void issue_prim_loads_off(uint64_t mask, const void *base, uint32_t off, f32x4 &a, f32x4 &b, f32x4 &c) {
    if constexpr (kExecFull) {
        asm volatile("s_mov_b64 exec, %5\n\t"
                     "global_load_dwordx4 %0, %3, %4\n\t"
                     "global_load_dwordx4 %1, %3, %4 offset:16\n\t"
                     "global_load_dwordx4 %2, %3, %4 offset:32\n\t"
                     "s_mov_b64 exec, -1"
                     : "+v"(a), "+v"(b), "+v"(c) : "v"(off), "s"(base), "s"(mask) : "memory");
        return;
    }
    uint64_t save;
    asm volatile("s_mov_b64 %3, exec\n\t"
                 "s_mov_b64 exec, %6\n\t"
                 "global_load_dwordx4 %0, %4, %5\n\t"
                 "global_load_dwordx4 %1, %4, %5 offset:16\n\t"
                 "global_load_dwordx4 %2, %4, %5 offset:32\n\t"
                 "s_mov_b64 exec, %3"
                 : "+v"(a), "+v"(b), "+v"(c), "=&s"(save) : "v"(off), "s"(base), "s"(mask) : "memory");
}
template <bool kExecFull = false>
__device__ __forceinline__ void issue_node_loads_off(uint64_t mask, const void *base, uint32_t off, u32x4 &a, u32x4 &b, u32x4 &c, u32x4 &d, u32x4 &e) {
    if constexpr (kExecFull) {
        asm volatile("s_mov_b64 exec, %7\n\t"
                     "global_load_dwordx4 %0, %5, %6\n\t"
                     "global_load_dwordx4 %1, %5, %6 offset:16\n\t"
                     "global_load_dwordx4 %2, %5, %6 offset:32\n\t"
                     "global_load_dwordx4 %3, %5, %6 offset:48\n\t"
                     "global_load_dwordx4 %4, %5, %6 offset:64\n\t"
                     "s_mov_b64 exec, -1"
                     : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e) : "v"(off), "s"(base), "s"(mask) : "memory");
        return;
    }
    uint64_t save;
    asm volatile("s_mov_b64 %5, exec\n\t"
                 "s_mov_b64 exec, %8\n\t"
                 "global_load_dwordx4 %0, %6, %7\n\t"
                 "global_load_dwordx4 %1, %6, %7 offset:16\n\t"
                 "global_load_dwordx4 %2, %6, %7 offset:32\n\t"
                 "global_load_dwordx4 %3, %6, %7 offset:48\n\t"
                 "global_load_dwordx4 %4, %6, %7 offset:64\n\t"
                 "s_mov_b64 exec, %5"
                 : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "=&s"(save) : "v"(off), "s"(base), "s"(mask) : "memory");
}

// kMaskIdle (k_path_idle, fused_idle.hip; trav_loop.h has the argument): the wave-wide primitive test / node step run for the lanes that loaded
// a record / a node only, in the loop copy where every lane is active (kFull).  The masks are the ones the loads go out under, so the moves
// are shared with them: the primitive group leaves its mask in exec, the node group sets its own and puts the PRIMITIVE mask back behind its
// loads -- what the primitive test, which comes next, runs under (an empty mask: the pass is skipped, and nothing but scalar instructions
// stands between here and the node step's move) --, the node step's wait sets the node mask, and all_lanes puts the literal back in front of
// the bookkeeping sequence.  Five moves where the plain forms have four, nothing saved, no branch.  The compiler does not know that exec
// changes, so each statement names, in/out, the registers that tie the arithmetic to its side of it: the landing registers (the phase's
// arithmetic all hangs on them: it comes after), for the node step also the best hit (the primitive test's updates come before it; the
// interval's k hangs on bt), for all_lanes what the node step made and the two work indices (the any-hit select on them comes after;
// child.x / tri.x ARE landing registers, and naming them would cost a copy each).  The node mask is set in one statement with the wait
// (trav_common.h: wait_node_loads), because the compiler puts an s_nop behind every statement that a vector instruction follows.
__device__ __forceinline__ void issue_prim_loads_lanes(uint64_t mask, const void *base, uint32_t off, f32x4 &a, f32x4 &b, f32x4 &c) {
    asm volatile("s_mov_b64 exec, %5\n\t"
                 "global_load_dwordx4 %0, %3, %4\n\t"
                 "global_load_dwordx4 %1, %3, %4 offset:16\n\t"
                 "global_load_dwordx4 %2, %3, %4 offset:32"
                 : "+v"(a), "+v"(b), "+v"(c) : "v"(off), "s"(base), "s"(mask) : "memory");
}
__device__ __forceinline__ void issue_node_loads_lanes(uint64_t mask, uint64_t prim_mask, const void *base, uint32_t off, u32x4 &a, u32x4 &b, u32x4 &c, u32x4 &d, u32x4 &e) {
    asm volatile("s_mov_b64 exec, %7\n\t"
                 "global_load_dwordx4 %0, %5, %6\n\t"
                 "global_load_dwordx4 %1, %5, %6 offset:16\n\t"
                 "global_load_dwordx4 %2, %5, %6 offset:32\n\t"
                 "global_load_dwordx4 %3, %5, %6 offset:48\n\t"
                 "global_load_dwordx4 %4, %5, %6 offset:64\n\t"
                 "s_mov_b64 exec, %8"
                 : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e) : "v"(off), "s"(base), "s"(mask), "s"(prim_mask) : "memory");
}
__device__ __forceinline__ void wait_node_loads_lanes(uint64_t mask, u32x4 &a, u32x4 &b, u32x4 &c, u32x4 &d, u32x4 &e, TravState &s) {
    asm volatile("s_mov_b64 exec, %10\n\ts_waitcnt vmcnt(0)"
                 : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "+v"(s.bt), "+v"(s.bu), "+v"(s.bv), "+v"(s.bprim), "+v"(s.binst) : "s"(mask) : "memory");
}
__device__ __forceinline__ void all_lanes(uint2 &child, uint2 &tri, uint32_t &nidx, uint32_t &pidx) {
    asm volatile("s_mov_b64 exec, -1" : "+v"(child.y), "+v"(tri.y), "+v"(nidx), "+v"(pidx));
}

// Everything after the node step as ONE hand-written instruction sequence: file the node's two groups, decide on the leaf pass,
// choose the primitive and the node of the next iteration, report finished rays.  (Written in C++ this is ~250 instructions,
// two thirds of them mask bookkeeping: every `if` on per-lane data a mask save, a branch and a restore; here it is 97.)
//   (1) the node's leaf group (tri: first primitive, bit per primitive that may be hit) goes into the hand (s.ptri) if that is
//       empty, else onto the leaf stack -- room is guaranteed by (7)
//   (2) the node's sibling group (child: first child, hit bits 31..24 | inner mask) becomes the group in hand (s.cur); siblings
//       still in hand go to the node stack first (lazy push)
//   (3) leaf pass?  (4) lanes with a leaf group in hand take one primitive of it  (5) an empty hand takes the top of the leaf stack
//   (6) a group in hand without hits left is replaced by the top of the node stack (entries [base, nsp) are the lane's own:
//       the bottom may have been given away, tail splitting)
//   (7) the next node: the nearest child of the group in hand -- unless the leaf stack could not take another group: such a
//       lane waits with its node work until primitives have been consumed, which is why the leaf stack needs no overflow path
//   (8) nothing left to do?
// Runs for the lanes of `act` that are active at the call (alive, not finished by an any-hit) and files the groups of the lanes of
// `nm` only (those that made a node step: the others' child / tri are whatever the wave-wide node step made of stale registers);
// other lanes keep their registers.  The masks are operands so that the caller needs no `if` around the call -- each would be a
// mask save, a branch and a restore.  The node stack has NO overflow path either: the caller guarantees a tree of at most
// kNodeStackLds levels below the root.
//   ldsn / ldsl: byte address in LDS of this lane's column of the node / leaf stack (entries are 512 bytes apart)
//   pct, quorum: leaf passes are skipped while fewer than pct % of the active lanes have leaf work and fewer than `quorum`
//   lanes have nothing else to do (those wait)
// Returns the mask of the lanes of `act` whose ray has nothing left to do, and hands out the two masks it has just had in exec: `next_p`,
// the lanes that took a primitive in (4), and -- in `nm`, which is read once, at the top -- the lanes that picked a node in (7): the lanes
// of `act` with pidx / nidx != kNoWork, which the caller would otherwise find again with a compare each.  (They are two of the
// sequence's own scalar temporaries, sv2 and c2: no operand more, and the node mask goes round the caller's loop in one register pair.)
// kExecFull, as for the loads above: every lane of the wave is active at the call, so exec is neither saved nor masked with `act`.
// The sequence is a macro so that both forms are the same text: ACT is the register pair that holds the lanes it runs for.
#define HRT_BOOK_BODY(ACT) \
        "s_and_b64 %[c2], " ACT ", %[sv2]\n\t"                  /* lanes that file the groups of a node step (sv2: `nm` until the next line) */ \
        "v_cmp_lt_u32_e64 %[sv2], %[k24], %[chy]\n\t"           /* ... whose children's group has hits */ \
        "v_cmp_lt_u32_e64 %[c6], %[k24], %[cy]\n\t"             /* ... and whose group in hand has siblings left */ \
        /* (1) the leaf group of this node: into the hand if it is free, else onto the leaf stack */ \
        "v_cmp_ne_u32_e32 vcc, 0, %[ty]\n\t" \
        "s_and_b64 exec, %[c2], vcc\n\t" \
        "v_cmp_eq_u32_e32 vcc, 0, %[py]\n\t" \
        "v_cndmask_b32_e32 %[px], %[px], %[tx], vcc\n\t" \
        "v_cndmask_b32_e32 %[py], %[py], %[ty], vcc\n\t" \
        "s_andn2_b64 exec, exec, vcc\n\t" \
        "v_lshl_add_u32 %[t0], %[lsp], 9, %[ldsl]\n\t" \
        "ds_write2_b32 %[t0], %[tx], %[ty] offset1:1\n\t" \
        "v_add_u32_e32 %[lsp], 1, %[lsp]\n\t" \
        /* (2) the sibling group of this node's children becomes the group in hand; siblings still in hand go to the stack first */ \
        "s_and_b64 %[sv1], %[c2], %[sv2]\n\t" \
        "s_and_b64 exec, %[sv1], %[c6]\n\t" \
        "v_lshl_add_u32 %[t0], %[nsp], 9, %[ldsn]\n\t" \
        "ds_write2_b32 %[t0], %[cx], %[cy] offset1:1\n\t" \
        "v_add_u32_e32 %[nsp], 1, %[nsp]\n\t" \
        "s_mov_b64 exec, " ACT "\n\t" \
        "v_cndmask_b32_e64 %[cx], %[cx], %[chx], %[sv1]\n\t" \
        "v_cndmask_b32_e64 %[cy], %[cy], %[chy], %[sv1]\n\t" \
        /* (3) leaf pass?  sv1: lanes with leaf work; sv2: lanes WITHOUT node work.  Yes when pct % of the lanes have leaf work, or */ \
        /* no lane has node work, or `quorum` lanes have nothing else to do, or a leaf stack is about to fill: each condition */ \
        /* leaves SCC, and c2 collects them (-1: yes) */ \
        "v_cmp_ne_u32_e64 %[sv1], 0, %[py]\n\t" \
        "v_cmp_ge_u32_e32 vcc, %[k24], %[cy]\n\t" \
        "v_cmp_eq_u32_e64 %[sv2], %[base], %[nsp]\n\t" \
        "s_andn2_b64 %[c6], vcc, %[sv2]\n\t"                    /* (6) below: no hits left in hand, something on the node stack */ \
        "s_and_b64 %[sv2], %[sv2], vcc\n\t" \
        "s_bcnt1_i32_b64 %[c0], %[sv1]\n\t" \
        "s_bcnt1_i32_b64 %[c1], exec\n\t" \
        "s_mulk_i32 %[c0], 0x64\n\t" \
        "s_mul_i32 %[c1], %[c1], %[pct]\n\t" \
        "s_cmp_ge_u32 %[c0], %[c1]\n\t" \
        "s_cselect_b64 %[c2], -1, 0\n\t" \
        "s_andn2_b64 vcc, exec, %[sv2]\n\t"                     /* lanes with node work (SCC: any) */ \
        "s_cselect_b64 %[c2], %[c2], -1\n\t" \
        "s_and_b64 %[sv2], %[sv2], %[sv1]\n\t"                  /* lanes with nothing but leaf work */ \
        "s_bcnt1_i32_b64 %[c0], %[sv2]\n\t" \
        "s_cmp_ge_u32 %[c0], %[quorum]\n\t" \
        "s_cselect_b64 %[c2], -1, %[c2]\n\t" \
        "v_cmp_lt_u32_e32 vcc, %[hold2], %[lsp]\n\t"            /* "about to fill": one group below the hold (4 -> more than 2 queued, as ever; 1 -> any) */ \
        "s_and_b64 vcc, vcc, %[sv1]\n\t"                        /* a leaf stack about to fill (SCC) */ \
        "s_cselect_b64 %[c2], -1, %[c2]\n\t" \
        "s_and_b64 %[c2], %[c2], %[sv1]\n\t"                    /* (stays: next_p) */ \
        /* (4) one primitive of the leaf group in hand */ \
        "v_mov_b32_e32 %[pidx], -1\n\t" \
        "s_mov_b64 exec, %[c2]\n\t" \
        "v_ffbl_b32_e32 %[t0], %[py]\n\t" \
        "v_add_u32_e32 %[t1], -1, %[py]\n\t" \
        "v_add_u32_e32 %[pidx], %[px], %[t0]\n\t" \
        "v_and_b32_e32 %[py], %[py], %[t1]\n\t" \
        "s_mov_b64 exec, " ACT "\n\t" \
        /* (5) an empty hand takes the top of the leaf stack */ \
        "v_cmp_eq_u32_e32 vcc, 0, %[py]\n\t" \
        "v_cmp_ne_u32_e64 %[sv1], 0, %[lsp]\n\t" \
        "s_and_b64 exec, vcc, %[sv1]\n\t" \
        "v_add_u32_e32 %[lsp], -1, %[lsp]\n\t" \
        "v_lshl_add_u32 %[t0], %[lsp], 9, %[ldsl]\n\t" \
        "ds_read_b32 %[px], %[t0]\n\t" \
        "ds_read_b32 %[py], %[t0] offset:4\n\t" \
        /* (6) a group in hand without hits left is replaced by the top of the node stack (the lanes were chosen in (3): cy and nsp */ \
        /* have not changed since) */ \
        "s_mov_b64 exec, %[c6]\n\t" \
        "v_add_u32_e32 %[nsp], -1, %[nsp]\n\t" \
        "v_lshl_add_u32 %[t0], %[nsp], 9, %[ldsn]\n\t" \
        "ds_read_b32 %[cx], %[t0]\n\t" \
        "ds_read_b32 %[cy], %[t0] offset:4\n\t" \
        "s_mov_b64 exec, " ACT "\n\t" \
        "s_waitcnt lgkmcnt(0)\n\t" \
        /* (7) the next node: the nearest child (highest hit bit, octant order) of the group in hand -- unless the leaf stack is full */ \
        "v_mov_b32_e32 %[nidx], -1\n\t" \
        "v_cmp_lt_u32_e32 vcc, %[k24], %[cy]\n\t" \
        "v_cmp_gt_u32_e64 %[sv2], %[hold], %[lsp]\n\t" \
        "s_and_b64 %[sv2], vcc, %[sv2]\n\t"                     /* (stays: the nodes of the next iteration) */ \
        "s_mov_b64 exec, %[sv2]\n\t" \
        "v_ffbh_u32_e32 %[t0], %[cy]\n\t" \
        "v_sub_u32_e32 %[t0], 31, %[t0]\n\t" \
        "v_lshlrev_b32_e64 %[t1], %[t0], 1\n\t" \
        "v_add_u32_e32 %[t0], -24, %[t0]\n\t" \
        "v_and_b32_e32 %[t2], 0xff, %[oct]\n\t" \
        "v_xor_b32_e32 %[t0], %[t0], %[t2]\n\t" \
        "v_bfm_b32 %[t2], %[t0], 0\n\t" \
        "v_and_b32_e32 %[t2], %[t2], %[cy]\n\t" \
        "v_bcnt_u32_b32 %[nidx], %[t2], %[cx]\n\t" \
        "v_xor_b32_e32 %[cy], %[cy], %[t1]\n\t" \
        "s_mov_b64 exec, " ACT "\n\t" \
        /* (8) nothing left? */ \
        "v_and_b32_e32 %[t0], %[nidx], %[pidx]\n\t" \
        "v_sub_u32_e32 %[t2], %[nsp], %[base]\n\t" \
        "v_or3_b32 %[t1], %[py], %[t2], %[lsp]\n\t" \
        "v_cmp_eq_u32_e32 vcc, -1, %[t0]\n\t" \
        "v_cmp_eq_u32_e64 %[sv1], 0, %[t1]\n\t" \
        "s_and_b64 %[sv1], %[sv1], vcc\n\t" \
        "v_cmp_ge_u32_e32 vcc, %[k24], %[cy]\n\t" \
        "s_and_b64 %[fin], vcc, %[sv1]\n\t"                     /* (compares under exec = sv0: no bits outside it) */
template <bool kExecFull = false>
__device__ __forceinline__ uint64_t lean_bookkeeping_masked(LeanLane &L, uint2 child, uint2 tri, uint32_t ldsn, uint32_t ldsl, uint32_t pct, uint32_t quorum,
                                                            uint32_t hold, uint64_t act, uint64_t &nm, uint64_t &next_p) {
    static_assert(kLeafStackLds == 4 && kTraverseBlock == 64 && sizeof(uint2) == 8,
                  "the sequence below has the leaf stack's depth (4, 'about to fill' = 3) and the stacks' row pitch (64 lanes x 8 bytes = 1 << 9) as literals");
    uint32_t t0, t1, t2, c0, c1;
    uint64_t fin, sv1, c6;
    const uint32_t k24 = 0x00ffffffu;
    if constexpr (kExecFull) {
        // exec is all ones: `act` itself is the mask to come back to, and nothing is saved
        asm volatile(
            HRT_BOOK_BODY("%[act]")
            "s_mov_b64 exec, -1"
            : [cx] "+v"(L.s.cur.x), [cy] "+v"(L.s.cur.y), [px] "+v"(L.s.ptri.x), [py] "+v"(L.s.ptri.y), [nsp] "+v"(L.nsp), [lsp] "+v"(L.lsp),
              [nidx] "+v"(L.nidx), [pidx] "+v"(L.pidx), [fin] "=&s"(fin), [t0] "=&v"(t0), [t1] "=&v"(t1), [t2] "=&v"(t2),
              [sv1] "=&s"(sv1), [sv2] "+s"(nm), [c2] "=&s"(next_p), [c6] "=&s"(c6), [c0] "=&s"(c0), [c1] "=&s"(c1)
            : [chx] "v"(child.x), [chy] "v"(child.y), [tx] "v"(tri.x), [ty] "v"(tri.y), [oct] "v"(L.s.oct_inv4), [base] "v"(L.base), [ldsn] "v"(ldsn), [ldsl] "v"(ldsl),
              [k24] "s"(k24), [pct] "s"(pct), [quorum] "s"(quorum), [hold] "s"(hold), [hold2] "s"(hold >> 1), [act] "s"(act)
            : "vcc", "scc", "memory");
    } else {
        uint64_t svi, sv0;
        asm volatile(
            "s_mov_b64 %[svi], exec\n\t"
            "s_and_b64 %[sv0], exec, %[act]\n\t"
            HRT_BOOK_BODY("%[sv0]")
            "s_mov_b64 exec, %[svi]"
            : [cx] "+v"(L.s.cur.x), [cy] "+v"(L.s.cur.y), [px] "+v"(L.s.ptri.x), [py] "+v"(L.s.ptri.y), [nsp] "+v"(L.nsp), [lsp] "+v"(L.lsp),
              [nidx] "+v"(L.nidx), [pidx] "+v"(L.pidx), [fin] "=&s"(fin), [t0] "=&v"(t0), [t1] "=&v"(t1), [t2] "=&v"(t2),
              [svi] "=&s"(svi), [sv0] "=&s"(sv0), [sv1] "=&s"(sv1), [sv2] "+s"(nm), [c2] "=&s"(next_p), [c6] "=&s"(c6), [c0] "=&s"(c0), [c1] "=&s"(c1)
            : [chx] "v"(child.x), [chy] "v"(child.y), [tx] "v"(tri.x), [ty] "v"(tri.y), [oct] "v"(L.s.oct_inv4), [base] "v"(L.base), [ldsn] "v"(ldsn), [ldsl] "v"(ldsl),
              [k24] "s"(k24), [pct] "s"(pct), [quorum] "s"(quorum), [hold] "s"(hold), [hold2] "s"(hold >> 1), [act] "s"(act)
            : "vcc", "scc", "memory");
    }
    return fin;
}
#undef HRT_BOOK_BODY

}  // namespace hrt
