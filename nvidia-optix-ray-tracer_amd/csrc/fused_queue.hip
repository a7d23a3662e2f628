// fused_queue.hip -- k_trace_queue: the traverse kernel of the WAVEFRONT pipeline (generate / traverse / bin / shade / accumulate as
// separate launches, hrt_api.cpp).  Its traversal loop is the production path kernel's, the very same code (trav_loop.h: two small LDS
// stacks, the hand-written bookkeeping, hand-counted vmcnt, issue priorities per phase, tail splitting with a shared best hit); what is
// here is what feeds it from ray queues instead of pixels: a lane takes a RayRec from one of up to two queue segments
// (their lengths are read from device memory, so a render is a fixed sequence of launches; trav_common.h's queue_* helpers, shared
// with k_traverse), traverses it, and writes the hit record; no path state, no RNG.  Replaces optixTrace = RT-core traversal + built-in intersection (shader/Shader.cu:70,
// src/Global/RendererImpl.cu:295-314) for the rays of one wavefront stage.  Round 1's k_traverse (kernels.hip) stays for the
// counting build and for trees outside k_fused's limits (deeper than its node stack, or beyond 32-bit offsets).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "device_types.h"
#include "trav_common.h"
#include "trav_loop.h"

#pragma clang fp contract(off)

namespace hrt {

template <bool HAS_SPHERES>
__global__ __launch_bounds__(kTraverseBlock, 4) void k_trace_queue(TraverseArgs a) {
    static_assert(kTraverseBlock == 64, "one wave per workgroup: the stacks are per wave");
    using V = PlainVariant<HAS_SPHERES>;      // (no pixels, no seed: the loop with the uniform tmin, primitive test and tail splitting in their plain forms)
    __shared__ uint2 s_nodes[kNodeStackLds][kTraverseBlock];
    __shared__ uint2 s_leaves[kLeafStackLds][kTraverseBlock];
    __shared__ float s_mb_t[kTraverseBlock], s_mb_u[kTraverseBlock], s_mb_v[kTraverseBlock];
    __shared__ uint32_t s_mb_prim[kTraverseBlock], s_mb_inst[kTraverseBlock], s_mb_pending[kTraverseBlock];
    __shared__ uint32_t s_pair[kTraverseBlock];

    // up to two queue segments per launch (trav_common.h: queue_*)
    const uint32_t n_a = queue_length(a.seg[0]), n_b = a.seg[1].rays ? queue_length(a.seg[1]) : 0u;
    const uint32_t n_rays = n_a + n_b;
    const char *__restrict__ node_bytes = reinterpret_cast<const char *>(a.nodes);
    const char *__restrict__ prim_bytes = reinterpret_cast<const char *>(a.prims);
    const float tmin = a.tmin, tmax_ray = a.tmax;
    // the traversal loop ends once at least refill_threshold lanes are idle -- or all of them: at most max_alive lanes alive
    const uint32_t max_alive = (uint32_t)a.refill_threshold >= 64u ? 0u : 64u - (uint32_t)a.refill_threshold;
    const uint32_t tx = threadIdx.x;
    const uint32_t ldsn = (uint32_t)reinterpret_cast<uintptr_t>(&s_nodes[0][tx]), ldsl = (uint32_t)reinterpret_cast<uintptr_t>(&s_leaves[0][tx]);

    const Mailboxes mb{s_mb_t, s_mb_u, s_mb_v, s_mb_prim, s_mb_inst, s_mb_pending, s_pair};

    LeanLane L;
    lean_idle(L, tmax_ray, tmin);
    LaneFlags F;                            // alive / waiting (the hit record is written at the next refill) / any / shared: trav_loop.h
    F.home = tx;
    NoInstLane I;
    LaneStats stats;
    bool exhausted = false;                 // wave-uniform: the queue is used up
    uint32_t q_index = 0u;                  // the lane's ray: position in the concatenated queue

    uint32_t wbeg = 0, wend = 0, kstart = 0;
    const uint32_t home_shard = blockIdx.x & (kFetchShards - 1);

    for (;;) {
        const uint64_t idle = ~F.alive;
        const uint32_t n_idle = (uint32_t)__popcll(idle);
        if (idle == ~0ull || (exhausted ? (uint32_t)__popcll(F.waiting) >= (uint32_t)a.tail_regen : n_idle >= (uint32_t)a.refill_threshold)) {
            __builtin_amdgcn_s_setprio(HRT_PRIO_REGEN);
            const uint64_t finished = F.waiting & ~F.alive;
            F.waiting &= F.alive;
            if (lane_bit(finished)) {
                const TravState &s = L.s;
                queue_write_hit(a, queue_pos(q_index, n_a), lean_miss_t(s.bt, s.bprim, tmax_ray), s.bu, s.bv, s.bprim, s.binst);
            }
            const uint64_t need = ~F.alive;
            bool launch = false;
            if (need != 0ull && !exhausted) {
                if (wbeg >= wend) {
                    wave_next_slice(wbeg, wend, kstart, home_shard, a.fetch_counter, a.fetch_chunk, n_rays, tx, [](uint64_t q) { return q; });
                    if (wbeg >= wend) exhausted = true;
                }
                if (!exhausted) {
                    const uint32_t n_need = (uint32_t)__popcll(need);
                    const uint32_t take = n_need < wend - wbeg ? n_need : wend - wbeg;
                    const uint32_t rank = lane_prefix(need);
                    const uint32_t mine = wbeg + rank;
                    wbeg += take;
                    if (lane_bit(need) && rank < take) { q_index = mine; launch = true; }
                }
            }
            bool any_hit = false;
            if (launch) {
                const QueuePos qp = queue_pos(q_index, n_a);
                const RayRec r = queue_ray(a, qp);
                any_hit = queue_any_hit(a, qp);
                lean_start(L, mk3(r.o.x, r.o.y, r.o.z), mk3(r.d.x, r.d.y, r.d.z), tmax_ray, tmin);      // (the loop culls with the uniform tmin here: no windows)
            }
            const uint64_t launched = __ballot(launch);
            F.alive |= launched; F.any = (F.any & ~launched) | __ballot(any_hit);
        }
        if (F.alive == 0ull) break;

        // ---- traverse until enough lanes have finished (trav_loop.h); once the queue is used up, the copy with tail splitting: every idle
        //      lane may take a piece.  The leaf stack is used to its full depth (leaf_hold 4). ----
        if (exhausted) traverse_to_regen<V, true>(L, F, I, stats, mb, s_nodes, s_leaves, ldsn, ldsl, a, node_bytes, prim_bytes, tmin, tmax_ray, 4u, max_alive, true, tx);
        else traverse_to_regen<V, false>(L, F, I, stats, mb, s_nodes, s_leaves, ldsn, ldsl, a, node_bytes, prim_bytes, tmin, tmax_ray, 4u, max_alive, true, tx);
    }
}

void launch_trace_queue(const TraverseArgs &a, bool has_spheres, uint32_t grid_blocks, hipStream_t s) {
    const dim3 g(grid_blocks), b(kTraverseBlock);
    if (has_spheres) hipLaunchKernelGGL((k_trace_queue<true>), g, b, 0, s, a);
    else hipLaunchKernelGGL((k_trace_queue<false>), g, b, 0, s, a);
}

}  // namespace hrt
