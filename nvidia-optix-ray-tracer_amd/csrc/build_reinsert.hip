// build_reinsert.hip -- insertion-based optimisation of the finished BVH2 of a fast-trace build, before the collapse (Bittner, Hapala,
// Havran 2013; the parallel form after Meister and Bittner 2018).  A top-down SAH tree and PLOC's cells are one-shot constructions; this
// pass reconsiders the topology: a node is taken out with its parent (the sibling moves up) and put back, the freed parent as the new inner
// node, beside the node where the summed area of the inner nodes grows least.  Per round:
//   search   one thread per node: what the removal saves (a walk up: every ancestor's box without the node), then a bounded descent into
//            the subtrees that hang off the node's ancestor chain, pruned on the area already accumulated against the best found, which
//            starts at the saving -- so only strict improvements are found.  The tree is read only.
//   claim    a move touches the nodes on the path node -> common ancestor -> target; its key (the improvement, then the node's number) goes
//            to every one of them with an atomic maximum.  Keys are unique, so the outcome does not depend on timing.
//   apply    a move that still holds every node of its path is made; the others wait for the next round.  Paths of moves that are made are
//            disjoint, so the six pointers each one writes are its own, and two subtrees cannot be moved into each other.
//   refit    boxes, reference counts and the collapse's cost tables bottom-up: a launch takes the nodes whose children an EARLIER launch
//            finished, so nothing is handed from workgroup to workgroup inside a launch.
// The node pool does not grow (the removed parent is the new inner node); a reference's box is its own, so every primitive stays covered.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstdio>
#include "build_dev.h"

#pragma clang fp contract(off)

namespace hrt {

namespace {

constexpr int kRiStack = 64;            // the descent's stack (a subtree's farther children); a push beyond it is dropped: a position not looked at
constexpr uint32_t kRiMaxUp = 4096u;    // no walk up is longer (a healthy tree: its height)

struct RiArgs {
    GpuBuildArgs a;
    uint32_t n_nodes, root;
    uint32_t *parent;                   // per BVH2 node
    uint32_t *target, *lca;             // per node: where the search wants it (kNone: stays), and the ancestor the path turns at
    unsigned long long *key, *lock;     // per node: the move's key; the highest key that claimed the node
    uint32_t *ready;                    // refit: the launch that finished the node (0: not yet)
    uint32_t *moved;                    // moves made this round
};

__device__ __forceinline__ uint32_t left_of(const GpuBuildArgs &a, uint32_t n) { return __float_as_uint(a.node_lo[n].w); }
__device__ __forceinline__ uint32_t right_of(const GpuBuildArgs &a, uint32_t n) { return __float_as_uint(a.node_hi[n].w); }
__device__ __forceinline__ uint32_t sibling_of(const GpuBuildArgs &a, uint32_t p, uint32_t c) { const uint32_t l = left_of(a, p); return l == c ? right_of(a, p) : l; }
__device__ __forceinline__ void set_left(const GpuBuildArgs &a, uint32_t n, uint32_t c) { reinterpret_cast<uint32_t *>(a.node_lo + n)[3] = c; }
__device__ __forceinline__ void set_right(const GpuBuildArgs &a, uint32_t n, uint32_t c) { reinterpret_cast<uint32_t *>(a.node_hi + n)[3] = c; }
__device__ __forceinline__ void replace_child(const GpuBuildArgs &a, uint32_t p, uint32_t from, uint32_t to) { if (left_of(a, p) == from) set_left(a, p, to); else set_right(a, p, to); }

struct RiBox { float lo[3], hi[3]; };
__device__ __forceinline__ RiBox box_of(const GpuBuildArgs &a, uint32_t n) {
    const float4 lo = a.node_lo[n], hi = a.node_hi[n];
    return RiBox{{lo.x, lo.y, lo.z}, {hi.x, hi.y, hi.z}};
}
__device__ __forceinline__ void grow(RiBox &b, const RiBox &o) { for (int c = 0; c < 3; ++c) { b.lo[c] = fminf(b.lo[c], o.lo[c]); b.hi[c] = fmaxf(b.hi[c], o.hi[c]); } }
__device__ __forceinline__ double area_of(const RiBox &b) {
    const float dx = b.hi[0] - b.lo[0], dy = b.hi[1] - b.lo[1], dz = b.hi[2] - b.lo[2];
    return (double)(dx * dy + dy * dz + dz * dx);
}
__device__ __forceinline__ double area_with(const RiBox &a, const RiBox &b) { RiBox u = a; grow(u, b); return area_of(u); }

__global__ __launch_bounds__(256) void k_ri_parents(RiArgs r) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= r.n_nodes) return;
    const uint32_t l = left_of(r.a, i);
    if (l == kNone) return;
    const uint32_t rt = right_of(r.a, i);
    if (l < r.n_nodes) r.parent[l] = i;
    if (rt < r.n_nodes) r.parent[rt] = i;
}

struct RiSearch { double best; uint32_t best_y, best_lca; };
// positions in the subtree `sub`, which hangs off the chain at `turn`; ind: the growth of everything above the subtree
__device__ __forceinline__ void ri_descend(const RiArgs &r, const RiBox &X, double ax, uint32_t s, uint32_t sub, double ind0, uint32_t turn, RiSearch &q) {
    const GpuBuildArgs &a = r.a;
    uint32_t st_node[kRiStack]; double st_ind[kRiStack]; int sp = 0;
    uint32_t node = sub; double ind = ind0;
    bool have = sub < r.n_nodes && ind + ax < q.best;
    while (have) {
        const RiBox Y = box_of(a, node);
        const double total = ind + area_with(Y, X);
        if (total < q.best && node != s) { q.best = total; q.best_y = node; q.best_lca = turn; }
        const uint32_t l = left_of(a, node);
        const double child_ind = total - area_of(Y);
        have = false;
        if (l != kNone && child_ind + ax < q.best) {
            const uint32_t rt = right_of(a, node);
            if (l < r.n_nodes && rt < r.n_nodes) {
                const double dl = area_with(box_of(a, l), X), dr = area_with(box_of(a, rt), X);
                const uint32_t near = dl <= dr ? l : rt, far = dl <= dr ? rt : l;
                if (sp < kRiStack) { st_node[sp] = far; st_ind[sp] = child_ind; ++sp; }      // (full: the farther child is not looked at)
                node = near; ind = child_ind; have = true;
            }
        }
        while (!have && sp > 0) { --sp; node = st_node[sp]; ind = st_ind[sp]; have = ind + ax < q.best; }
    }
}

__global__ __launch_bounds__(256) void k_ri_search(RiArgs r) {
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    if (x >= r.n_nodes) return;
    const GpuBuildArgs &a = r.a;
    r.target[x] = kNone;
    const uint32_t p = x == r.root ? kNone : r.parent[x];
    if (p == kNone || p == r.root || p >= r.n_nodes) return;             // the root and its children stay
    const RiBox X = box_of(a, x);
    const double ax = area_of(X);
    const uint32_t s = sibling_of(a, p, x);
    if (s >= r.n_nodes) return;
    // what the removal saves: p's area, and what every ancestor's box shrinks by without x
    double gain = area_of(box_of(a, p));
    {
        RiBox nb = box_of(a, s);
        uint32_t cur = p;
        for (uint32_t it = 0; it < kRiMaxUp; ++it) {
            const uint32_t up = r.parent[cur];
            if (up == kNone || up >= r.n_nodes) break;
            const uint32_t o = sibling_of(a, up, cur);
            if (o >= r.n_nodes) return;
            grow(nb, box_of(a, o));
            gain += area_of(box_of(a, up)) - area_of(nb);
            cur = up;
        }
        if (cur != r.root) return;                                      // (not a tree: leave it alone)
    }
    // the descent, subtree by subtree up the chain: s's own first (below the place x came from), then what hangs off g, off g's parent, ...
    // A position's cost: the area of the new inner node plus the growth of everything above it -- inside the subtree, and of the chain's
    // ancestors from the turning point up, whose boxes without x grow back by exactly what they shrank.
    RiSearch q; q.best = gain; q.best_y = kNone; q.best_lca = kNone;
    double ind = gain - area_of(box_of(a, p)), pending = 0.0;
    ri_descend(r, X, ax, s, s, ind, p, q);
    RiBox nb = box_of(a, s);
    uint32_t cur = p;
    for (uint32_t it = 0; it < kRiMaxUp; ++it) {
        const uint32_t up = r.parent[cur];
        if (up == kNone || up >= r.n_nodes) break;
        ind -= pending;                                                  // the level just left is not above the next subtree
        const uint32_t o = sibling_of(a, up, cur);
        grow(nb, box_of(a, o));
        pending = area_of(box_of(a, up)) - area_of(nb);
        ri_descend(r, X, ax, s, o, ind, up, q);
        cur = up;
    }
    if (q.best_y == kNone) return;
    // the key: the improvement (positive, so its bits order like the number), then the node; unique and never 0
    const float imp = (float)(gain - q.best);
    const unsigned long long key = ((unsigned long long)__float_as_uint(imp > 0.0f ? imp : 0.0f) << 32) | (unsigned long long)(x + 1u);
    r.target[x] = q.best_y; r.lca[x] = q.best_lca; r.key[x] = key;
    // claim the path: x .. the turning point, g, s, and the target .. below the turning point
    atomicMax(&r.lock[s], key);
    uint32_t n = x;
    for (uint32_t it = 0; it < kRiMaxUp; ++it) { atomicMax(&r.lock[n], key); if (n == q.best_lca) break; n = r.parent[n]; if (n == kNone || n >= r.n_nodes) break; }
    if (q.best_lca == p) atomicMax(&r.lock[r.parent[p]], key);
    n = q.best_y;
    for (uint32_t it = 0; it < kRiMaxUp && n != q.best_lca; ++it) { atomicMax(&r.lock[n], key); n = r.parent[n]; if (n == kNone || n >= r.n_nodes) break; }
}

// a move that holds its whole path is made
__global__ __launch_bounds__(256) void k_ri_apply(RiArgs r) {
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    if (x >= r.n_nodes) return;
    const GpuBuildArgs &a = r.a;
    const uint32_t y = r.target[x];
    if (y == kNone) return;
    const unsigned long long key = r.key[x];
    // (a pointer is read only once its node is known to be this move's: another move may be rewriting the ones it holds)
    if (r.lock[x] != key) return;
    const uint32_t lca = r.lca[x], p = r.parent[x];
    if (p >= r.n_nodes || r.lock[p] != key) return;
    const uint32_t g = r.parent[p], s = sibling_of(a, p, x);
    if (g >= r.n_nodes || s >= r.n_nodes || y >= r.n_nodes || lca >= r.n_nodes) return;
    if (r.lock[s] != key || r.lock[g] != key) return;
    uint32_t n = x; bool ok = false;
    for (uint32_t it = 0; it < kRiMaxUp; ++it) {
        if (r.lock[n] != key) return;
        if (n == lca) { ok = true; break; }
        n = r.parent[n];
        if (n == kNone || n >= r.n_nodes) return;
    }
    if (!ok) return;
    n = y; ok = false;
    for (uint32_t it = 0; it < kRiMaxUp; ++it) {
        if (n == lca) { ok = true; break; }
        if (r.lock[n] != key) return;
        n = r.parent[n];
        if (n == kNone || n >= r.n_nodes) return;
    }
    if (!ok) return;
    // s moves up; p goes between y and y's parent, its children y and x
    const uint32_t q = r.parent[y];                                      // (y is not s, so the first step leaves it alone)
    if (q >= r.n_nodes) return;
    replace_child(a, g, p, s); r.parent[s] = g;
    replace_child(a, q, y, p); r.parent[p] = q;
    set_left(a, p, y); set_right(a, p, x); r.parent[y] = p;
    atomicAdd(r.moved, 1u);
}

// refit, launch number `launch` (1, 2, ...): the inner nodes whose children an earlier launch finished (leaves are finished from the start)
__global__ __launch_bounds__(256) void k_ri_refit(RiArgs r, uint32_t launch) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= r.n_nodes || r.ready[i] != 0u) return;
    const GpuBuildArgs &a = r.a;
    const float4 lo = a.node_lo[i], hi = a.node_hi[i];
    const uint32_t l = __float_as_uint(lo.w), rt = __float_as_uint(hi.w);
    if (l == kNone) return;
    if (l >= r.n_nodes || rt >= r.n_nodes) return;
    const float4 llo = a.node_lo[l], lhi = a.node_hi[l], rlo = a.node_lo[rt], rhi = a.node_hi[rt];
    const bool l_done = __float_as_uint(llo.w) == kNone || (r.ready[l] != 0u && r.ready[l] < launch);
    const bool r_done = __float_as_uint(rlo.w) == kNone || (r.ready[rt] != 0u && r.ready[rt] < launch);
    if (!l_done || !r_done) return;
    a.node_lo[i] = make_float4(fminf(llo.x, rlo.x), fminf(llo.y, rlo.y), fminf(llo.z, rlo.z), lo.w);
    a.node_hi[i] = make_float4(fmaxf(lhi.x, rhi.x), fmaxf(lhi.y, rhi.y), fmaxf(lhi.z, rhi.z), hi.w);
    a.node_nprims[i] = a.node_nprims[l] + a.node_nprims[rt];
    CostRow row; cost_of_node(a, i, false, row); store_row(a, i, row);
    r.ready[i] = launch;
}

}  // namespace

#define RI_TRY(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) { *where = #expr; arena.used = mark; return e_; } } while (0)

// rounds of the pass over the BVH2 in `a` (node_lo / node_hi / node_nprims / cost; nodes [0, n_nodes), every one of them in the tree).  Working
// memory: 32 bytes per node from the arena, given back before it returns.  moved: the moves made, summed over the rounds.  The rounds end
// early once one of them moves fewer than 1 / kReinsertStopShare of the nodes.
hipError_t gpu_reinsert_bvh2(const GpuBuildArgs &a, uint32_t n_nodes, uint32_t root, int rounds, BuildArena &arena, hipStream_t s, bool verbose, uint32_t *moved, const char **where) {
    const size_t mark = arena.used;
    *moved = 0u; *where = "";
    if (rounds <= 0 || n_nodes < 7u || root >= n_nodes) return hipSuccess;
    RiArgs r{};
    r.a = a; r.n_nodes = n_nodes; r.root = root;
    const size_t nn = n_nodes;
    RI_TRY(arena.alloc((void **)&r.parent, sizeof(uint32_t) * nn)); RI_TRY(arena.alloc((void **)&r.target, sizeof(uint32_t) * nn));
    RI_TRY(arena.alloc((void **)&r.lca, sizeof(uint32_t) * nn)); RI_TRY(arena.alloc((void **)&r.ready, sizeof(uint32_t) * nn));
    RI_TRY(arena.alloc((void **)&r.key, sizeof(unsigned long long) * nn)); RI_TRY(arena.alloc((void **)&r.lock, sizeof(unsigned long long) * nn));
    RI_TRY(arena.alloc((void **)&r.moved, sizeof(uint32_t) * 2));
    const dim3 grid(blocks(n_nodes, 256)), block(256);
    RI_TRY(hipMemsetAsync(r.parent, 0xff, sizeof(uint32_t) * nn, s));
    hipLaunchKernelGGL(k_ri_parents, grid, block, 0, s, r);
    for (int round = 0; round < rounds; ++round) {
        RI_TRY(hipMemsetAsync(r.lock, 0, sizeof(unsigned long long) * nn, s));
        RI_TRY(hipMemsetAsync(r.ready, 0, sizeof(uint32_t) * nn, s));
        RI_TRY(hipMemsetAsync(r.moved, 0, sizeof(uint32_t) * 2, s));
        hipLaunchKernelGGL(k_ri_search, grid, block, 0, s, r);
        hipLaunchKernelGGL(k_ri_apply, grid, block, 0, s, r);
        RI_TRY(hipGetLastError());
        uint32_t made = 0u;
        RI_TRY(hipMemcpyAsync(&made, r.moved, sizeof made, hipMemcpyDeviceToHost, s));
        RI_TRY(hipStreamSynchronize(s));
        if (verbose) std::fprintf(stderr, "[hrt] device build: reinsertion round %d: %u of %u nodes moved\n", round + 1, made, n_nodes);
        if (made == 0u) break;
        *moved += made;
        // refit: a launch per level of the tree's height, in batches; the root's mark says when it is done
        uint32_t launch = 0u, root_ready = 0u;
        for (int batch = 0; batch < 64 && root_ready == 0u; ++batch) {
            for (int k = 0; k < 16; ++k) hipLaunchKernelGGL(k_ri_refit, grid, block, 0, s, r, ++launch);
            RI_TRY(hipGetLastError());
            RI_TRY(hipMemcpyAsync(&root_ready, r.ready + root, sizeof root_ready, hipMemcpyDeviceToHost, s));
            RI_TRY(hipStreamSynchronize(s));
        }
        if (root_ready == 0u) { *where = "reinsertion: the refit did not reach the root"; arena.used = mark; return hipErrorUnknown; }
        if (made < n_nodes / kReinsertStopShare) break;                  // (what is left to move no longer pays for a round)
    }
    RI_TRY(hipStreamSynchronize(s));
    arena.used = mark;
    return hipSuccess;
}

}  // namespace hrt
