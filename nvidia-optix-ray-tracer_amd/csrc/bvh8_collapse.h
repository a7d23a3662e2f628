// bvh8_collapse.h -- the optimal SAH collapse of a BVH2 to nodes of up to eight children (Ylitie, Karras, Laine 2017, sec. 4.1), once, for
// the host builder (bvh8_build.cpp) and the device builder (build.hip, build_reinsert.hip): the cost table of a BVH2 node, the roots of
// the forest the tables choose below a node, and the octant slots of a node's children.  Plain arithmetic over values the caller
// fetched: no HIP types, no memory of its own.  Compiled with -ffp-contract=off on both sides (tests/test_collapse_cpu.py).
#pragma once
#include "bvh8_geom.h"      // HRT_HD, <math.h>, <stdint.h>, <string.h>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace hrt {

// Cost table of a BVH2 node: c[i], i = 1..7 = the cheapest representation of its subtree as a forest of at most i roots.  c[0] holds bits:
// leaf1 (one root: the subtree as a leaf, not as a node) | use_dist[i] << i, i = 2..7 (i roots are cheaper than i - 1: distribute them over
// the children) | split[j] << (8 + 3 (j - 2)), j = 2..8 (the roots given to the left child when j are distributed over the two children).
struct CostRow { float c[8]; };
HRT_HD uint32_t row_bits(const CostRow &r) { uint32_t b; memcpy(&b, &r.c[0], 4); return b; }
HRT_HD void row_set_bits(CostRow &r, uint32_t b) { memcpy(&r.c[0], &b, 4); }
HRT_HD bool row_leaf1(uint32_t bits) { return (bits & 1u) != 0u; }
HRT_HD bool row_use_dist(uint32_t bits, int i) { return ((bits >> i) & 1u) != 0u; }
HRT_HD uint32_t row_split(uint32_t bits, int j) { return (bits >> (8 + 3 * (j - 2))) & 7u; }

// a subtree as one leaf: allowed while it holds at most max_leaf_prims references
HRT_HD float leaf_cost(float area, uint32_t nprims, uint32_t max_leaf_prims, float c_prim) { return nprims <= max_leaf_prims ? area * c_prim * (float)nprims : INFINITY; }

// the table of a BVH2 leaf
HRT_HD void cost_row_leaf(float area, uint32_t nprims, uint32_t max_leaf_prims, float c_prim, CostRow &out) {
    for (int i = 1; i <= 7; ++i) out.c[i] = leaf_cost(area, nprims, max_leaf_prims, c_prim);
    row_set_bits(out, 1u);
}

// the table of an inner BVH2 node from its children's; width = children of a wide node at most (2..8).  `area` is the caller's: the device
// floors it (a box without area still costs a visit), the host passes the half area as it is.
HRT_HD void cost_row_inner(const CostRow &cl, const CostRow &cr, float area, uint32_t nprims, uint32_t max_leaf_prims, float c_node, float c_prim,
                           uint32_t width, CostRow &out) {
    const float c_leaf = leaf_cost(area, nprims, max_leaf_prims, c_prim);
    float dist[9]; uint32_t bits = 0u;
    for (int j = 2; j <= 8; ++j) {
        float best = INFINITY; int bk = 1;
        for (int k = 1; k < j; ++k) {
            const float v = cl.c[k < 7 ? k : 7] + cr.c[(j - k) < 7 ? (j - k) : 7];
            if (v < best) { best = v; bk = k; }
        }
        dist[j] = best; bits |= (uint32_t)bk << (8 + 3 * (j - 2));
    }
    const float c_internal = dist[width] + area * c_node;
    if (c_leaf <= c_internal) bits |= 1u;
    // fminf and std::min differ only where c_leaf is NaN and c_internal is not.  With finite positive c_prim and c_node, c_leaf is NaN only
    // when area is, and then c_internal is NaN too: one form for both builders.
    out.c[1] = fminf(c_leaf, c_internal);
    for (int i = 2; i <= 7; ++i) {
        if (dist[i] < out.c[i - 1]) { out.c[i] = dist[i]; bits |= 1u << i; } else out.c[i] = out.c[i - 1];
    }
    row_set_bits(out, bits);
}

// The roots of the forest that represents the OPENED subtree `root` with at most `width` roots, as the tables chose, left to right, into
// out[8]; returns their number.  (node, budget) pairs on a small stack, right pushed first.  Tree answers bits(x) (row_bits of x's table),
// leaf(x) (x is a BVH2 leaf) and children(x, l, r).
template <class Tree>
HRT_HD int collect_forest(const Tree &t, uint32_t root, int width, uint32_t *out) {
    uint32_t st_node[16]; int st_budget[16]; bool st_open[16]; int sp = 0, n = 0;
    st_node[sp] = root; st_budget[sp] = width; st_open[sp] = true; ++sp;
    while (sp > 0) {
        --sp;
        const uint32_t x = st_node[sp]; int i = st_budget[sp]; const bool open = st_open[sp];
        const uint32_t bits = t.bits(x);
        const bool leaf = t.leaf(x);                            // (asked for beside the bits, not after them: on the device both are loads, and the walk waits for each)
        if (!open) {                                            // at most i roots for subtree x
            while (i > 1 && !row_use_dist(bits, i)) --i;
            if (i == 1 || leaf) { out[n++] = x; continue; }
        }
        const int k = (int)row_split(bits, i);                  // x opened: i roots over its two children
        uint32_t l, r; t.children(x, l, r);
        st_node[sp] = r; st_budget[sp] = (i - k) < 7 ? (i - k) : 7; st_open[sp] = false; ++sp;
        st_node[sp] = l; st_budget[sp] = k < 7 ? k : 7; st_open[sp] = false; ++sp;
    }
    return n;
}

// Octant slots of a node's n children (n <= 8), d[k] = child k's centre - the node's centre: slot s is visited first by rays of octant s
// (bit2 = -x, bit1 = -y, bit0 = -z).  Greedy: the cheapest (child, slot) pair of those left, n times; strict <, so the lowest child, then the
// lowest slot wins a tie.  slot_child[s] = the child in slot s, or -1.
HRT_HD void assign_octant_slots(int n, const float (*d)[3], int *slot_child) {
    float cost[8][8];
    for (int k = 0; k < n; ++k)
        for (int q = 0; q < 8; ++q) {
            const float sx = (q & 4) ? -1.0f : 1.0f, sy = (q & 2) ? -1.0f : 1.0f, sz = (q & 1) ? -1.0f : 1.0f;
            cost[k][q] = d[k][0] * sx + d[k][1] * sy + d[k][2] * sz;
        }
    bool child_done[8];
    for (int q = 0; q < 8; ++q) { slot_child[q] = -1; child_done[q] = false; }
    for (int round = 0; round < n; ++round) {
        int bk = -1, bs = -1; float bc = INFINITY;
        for (int k = 0; k < n; ++k) {
            if (child_done[k]) continue;
            for (int q = 0; q < 8; ++q) {
                if (slot_child[q] >= 0) continue;
                if (cost[k][q] < bc) { bc = cost[k][q]; bk = k; bs = q; }
            }
        }
        if (bk < 0) {   // NaN costs (degenerate boxes): first free pair
            for (int k = 0; k < n && bk < 0; ++k) if (!child_done[k]) bk = k;
            for (int q = 0; q < 8 && bs < 0; ++q) if (slot_child[q] < 0) bs = q;
        }
        slot_child[bs] = bk; child_done[bk] = true;
    }
}

}  // namespace hrt
