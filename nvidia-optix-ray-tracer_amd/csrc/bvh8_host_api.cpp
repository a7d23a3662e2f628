// bvh8_host_api.cpp -- the host-only entry points of include/hrt.h: the BVH8 builder over host triangles and the blob helpers.
// No HIP in here: the file is part of libhrt.so and, alone with bvh8_build.cpp, of the sanitizer build (make asan:
// HRT_HOST_ONLY), which runs the builder under AddressSanitizer / UBSan on the CPU.
#include "../../include/hrt.h"
#include "bvh8.h"
#include "bvh8_geom.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

namespace hrt {
#ifdef HRT_HOST_ONLY
namespace { thread_local std::string g_host_error; }
static int host_fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    g_host_error = buf;
    return code;
}
#else
int fail(HrtContext *ctx, int code, const char *fmt, ...);       // hrt_api.cpp
#define host_fail(code, ...) fail(nullptr, code, __VA_ARGS__)
#endif
}  // namespace hrt

using namespace hrt;

extern "C" {

#ifdef HRT_HOST_ONLY
const char *hrt_last_error(const HrtContext *) { return g_host_error.c_str(); }
#endif

int alloc_bvh_blob(size_t n_nodes, size_t n_prims, const float *lo, const float *hi, HrtBvhBlob *out) {
    std::memset(out, 0, sizeof *out);
    out->n_nodes = n_nodes; out->n_triangles = n_prims;
    out->nodes = std::malloc(std::max<size_t>(1, sizeof(Bvh8Node) * n_nodes));
    out->triangles = std::malloc(std::max<size_t>(1, sizeof(PrimRecord) * n_prims));
    if (!out->nodes || !out->triangles) { std::free(out->nodes); std::free(out->triangles); std::memset(out, 0, sizeof *out); return HRT_ERR_OOM; }
    for (int a = 0; a < 3; ++a) { out->bounds[a] = lo[a]; out->bounds[3 + a] = hi[a]; }
    return HRT_OK;
}

int hrt_host_build_bvh8(const float *h_triangles, uint32_t n_triangles, HrtBvhBlob *out) {
    if (!out || (n_triangles && !h_triangles)) return HRT_ERR_INVALID;
    std::vector<BuildPrim> prims(n_triangles);
    for (uint32_t p = 0; p < n_triangles; ++p) {
        BuildPrim &bp = prims[p]; std::memset(&bp, 0, sizeof bp);
        const float *v = h_triangles + 9 * (size_t)p;
        for (int a = 0; a < 3; ++a) {
            bp.rec.a[a] = v[a]; bp.rec.b[a] = v[3 + a] - v[a]; bp.rec.c[a] = v[6 + a] - v[a];
            bp.lo[a] = std::fmin(v[a], std::fmin(v[3 + a], v[6 + a]));
            bp.hi[a] = std::fmax(v[a], std::fmax(v[3 + a], v[6 + a]));
        }
        bp.rec.prim = p; bp.rec.inst = 0; bp.rec.kind = kPrimKindTriangle;
    }
    Bvh8 b;
    build_bvh8(prims, b, 0);
    const char *err = validate_bvh8(b);
    if (err[0]) return host_fail(HRT_ERR_STATE, "bvh8 validation: %s", err);
    const int rc = alloc_bvh_blob(b.nodes.size(), b.prims.size(), b.lo, b.hi, out);
    if (rc != HRT_OK) return rc;
    if (!b.nodes.empty()) std::memcpy(out->nodes, b.nodes.data(), sizeof(Bvh8Node) * b.nodes.size());
    if (!b.prims.empty()) std::memcpy(out->triangles, b.prims.data(), sizeof(PrimRecord) * b.prims.size());      // (memcpy from NULL is undefined even for 0 bytes: UBSan)
    return HRT_OK;
}

// The arithmetic of a tree that keeps its splits (bvh8_geom.h), for the CPU suite: the triangle in record form, as the builders have it.
int hrt_host_clip_barycentric(const float tri9[9], const float box6[6], float out6[6]) {
    if (!tri9 || !box6 || !out6) return HRT_ERR_INVALID;
    float e1[3], e2[3];
    for (int a = 0; a < 3; ++a) { e1[a] = tri9[3 + a] - tri9[a]; e2[a] = tri9[6 + a] - tri9[a]; }
    clip_triangle_barycentric(tri9, e1, e2, box6, box6 + 3, out6);
    return HRT_OK;
}

// leaf_parent[record] = the node whose leaf slot covers the record (device_types.h: LeafParentArgs; refit.hip's k_leaf_parent makes the same
// table from the same bytes on the device).  Checks what the kernel takes for granted: every record is covered exactly once.
int hrt_host_leaf_parent(const HrtBvhBlob *blob, uint32_t *out, uint64_t capacity) {
    if (!blob || (blob->n_triangles && !out) || (blob->n_nodes && !blob->nodes)) return HRT_ERR_INVALID;
    if (capacity < blob->n_triangles) return host_fail(HRT_ERR_INVALID, "leaf_parent: room for %llu records, the tree has %llu", (unsigned long long)capacity, (unsigned long long)blob->n_triangles);
    const uint32_t none = 0xffffffffu;
    std::fill(out, out + blob->n_triangles, none);
    const Bvh8Node *nodes = static_cast<const Bvh8Node *>(blob->nodes);
    for (uint64_t n = 0; n < blob->n_nodes; ++n)
        for (int slot = 0; slot < 8; ++slot) {
            const uint32_t meta = nodes[n].meta[slot];
            if (meta == 0u || (meta & 0x18u) == 0x18u) continue;          // empty, inner
            const uint64_t first = (uint64_t)nodes[n].prim_base + (meta & 0x1fu);
            for (uint32_t k = 0, count = (uint32_t)__builtin_popcount(meta >> 5); k < count; ++k) {
                if (first + k >= blob->n_triangles) return host_fail(HRT_ERR_STATE, "leaf_parent: node %llu slot %d names record %llu of %llu", (unsigned long long)n, slot, (unsigned long long)(first + k), (unsigned long long)blob->n_triangles);
                if (out[first + k] != none) return host_fail(HRT_ERR_STATE, "leaf_parent: record %llu is covered twice (nodes %u and %llu)", (unsigned long long)(first + k), out[first + k], (unsigned long long)n);
                out[first + k] = (uint32_t)n;
            }
        }
    for (uint64_t r = 0; r < blob->n_triangles; ++r)
        if (out[r] == none) return host_fail(HRT_ERR_STATE, "leaf_parent: record %llu is covered by no leaf slot", (unsigned long long)r);
    return HRT_OK;
}

void hrt_host_free(HrtBvhBlob *blob) {
    if (!blob) return;
    std::free(blob->nodes); std::free(blob->triangles);
    std::memset(blob, 0, sizeof *blob);
}

}  // extern "C"
