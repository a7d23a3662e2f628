// hrt_accel.cpp -- acceleration structures behind the C ABI: BLAS objects, the merged world-space build, trees over
// instances, the per-frame device refit (updateIAS), the Time-mode pose kernel's entry point, and the download /
// host-build helpers the tests use.  Entry points and the reference call sites they replace: include/hrt.h.
#include <thread>
#include "hrt_internal.hpp"
#include "build.h"

namespace hrt {

// ---- transforms (fixed operation order; DESIGN.md "instances") ----
bool is_identity(const float *m) {
    static const float id[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    return std::memcmp(m, id, sizeof id) == 0;
}
void invert_affine(const float *m, float *o) {
    const double a = m[0], b = m[1], c = m[2], d = m[4], e = m[5], f = m[6], g = m[8], h = m[9], i = m[10];
    const double A = e * i - f * h, B = -(d * i - f * g), C = d * h - e * g;
    const double det = a * A + b * B + c * C;
    const double r = 1.0 / det;
    const double n00 = A * r, n01 = -(b * i - c * h) * r, n02 = (b * f - c * e) * r;
    const double n10 = B * r, n11 = (a * i - c * g) * r, n12 = -(a * f - c * d) * r;
    const double n20 = C * r, n21 = -(a * h - b * g) * r, n22 = (a * e - b * d) * r;
    const double tx = m[3], ty = m[7], tz = m[11];
    o[0] = (float)n00; o[1] = (float)n01; o[2] = (float)n02; o[3] = (float)(-(n00 * tx + n01 * ty + n02 * tz));
    o[4] = (float)n10; o[5] = (float)n11; o[6] = (float)n12; o[7] = (float)(-(n10 * tx + n11 * ty + n12 * tz));
    o[8] = (float)n20; o[9] = (float)n21; o[10] = (float)n22; o[11] = (float)(-(n20 * tx + n21 * ty + n22 * tz));
}

void free_tlas_device(HrtContext *ctx, Tlas &t) {
    TlasDevice &d = t.dev;
    if (d.d_nodes || d.d_prims || d.d_inst_inv || d.d_inst_xf) (void)hipDeviceSynchronize();      // (what each hipFree used to do; the blocks go to the context's pool)
    void *blocks[sizeof(TlasDevice) / sizeof(void *)];
    std::memcpy(blocks, &d, sizeof d);
    for (void *p : blocks) pool_release(ctx, p);
    d = TlasDevice();
    t.area_pending = false;
}
// The table record -> node of a one-level tree of triangles (device_types.h: LeafParentArgs), which k_path_restart starts a pixel's repeat
// primary rays from.  Made from the finished nodes, once per tree: every builder leaves a new TlasDevice behind (build_tlas_fresh frees first,
// a rebuild swaps a fresh Tlas in), so a tree without the table is a tree nobody has asked yet; a refit rewrites boxes and records in
// place and keeps both the topology and the record order.  Filled with the root first, so that a record no slot names sends its ray
// the long way instead of anywhere else.  The stream is synchronised once, here: launches on other streams may read the table next.
int ensure_leaf_parent(HrtContext *ctx, Tlas &t, hipStream_t s) {
    TlasDevice &d = t.dev;
    if (d.d_leaf_parent || t.n_prims == 0u || t.n_nodes == 0u) return HRT_OK;
    if (t.two_level || t.has_spheres) return fail(ctx, HRT_ERR_STATE, "leaf_parent: one-level trees of triangles only");
    HIP_TRY(ctx, pool_alloc(ctx, (void **)&d.d_leaf_parent, sizeof(uint32_t) * (size_t)t.n_prims));
    HIP_TRY(ctx, hipMemsetAsync(d.d_leaf_parent, 0, sizeof(uint32_t) * (size_t)t.n_prims, s));
    LeafParentArgs la{reinterpret_cast<const unsigned char *>(d.d_nodes), t.node_stride, t.n_nodes, t.n_prims, d.d_leaf_parent};
    launch_leaf_parent(la, s);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return HRT_OK;
}
void free_tlas_host(Tlas &t) {
    if (t.h_area) (void)hipHostFree(t.h_area);
    if (t.h_update_flags) (void)hipHostFree(t.h_update_flags);
    t.h_update_flags = nullptr;
    if (t.area_ready) (void)hipEventDestroy(t.area_ready);
    t.h_area = nullptr; t.area_ready = nullptr;
}

int g_instance_table_threads = 8;      // HRT_TABLE_THREADS

// Which instances a tree holds.  The reference traces with mask 1 (Shader.cu:71): an instance counts when that bit is set and its BLAS has a
// box (a BLAS without a valid primitive keeps lo > hi).  What works on the boxes asks instance_has_box: the scene scale (instance_tables),
// the tree over instances, the templates hrt_tlas_build makes ahead, instances_moved_far.
static bool instance_has_box(const HrtInstance &in, const Blas &b) { return (in.visibilityMask & 1u) != 0 && b.lo[0] <= b.hi[0]; }
// ... and its BLAS has primitives: asked where an instance becomes ONE primitive of a two-level tree's top level (whether to build such a
// tree, and the top level's numbering).  A BLAS without primitives has no box either, so the two agree today; these callers count, and say so.
static bool instance_has_prims(const HrtInstance &in, const Blas &b) { return instance_has_box(in, b) && b.n_prims != 0u; }

// The eight corners of a BLAS's box under an instance's transform (identity: as they are).
static void blas_box_corners(const Blas &b, const float *m, bool identity, float w[8][3]) {
    for (int c = 0; c < 8; ++c) {
        const float q[3] = {(c & 1) ? b.hi[0] : b.lo[0], (c & 2) ? b.hi[1] : b.lo[1], (c & 4) ? b.hi[2] : b.lo[2]};
        if (identity) { w[c][0] = q[0]; w[c][1] = q[1]; w[c][2] = q[2]; } else xf_point(m, q, w[c]);
    }
}

// Per-instance tables of a set of instances: object->world, world->object, identity flags, and the
// largest |coordinate| of the transformed BLAS boxes (what the padding of the tree is derived from).
float instance_tables(const std::vector<HrtInstance> &inst, const std::vector<std::shared_ptr<Blas>> &blas,
                      std::vector<float> &xf, std::vector<float> &inv, std::vector<uint32_t> &ident) {
    const size_t n = inst.size();
    xf.assign(12 * std::max<size_t>(n, 1), 0.0f); inv.assign(12 * std::max<size_t>(n, 1), 0.0f); ident.assign(std::max<size_t>(n, 1), 1u);
    const auto range = [&](size_t i0, size_t i1) {
        float smax = 1.0f;
        for (size_t i = i0; i < i1; ++i) {
            const float *m = inst[i].transform;
            std::memcpy(&xf[12 * i], m, 12 * sizeof(float));
            const bool id = is_identity(m);
            ident[i] = id ? 1u : 0u;
            invert_affine(m, &inv[12 * i]);
            if (!instance_has_box(inst[i], *blas[i])) continue;
            float w[8][3];
            blas_box_corners(*blas[i], m, id, w);
            for (int c = 0; c < 8; ++c)
                for (int a = 0; a < 3; ++a) if (std::isfinite(w[c][a])) smax = std::max(smax, std::fabs(w[c][a]));
        }
        return smax;
    };
    // (a DEM time step has 10^5 instances and a synchronous hrt_tlas_update derives these on the host in every frame: a few threads then --
    // every instance writes its own entries, the largest coordinate is a maximum: the result does not depend on the split)
    const unsigned hw = std::min((unsigned)std::max(g_instance_table_threads, 1), std::max(1u, std::thread::hardware_concurrency()));
    if (n < 32768u || hw < 2u) return range(0, n);
    std::vector<float> part(hw, 1.0f);
    std::vector<std::thread> pool;
    for (unsigned k = 1; k < hw; ++k) pool.emplace_back([&, k] { part[k] = range(n * k / hw, n * (k + 1) / hw); });
    part[0] = range(0, n / hw);
    for (std::thread &th : pool) th.join();
    return *std::max_element(part.begin(), part.end());
}

// The host builder needs the geometry on the host: fetched from the BLAS's device copy the first time it is asked for
// (HRT_BUILD=host only; the device build never brings geometry across the bus).
int ensure_host_geometry(HrtContext *ctx, Blas &b, hipStream_t s) {
    std::lock_guard<std::mutex> lk(b.tmpl_mu);
    if (b.host_geometry || b.n_prims == 0) { b.host_geometry = true; return HRT_OK; }
    if (b.kind == kPrimKindTriangle) {
        b.verts.resize(9 * (size_t)b.n_prims);
        HIP_TRY(ctx, hipMemcpyAsync(b.verts.data(), b.d_verts, sizeof(float) * b.verts.size(), hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipStreamSynchronize(s));
    } else {
        std::vector<float> cr(4 * (size_t)b.n_prims);
        HIP_TRY(ctx, hipMemcpyAsync(cr.data(), b.d_verts, sizeof(float) * cr.size(), hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipStreamSynchronize(s));
        b.centers.resize(3 * (size_t)b.n_prims); b.radii.resize(b.n_prims);
        for (size_t p = 0; p < b.n_prims; ++p) { for (int a = 0; a < 3; ++a) b.centers[3 * p + a] = cr[4 * p + a]; b.radii[p] = cr[4 * p + 3]; }
    }
    b.host_geometry = true;
    return HRT_OK;
}

// ---- what the device builds share (ensure_template, ensure_split_template, build_merged_on_device, build_two_level) ----
static size_t align256(size_t x) { return (x + 255u) & ~(size_t)255u; }
static float refit_pad(float scene_scale) { return 4e-6f * std::max(1.0f, scene_scale); }

// A build's arena holds its staged output and small tables in front of the build's own working memory.  take() lays them out, each
// 256-aligned, before the arena exists (`used` is what they need in all); at() gives the pointers once it does.
struct ArenaLayout {
    size_t used = 0;
    unsigned char *base = nullptr;
    size_t take(size_t bytes) { const size_t at = used; used += align256(bytes); return at; }
    template <class T> T *at(size_t offset) const { return reinterpret_cast<T *>(base + offset); }
};

// The part of a device build's input that comes from the context's knobs; what differs between the builds is in the arguments (`topdown`: the
// top-down phase of build_split.hip in front of PLOC, with `split_budget` extra references per primitive for spatial splits; `pad`: the
// padding its SAH areas are computed with).  The instance tables and the output buffers are the caller's.
static GpuBuildInput build_input(const HrtContext *ctx, uint32_t max_leaf_prims, float c_prim, bool instance_leaves, bool topdown, float split_budget, float pad) {
    GpuBuildInput in{};
    in.max_leaf_prims = max_leaf_prims; in.instance_leaves = instance_leaves;
    in.width = (uint32_t)ctx->build_width; in.c_node = ctx->build_c_node; in.c_prim = c_prim; in.ploc_radius = ctx->ploc_radius; in.quant_guard = ctx->quant_guard;
    in.split.enabled = topdown; in.split.budget_frac = split_budget; in.split.alpha = ctx->split_alpha; in.split.bias = ctx->split_bias; in.split.cut_bias = ctx->split_cut_bias;
    in.split.cell_refs = (uint32_t)ctx->split_cell_refs; in.split.pad = pad; in.split.verbose = ctx->build_verbose;
    return in;
}

// One device build (build.hip) staged in ONE block of the context's working memory: the caller's own small tables in front (lay.take,
// before stage()), then the build's worst-case output -- a node and two reference floats per entry (primitive, or reference of a spatial
// split), the records where the caller has no block of its own for them, their clip boxes where the build splits -- then the build's own
// arrays: a build allocates and frees nothing (eight hipMalloc / hipFree pairs used to cost more than a template's build).  `in`: build_input's,
// with the counts, the instance tables and the strides filled in.
enum class StagedRecords { None, Records, RecordsAndClip };
struct StagedBuild {
    HrtContext *ctx; hipStream_t s;
    ArenaLayout lay; ScratchArena arena;
    size_t want = 0;      // what stage() asked for (first)
    // The arena goes back to the context when the build's scope ends, however it ends.  On an error path kernels may still be writing to
    // it: the stream is synchronised first, so that another loader thread is not handed it before they are done.
    ~StagedBuild() { if (arena.p) { (void)hipStreamSynchronize(s); scratch_release(ctx, arena); } }

    // Lays the output out, acquires the arena and points in.out_* / in.scratch into it.  False when the working memory is not to be had --
    // what then is the caller's business; or_without_topdown: then the build goes without the top-down phase's buffers, PLOC alone.
    bool stage(GpuBuildInput &in, size_t max_entries, StagedRecords records, bool or_without_topdown) {
        const size_t o_nodes = lay.take((size_t)in.node_stride * max_entries), o_ref = lay.take(sizeof(float) * 2 * max_entries);
        const size_t o_prims = lay.take(records != StagedRecords::None ? (size_t)in.prim_stride * max_entries : 0u);
        const size_t o_clip = lay.take(records == StagedRecords::RecordsAndClip ? sizeof(float) * 6 * max_entries : 0u);
        want = lay.used + gpu_build_scratch_bytes(in.n_prims, &in.split);
        arena = scratch_acquire(ctx, want);
        if (!arena.p && or_without_topdown && in.split.enabled) {
            in.split.enabled = false;
            arena = scratch_acquire(ctx, lay.used + gpu_build_scratch_bytes(in.n_prims, &in.split));
        }
        if (!arena.p) return false;
        lay.base = static_cast<unsigned char *>(arena.p);
        in.out_nodes = lay.at<unsigned char>(o_nodes); in.out_node_ref = lay.at<float>(o_ref);
        if (records != StagedRecords::None) in.out_prims = lay.at<unsigned char>(o_prims);
        if (records == StagedRecords::RecordsAndClip) in.out_clip = lay.at<float>(o_clip);
        in.scratch = lay.base + lay.used; in.scratch_bytes = arena.bytes - lay.used;
        return true;
    }
    // The build itself (it synchronises the stream before it returns); `what`: the caller's name for it in the error text.
    int build(const GpuBuildInput &in, const char *what, GpuBuildResult &r) {
        r = gpu_build_bvh8(in, s);
        if (r.error != hipSuccess) return fail(ctx, r.error == hipErrorOutOfMemory ? HRT_ERR_OOM : HRT_ERR_HIP, "%s failed: %s (%s)", what, hipGetErrorString(r.error), r.where);
        return HRT_OK;
    }
};

// The build over ONE BLAS in its own space, a single identity instance (`in`: the knobs), into packed 80 / 48 byte records staged in `sb`.
// The five small instance tables share the arena.  no_memory: nothing was built, the working memory is not to be had.
static int build_blas_tree(const Blas &b, GpuBuildInput &in, StagedRecords records, const char *what, StagedBuild &sb, GpuBuildResult &r, bool &no_memory) {
    HrtContext *ctx = sb.ctx; const hipStream_t s = sb.s;
    const uint32_t h_first[2] = {0u, b.n_prims}, h_kind = b.kind, h_ident = 1u;
    const float h_xf[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    const void *h_src = b.d_verts;
    ArenaLayout &lay = sb.lay;
    const size_t o_first = lay.take(sizeof h_first), o_kind = lay.take(sizeof h_kind), o_src = lay.take(sizeof h_src), o_xf = lay.take(sizeof h_xf), o_ident = lay.take(sizeof h_ident);
    in.n_prims = b.n_prims; in.n_inst = 1; in.node_stride = sizeof(Bvh8Node); in.prim_stride = sizeof(PrimRecord);
    no_memory = !sb.stage(in, gpu_build_max_refs(b.n_prims, &in.split), records, false);
    if (no_memory) return HRT_OK;
    HIP_TRY(ctx, hipMemcpyAsync(lay.base + o_first, h_first, sizeof h_first, hipMemcpyHostToDevice, s)); HIP_TRY(ctx, hipMemcpyAsync(lay.base + o_kind, &h_kind, 4, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(lay.base + o_src, &h_src, sizeof(void *), hipMemcpyHostToDevice, s)); HIP_TRY(ctx, hipMemcpyAsync(lay.base + o_xf, h_xf, sizeof h_xf, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(lay.base + o_ident, &h_ident, 4, hipMemcpyHostToDevice, s));
    in.d_inst_first = lay.at<const uint32_t>(o_first); in.d_inst_kind = lay.at<const uint32_t>(o_kind);
    in.d_inst_src = lay.at<const void *const>(o_src); in.d_inst_xf = lay.at<const float>(o_xf);
    in.d_inst_identity = lay.at<const uint32_t>(o_ident);
    return sb.build(in, what, r);
}

// Refit phases of a tree stored breadth first (nodes of level l: [level_begin[l], level_begin[l + 1])): a level each, children before parents.
static std::vector<std::pair<uint32_t, uint32_t>> phases_from_levels(const std::vector<uint32_t> &level_begin) {
    std::vector<std::pair<uint32_t, uint32_t>> phases;
    for (size_t l = level_begin.size(); l-- > 1;) phases.emplace_back(level_begin[l - 1], level_begin[l] - level_begin[l - 1]);
    return phases;
}

// A tree no kernel can walk: 2 * depth + 2 entries of the traversal stack (device_types.h)
static bool too_deep(uint32_t max_depth) { return 2 * max_depth + 2 > kTraversalStackEntries; }

// Primitive p of a BLAS under an instance's transform, as the host builder takes it (the host geometry is there: ensure_host_geometry).
static BuildPrim build_prim_of(const Blas &b, uint32_t p, const float *m, bool identity, uint32_t inst) {
    BuildPrim bp; std::memset(&bp, 0, sizeof bp);
    if (b.kind == kPrimKindTriangle) {
        triangle_world(&b.verts[9 * (size_t)p], m, identity, bp.rec.a, bp.rec.b, bp.rec.c, bp.lo, bp.hi);
    } else {
        const float *c = &b.centers[3 * (size_t)p];
        bp.rec.a[0] = c[0]; bp.rec.a[1] = c[1]; bp.rec.a[2] = c[2]; bp.rec.b[0] = b.radii[p];
        sphere_world_bounds(c, b.radii[p], m, identity, bp.lo, bp.hi);
    }
    bp.rec.prim = p; bp.rec.inst = inst; bp.rec.kind = b.kind;
    return bp;
}

// the split build's working memory (~1.2 KB per primitive with the staged output) has to be there: otherwise the default build
static bool split_build_fits(HrtContext *ctx, uint32_t n_prims) {
    SplitParams probe; probe.enabled = true; probe.budget_frac = ctx->split_budget; probe.cell_refs = (uint32_t)ctx->split_cell_refs;
    const size_t leaves = gpu_build_max_refs(n_prims, &probe);
    const size_t want = gpu_build_scratch_bytes(n_prims, &probe) + leaves * (size_t)(128 + 8 + ctx->prim_stride + 24);
    size_t free_b = 0, total_b = 0, kept = 0;      // (what the context keeps for later counts as free: an allocation that fails gives it back first)
    { std::lock_guard<std::mutex> lk(ctx->scratch_mu); for (const ScratchArena &x : ctx->scratch_free) kept += x.bytes; }
    { std::lock_guard<std::mutex> lk(ctx->pool_mu); kept += ctx->pool_bytes; }
    return leaves <= (1u << 30) && hipMemGetInfo(&free_b, &total_b) == hipSuccess && want <= (free_b + kept) / 10 * 9;
}

// ---- refits: of an update (refit_tlas, hrt_tlas_update) and the one that completes a build ----
// The phases of a refit, children before parents: wide phases get a launch each, the narrow ones at the end (the top
// of the tree, or all of a small tree) run in one single-workgroup launch.
void launch_refit_phases(RefitArgs ra, const std::vector<std::pair<uint32_t, uint32_t>> &phases, hipStream_t s) {
    launch_refit_records(ra, s);                               // (small trees: ra.rec_box)
    size_t tail = phases.size();
    while (tail > 0 && phases.size() - tail < kRefitTopLevels && phases[tail - 1].second <= kRefitTopLevelNodes) --tail;
    for (size_t i = 0; i < tail; ++i) { ra.first_node = phases[i].first; ra.n_nodes = phases[i].second; launch_refit_level(ra, s); }
    RefitLevels top{};
    for (size_t i = tail; i < phases.size(); ++i) { top.first[top.n_levels] = phases[i].first; top.count[top.n_levels] = phases[i].second; ++top.n_levels; }
    launch_refit_top(ra, top, s);
}

// Small trees (the reference's own scenes) are refitted in one workgroup that walks the levels; the records' arithmetic -- most of the
// work, and a chain of dependent loads -- runs before that, a thread per record, into 24 bytes per record (k_refit_records).
constexpr uint32_t kRecBoxMaxRecords = 65536;
static void attach_rec_box(HrtContext *ctx, Tlas &t, RefitArgs &ra, uint32_t n_records) {
    if (n_records == 0u || n_records > kRecBoxMaxRecords) return;
    if (!t.dev.d_rec_box && pool_alloc(ctx, (void **)&t.dev.d_rec_box, sizeof(float) * 6 * (size_t)n_records) != hipSuccess) { (void)hipGetLastError(); t.dev.d_rec_box = nullptr; return; }
    ra.rec_box = t.dev.d_rec_box; ra.n_records = n_records;
}

// What every refit of a tree takes from it (its counts and two_level are set).  The caller adds what differs: the padding (`pad`, or `scale_bits`
// when the scene scale is on the device), `area_sum` or `write_reference`, `clip`.
static RefitArgs refit_args(HrtContext *ctx, Tlas &t) {
    const TlasDevice &d = t.dev;
    RefitArgs ra{};
    ra.nodes = reinterpret_cast<unsigned char *>(d.d_nodes); ra.node_stride = t.node_stride;
    ra.prims = reinterpret_cast<unsigned char *>(d.d_prims); ra.prim_stride = t.prim_stride;
    ra.node_box = d.d_node_box; ra.node_ref = d.d_node_ref; ra.inst_xf = d.d_inst_xf; ra.inst_identity = d.d_inst_identity; ra.inst_src = d.d_inst_src;
    ra.order = d.d_order;
    if (t.two_level) { ra.inst_inv = d.d_inst_inv; ra.inst_root = d.d_inst_root; }      // (the top level only: transform nodes and the boxes above them)
    else attach_rec_box(ctx, t, ra, t.n_prims);
    if (t.keeps_splits) { ra.clip = d.d_keep_clip; ra.bary = d.d_keep_bary; ra.inst_changed = d.d_inst_changed; }      // (every refit after the build's own)
    return ra;
}

// The refit that completes a build (t.phases are set; enqueued only): the device computes what the builder left blank -- world-space records,
// boxes, origins, exponents, quantised children -- and the built areas the quality guard compares later refits with.  clip: RefitArgs::clip.
static int reference_refit(HrtContext *ctx, Tlas &t, float pad, const float *clip, hipStream_t s) {
    RefitArgs ra = refit_args(ctx, t);
    ra.pad = pad; ra.write_reference = 1u; ra.clip = clip;
    launch_refit_phases(ra, t.phases, s);
    HIP_TRY(ctx, hipGetLastError());
    return HRT_OK;
}

// ---- the object-space trees of a BLAS (BlasTree): the template and, under HRT_CTX_FAST_TRACE, the tree with spatial splits ----
// Device memory a BLAS will own, while it is being filled: freed again unless everything arrived and the pointers were handed over -- a BLAS
// never shows a tree of which only a part is there (several loader threads share the BLASes).
struct PendingBlocks {
    void *p[3] = {nullptr, nullptr, nullptr};
    ~PendingBlocks() { for (void *q : p) if (q) (void)hipFree(q); }
};
// A finished object-space tree -- `staged`: its counts and levels, with pointers into the host's copy or the build's arena (`kind` says
// which) -- goes into blocks of its own, and `out` gets all of it once all of it is there.  oom_is_not_now: no room for the tree to stay is no
// error, `out` stays empty (d_nodes == NULL) and a later TLAS may try again.
static int keep_blas_tree(HrtContext *ctx, const BlasTree &staged, hipMemcpyKind kind, bool oom_is_not_now, hipStream_t s, BlasTree &out) {
    PendingBlocks blk;
    const void *src[3] = {staged.d_nodes, staged.d_prims, staged.d_clip};
    const size_t bytes[3] = {sizeof(Bvh8Node) * (size_t)staged.n_nodes, sizeof(PrimRecord) * (size_t)staged.n_records, sizeof(float) * 6 * (size_t)staged.n_records};
    const int n_blocks = staged.d_clip ? 3 : 2;
    for (int k = 0; k < n_blocks; ++k) {
        const hipError_t e = hipMalloc(&blk.p[k], std::max(bytes[k], k == 1 ? sizeof(PrimRecord) : (size_t)0));
        if (e == hipErrorOutOfMemory && oom_is_not_now) { (void)hipGetLastError(); blk.p[k] = nullptr; return HRT_OK; }
        HIP_TRY(ctx, e);
    }
    for (int k = 0; k < n_blocks; ++k) if (bytes[k]) HIP_TRY(ctx, hipMemcpyAsync(blk.p[k], src[k], bytes[k], kind, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    out = staged;
    out.d_nodes = static_cast<unsigned char *>(blk.p[0]); out.d_prims = static_cast<unsigned char *>(blk.p[1]); out.d_clip = static_cast<float *>(blk.p[2]);
    for (void *&q : blk.p) q = nullptr;      // (handed over)
    return HRT_OK;
}
// Object-space BVH8 of one BLAS (built once): the subtree every instance of it gets in a tree over instances.  Built on the
// device like everything else (one identity instance); only its topology -- nodes' child / primitive bases, masks, the
// primitive ids -- comes back to the host, where assemble_instanced_bvh8 stitches instance subtrees under a top tree.
static int template_to_device(HrtContext *ctx, Blas &b, hipStream_t s) {
    if (b.tmpl_dev.d_nodes || b.tmpl.nodes.empty()) return HRT_OK;
    BlasTree staged;
    staged.d_nodes = reinterpret_cast<unsigned char *>(b.tmpl.nodes.data()); staged.d_prims = reinterpret_cast<unsigned char *>(b.tmpl.prims.data());
    staged.n_nodes = (uint32_t)b.tmpl.nodes.size(); staged.n_records = (uint32_t)b.tmpl.prims.size();
    staged.n_triangles = b.tmpl.n_triangles; staged.n_spheres = b.tmpl.n_spheres; staged.max_depth = b.tmpl.max_depth; staged.level_begin = b.tmpl.level_begin;
    return keep_blas_tree(ctx, staged, hipMemcpyHostToDevice, false, s, b.tmpl_dev);
}
// keep_device: the topology also stays on the device (Blas::tmpl_dev), for two-level TLASes to copy from
int ensure_template(HrtContext *ctx, Blas &b, hipStream_t s, bool keep_device = false) {
    if (!ctx->build_on_device) {
        const int rc = ensure_host_geometry(ctx, b, s);
        if (rc != HRT_OK) return rc;
    }
    std::lock_guard<std::mutex> lk(b.tmpl_mu);
    if (b.tmpl_built) return keep_device ? template_to_device(ctx, b, s) : HRT_OK;
    if (!ctx->build_on_device) {
        std::vector<BuildPrim> prims;
        prims.reserve(b.n_prims);
        for (uint32_t p = 0; p < b.n_prims; ++p) {
            const BuildPrim bp = build_prim_of(b, p, nullptr, true, 0u);
            if (finite_box(bp.lo, bp.hi)) prims.push_back(bp);
        }
        build_bvh8(prims, b.tmpl, 0);
        b.tmpl_built = true;
        return keep_device ? template_to_device(ctx, b, s) : HRT_OK;
    }
    b.tmpl = Bvh8();
    const uint32_t n = b.n_prims;
    if (n == 0) { build_bvh8({}, b.tmpl, 1); b.tmpl_built = true; return HRT_OK; }
    GpuBuildInput in = build_input(ctx, kMaxLeafPrims, ctx->build_c_prim_bodies, false, false, 0.0f, 0.0f);      // (no top-down phase)
    StagedBuild sb{ctx, s}; GpuBuildResult r; bool no_memory;
    const int rc = build_blas_tree(b, in, StagedRecords::Records, "device build of a BLAS template", sb, r, no_memory);
    if (rc != HRT_OK) return rc;
    if (no_memory) return fail(ctx, HRT_ERR_OOM, "device build of a BLAS template: no working memory");
    if (r.n_prims == 0) { build_bvh8({}, b.tmpl, 1); b.tmpl_built = true; return HRT_OK; }
    b.tmpl.nodes.resize(r.n_nodes); b.tmpl.prims.resize(r.n_prims);
    HIP_TRY(ctx, hipMemcpyAsync(b.tmpl.nodes.data(), in.out_nodes, sizeof(Bvh8Node) * (size_t)r.n_nodes, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(b.tmpl.prims.data(), in.out_prims, sizeof(PrimRecord) * (size_t)r.n_prims, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    b.tmpl.max_depth = r.max_depth; b.tmpl.level_begin = r.level_begin;
    if (b.kind == kPrimKindTriangle) b.tmpl.n_triangles = r.n_prims; else b.tmpl.n_spheres = r.n_prims;
    b.tmpl_built = true;
    return keep_device ? template_to_device(ctx, b, s) : HRT_OK;
}

// The split tree of a BLAS (Blas::split): the same build over one identity instance, with the top-down phase and the context's budget of
// extra references -- as build_merged_on_device(.., device_split = true) builds the flattened scene.  Its record count is known afterwards:
// nodes, records and clip boxes are staged in the arena and copied into blocks of their own, which the BLAS gets once all of it is there.
// Leaves b.split empty (and the unsplit template in charge, byte for byte as without HRT_CTX_FAST_TRACE) where the split phase does not run:
// 4096 primitives or fewer (build.hip), a phase that gave up, a tree no kernel could walk; and where its working memory is not to be had.
static int ensure_split_template(HrtContext *ctx, Blas &b, hipStream_t s) {
    std::lock_guard<std::mutex> lk(b.tmpl_mu);
    if (b.split_decided) return HRT_OK;
    const uint32_t n = b.n_prims;
    if (n <= 4096u) { b.split_decided = true; return HRT_OK; }
    if (!split_build_fits(ctx, n)) return HRT_OK;      // (not for ever: a later TLAS may find the memory)
    float scale = 1.0f;
    for (int a = 0; a < 3; ++a) { if (std::isfinite(b.lo[a])) scale = std::max(scale, std::fabs(b.lo[a])); if (std::isfinite(b.hi[a])) scale = std::max(scale, std::fabs(b.hi[a])); }
    GpuBuildInput in = build_input(ctx, kMaxLeafPrims, ctx->build_c_prim_bodies, false, true, ctx->split_budget, refit_pad(scale));
    StagedBuild sb{ctx, s}; GpuBuildResult r; bool no_memory;
    int rc = build_blas_tree(b, in, StagedRecords::RecordsAndClip, "device build of a BLAS's split tree", sb, r, no_memory);
    if (rc != HRT_OK || no_memory) return rc;                        // (no working memory: as above)
    if (ctx->build_verbose)
        std::fprintf(stderr, "[hrt] split tree of a BLAS: %u primitives -> %u records, %u nodes, depth %u, %u split levels, %u cells%s\n",
                     r.n_prims, r.n_records, r.n_nodes, r.max_depth, r.split_levels, r.n_cells, r.split_levels ? "" : " (not used: the unsplit template serves)");
    if (r.n_prims == 0u || r.split_levels == 0u || too_deep(r.max_depth)) { b.split_decided = true; return HRT_OK; }
    BlasTree staged;
    staged.d_nodes = in.out_nodes; staged.d_prims = in.out_prims; staged.d_clip = in.out_clip;
    staged.n_nodes = r.n_nodes; staged.n_records = r.n_records; staged.max_depth = r.max_depth; staged.level_begin = r.level_begin;
    staged.n_triangles = b.kind == kPrimKindTriangle ? r.n_prims : 0u; staged.n_spheres = b.kind == kPrimKindTriangle ? 0u : r.n_prims;
    // (no room for the tree to stay: like working memory that is not to be had -- the unsplit template serves, and a later TLAS may try again)
    rc = keep_blas_tree(ctx, staged, hipMemcpyDeviceToDevice, true, s, b.split);
    if (rc == HRT_OK && b.split.d_nodes) b.split_decided = true;
    return rc;
}

// Build a TLAS and upload it together with the tables the device refit needs (hrt_tlas_update).  What is built (TreeKind):
//  * merged (default of hrt_tlas_build): every instance is flattened into world space and ONE tree is built over all
//    primitives -- the best tree, at the price of a full SAH build; on the device (with spatial splits under HRT_CTX_FAST_TRACE),
//    or by the host builder (HRT_BUILD=host);
//  * over instances: a top tree over the instances' boxes whose leaves are per-instance copies of object-space template
//    trees; only the topology comes from the host (milliseconds for thousands of instances), the device refit
//    computes every box and world-space record.  The shape the reference's own scenes have (particles instancing a
//    few shapes); used when a refitted tree has degraded and has to be rebuilt while frames are being rendered;
//  * two levels: transform nodes over one shared tree per BLAS.
// But for the last, the result is one world-space BVH8: the traversal kernels do not know the difference.
enum class TreeKind { HostFlattened, OverInstances, DeviceMerged, DeviceSplit, TwoLevel };
struct BuildPlan {
    TreeKind kind = TreeKind::HostFlattened;
    // global primitive numbering of the merged builds: instance after instance, invisible instances contribute nothing
    std::vector<uint32_t> first;
    uint32_t n_tri_in = 0;                                           // triangles among them
    std::vector<Blas *> uniq; std::vector<uint32_t> slot_of;        // TwoLevel: the BLASes that have instances in the tree; per instance, which of them
};

// ---- the tables every structure needs: per instance the transform, its inverse, the identity flag and `src`, what the refit takes as the
//      instance's geometry (the BLAS's vertices; the top level of a two-level tree: its bounds); the word the refit's area sum goes to; and
//      what asynchronous updates compare against and transform on the device ----
static int upload_instance_tables(HrtContext *ctx, Tlas &t, const std::vector<const void *> &src, hipStream_t s) {
    const uint32_t n = t.n_instances;
    TlasDevice &d = t.dev;
    HIP_TRY(ctx, pool_alloc(ctx, (void **)&d.d_inst_inv, sizeof(float) * t.h_inv.size()));
    HIP_TRY(ctx, pool_alloc(ctx, (void **)&d.d_inst_xf, sizeof(float) * t.h_xf.size()));
    HIP_TRY(ctx, pool_alloc(ctx, (void **)&d.d_inst_identity, sizeof(uint32_t) * t.h_ident.size()));
    HIP_TRY(ctx, pool_alloc(ctx, (void **)&d.d_inst_src, sizeof(void *) * src.size()));
    HIP_TRY(ctx, pool_alloc(ctx, (void **)&d.d_area, sizeof(float)));
    if (!t.h_area) HIP_TRY(ctx, hipHostMalloc((void **)&t.h_area, sizeof(float), hipHostMallocDefault));
    if (!t.area_ready) HIP_TRY(ctx, hipEventCreateWithFlags(&t.area_ready, hipEventDisableTiming));
    HIP_TRY(ctx, hipMemcpyAsync(d.d_inst_inv, t.h_inv.data(), sizeof(float) * t.h_inv.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(d.d_inst_xf, t.h_xf.data(), sizeof(float) * t.h_xf.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(d.d_inst_identity, t.h_ident.data(), sizeof(uint32_t) * t.h_ident.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync((void *)d.d_inst_src, src.data(), sizeof(void *) * src.size(), hipMemcpyHostToDevice, s));
    // what asynchronous updates compare against and transform on the device
    std::vector<float> bbox(6 * (size_t)std::max(n, 1u), 0.0f);
    for (uint32_t i = 0; i < n; ++i) for (int a = 0; a < 3; ++a) { bbox[6 * (size_t)i + a] = t.blas_refs[i]->lo[a]; bbox[6 * (size_t)i + 3 + a] = t.blas_refs[i]->hi[a]; }
    std::vector<unsigned long long> sigh(std::max(n, 1u), 0ull);
    for (uint32_t i = 0; i < n; ++i) sigh[i] = t.sig_handle[i];
    HIP_TRY(ctx, pool_alloc(ctx, (void **)&d.d_sig_handle, sizeof(unsigned long long) * sigh.size()));
    HIP_TRY(ctx, pool_alloc(ctx, (void **)&d.d_sig_visibility, sizeof(uint32_t) * std::max(n, 1u)));
    HIP_TRY(ctx, pool_alloc(ctx, (void **)&d.d_sig_sbt, sizeof(uint32_t) * std::max(n, 1u)));
    HIP_TRY(ctx, pool_alloc(ctx, (void **)&d.d_blas_box, sizeof(float) * bbox.size()));
    HIP_TRY(ctx, pool_alloc(ctx, (void **)&d.d_update_flags, sizeof(uint32_t) * 2));
    if (!t.h_update_flags) HIP_TRY(ctx, hipHostMalloc((void **)&t.h_update_flags, sizeof(uint32_t) * 4, hipHostMallocDefault));
    t.h_update_flags[0] = t.h_update_flags[2] = 0x3f800000u; t.h_update_flags[1] = t.h_update_flags[3] = 0u;
    HIP_TRY(ctx, hipMemcpyAsync(d.d_sig_handle, sigh.data(), sizeof(unsigned long long) * sigh.size(), hipMemcpyHostToDevice, s));
    if (n) HIP_TRY(ctx, hipMemcpyAsync(d.d_sig_visibility, t.sig_visibility.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice, s));
    if (n) HIP_TRY(ctx, hipMemcpyAsync(d.d_sig_sbt, t.sbt_offset.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(d.d_blas_box, bbox.data(), sizeof(float) * bbox.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));            // (the staging vectors, and the caller's `src`, go out of scope)
    return HRT_OK;
}
// ... with the BLASes' vertices as the geometry: every structure but the two-level one
static int upload_instance_tables(HrtContext *ctx, Tlas &t, hipStream_t s) {
    std::vector<const void *> src(std::max(t.n_instances, 1u), nullptr);
    for (uint32_t i = 0; i < t.n_instances; ++i) src[i] = t.blas_refs[i]->d_verts;
    return upload_instance_tables(ctx, t, src, s);
}

// ---- the pool blocks every tree has: nodes (n_nodes of them and node_tail bytes), a box and a reference area per node, records (one at
//      least; the block the caller already made for them stays).  Leaves the tree's size on the device in t.alloc_bytes. ----
static int alloc_tree_blocks(HrtContext *ctx, Tlas &t, size_t n_nodes, size_t node_tail, size_t n_records) {
    TlasDevice &d = t.dev;
    const size_t nb = (size_t)t.node_stride * n_nodes, rows = std::max<size_t>(n_nodes, 1), pb = (size_t)t.prim_stride * std::max<size_t>(n_records, 1);
    HIP_TRY(ctx, pool_alloc(ctx, &d.d_nodes, nb + node_tail));
    HIP_TRY(ctx, pool_alloc(ctx, (void **)&d.d_node_box, sizeof(float) * 6 * rows));
    HIP_TRY(ctx, pool_alloc(ctx, (void **)&d.d_node_ref, sizeof(float) * 2 * rows));
    if (!d.d_prims) HIP_TRY(ctx, pool_alloc(ctx, &d.d_prims, pb));
    t.alloc_bytes = (uint64_t)nb + sizeof(float) * 8 * rows + pb;
    return HRT_OK;
}

// ---- a host-built tree (t.bvh; `order`: the refit order of a tree over instances, empty otherwise) goes to the device ----
static int upload_host_tree(HrtContext *ctx, Tlas &t, const std::vector<uint32_t> &order, hipStream_t s) {
    if (too_deep(t.bvh.max_depth)) return fail(ctx, HRT_ERR_INVALID, "BVH depth %u exceeds the traversal stack", t.bvh.max_depth);
    int rc = upload_instance_tables(ctx, t, s);
    if (rc != HRT_OK) return rc;
    TlasDevice &d = t.dev;
    const size_t n_nodes = t.bvh.nodes.size(), n_prims = t.bvh.prims.size();
    const size_t nb = (size_t)t.node_stride * n_nodes;
    const size_t pb = (size_t)t.prim_stride * std::max<size_t>(n_prims, 1);
    rc = alloc_tree_blocks(ctx, t, n_nodes, 0, n_prims);
    if (rc != HRT_OK) return rc;
    if (!order.empty()) HIP_TRY(ctx, pool_alloc(ctx, (void **)&d.d_order, sizeof(uint32_t) * order.size()));
    if (t.node_stride == sizeof(Bvh8Node) && t.prim_stride == sizeof(PrimRecord)) {
        HIP_TRY(ctx, hipMemcpyAsync(d.d_nodes, t.bvh.nodes.data(), nb, hipMemcpyHostToDevice, s));
        if (n_prims) HIP_TRY(ctx, hipMemcpyAsync(d.d_prims, t.bvh.prims.data(), sizeof(PrimRecord) * n_prims, hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipStreamSynchronize(s));
    } else {
        std::vector<unsigned char> hn(nb, 0), hp(pb, 0);
        for (size_t i = 0; i < n_nodes; ++i) std::memcpy(&hn[i * t.node_stride], &t.bvh.nodes[i], sizeof(Bvh8Node));
        for (size_t i = 0; i < n_prims; ++i) std::memcpy(&hp[i * t.prim_stride], &t.bvh.prims[i], sizeof(PrimRecord));
        HIP_TRY(ctx, hipMemcpyAsync(d.d_nodes, hn.data(), nb, hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipMemcpyAsync(d.d_prims, hp.data(), pb, hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipStreamSynchronize(s));
    }
    if (!t.bvh.node_box.empty())
        HIP_TRY(ctx, hipMemcpyAsync(d.d_node_box, t.bvh.node_box.data(), sizeof(float) * t.bvh.node_box.size(), hipMemcpyHostToDevice, s));
    if (!t.bvh.node_ref.empty())
        HIP_TRY(ctx, hipMemcpyAsync(d.d_node_ref, t.bvh.node_ref.data(), sizeof(float) * t.bvh.node_ref.size(), hipMemcpyHostToDevice, s));
    if (!order.empty()) HIP_TRY(ctx, hipMemcpyAsync(d.d_order, order.data(), sizeof(uint32_t) * order.size(), hipMemcpyHostToDevice, s));
    t.n_nodes = (uint32_t)n_nodes; t.n_prims = (uint32_t)n_prims;
    t.n_triangles = t.bvh.n_triangles; t.n_spheres = t.bvh.n_spheres; t.max_depth = t.bvh.max_depth;
    for (int a = 0; a < 3; ++a) { t.lo[a] = t.bvh.lo[a]; t.hi[a] = t.bvh.hi[a]; }
    return HRT_OK;
}

// ---- the host's binned-SAH build over the flattened scene (HRT_BUILD=host), and the empty scene ----
static int build_flattened_on_host(HrtContext *ctx, Tlas &t, const std::vector<HrtInstance> &inst, uint32_t n_prims_in, float scene_scale, bool fast_trace, hipStream_t s) {
    std::vector<BuildPrim> prims;
    prims.reserve(n_prims_in);
    for (uint32_t i = 0; i < t.n_instances && n_prims_in; ++i) {
        Blas &b = *t.blas_refs[i];
        if ((inst[i].visibilityMask & 1u) == 0) continue;
        const int rc = ensure_host_geometry(ctx, b, s);
        if (rc != HRT_OK) return rc;
        for (uint32_t p = 0; p < b.n_prims; ++p) {
            const BuildPrim bp = build_prim_of(b, p, inst[i].transform, t.h_ident[i] != 0u, i);
            // NaN / Inf geometry never hits anything; keep it out of the tree
            if (!finite_box(bp.lo, bp.hi)) continue;
            prims.push_back(bp);
        }
    }
    // HRT_CTX_FAST_TRACE: the static-scene tree, with spatial splits (a later refit recomputes the boxes from whole primitives:
    // valid, conservative, and without the splits' benefit -- the quality guard of hrt_tlas_update then rebuilds on the device)
    build_bvh8(prims, t.bvh, 0, scene_scale, kMaxLeafPrims, fast_trace);
    t.has_split_refs = t.bvh.prims.size() > prims.size();
    t.phases = phases_from_levels(t.bvh.level_begin);
    return upload_host_tree(ctx, t, {}, s);
}

// ---- a tree over instances: the host stitches per-instance copies of the BLASes' template trees under a top tree over the instances' boxes
//      (topology only); the device refit computes the rest ----
static int build_over_instances(HrtContext *ctx, Tlas &t, const std::vector<HrtInstance> &inst, float scene_scale, hipStream_t s) {
    const uint32_t n = t.n_instances;
    std::vector<const Bvh8 *> tmpl(n, nullptr);
    std::vector<float> box(6 * (size_t)std::max(n, 1u), 0.0f);
    for (uint32_t i = 0; i < n; ++i) {
        Blas &b = *t.blas_refs[i];
        if (!instance_has_box(inst[i], b)) continue;
        float w[8][3], lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        blas_box_corners(b, inst[i].transform, t.h_ident[i] != 0u, w);
        for (int c = 0; c < 8; ++c)
            for (int a = 0; a < 3; ++a) { lo[a] = std::fmin(lo[a], w[c][a]); hi[a] = std::fmax(hi[a], w[c][a]); }
        if (!finite_box(lo, hi)) continue;                                                 // a NaN transform: nothing to hit
        const int rc = ensure_template(ctx, b, s);
        if (rc != HRT_OK) return rc;
        tmpl[i] = &b.tmpl;
        for (int a = 0; a < 3; ++a) { box[6 * (size_t)i + a] = lo[a]; box[6 * (size_t)i + 3 + a] = hi[a]; }
    }
    InstancedTree it;
    assemble_instanced_bvh8(tmpl, box, it);
    t.bvh = Bvh8();
    t.bvh.nodes = std::move(it.nodes); t.bvh.prims = std::move(it.prims);
    t.bvh.n_triangles = it.n_triangles; t.bvh.n_spheres = it.n_spheres; t.bvh.max_depth = it.max_depth;
    t.bvh.node_box.assign(6 * t.bvh.nodes.size(), 0.0f);
    t.bvh.node_ref.assign(2 * t.bvh.nodes.size(), 0.0f);
    for (size_t i = 0; i < it.weight.size(); ++i) t.bvh.node_ref[2 * i] = it.weight[i];
    for (size_t h = 0; h + 1 < it.phase_begin.size(); ++h) t.phases.emplace_back(it.phase_begin[h], it.phase_begin[h + 1] - it.phase_begin[h]);
    int rc = upload_host_tree(ctx, t, it.order, s);
    if (rc == HRT_OK && t.n_prims) rc = reference_refit(ctx, t, refit_pad(scene_scale), nullptr, s);      // (the host left all but the topology blank)
    if (rc != HRT_OK) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(s));            // (it.order goes out of scope)
    return HRT_OK;
}

// ---- HRT_CTX_KEEP_SPLITS: what a flattened split tree keeps so that later refits keep its split references' boxes --
//      the as-built world clip boxes, out of the build's working memory; every triangle record's part of its triangle as barycentric ranges,
//      which hold wherever the triangle goes; the build's transforms and the per-instance word "changed since the build".  The build's own
//      refit has been enqueued and is not touched: the tree is byte for byte the one built without the flag. ----
static int keep_split_tables(HrtContext *ctx, Tlas &t, const float *staged_clip, hipStream_t s) {
    TlasDevice &d = t.dev;
    const size_t n = std::max(t.n_instances, 1u), rec_bytes = sizeof(float) * 6 * (size_t)t.n_prims;
    HIP_TRY(ctx, pool_alloc(ctx, (void **)&d.d_keep_clip, rec_bytes));
    HIP_TRY(ctx, pool_alloc(ctx, (void **)&d.d_keep_bary, rec_bytes));
    HIP_TRY(ctx, pool_alloc(ctx, (void **)&d.d_build_xf, sizeof(float) * 12 * n));
    HIP_TRY(ctx, pool_alloc(ctx, (void **)&d.d_inst_changed, sizeof(uint32_t) * n));
    HIP_TRY(ctx, hipMemcpyAsync(d.d_keep_clip, staged_clip, rec_bytes, hipMemcpyDeviceToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(d.d_build_xf, d.d_inst_xf, sizeof(float) * 12 * n, hipMemcpyDeviceToDevice, s));
    HIP_TRY(ctx, hipMemsetAsync(d.d_inst_changed, 0, sizeof(uint32_t) * n, s));
    const BaryClipArgs ba{reinterpret_cast<const unsigned char *>(d.d_prims), t.prim_stride, t.n_prims, d.d_inst_xf, d.d_inst_identity, d.d_inst_src, d.d_keep_clip, d.d_keep_bary};
    launch_bary_clip(ba, s);
    HIP_TRY(ctx, hipGetLastError());
    t.h_build_xf = t.h_xf; t.h_inst_changed.assign(n, 0u);
    t.alloc_bytes += 2 * (uint64_t)rec_bytes + (sizeof(float) * 12 + sizeof(uint32_t)) * (uint64_t)n;
    t.keeps_splits = true;
    return HRT_OK;
}

// ---- the merged device build: every visible instance's primitives in ONE world-space tree -- topology and primitive ids from build.hip (the
//      top-down SAH phase, with spatial splits when device_split, then PLOC in the cells, the optimal collapse, the emission); the refit
//      computes every record, box and quantised child, exactly as after an instance update ----
static int build_merged_on_device(HrtContext *ctx, Tlas &t, const BuildPlan &plan, bool device_split, float scene_scale, hipStream_t s) {
    const uint32_t n = t.n_instances;
    const std::vector<uint32_t> &first = plan.first;
    TlasDevice &d = t.dev;
    int rc = upload_instance_tables(ctx, t, s);
    if (rc != HRT_OK) return rc;
    // (the records go where they stay; a split build knows its record count afterwards, and stages them)
    if (!device_split) HIP_TRY(ctx, pool_alloc(ctx, &d.d_prims, (size_t)t.prim_stride * std::max<size_t>(first[n], 1)));
    HIP_TRY(ctx, pool_alloc(ctx, (void **)&d.d_inst_first, sizeof(uint32_t) * first.size()));
    HIP_TRY(ctx, pool_alloc(ctx, (void **)&d.d_inst_kind, sizeof(uint32_t) * std::max(n, 1u)));
    HIP_TRY(ctx, hipMemcpyAsync(d.d_inst_first, first.data(), sizeof(uint32_t) * first.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(d.d_inst_kind, t.kind.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice, s));
    // the top-down phase always (object splits: what gives the tree its shape above the cells PLOC builds -- on the reference's kind of
    // scene, separate bodies over a huge ground sphere, PLOC alone costs seven times the node visits); spatial splits under HRT_CTX_FAST_TRACE
    GpuBuildInput in = build_input(ctx, kMaxLeafPrims, t.scene_of_bodies ? ctx->build_c_prim_bodies : ctx->build_c_prim, false,
                                   device_split || ctx->build_topdown != 0, device_split ? ctx->split_budget : 0.0f, refit_pad(scene_scale));
    in.n_prims = first[n]; in.n_inst = n; in.d_inst_first = d.d_inst_first; in.d_inst_kind = d.d_inst_kind; in.d_inst_src = d.d_inst_src;
    in.d_inst_xf = d.d_inst_xf; in.d_inst_identity = d.d_inst_identity; in.node_stride = t.node_stride; in.prim_stride = t.prim_stride;
    in.out_prims = static_cast<unsigned char *>(d.d_prims);
    // a fast-trace build: the reinsertion pass over the finished BVH2 (not where the top-down phase gives up and PLOC alone builds the tree: build.hip)
    if (device_split) { in.reinsert_rounds = ctx->reinsert_rounds; in.reinsert_max_depth = (uint32_t)ctx->fused_max_depth; }
    StagedBuild sb{ctx, s};
    if (!sb.stage(in, gpu_build_max_refs(in.n_prims, &in.split), device_split ? StagedRecords::RecordsAndClip : StagedRecords::None, !device_split))
        return fail(ctx, HRT_ERR_OOM, "device build: no working memory (%zu bytes)", sb.want);
    GpuBuildResult r;
    rc = sb.build(in, "device build", r);
    // A tree deeper than any kernel's stack (a chain of primitives over many orders of magnitude: nearest-neighbour clustering, like SAH, takes
    // one off the rest at every level): built again by position -- every cluster with its Morton neighbour, log2(n) levels, whatever the areas
    // (a split build too: the tree by position has no splits, its records are the primitives -- the staged buffers hold them all the same)
    if (rc == HRT_OK && r.n_prims != 0u && too_deep(r.max_depth)) {
        if (ctx->build_verbose) std::fprintf(stderr, "[hrt] the tree is %u levels deep: built again by position\n", r.max_depth);
        in.balanced = true; in.split.enabled = false; in.reinsert_rounds = 0;
        rc = sb.build(in, "device build", r);
    }
    if (rc != HRT_OK) return rc;
    {   // the tree's own buffers, as large as the build turned out to need (the build emitted its nodes into the working memory, sized for
        // the worst case: one node per primitive; typically a seventh is used)
        const size_t nn = std::max<size_t>(r.n_prims ? r.n_nodes : 1u, 1u);
        rc = alloc_tree_blocks(ctx, t, nn, 0, device_split ? r.n_records : first[n]);
        if (rc != HRT_OK) return rc;
        if (device_split && r.n_records) HIP_TRY(ctx, hipMemcpyAsync(d.d_prims, in.out_prims, (size_t)t.prim_stride * r.n_records, hipMemcpyDeviceToDevice, s));
        if (r.n_prims) {
            HIP_TRY(ctx, hipMemcpyAsync(d.d_nodes, in.out_nodes, (size_t)t.node_stride * nn, hipMemcpyDeviceToDevice, s));
            HIP_TRY(ctx, hipMemcpyAsync(d.d_node_ref, in.out_node_ref, sizeof(float) * 2 * nn, hipMemcpyDeviceToDevice, s));
            HIP_TRY(ctx, hipStreamSynchronize(s));         // the working memory goes back to the context when this scope ends
        }
    }
    t.bvh = Bvh8();
    if (r.n_prims == 0u) {
        // every primitive had non-finite bounds: the empty root (every ray misses)
        build_bvh8({}, t.bvh, 1, scene_scale);
        HIP_TRY(ctx, hipMemcpyAsync(d.d_nodes, t.bvh.nodes.data(), sizeof(Bvh8Node), hipMemcpyHostToDevice, s));
        t.phases.clear();
        t.n_nodes = 1; t.n_prims = 0; t.n_triangles = t.n_spheres = 0; t.max_depth = 0;
        return HRT_OK;
    }
    if (too_deep(r.max_depth)) return fail(ctx, HRT_ERR_INVALID, "BVH depth %u exceeds the traversal stack", r.max_depth);
    const uint32_t dropped = first[n] - r.n_prims;      // non-finite primitives (counted against the triangles unless there are none)
    t.n_nodes = r.n_nodes; t.n_prims = r.n_records; t.max_depth = r.max_depth;
    t.n_triangles = plan.n_tri_in >= dropped ? plan.n_tri_in - dropped : 0u; t.n_spheres = r.n_prims - t.n_triangles;
    for (int a = 0; a < 3; ++a) { t.lo[a] = r.lo[a]; t.hi[a] = r.hi[a]; }
    t.phases = phases_from_levels(r.level_begin);
    // (a split build: every record's box is the one its cell is responsible for, not the primitive's -- this once; a later
    // update would recompute the boxes from whole primitives, so the first update rebuilds instead: has_split_refs)
    t.has_split_refs = device_split && r.split_levels;
    rc = reference_refit(ctx, t, in.split.pad, t.has_split_refs ? in.out_clip : nullptr, s);
    if (rc != HRT_OK) return rc;
    t.build_dropped = dropped;
    if (t.has_split_refs && ctx->keep_splits) rc = keep_split_tables(ctx, t, in.out_clip, s);
    if (rc != HRT_OK) return rc;
    if (t.has_split_refs) HIP_TRY(ctx, hipStreamSynchronize(s));      // (the clip boxes live in the working memory)
    if (ctx->build_verbose)
        std::fprintf(stderr, "[hrt] device build: %u primitives -> %u records, %u nodes, depth %u, %u PLOC rounds (radius %d), %u split levels, %u cells\n",
                     r.n_prims, r.n_records, r.n_nodes, r.max_depth, r.ploc_rounds, ctx->ploc_radius, r.split_levels, r.n_cells);
    return HRT_OK;
}

// ---- a two-level tree.  (1) every unique BLAS has its object-space tree (topology), built once per BLAS and kept on
//      the device; (2) the device build over the instances' bounds, whose leaves come out as transform nodes; (3) the BLAS trees are copied
//      in behind the top level and refitted in object space; (4) the top level's refit -- the only part an update repeats. ----

// The top level's "geometry": per instance its BLAS's box and bounding sphere, on the device; `src` points the instances at them.
// (one instance's ten floats; the bounding sphere is computed the first time a BLAS is asked for it, and again after hrt_blas_update_triangles)
static int blas_bound_row(HrtContext *ctx, Blas &b, float *q, hipStream_t s) {
    for (int a = 0; a < 3; ++a) { q[a] = b.lo[a]; q[3 + a] = b.hi[a]; }
    q[6] = q[7] = q[8] = 0.0f; q[9] = -1.0f;
    if (b.n_prims != 0u && b.lo[0] <= b.hi[0]) {
        std::lock_guard<std::mutex> lk(b.tmpl_mu);
        if (!b.bsphere_ready) {
            for (int a = 0; a < 3; ++a) b.bsphere[a] = 0.5f * b.lo[a] + 0.5f * b.hi[a];
            const ScratchArena arena = scratch_acquire(ctx, kBoundsScratchBytes);
            const hipError_t e = gpu_blas_radius(b.d_verts, b.n_prims, b.kind, b.bsphere, &b.bsphere[3], arena.p, s);
            scratch_release(ctx, arena);
            HIP_TRY(ctx, e);
            b.bsphere_ready = true;
        }
        for (int a = 0; a < 4; ++a) q[6 + a] = b.bsphere[a];
    }
    return HRT_OK;
}
static int upload_blas_bounds(HrtContext *ctx, Tlas &t, std::vector<const void *> &src, hipStream_t s) {
    const uint32_t n = t.n_instances;
    std::vector<float> &bound = t.h_blas_bound;      // (kept: pick_up_geometry renews the rows of BLASes whose geometry changes)
    bound.assign(10 * (size_t)std::max(n, 1u), 0.0f);
    for (uint32_t i = 0; i < n; ++i) RC_TRY(blas_bound_row(ctx, *t.blas_refs[i], &bound[10 * (size_t)i], s));
    HIP_TRY(ctx, pool_alloc(ctx, (void **)&t.dev.d_blas_bound, sizeof(float) * bound.size()));
    HIP_TRY(ctx, hipMemcpyAsync(t.dev.d_blas_bound, bound.data(), sizeof(float) * bound.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    src.assign(std::max(n, 1u), nullptr);
    for (uint32_t i = 0; i < n; ++i) src[i] = t.dev.d_blas_bound + 10 * (size_t)i;
    return HRT_OK;
}

// The object-space tree a two-level TLAS copies in for one of its BLASes: the template (Blas::tmpl_dev), or under HRT_CTX_FAST_TRACE the tree
// with spatial splits (Blas::split) where the BLAS has one.  (Both are written once, under Blas::tmpl_mu, and never change.)
static int packed_tree_of(HrtContext *ctx, Blas &b, bool fast_trace, hipStream_t s, const BlasTree *&out) {
    if (fast_trace) {
        const int rc = ensure_split_template(ctx, b, s);
        if (rc != HRT_OK) return rc;
        bool have;
        { std::lock_guard<std::mutex> lk(b.tmpl_mu); have = b.split.d_nodes != nullptr; }
        if (have) { out = &b.split; return HRT_OK; }
    }
    out = &b.tmpl_dev;
    return ensure_template(ctx, b, s, true);
}

// The refit of the packed BLAS trees, all BLASes at once: phase k = the k-th level from the bottom of every tree (a template is stored breadth
// first, children one level below their parents), walked through an order array of node indices.  slices[j].phases: BLAS j's part of
// every phase (contiguous in `order`), what the refit of that BLAS alone walks after hrt_blas_update_triangles.
static void pack_refit_order(const std::vector<const BlasTree *> &trees, const std::vector<uint32_t> &node_off, uint32_t n_top, uint32_t blas_depth,
                             std::vector<uint32_t> &order, std::vector<std::pair<uint32_t, uint32_t>> &pack_phases, std::vector<PackSlice> &slices) {
    const uint32_t nu = (uint32_t)trees.size();
    order.reserve(node_off[nu]);
    for (uint32_t k = 0; k <= blas_depth; ++k) {
        const uint32_t begin = (uint32_t)order.size();
        for (uint32_t j = 0; j < nu; ++j) {
            const std::vector<uint32_t> &lb = trees[j]->level_begin;
            const uint32_t levels = lb.empty() ? 0u : (uint32_t)lb.size() - 1u;
            if (k >= levels) continue;
            const uint32_t l = levels - 1u - k;
            if (lb[l + 1] > lb[l]) slices[j].phases.emplace_back((uint32_t)order.size(), lb[l + 1] - lb[l]);
            for (uint32_t x = lb[l]; x < lb[l + 1]; ++x) order.push_back(n_top + node_off[j] + x);
        }
        if (order.size() > begin) pack_phases.emplace_back(begin, (uint32_t)order.size() - begin);
    }
}

// The boxes inside a BLAS are padded for the object-space rays that will come: the slab test's error grows with the distance
// of the ray's origin, which in object space is the world's extent seen through the instance's inverse (a rigid pose: the
// world's own extent, as for the flattened tree).  first2: the top level's numbering (instances outside the tree take no number).
static float object_space_reach(const Tlas &t, const std::vector<Blas *> &uniq, const std::vector<uint32_t> &first2, float scene_scale) {
    float obj_coord = 1.0f, reach = 1.0f;
    for (const Blas *b : uniq)
        for (int a = 0; a < 3; ++a) obj_coord = std::max(obj_coord, std::max(std::fabs(b->lo[a]), std::fabs(b->hi[a])));
    for (uint32_t i = 0; i < t.n_instances; ++i) {
        if (first2[i + 1] == first2[i]) continue;
        const float *v = &t.h_inv[12 * (size_t)i];
        float rown = 0.0f;
        for (int rr = 0; rr < 3; ++rr) rown = std::max(rown, std::fabs(v[4 * rr]) + std::fabs(v[4 * rr + 1]) + std::fabs(v[4 * rr + 2]));
        if (std::isfinite(rown)) reach = std::max(reach, rown * scene_scale);
    }
    return std::max(reach, obj_coord);
}

// The refit of BLAS subtrees behind the top level of a two-level tree, in object space: the pack's own tables (not refit_args), the identity
// transform, the BLASes' vertices, the padding the tree was built with.  The caller adds what differs: write_reference and clip at the build.
static RefitArgs pack_refit_args(const Tlas &t) {
    const TlasDevice &d = t.dev;
    RefitArgs rp{};
    rp.nodes = reinterpret_cast<unsigned char *>(d.d_nodes); rp.node_stride = t.node_stride; rp.prims = reinterpret_cast<unsigned char *>(d.d_prims); rp.prim_stride = t.prim_stride;
    rp.node_box = d.d_node_box; rp.node_ref = d.d_node_ref; rp.inst_xf = d.d_pack_xf; rp.inst_identity = d.d_pack_identity; rp.inst_src = d.d_pack_src; rp.order = d.d_pack_order;
    rp.pad = 4e-6f * t.built_reach;
    return rp;
}

// flatten_instead: the two-level tree asked for cannot be had (nothing valid to instance; too deep for the path kernel's stack, or too large
// for it): nothing is wrong, and the caller builds the flattened one.
static int build_two_level(HrtContext *ctx, Tlas &t, const std::vector<HrtInstance> &inst, const BuildPlan &plan, bool fast_trace, float scene_scale, hipStream_t s, bool &flatten_instead) {
    const uint32_t n = t.n_instances;
    const std::vector<Blas *> &uniq = plan.uniq;
    const uint32_t nu = (uint32_t)uniq.size();
    TlasDevice &d = t.dev;
    std::vector<const void *> src;
    int rc = upload_blas_bounds(ctx, t, src, s);
    if (rc == HRT_OK) rc = upload_instance_tables(ctx, t, src, s);
    if (rc != HRT_OK) return rc;
    std::vector<uint32_t> node_off(nu + 1, 0u), prim_off(nu + 1, 0u);
    std::vector<const BlasTree *> trees(nu, nullptr);
    uint32_t blas_depth = 0, n_split = 0;
    for (uint32_t j = 0; j < nu; ++j) {
        rc = packed_tree_of(ctx, *uniq[j], fast_trace, s, trees[j]);
        if (rc != HRT_OK) return rc;
        const BlasTree &tp = *trees[j];
        if ((uint64_t)node_off[j] + tp.n_nodes > 0x7fffffffull || (uint64_t)prim_off[j] + tp.n_records > 0x7fffffffull) return fail(ctx, HRT_ERR_INVALID, "two-level tree: more than 2^31 nodes or records");
        node_off[j + 1] = node_off[j] + tp.n_nodes; prim_off[j + 1] = prim_off[j] + tp.n_records;
        blas_depth = std::max(blas_depth, tp.max_depth);
        n_split += tp.d_clip ? 1u : 0u;
    }
    // the top level's primitives: one per visible instance of a non-empty BLAS
    std::vector<uint32_t> first2(n + 1, 0u), kind2(std::max(n, 1u), kPrimKindInstance);
    for (uint32_t i = 0; i < n; ++i) first2[i + 1] = first2[i] + (instance_has_prims(inst[i], *t.blas_refs[i]) ? 1u : 0u);
    const uint32_t n2 = first2[n];
    HIP_TRY(ctx, pool_alloc(ctx, (void **)&d.d_inst_first, sizeof(uint32_t) * first2.size()));
    HIP_TRY(ctx, pool_alloc(ctx, (void **)&d.d_inst_kind, sizeof(uint32_t) * kind2.size()));
    HIP_TRY(ctx, pool_alloc(ctx, (void **)&d.d_inst_root, sizeof(uint32_t) * std::max(n, 1u)));
    HIP_TRY(ctx, hipMemcpyAsync(d.d_inst_first, first2.data(), sizeof(uint32_t) * first2.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(d.d_inst_kind, kind2.data(), sizeof(uint32_t) * kind2.size(), hipMemcpyHostToDevice, s));
    GpuBuildInput in = build_input(ctx, 1, ctx->build_c_prim, true, ctx->build_topdown != 0, 0.0f, refit_pad(scene_scale));
    in.width = 8;      // (HRT_BVH_WIDTH, the flattened trees' measuring knob, does not reach the top level)
    in.n_prims = n2; in.n_inst = n; in.d_inst_first = d.d_inst_first; in.d_inst_kind = d.d_inst_kind; in.d_inst_src = d.d_inst_src;
    in.d_inst_xf = d.d_inst_xf; in.d_inst_identity = d.d_inst_identity; in.node_stride = t.node_stride; in.prim_stride = t.prim_stride;
    StagedBuild sb{ctx, s};
    ArenaLayout &lay = sb.lay;
    // (the pack's refit tables and walk order stay with the tree -- nu small tables, one entry per BLAS node: the refit of one BLAS's subtree
    // after hrt_blas_update_triangles walks them again)
    HIP_TRY(ctx, pool_alloc(ctx, (void **)&d.d_pack_xf, sizeof(float) * 12 * nu));
    HIP_TRY(ctx, pool_alloc(ctx, (void **)&d.d_pack_identity, sizeof(uint32_t) * nu));
    HIP_TRY(ctx, pool_alloc(ctx, (void **)&d.d_pack_src, sizeof(void *) * nu));
    HIP_TRY(ctx, pool_alloc(ctx, (void **)&d.d_pack_order, sizeof(uint32_t) * std::max<size_t>(node_off[nu], 1)));
    // (where a BLAS tree has spatial splits, the box the pack's refit takes for every record of the TLAS shares the build's block: the BLASes keep their own copies)
    const size_t o_pclip = lay.take(n_split ? sizeof(float) * 6 * (size_t)prim_off[nu] : 0u);
    // worst case: a transform node per instance and fewer box nodes than instances
    if (!sb.stage(in, 2 * (size_t)n2 + 2, StagedRecords::None, false)) return fail(ctx, HRT_ERR_OOM, "device build: no working memory (%zu bytes)", sb.want);
    in.out_prims = in.out_nodes;        // (no record is written: the leaves are transform nodes)
    GpuBuildResult r;
    rc = sb.build(in, "device build of the top level", r);
    if (rc != HRT_OK) return rc;
    // nothing valid to instance (the flattened path emits the empty root); the path kernel keeps one sibling group per level of BOTH trees on its node stack
    if (r.n_prims == 0u || r.max_depth + 1u + blas_depth > (uint32_t)ctx->fused_max_depth) { flatten_instead = true; return HRT_OK; }
    const uint32_t n_top = r.n_nodes, n_all = n_top + node_off[nu], n_rec = prim_off[nu];
    if ((uint64_t)n_all * t.node_stride >= ctx->fused_max_bytes || (uint64_t)std::max(n_rec, 1u) * t.prim_stride >= ctx->fused_max_bytes) { flatten_instead = true; return HRT_OK; }
    rc = alloc_tree_blocks(ctx, t, n_all, 16, n_rec);       // (+16: the path kernel reads 80 bytes of the last node whatever its stride)
    if (rc != HRT_OK) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(d.d_nodes, in.out_nodes, (size_t)t.node_stride * n_top, hipMemcpyDeviceToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(d.d_node_ref, in.out_node_ref, sizeof(float) * 2 * (size_t)n_top, hipMemcpyDeviceToDevice, s));
    // (3) the BLAS trees behind the top level
    std::vector<uint32_t> roots(std::max(n, 1u), 0u);
    for (uint32_t i = 0; i < n; ++i) roots[i] = n_top + node_off[plan.slot_of[i]];
    HIP_TRY(ctx, hipMemcpyAsync(d.d_inst_root, roots.data(), sizeof(uint32_t) * roots.size(), hipMemcpyHostToDevice, s));
    for (uint32_t j = 0; j < nu; ++j) {
        PackBlasArgs pa{};
        pa.src_nodes = trees[j]->d_nodes; pa.src_prims = trees[j]->d_prims; pa.n_nodes = node_off[j + 1] - node_off[j]; pa.n_prims = prim_off[j + 1] - prim_off[j];
        pa.dst_nodes = reinterpret_cast<unsigned char *>(d.d_nodes); pa.dst_prims = reinterpret_cast<unsigned char *>(d.d_prims); pa.node_stride = t.node_stride; pa.prim_stride = t.prim_stride;
        pa.node_off = n_top + node_off[j]; pa.prim_off = prim_off[j]; pa.slot = j;
        if (n_split) { pa.dst_clip = lay.at<float>(o_pclip); pa.src_clip = trees[j]->d_clip; pa.src_geom = uniq[j]->d_verts; }
        launch_pack_blas(pa, s);
    }
    // their refit: per-BLAS tables with the identity transform
    std::vector<float> pxf(12 * (size_t)nu, 0.0f); std::vector<uint32_t> pid(nu, 1u); std::vector<const void *> psrc(nu, nullptr);
    for (uint32_t j = 0; j < nu; ++j) { pxf[12 * (size_t)j] = pxf[12 * (size_t)j + 5] = pxf[12 * (size_t)j + 10] = 1.0f; psrc[j] = uniq[j]->d_verts; }
    std::vector<uint32_t> order;
    std::vector<std::pair<uint32_t, uint32_t>> pack_phases;
    t.pack.assign(nu, PackSlice());
    for (uint32_t j = 0; j < nu; ++j) { t.pack[j].blas = uniq[j]; t.pack[j].n_records = trees[j]->n_records; t.pack[j].split = trees[j]->d_clip != nullptr; }
    pack_refit_order(trees, node_off, n_top, blas_depth, order, pack_phases, t.pack);
    if (order.size() != node_off[nu]) return fail(ctx, HRT_ERR_HIP, "two-level tree: a BLAS template's levels do not cover its nodes");
    HIP_TRY(ctx, hipMemcpyAsync(d.d_pack_xf, pxf.data(), sizeof(float) * pxf.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(d.d_pack_identity, pid.data(), sizeof(uint32_t) * nu, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync((void *)d.d_pack_src, psrc.data(), sizeof(void *) * nu, hipMemcpyHostToDevice, s));
    if (!order.empty()) HIP_TRY(ctx, hipMemcpyAsync(d.d_pack_order, order.data(), sizeof(uint32_t) * order.size(), hipMemcpyHostToDevice, s));
    t.built_reach = object_space_reach(t, uniq, first2, scene_scale);
    RefitArgs rp = pack_refit_args(t);
    rp.write_reference = 1u;
    // (a record of a tree with spatial splits: the box of its part of the primitive, padded alike -- and for ever: an update refits the top level only)
    if (n_split) rp.clip = lay.at<float>(o_pclip);
    launch_refit_phases(rp, pack_phases, s);
    HIP_TRY(ctx, hipGetLastError());
    // (4) the top level
    t.two_level = true; t.n_top_nodes = n_top; t.n_unique_blas = nu;
    t.phases = phases_from_levels(r.level_begin);
    rc = reference_refit(ctx, t, in.split.pad, nullptr, s);
    if (rc != HRT_OK) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(s));
    if (ctx->build_verbose)
        std::fprintf(stderr, "[hrt] two-level build: %u instances over %u BLASes (%u with spatial splits) -> %u top nodes (depth %u, %u split levels), %u BLAS nodes (depth <= %u), %u records (flattened: %u)\n",
                     n2, nu, n_split, n_top, r.max_depth, r.split_levels, node_off[nu], blas_depth, n_rec, plan.first[n]);
    t.bvh = Bvh8();
    t.n_nodes = n_all; t.n_prims = n_rec; t.max_depth = r.max_depth + 1u + blas_depth;
    t.n_triangles = t.n_spheres = 0;
    for (uint32_t j = 0; j < nu; ++j) { t.n_triangles += trees[j]->n_triangles; t.n_spheres += trees[j]->n_spheres; }
    for (int a = 0; a < 3; ++a) { t.lo[a] = r.lo[a]; t.hi[a] = r.hi[a]; }
    return HRT_OK;
}

// ---- what to build, decided once ----

// Two levels or one?  Flattening costs memory, build and refit time in proportion to instances x primitives; a two-level tree
// (transform nodes over one shared tree per BLAS) in proportion to instances + unique primitives, at the price of a ray
// transform per instance entered.  Asked for (two_level_mode > 0), or chosen when the flattened tree would leave the caches
// while the shared one stays in them.  Only k_fused walks such trees: not under HRT_CTX_COUNT / HRT_FUSED != 1.  Fills plan.uniq / slot_of.
static bool wants_two_level(const HrtContext *ctx, const std::vector<HrtInstance> &inst, const std::vector<std::shared_ptr<Blas>> &refs, int two_level_mode, BuildPlan &plan) {
    const uint32_t n = (uint32_t)inst.size();
    plan.slot_of.assign(n, 0u);
    if (two_level_mode < 0 || (ctx->flags & HRT_CTX_COUNT) != 0 || ctx->fused != 1) return false;
    std::unordered_map<Blas *, uint32_t> seen;
    uint64_t unique_prims = 0;
    for (uint32_t i = 0; i < n; ++i) {
        Blas *b = refs[i].get();
        if (!instance_has_prims(inst[i], *b)) continue;
        auto it = seen.find(b);
        if (it == seen.end()) { it = seen.emplace(b, (uint32_t)plan.uniq.size()).first; plan.uniq.push_back(b); unique_prims += b->n_prims; }
        plan.slot_of[i] = it->second;
    }
    const uint32_t total = plan.first[n];
    return !plan.uniq.empty() && (two_level_mode > 0 || ((uint64_t)total >= ctx->two_level_min_prims && (double)total >= (double)ctx->two_level_min_share * (double)unique_prims));
}

static int plan_build(HrtContext *ctx, Tlas &t, const std::vector<HrtInstance> &inst, const std::vector<std::shared_ptr<Blas>> &refs, bool instanced, bool fast_trace, int two_level_mode, BuildPlan &plan) {
    const uint32_t n = (uint32_t)inst.size();
    plan.first.assign(n + 1, 0u);
    uint32_t n_vis = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const bool vis = (inst[i].visibilityMask & 1u) != 0;       // the reference traces with mask 1 (Shader.cu:71)
        const uint32_t cnt = vis ? refs[i]->n_prims : 0u;
        if ((uint64_t)plan.first[i] + cnt > 0xfffffff0ull) return fail(ctx, HRT_ERR_INVALID, "more than 2^32 primitives in one TLAS");
        plan.first[i + 1] = plan.first[i] + cnt;
        if (refs[i]->kind == kPrimKindTriangle) plan.n_tri_in += cnt;
        n_vis += cnt ? 1u : 0u;
    }
    const uint32_t total = plan.first[n];
    // a scene of bodies (the reference's kind: particles instancing a few shapes) or a soup?  (the collapse's primitive cost: hrt_internal.hpp)
    t.scene_of_bodies = n_vis >= 4u && (uint64_t)total < 20000ull * n_vis;      // (the launch picks the path kernel's leaf-hold by it, hrt_api.cpp)
    t.node_stride = (uint32_t)ctx->node_stride; t.prim_stride = (uint32_t)ctx->prim_stride;
    if (ctx->node_stride_auto && total > 3500000u) t.node_stride = 128u;      // a tree that will not fit the Infinity Cache: one 128-byte line per node
    // HRT_CTX_FAST_TRACE: the static-scene tree with spatial splits -- from the device's builder, or (HRT_FAST_TRACE_BUILD=host) from the host's.
    // It gets the flattened tree unless two levels were ASKED for (two_level_mode > 0, not chosen by size) and the device builds: then the
    // splits go into the shared BLAS trees, where they last through every update (build_two_level)
    if (instanced) plan.kind = TreeKind::OverInstances;
    else if (!ctx->build_on_device || (fast_trace && !ctx->fast_trace_on_device) || total == 0u) plan.kind = TreeKind::HostFlattened;
    else if (fast_trace && two_level_mode > 0 && wants_two_level(ctx, inst, refs, two_level_mode, plan)) plan.kind = TreeKind::TwoLevel;
    else if (fast_trace) plan.kind = split_build_fits(ctx, total) ? TreeKind::DeviceSplit : TreeKind::DeviceMerged;
    else plan.kind = wants_two_level(ctx, inst, refs, two_level_mode, plan) ? TreeKind::TwoLevel : TreeKind::DeviceMerged;
    return HRT_OK;
}

// flatten_instead: nothing was built, because the two-level tree that was asked for or chosen cannot be had (build_two_level) -- to be called
// again with two_level_mode < 0
static int build_tlas_fresh(HrtContext *ctx, Tlas &t, const std::vector<HrtInstance> &inst, hipStream_t s, bool instanced, bool fast_trace, int two_level_mode, bool &flatten_instead) {
    flatten_instead = false;
    const uint32_t n = (uint32_t)inst.size();
    std::vector<std::shared_ptr<Blas>> refs(n);
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        for (uint32_t i = 0; i < n; ++i) {
            auto it = ctx->blas.find(inst[i].traversableHandle);
            if (it == ctx->blas.end()) return fail(ctx, HRT_ERR_INVALID, "instance %u: unknown BLAS handle 0x%llx", i, (unsigned long long)inst[i].traversableHandle);
            refs[i] = it->second;
        }
    }
    // the per-instance host tables
    const float scene_scale = instance_tables(inst, refs, t.h_xf, t.h_inv, t.h_ident);
    t.sbt_offset.assign(n, 0); t.kind.assign(n, 0); t.has_spheres = false;
    t.sig_handle.assign(n, 0); t.sig_visibility.assign(n, 0);
    for (uint32_t i = 0; i < n; ++i) {
        t.sbt_offset[i] = inst[i].sbtOffset;
        t.kind[i] = refs[i]->kind;
        t.sig_handle[i] = inst[i].traversableHandle; t.sig_visibility[i] = inst[i].visibilityMask & 1u;
        if ((inst[i].visibilityMask & 1u) != 0 && refs[i]->kind == kPrimKindSphere && refs[i]->n_prims) t.has_spheres = true;
    }
    t.phases.clear();
    BuildPlan plan;
    int rc = plan_build(ctx, t, inst, refs, instanced, fast_trace, two_level_mode, plan);
    if (rc != HRT_OK) return rc;
    free_tlas_device(ctx, t);
    t.n_instances = n;
    t.blas_refs = std::move(refs);
    t.blas_epoch.assign(n, 0);      // (the geometry every path below builds from)
    for (uint32_t i = 0; i < n; ++i) t.blas_epoch[i] = t.blas_refs[i]->geometry_epoch;
    t.pack.clear();
    // every path below uploads the tables all structures need (upload_instance_tables), makes the allocations of its own, and leaves the tree's counts in t
    switch (plan.kind) {
    case TreeKind::HostFlattened: rc = build_flattened_on_host(ctx, t, inst, plan.first[n], scene_scale, fast_trace, s); break;
    case TreeKind::OverInstances: rc = build_over_instances(ctx, t, inst, scene_scale, s); break;
    case TreeKind::DeviceMerged:  rc = build_merged_on_device(ctx, t, plan, false, scene_scale, s); break;
    case TreeKind::DeviceSplit:   rc = build_merged_on_device(ctx, t, plan, true, scene_scale, s); break;
    case TreeKind::TwoLevel:      rc = build_two_level(ctx, t, inst, plan, fast_trace, scene_scale, s, flatten_instead); break;
    }
    if (rc != HRT_OK || flatten_instead) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(s));
    t.instanced = plan.kind == TreeKind::OverInstances;
    t.fast_trace = fast_trace;
    t.refits_since_build = 0;
    return HRT_OK;
}

// (Re)build the tree of a TLAS.  The new tree is built on the side and takes the place of the old one only when
// everything has succeeded: a failed rebuild (depth limit, out of memory) leaves the registered TLAS as it was --
// valid and traceable -- instead of half overwritten.
int build_tlas_into(HrtContext *ctx, Tlas &t, const std::vector<HrtInstance> &inst, hipStream_t s, bool instanced, bool fast_trace = false, int two_level_mode = -1) {
    Tlas fresh;
    // (the pinned host words and the event move to the new tree: hipHostMalloc / hipHostFree are as slow as their device counterparts)
    if (t.area_ready && t.area_pending) (void)hipEventSynchronize(t.area_ready);
    fresh.h_area = t.h_area; fresh.h_update_flags = t.h_update_flags; fresh.area_ready = t.area_ready;
    t.h_area = nullptr; t.h_update_flags = nullptr; t.area_ready = nullptr;
    bool flatten_instead;
    int rc = build_tlas_fresh(ctx, fresh, inst, s, instanced, fast_trace, two_level_mode, flatten_instead);
    if (rc == HRT_OK && flatten_instead) {
        free_tlas_device(ctx, fresh);
        fresh.two_level = false; fresh.phases.clear();
        rc = build_tlas_fresh(ctx, fresh, inst, s, instanced, fast_trace, -1, flatten_instead);
    }
    if (rc != HRT_OK) {
        t.h_area = fresh.h_area; t.h_update_flags = fresh.h_update_flags; t.area_ready = fresh.area_ready;
        fresh.h_area = nullptr; fresh.h_update_flags = nullptr; fresh.area_ready = nullptr;
        free_tlas_device(ctx, fresh); free_tlas_host(fresh); return rc;
    }
    fresh.generation = t.generation + 1;
    fresh.refits = t.refits; fresh.rebuilds = t.rebuilds + 1;
    std::swap(t, fresh);
    free_tlas_device(ctx, fresh); free_tlas_host(fresh);        // the old tree
    ctx->tlas_rebuilds++;
    return HRT_OK;
}

int download_instances(HrtContext *ctx, const HrtInstance *d_instances, uint32_t n, hipStream_t s, std::vector<HrtInstance> &inst) {
    const size_t bytes = sizeof(HrtInstance) * (size_t)n;
    if (n >= 16384u) {
        // many instances (a DEM time step: 8 MB), every frame of a synchronous update loop: through pinned memory the context keeps
        std::lock_guard<std::mutex> lk(ctx->pin_mu);
        if (ctx->pin_bytes < bytes) {
            if (ctx->pin_stage) (void)hipHostFree(ctx->pin_stage);
            ctx->pin_stage = nullptr; ctx->pin_bytes = 0;
            if (hipHostMalloc(&ctx->pin_stage, bytes, hipHostMallocDefault) == hipSuccess) ctx->pin_bytes = bytes;
            else { (void)hipGetLastError(); ctx->pin_stage = nullptr; }
        }
        if (ctx->pin_stage) {
            HIP_TRY(ctx, hipMemcpyAsync(ctx->pin_stage, d_instances, bytes, hipMemcpyDeviceToHost, s));
            HIP_TRY(ctx, hipStreamSynchronize(s));
            const HrtInstance *p = static_cast<const HrtInstance *>(ctx->pin_stage);
            inst.assign(p, p + n);
            return HRT_OK;
        }
    }
    inst.resize(n);
    if (n) {
        HIP_TRY(ctx, hipMemcpyAsync(inst.data(), d_instances, bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipStreamSynchronize(s));
    }
    return HRT_OK;
}

// ---- updates (hrt_tlas_update) ----

// (an update's refit has been enqueued; its verdict is asked for later: take_refit_verdict)
static void refit_enqueued(HrtContext *ctx, Tlas &t) { t.area_pending = true; t.refits++; t.refits_since_build++; ctx->tlas_refits++; }

// Device refit of a built tree under new instance transforms: upload the per-instance tables, then one
// k_refit_level launch per tree level, deepest first.  Asynchronous on s.
int refit_tlas(HrtContext *ctx, Tlas &t, const std::vector<HrtInstance> &inst, hipStream_t s) {
    const float scene_scale = instance_tables(inst, t.blas_refs, t.h_xf, t.h_inv, t.h_ident);
    HIP_TRY(ctx, hipMemcpyAsync(t.dev.d_inst_inv, t.h_inv.data(), sizeof(float) * t.h_inv.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(t.dev.d_inst_xf, t.h_xf.data(), sizeof(float) * t.h_xf.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(t.dev.d_inst_identity, t.h_ident.data(), sizeof(uint32_t) * t.h_ident.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemsetAsync(t.dev.d_area, 0, sizeof(float), s));
    if (t.keeps_splits) {      // which instances are where the build had them, bit for bit (the asynchronous path: k_instance_tables)
        for (uint32_t i = 0; i < t.n_instances; ++i)
            t.h_inst_changed[i] = (t.h_inst_changed[i] & 2u) | (std::memcmp(&t.h_xf[12 * (size_t)i], &t.h_build_xf[12 * (size_t)i], 12 * sizeof(float)) != 0 ? 1u : 0u);
        HIP_TRY(ctx, hipMemcpyAsync(t.dev.d_inst_changed, t.h_inst_changed.data(), sizeof(uint32_t) * t.h_inst_changed.size(), hipMemcpyHostToDevice, s));
    }
    t.async_words_ready = false;
    RefitArgs ra = refit_args(ctx, t);
    ra.pad = refit_pad(scene_scale);
    ra.area_sum = t.dev.d_area;
    { Timer tm(ctx, s, HRT_K_REFIT); launch_refit_phases(ra, t.phases, s); }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(t.h_area, t.dev.d_area, sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipEventRecord(t.area_ready, s));
    refit_enqueued(ctx, t);
    return HRT_OK;
}

// The verdict of the last refit (pending: t.area_pending), waited for: how much the boxes have grown since the build.  A refit keeps the
// topology; `still_good`: not by so much yet that a fresh build pays for itself.
static int take_refit_verdict(HrtContext *ctx, Tlas &t, bool &still_good) {
    HIP_TRY(ctx, hipEventSynchronize(t.area_ready));
    t.area_pending = false;
    ctx->tlas_refit_ratio = (double)*t.h_area;
    still_good = ctx->tlas_refit_ratio <= (double)ctx->refit_rebuild_ratio;
    return HRT_OK;
}

// An asynchronous update (HRT_CTX_ASYNC_UPDATE): nothing is read back now.  First the verdict of the previous one (long complete), which
// may say that this update has to take the synchronous path instead: to rebuild, or to re-read the sbtOffsets.
enum class AsyncUpdate { Done, Rebuild, RereadSbt };
static int update_async(HrtContext *ctx, Tlas *t, const HrtInstance *d_instances, uint32_t n, hipStream_t s, AsyncUpdate &outcome) {
    if (t->area_pending) {
        bool still_good;
        const int rc = take_refit_verdict(ctx, *t, still_good);
        if (rc != HRT_OK) return rc;
        const uint32_t changed = t->h_update_flags[1];      // (bit 0: a handle or visibility bit; bit 1: an sbtOffset)
        t->h_update_flags[1] = 0u;
        if (!still_good || (changed & 1u) != 0u) { outcome = AsyncUpdate::Rebuild; return HRT_OK; }
        if ((changed & 2u) != 0u) { outcome = AsyncUpdate::RereadSbt; return HRT_OK; }
    }
    // (the device words the tables kernel and the refit accumulate into -- scene scale, verdict bits, area sum -- are left in their
    // initial state by the previous asynchronous update's epilogue; after a build or a synchronous update they are set here)
    if (!t->async_words_ready) {
        HIP_TRY(ctx, hipMemcpyAsync(t->dev.d_update_flags, t->h_update_flags + 2, sizeof(uint32_t) * 2, hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipMemsetAsync(t->dev.d_area, 0, sizeof(float), s));
        t->async_words_ready = true;
    }
    InstanceTableArgs ia{};
    ia.instances = d_instances; ia.n = n; ia.sig_handle = t->dev.d_sig_handle; ia.sig_visibility = t->dev.d_sig_visibility; ia.sig_sbt = t->dev.d_sig_sbt; ia.blas_box = t->dev.d_blas_box;
    ia.inst_xf = t->dev.d_inst_xf; ia.inst_inv = t->dev.d_inst_inv; ia.inst_identity = t->dev.d_inst_identity; ia.flags = t->dev.d_update_flags;
    if (t->keeps_splits) { ia.build_xf = t->dev.d_build_xf; ia.inst_changed = t->dev.d_inst_changed; }
    launch_instance_tables(ia, s);
    RefitArgs ra = refit_args(ctx, *t);
    ra.scale_bits = t->dev.d_update_flags; ra.area_sum = t->dev.d_area;
    { Timer tm(ctx, s, HRT_K_REFIT); launch_refit_phases(ra, t->phases, s); }
    // one launch where there were two copies to the host, one from it and a fill: results to pinned memory, device words reset
    UpdateEpilogueArgs ue{t->dev.d_area, t->dev.d_update_flags, t->h_area, t->h_update_flags, t->h_update_flags[2], t->h_update_flags[3]};
    launch_update_epilogue(ue, s);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(t->area_ready, s));
    refit_enqueued(ctx, *t);
    outcome = AsyncUpdate::Done;
    return HRT_OK;
}

// ---- geometry that changed under a tree (hrt_blas_update_triangles / _spheres): every instance remembers the Blas::geometry_epoch its tree was last
//      built or refitted for (Tlas::blas_epoch).  Host state only: an asynchronous update still reads nothing back. ----
enum class GeometryChange { None, Refit, Rebuild };

// Refit: the refit of the update brings the tree up to the new vertices (it reads them where they lie), once pick_up_geometry has renewed the
// tables around it.  Rebuild: it cannot -- updates rebuild anyway (HRT_REFIT=0, a flattened tree with split references, an empty tree), or the
// tree does not hold every primitive of a changed BLAS as a record of its own: the build left non-finite primitives out (and a BLAS that was
// all of them has no subtree at all), or the BLAS's subtree in a two-level tree is its tree with spatial splits, whose clip boxes were the
// old geometry's.
static GeometryChange geometry_change(const HrtContext *ctx, const Tlas &t) {
    const uint32_t n = t.n_instances;
    bool changed = false;
    for (uint32_t i = 0; i < n && !changed; ++i) changed = t.blas_refs[i]->geometry_epoch != t.blas_epoch[i];
    if (!changed) return GeometryChange::None;
    if (ctx->refit == 0 || (t.has_split_refs && !t.keeps_splits) || t.n_prims == 0u) return GeometryChange::Rebuild;
    // (its records outnumber the primitives: what the build left out is counted there.  Triangle k stays triangle k: so do its barycentric
    // ranges; every record of a sphere takes the sphere's whole box at its new place, as under a moved instance)
    if (t.keeps_splits) return t.build_dropped != 0u ? GeometryChange::Rebuild : GeometryChange::Refit;
    if (!t.two_level) {
        uint64_t visible = 0;
        for (uint32_t i = 0; i < n; ++i) visible += t.sig_visibility[i] ? t.blas_refs[i]->n_prims : 0u;
        return (uint64_t)t.n_prims < visible ? GeometryChange::Rebuild : GeometryChange::Refit;
    }
    std::unordered_map<const Blas *, const PackSlice *> slice_of;
    for (const PackSlice &ps : t.pack) slice_of[ps.blas] = &ps;
    for (uint32_t i = 0; i < n; ++i) {
        const Blas *b = t.blas_refs[i].get();
        if (b->geometry_epoch == t.blas_epoch[i] || !t.sig_visibility[i] || b->n_prims == 0u) continue;
        const auto it = slice_of.find(b);
        if (it == slice_of.end() || it->second->split || it->second->n_records < b->n_prims) return GeometryChange::Rebuild;
    }
    return GeometryChange::Refit;
}

// Ahead of a refit that follows changed geometry, on its stream: the BLAS boxes the asynchronous tables kernel derives the scene scale from;
// in a two-level tree the changed instances' "geometry" (their BLAS's box and bounding sphere: ten floats, the sphere computed anew --
// the one read-back of this path, four bytes per changed BLAS) and the refit of the changed BLASes' subtrees -- the pack's refit of
// build_two_level over their slices of its walk order: same topology, the new vertices.  (The flattened trees need no more: their refit
// derives every record from the BLASes' vertices anyway.)  The subtrees' boxes do not enter the update's verdict.
static int pick_up_geometry(HrtContext *ctx, Tlas &t, hipStream_t s) {
    const uint32_t n = t.n_instances;
    TlasDevice &d = t.dev;
    t.h_blas_box.assign(6 * (size_t)std::max(n, 1u), 0.0f);
    for (uint32_t i = 0; i < n; ++i) for (int a = 0; a < 3; ++a) { t.h_blas_box[6 * (size_t)i + a] = t.blas_refs[i]->lo[a]; t.h_blas_box[6 * (size_t)i + 3 + a] = t.blas_refs[i]->hi[a]; }
    HIP_TRY(ctx, hipMemcpyAsync(d.d_blas_box, t.h_blas_box.data(), sizeof(float) * t.h_blas_box.size(), hipMemcpyHostToDevice, s));
    if (t.two_level) {
        std::unordered_map<const Blas *, bool> moved;
        uint32_t first = n, last = 0;                  // (one copy over the rows from the first changed instance to the last: a copy per row costs microseconds each)
        for (uint32_t i = 0; i < n; ++i) {
            Blas &b = *t.blas_refs[i];
            if (b.geometry_epoch == t.blas_epoch[i]) continue;
            moved[&b] = true;
            RC_TRY(blas_bound_row(ctx, b, &t.h_blas_bound[10 * (size_t)i], s));
            first = std::min(first, i); last = i;
        }
        if (first <= last) HIP_TRY(ctx, hipMemcpyAsync(d.d_blas_bound + 10 * (size_t)first, &t.h_blas_bound[10 * (size_t)first], sizeof(float) * 10 * (size_t)(last - first + 1), hipMemcpyHostToDevice, s));
        const RefitArgs rp = pack_refit_args(t);
        Timer tm(ctx, s, HRT_K_REFIT);
        for (const PackSlice &ps : t.pack) if (moved.count(ps.blas)) launch_refit_phases(rp, ps.phases, s);
        HIP_TRY(ctx, hipGetLastError());
    }
    if (t.keeps_splits) {      // the instances of the changed BLASes are "changed" for good: their as-built clip boxes are the old geometry's
        for (uint32_t i = 0; i < n; ++i) if (t.blas_refs[i]->geometry_epoch != t.blas_epoch[i]) t.h_inst_changed[i] |= 2u;
        HIP_TRY(ctx, hipMemcpyAsync(d.d_inst_changed, t.h_inst_changed.data(), sizeof(uint32_t) * t.h_inst_changed.size(), hipMemcpyHostToDevice, s));
    }
    for (uint32_t i = 0; i < n; ++i) t.blas_epoch[i] = t.blas_refs[i]->geometry_epoch;
    return HRT_OK;
}

}  // namespace hrt

// A rebuild in the middle of an animation.  Large scenes: the merged device build (3.1 ms for 2000 particles / 435 k triangles, 3.3 ms
// for a million triangles: profiles/r03_device_split_build.txt) -- the better tree.  Small scenes and host-build contexts: the tree over
// instances, whose top tree the host assembles in well under a millisecond.
static bool rebuild_over_instances(const HrtContext *ctx, const Tlas &t) {
    uint64_t total = 0;
    for (uint32_t i = 0; i < t.n_instances; ++i) total += t.blas_refs[i] ? t.blas_refs[i]->n_prims : 0u;
    return ctx->tlas_instanced >= 0 && t.n_instances >= 2 && (!ctx->build_on_device || total < 100000ull || ctx->tlas_instanced > 0);
}

// The first update after a build, before anything is refitted: have the instances gone somewhere else altogether?  The reference
// builds every file's IAS with identity transforms and poses it afterwards (RendererTime.cu:111-127): the tree was built over particles
// lying on top of each other, a refit of it is a tree in name only, and the refit, the wait for its verdict and the rebuild that follows
// are the rebuild alone when this says so.  Moved far = an instance's box centre is further from where it was than the box is wide.
static bool instances_moved_far(const Tlas &t, const std::vector<HrtInstance> &inst) {
    uint32_t valid = 0, far = 0;
    for (uint32_t i = 0; i < t.n_instances; ++i) {
        const Blas *b = t.blas_refs[i].get();
        if (!b || !instance_has_box(inst[i], *b)) continue;
        const float c[3] = {0.5f * (b->lo[0] + b->hi[0]), 0.5f * (b->lo[1] + b->hi[1]), 0.5f * (b->lo[2] + b->hi[2])};
        const float e[3] = {b->hi[0] - b->lo[0], b->hi[1] - b->lo[1], b->hi[2] - b->lo[2]};
        float was[3], now[3], ext[3];
        xf_point(&t.h_xf[12 * (size_t)i], c, was); xf_point(inst[i].transform, c, now);
        const float *m = &t.h_xf[12 * (size_t)i];
        for (int k = 0; k < 3; ++k) ext[k] = std::fabs(m[4 * k]) * e[0] + std::fabs(m[4 * k + 1]) * e[1] + std::fabs(m[4 * k + 2]) * e[2];
        const float d2 = (now[0] - was[0]) * (now[0] - was[0]) + (now[1] - was[1]) * (now[1] - was[1]) + (now[2] - was[2]) * (now[2] - was[2]);
        const float w2 = ext[0] * ext[0] + ext[1] * ext[1] + ext[2] * ext[2];
        ++valid;
        if (d2 > w2) ++far;
    }
    return valid >= 4 && 2 * far > valid;
}

static int register_blas(HrtContext *ctx, std::shared_ptr<Blas> b, HrtTraversable *out_blas) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    const uint64_t h = ctx->next_handle++;
    ctx->blas[h] = std::move(b);
    *out_blas = h;
    return HRT_OK;
}

// The BLAS's own copy holds new geometry (hrt_blas_update_triangles / _spheres) with these bounds: what was derived from the old goes -- the
// host copy, the bounding sphere, the cached object-space trees, whose clip boxes are the old geometry's -- and the epoch tells every TLAS
// over the BLAS, at its next hrt_tlas_update, that its tree is of the geometry as it was.
static int geometry_replaced(HrtContext *ctx, Blas &b, const float *lo, const float *hi) {
    BlasTree old_tmpl, old_split;
    {
        std::lock_guard<std::mutex> lk(b.tmpl_mu);
        for (int a = 0; a < 3; ++a) { b.lo[a] = lo[a]; b.hi[a] = hi[a]; }
        b.bsphere_ready = false; b.bsphere[3] = -1.0f;
        b.host_geometry = false; b.verts.clear(); b.centers.clear(); b.radii.clear();      // (ensure_host_geometry fetches again)
        b.tmpl = Bvh8(); b.tmpl_built = false; b.split_decided = false;   // (rebuilt by the next build that wants them)
        std::swap(old_tmpl, b.tmpl_dev); std::swap(old_split, b.split);
        b.geometry_epoch++;
    }
    if (old_tmpl.d_nodes || old_split.d_nodes) {
        // (a two-level build on another stream may still be copying from them)
        HIP_TRY(ctx, hipDeviceSynchronize());
        for (BlasTree *tr : {&old_tmpl, &old_split}) for (void *p : {(void *)tr->d_nodes, (void *)tr->d_prims, (void *)tr->d_clip}) if (p) (void)hipFree(p);
    }
    return HRT_OK;
}

extern "C" {

// ---- acceleration structures ---------------------------------------------------------
int hrt_blas_build_triangles(HrtContext *ctx, const HrtFloat3 *d_vertices, uint32_t n_vertices, void *stream, HrtTraversable *out_blas) {
    if (!ctx || !out_blas) return HRT_ERR_INVALID;
    if (n_vertices % 3 != 0) return fail(ctx, HRT_ERR_INVALID, "n_vertices (%u) is not a multiple of 3", n_vertices);
    if (n_vertices && !d_vertices) return fail(ctx, HRT_ERR_INVALID, "d_vertices is NULL");
    (void)hipSetDevice(ctx->device);
    std::shared_ptr<Blas> b(new Blas());
    b->kind = kPrimKindTriangle; b->n_prims = n_vertices / 3;
    if (n_vertices) {
        // the geometry stays on the device: a copy of it (the caller may free its buffer, RendererMesh.cu:116) and its
        // object-space bounds (24 bytes come back); trees are built from the copy when a TLAS is built over the BLAS
        const size_t bytes = sizeof(float) * 3 * (size_t)n_vertices;
        HIP_TRY(ctx, hipMalloc((void **)&b->d_verts, bytes));
        HIP_TRY(ctx, hipMemcpyAsync(b->d_verts, d_vertices, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
        const ScratchArena arena = scratch_acquire(ctx, kBoundsScratchBytes);
        const hipError_t e = gpu_blas_bounds(b->d_verts, b->n_prims, kPrimKindTriangle, b->lo, b->hi, arena.p, (hipStream_t)stream);
        scratch_release(ctx, arena);
        HIP_TRY(ctx, e);
    }
    return register_blas(ctx, std::move(b), out_blas);
}

int hrt_blas_build_spheres(HrtContext *ctx, const HrtFloat3 *d_centers, const float *d_radii, uint32_t n, void *stream, HrtTraversable *out_blas) {
    if (!ctx || !out_blas) return HRT_ERR_INVALID;
    if (n && (!d_centers || !d_radii)) return fail(ctx, HRT_ERR_INVALID, "sphere arrays are NULL");
    (void)hipSetDevice(ctx->device);
    std::shared_ptr<Blas> b(new Blas());
    b->kind = kPrimKindSphere; b->n_prims = n;
    if (n) {
        HIP_TRY(ctx, hipMalloc((void **)&b->d_verts, sizeof(float) * 4 * (size_t)n));        // {cx, cy, cz, r} per sphere
        launch_pack_spheres(reinterpret_cast<const float *>(d_centers), d_radii, n, b->d_verts, (hipStream_t)stream);
        HIP_TRY(ctx, hipGetLastError());
        const ScratchArena arena = scratch_acquire(ctx, kBoundsScratchBytes);
        const hipError_t e = gpu_blas_bounds(b->d_verts, n, kPrimKindSphere, b->lo, b->hi, arena.p, (hipStream_t)stream);
        scratch_release(ctx, arena);
        HIP_TRY(ctx, e);
    }
    return register_blas(ctx, std::move(b), out_blas);
}

// OPTIX_BUILD_OPERATION_UPDATE for a triangle GAS (include/hrt.h): new vertices into the BLAS's own copy and its bounds in one pass
// (blas_update.hip); what was derived from the old ones goes -- the host copy, the bounding sphere, the cached object-space trees -- and the
// epoch tells every TLAS over the BLAS, at its next hrt_tlas_update, that its tree is of the geometry as it was.
int hrt_blas_update_triangles(HrtContext *ctx, HrtTraversable blas, const HrtFloat3 *d_vertices, uint32_t n_vertices, void *stream) {
    if (!ctx) return HRT_ERR_INVALID;
    std::shared_ptr<Blas> b;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        const auto it = ctx->blas.find(blas);
        if (it == ctx->blas.end()) return fail(ctx, HRT_ERR_INVALID, "hrt_blas_update_triangles: unknown BLAS handle 0x%llx", (unsigned long long)blas);
        b = it->second;
    }
    if (b->kind != kPrimKindTriangle) return fail(ctx, HRT_ERR_INVALID, "hrt_blas_update_triangles: 0x%llx is a sphere BLAS", (unsigned long long)blas);
    if ((uint64_t)n_vertices != 3ull * b->n_prims)
        return fail(ctx, HRT_ERR_INVALID, "hrt_blas_update_triangles: n_vertices (%u) is not what the BLAS was built with (%llu)", n_vertices, 3ull * b->n_prims);
    if (n_vertices && !d_vertices) return fail(ctx, HRT_ERR_INVALID, "d_vertices is NULL");
    if (reinterpret_cast<uintptr_t>(d_vertices) & 3u) return fail(ctx, HRT_ERR_INVALID, "d_vertices is not aligned for a float");
    if (n_vertices == 0) return HRT_OK;
    (void)hipSetDevice(ctx->device);
    {   // a pending by-primitive link that reads this BLAS as its OLD geometry: what "previous" means is about to change under it
        std::lock_guard<std::mutex> lk(ctx->mu);
        DenoiseHistory &h = ctx->denoise_history;
        if (h.link_pending && std::find(h.link_blas.begin(), h.link_blas.end(), b) != h.link_blas.end()) h.drop_link();
    }
    float lo[3], hi[3];
    const ScratchArena arena = scratch_acquire(ctx, kBoundsScratchBytes);
    const hipError_t e = gpu_blas_update_triangles(reinterpret_cast<const float *>(d_vertices), b->d_verts, b->n_prims, lo, hi, arena.p, (hipStream_t)stream);
    scratch_release(ctx, arena);
    HIP_TRY(ctx, e);
    return geometry_replaced(ctx, *b, lo, hi);
}

// ... and for a sphere GAS (include/hrt.h): new centres and radii into the BLAS's {cx, cy, cz, r} copy and its bounds in one pass.
int hrt_blas_update_spheres(HrtContext *ctx, HrtTraversable blas, const HrtFloat3 *d_centers, const float *d_radii, uint32_t n_spheres, void *stream) {
    if (!ctx) return HRT_ERR_INVALID;
    std::shared_ptr<Blas> b;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        const auto it = ctx->blas.find(blas);
        if (it == ctx->blas.end()) return fail(ctx, HRT_ERR_INVALID, "hrt_blas_update_spheres: unknown BLAS handle 0x%llx", (unsigned long long)blas);
        b = it->second;
    }
    if (b->kind != kPrimKindSphere) return fail(ctx, HRT_ERR_INVALID, "hrt_blas_update_spheres: 0x%llx is a triangle BLAS", (unsigned long long)blas);
    if (n_spheres != b->n_prims)
        return fail(ctx, HRT_ERR_INVALID, "hrt_blas_update_spheres: n_spheres (%u) is not what the BLAS was built with (%u)", n_spheres, b->n_prims);
    if (n_spheres && (!d_centers || !d_radii)) return fail(ctx, HRT_ERR_INVALID, "sphere arrays are NULL");
    if ((reinterpret_cast<uintptr_t>(d_centers) & 3u) || (reinterpret_cast<uintptr_t>(d_radii) & 3u)) return fail(ctx, HRT_ERR_INVALID, "sphere arrays are not aligned for a float");
    if (n_spheres == 0) return HRT_OK;
    (void)hipSetDevice(ctx->device);
    // (no pending by-primitive link of the denoiser can read a sphere BLAS: they link triangle BLASes only)
    float lo[3], hi[3];
    const ScratchArena arena = scratch_acquire(ctx, kBoundsScratchBytes);
    const hipError_t e = gpu_blas_update_spheres(reinterpret_cast<const float *>(d_centers), d_radii, b->d_verts, n_spheres, lo, hi, arena.p, (hipStream_t)stream);
    scratch_release(ctx, arena);
    HIP_TRY(ctx, e);
    return geometry_replaced(ctx, *b, lo, hi);
}

int hrt_blas_destroy(HrtContext *ctx, HrtTraversable blas) {
    if (!ctx) return HRT_ERR_INVALID;
    std::lock_guard<std::mutex> lk(ctx->mu);
    return ctx->blas.erase(blas) ? HRT_OK : fail(ctx, HRT_ERR_INVALID, "unknown BLAS handle");
}

int hrt_tlas_build(HrtContext *ctx, const HrtInstance *d_instances, uint32_t n, void *stream, HrtTraversable *out_tlas) {
    if (!ctx || !out_tlas) return HRT_ERR_INVALID;
    if (n && !d_instances) return fail(ctx, HRT_ERR_INVALID, "d_instances is NULL");
    (void)hipSetDevice(ctx->device);
    std::unique_ptr<Tlas> t(new Tlas());
    std::vector<HrtInstance> inst;
    int rc = download_instances(ctx, d_instances, n, (hipStream_t)stream, inst);
    const int two_level_mode = (ctx->flags & HRT_CTX_TWO_LEVEL) != 0 ? 1 : ctx->two_level;
    if (rc == HRT_OK) rc = build_tlas_into(ctx, *t, inst, (hipStream_t)stream, ctx->tlas_instanced > 0 && two_level_mode <= 0, (ctx->flags & HRT_CTX_FAST_TRACE) != 0, two_level_mode);
    // A rebuild in the middle of an animation builds a tree over instances when the scene is small (hrt_tlas_update): the per-BLAS
    // template trees that needs are built now, while the scene is being loaded, not inside the first frame that rebuilds (the
    // reference's shipped sample: 9 templates, 8.7 ms of its first frame)
    if (rc == HRT_OK && !t->two_level && rebuild_over_instances(ctx, *t))
        for (uint32_t i = 0; i < n && rc == HRT_OK; ++i) {
            Blas &b = *t->blas_refs[i];
            if (instance_has_box(inst[i], b)) rc = ensure_template(ctx, b, (hipStream_t)stream);
        }
    if (rc != HRT_OK) { free_tlas_device(ctx, *t); free_tlas_host(*t); return rc; }
    std::lock_guard<std::mutex> lk(ctx->mu);
    const uint64_t h = ctx->next_handle++;
    ctx->tlas[h] = std::move(t);
    *out_tlas = h;
    return HRT_OK;
}

// updateIAS (RendererImpl.cu:210-242): the instance transforms changed.  When nothing else did, the tree
// keeps its topology and is refitted on the device (refit.hip), asynchronously on `stream`; a change of
// BLAS handle / visibility, or a refitted tree that has degraded past refit_rebuild_ratio, rebuilds.
int hrt_tlas_update(HrtContext *ctx, HrtTraversable tlas, const HrtInstance *d_instances, uint32_t n, void *stream) {
    if (!ctx) return HRT_ERR_INVALID;
    (void)hipSetDevice(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    Tlas *t;
    { std::lock_guard<std::mutex> lk(ctx->mu); auto it = ctx->tlas.find(tlas); if (it == ctx->tlas.end()) return fail(ctx, HRT_ERR_INVALID, "unknown TLAS handle"); t = it->second.get(); }
    if (ctx->capture.tlas == tlas) ctx->capture.valid = false;      // (the primary hits of the tree as it was: a refit keeps the generation)
    if (n != t->n_instances) return fail(ctx, HRT_ERR_INVALID, "update must keep the instance count (%u != %u)", n, t->n_instances);
    if (n && !d_instances) return fail(ctx, HRT_ERR_INVALID, "d_instances is NULL");
    // (a BLAS of the tree has new vertices or spheres, hrt_blas_update_triangles / _spheres: the refit picks them up where it can)
    const GeometryChange geometry = geometry_change(ctx, *t);
    bool force_rebuild = geometry == GeometryChange::Rebuild, pick_up = geometry == GeometryChange::Refit;
    // (the first update after a build takes the synchronous path below, which checks that refit on the spot: see there)
    if ((ctx->flags & HRT_CTX_ASYNC_UPDATE) != 0 && ctx->refit != 0 && t->n_prims != 0u && n != 0u && (t->refits_since_build != 0 || t->built_posed) && !force_rebuild) {
        if (pick_up) { RC_TRY(pick_up_geometry(ctx, *t, s)); pick_up = false; }
        AsyncUpdate outcome;
        const int rc = update_async(ctx, t, d_instances, n, s, outcome);
        if (rc != HRT_OK || outcome == AsyncUpdate::Done) return rc;
        force_rebuild = outcome == AsyncUpdate::Rebuild;      // (RereadSbt: an sbtOffset changed, the synchronous path below re-reads them)
    }
    std::vector<HrtInstance> inst;
    int rc = download_instances(ctx, d_instances, n, s, inst);
    if (rc != HRT_OK) return rc;
    // (a tree with split references is a static-scene tree: refitted, its leaves would fall back to whole-primitive boxes around
    // duplicated records -- worse than no splits -- so the first update replaces it by a device-built tree; not the tree that was built
    // under HRT_CTX_KEEP_SPLITS: its refit has every record's part of its primitive)
    bool same = ctx->refit != 0 && t->n_prims != 0u && !force_rebuild && (!t->has_split_refs || t->keeps_splits);
    for (uint32_t i = 0; i < n && same; ++i)
        same = inst[i].traversableHandle == t->sig_handle[i] && (inst[i].visibilityMask & 1u) == t->sig_visibility[i];
    bool moved_far = false;
    if (same && t->refits_since_build == 0 && ctx->refit_moved_far_check && instances_moved_far(*t, inst)) { same = false; moved_far = true; }
    if (same && t->area_pending) {
        rc = take_refit_verdict(ctx, *t, same);
        if (rc != HRT_OK) return rc;
    }
    if (same) {
        bool sbt_changed = false;
        for (uint32_t i = 0; i < n; ++i) if (inst[i].sbtOffset != t->sbt_offset[i]) { t->sbt_offset[i] = inst[i].sbtOffset; sbt_changed = true; }
        if (sbt_changed) {
            t->generation++;                              // the material tables are re-derived at the next launch
            HIP_TRY(ctx, hipMemcpyAsync(t->dev.d_sig_sbt, t->sbt_offset.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice, s));
            HIP_TRY(ctx, hipStreamSynchronize(s));
        }
        const bool first_after_build = t->refits_since_build == 0;
        if (pick_up) RC_TRY(pick_up_geometry(ctx, *t, s));
        rc = refit_tlas(ctx, *t, inst, s);
        if (rc != HRT_OK || !first_after_build) return rc;
        // The first refit after a build is checked on the spot (one stream synchronisation per build): the reference builds
        // every file's IAS with identity transforms and poses it afterwards (RendererTime.cu:111-127), so this is the refit
        // that turns a tree built over coinciding particles into the real scene -- and the frame that follows would be
        // traced through boxes that span everything.  Later refits are checked asynchronously, at the next update.
        rc = take_refit_verdict(ctx, *t, same);
        if (rc != HRT_OK || same) return rc;
    }
    if (ctx->build_verbose)
        std::fprintf(stderr, "[hrt] update %llu of this tree rebuilds: %s (area ratio %.3f, %llu refits since the build)\n", (unsigned long long)(t->refits + t->rebuilds),
                     geometry == GeometryChange::Rebuild ? "a BLAS has new vertices that a refit of this tree cannot follow" : force_rebuild ? "verdict of the previous asynchronous refit" : moved_far ? "most instances are further from where the tree was built than they are wide" : "handles / visibility changed or the refit just done degraded the tree", ctx->tlas_refit_ratio.load(),
                     (unsigned long long)t->refits_since_build);
    HIP_TRY(ctx, hipDeviceSynchronize());                 // launches on other streams may still read the old tree
    // a two-level tree stays one: its top level is rebuilt, the BLAS trees -- with their spatial splits, where it was built for trace speed -- are copied in again
    // ... and a tree that keeps its splits is built with them again: the flag asks for trace speed through the animation
    const int rb = t->two_level ? build_tlas_into(ctx, *t, inst, s, false, t->fast_trace, 1)
                 : t->keeps_splits ? build_tlas_into(ctx, *t, inst, s, false, true, -1) : build_tlas_into(ctx, *t, inst, s, rebuild_over_instances(ctx, *t));
    if (rb == HRT_OK) t->built_posed = true;      // (built for the instances as they are now: the next update need not be checked on the spot)
    return rb;
}

int hrt_pose_instances(HrtContext *ctx, HrtInstance *d_instances, uint32_t first_instance, uint32_t n_particles,
                       const HrtParticleState *d_current, const HrtParticleState *d_next, const HrtPoseParams *h_params, void *stream) {
    if (!ctx) return HRT_ERR_INVALID;
    if (n_particles == 0) return HRT_OK;
    if (!d_instances || !d_current || !d_next || !h_params) return fail(ctx, HRT_ERR_INVALID, "hrt_pose_instances: NULL argument");
    if (h_params->frame_count == 0) return fail(ctx, HRT_ERR_INVALID, "hrt_pose_instances: frame_count is 0");
    if ((reinterpret_cast<uintptr_t>(d_instances) & 15u) || (reinterpret_cast<uintptr_t>(d_current) & 15u) || (reinterpret_cast<uintptr_t>(d_next) & 15u))
        return fail(ctx, HRT_ERR_INVALID, "hrt_pose_instances: arrays must be 16-byte aligned");
    (void)hipSetDevice(ctx->device);
    PoseArgs a{};
    a.instances = d_instances; a.first_instance = first_instance; a.n = n_particles;
    a.current = reinterpret_cast<const float4 *>(d_current); a.next = reinterpret_cast<const float4 *>(d_next);
    a.duration = h_params->duration; a.frame = h_params->frame; a.frame_count = h_params->frame_count;
    std::memcpy(a.offset, &h_params->particle_offset, 12); std::memcpy(a.scale, &h_params->particle_scale, 12);
    a.mesh_mode = h_params->mesh_mode ? 1u : 0u;
    launch_pose_instances(a, (hipStream_t)stream);
    HIP_TRY(ctx, hipGetLastError());
    return HRT_OK;
}

int hrt_debug_trig(HrtContext *ctx, int function, const float *d_a, const float *d_b, uint32_t first_bits, uint32_t stride_bits, uint64_t n,
                   int force_slow, float *d_out, void *stream) {
    if (!ctx) return HRT_ERR_INVALID;
    if (function < 0 || function > 4) return fail(ctx, HRT_ERR_INVALID, "hrt_debug_trig: function %d (0 sin, 1 cos, 2 acos, 3 asin, 4 atan2)", function);
    if (n && (!d_out || (function == 4 && (!d_a || !d_b)))) return fail(ctx, HRT_ERR_INVALID, "hrt_debug_trig: NULL argument");
    (void)hipSetDevice(ctx->device);
    launch_debug_trig(function, d_a, d_b, first_bits, stride_bits, n, force_slow, d_out, (hipStream_t)stream);
    HIP_TRY(ctx, hipGetLastError());
    return HRT_OK;
}

int hrt_tlas_destroy(HrtContext *ctx, HrtTraversable tlas) {
    if (!ctx) return HRT_ERR_INVALID;
    (void)hipSetDevice(ctx->device);
    std::lock_guard<std::mutex> lk(ctx->mu);
    auto it = ctx->tlas.find(tlas);
    if (it == ctx->tlas.end()) return fail(ctx, HRT_ERR_INVALID, "unknown TLAS handle");
    (void)hipDeviceSynchronize();
    if (ctx->capture.tlas == tlas) ctx->capture.valid = false;
    if (ctx->denoise_history.link_tlas == tlas) ctx->denoise_history.drop_link();      // (hrt_denoise_temporal_rebind's link to it)
    free_tlas_device(ctx, *it->second); free_tlas_host(*it->second);
    ctx->tlas.erase(it);
    return HRT_OK;
}

int alloc_bvh_blob(size_t n_nodes, size_t n_prims, const float *lo, const float *hi, HrtBvhBlob *out);      // bvh8_host_api.cpp

int hrt_tlas_download(HrtContext *ctx, HrtTraversable tlas, HrtBvhBlob *out) {
    if (!ctx || !out) return HRT_ERR_INVALID;
    (void)hipSetDevice(ctx->device);
    Tlas *t;
    { std::lock_guard<std::mutex> lk(ctx->mu); auto it = ctx->tlas.find(tlas); if (it == ctx->tlas.end()) return fail(ctx, HRT_ERR_INVALID, "unknown TLAS handle"); t = it->second.get(); }
    const int rc = alloc_bvh_blob(t->n_nodes, t->n_prims, t->lo, t->hi, out);
    if (rc != HRT_OK) return rc;
    // the device copy is the truth: device builds exist nowhere else, and a refit rewrites the tree in place
    HIP_TRY(ctx, hipDeviceSynchronize());
    const size_t n_nodes = t->n_nodes, n_prims = t->n_prims;
    HIP_TRY(ctx, hipMemcpy2D(out->nodes, sizeof(Bvh8Node), t->dev.d_nodes, t->node_stride, sizeof(Bvh8Node), n_nodes, hipMemcpyDeviceToHost));
    if (n_prims) HIP_TRY(ctx, hipMemcpy2D(out->triangles, sizeof(PrimRecord), t->dev.d_prims, t->prim_stride, sizeof(PrimRecord), n_prims, hipMemcpyDeviceToHost));
    return HRT_OK;
}

int hrt_tlas_leaf_parent(HrtContext *ctx, HrtTraversable tlas, uint32_t *h_out, uint64_t capacity, uint64_t *n_records) {
    if (!ctx || !n_records) return HRT_ERR_INVALID;
    (void)hipSetDevice(ctx->device);
    Tlas *t;
    { std::lock_guard<std::mutex> lk(ctx->mu); auto it = ctx->tlas.find(tlas); if (it == ctx->tlas.end()) return fail(ctx, HRT_ERR_INVALID, "unknown TLAS handle"); t = it->second.get(); }
    if (t->two_level || t->has_spheres) return fail(ctx, HRT_ERR_STATE, "leaf_parent: a one-level tree of triangles has the table, this one is %s", t->two_level ? "a two-level tree" : "a tree with spheres");
    *n_records = t->n_prims;
    if (capacity < t->n_prims || (t->n_prims && !h_out)) return fail(ctx, HRT_ERR_INVALID, "leaf_parent: room for %llu records, the tree has %u", (unsigned long long)capacity, t->n_prims);
    HIP_TRY(ctx, hipDeviceSynchronize());
    const int rc = ensure_leaf_parent(ctx, *t, nullptr);
    if (rc != HRT_OK) return rc;
    if (t->n_prims) HIP_TRY(ctx, hipMemcpy(h_out, t->dev.d_leaf_parent, sizeof(uint32_t) * (size_t)t->n_prims, hipMemcpyDeviceToHost));
    return HRT_OK;
}

}  // extern "C"
