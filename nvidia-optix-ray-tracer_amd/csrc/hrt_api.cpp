// hrt_api.cpp -- C ABI of libhrt.so: context, acceleration structures, materials, RNG, launch.
// Entry points and the reference call sites they replace are documented in include/hrt.h.
// There is deliberately no CPU fallback anywhere in this file: every compute path ends in a
// HIP kernel launch, and context creation fails when no gfx950 device is present.
#include "hrt_internal.hpp"
#include "path_plan.h"

namespace hrt {

// Errors: *_build calls may run on several loader threads of one context (RendererMesh.cu:93-100), so a thread's last failure
// is kept per thread; hrt_last_error answers with the calling thread's own failure on that context when it has one, else with
// the context's most recent failure from any thread (copied under a lock).
namespace {
thread_local std::string g_create_error, g_thread_error, g_error_copy;
thread_local const HrtContext *g_thread_error_ctx = nullptr;
std::mutex g_error_mu;
}
const char *create_error() { return g_create_error.c_str(); }

int fail(HrtContext *ctx, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    if (ctx) {
        g_thread_error = buf; g_thread_error_ctx = ctx;
        std::lock_guard<std::mutex> lk(g_error_mu);
        ctx->error = buf;
    } else g_create_error = buf;
    return code;
}
const char *last_error_of(const HrtContext *ctx) {
    if (g_thread_error_ctx == ctx) return g_thread_error.c_str();
    std::lock_guard<std::mutex> lk(g_error_mu);
    g_error_copy = ctx->error;
    return g_error_copy.c_str();
}

// ---- XORWOW sub-sequence jump matrices: T^(2^(67+k)), k = 0..31, 160 columns x 5 words ----
struct Gf2m { uint32_t col[160][5]; };
void gf2_apply(const Gf2m &m, const uint32_t in[5], uint32_t out[5]) {
    uint32_t r[5] = {0, 0, 0, 0, 0};
    for (int w = 0; w < 5; ++w)
        for (int b = 0; b < 32; ++b)
            if ((in[w] >> b) & 1u)
                for (int k = 0; k < 5; ++k) r[k] ^= m.col[w * 32 + b][k];
    std::memcpy(out, r, sizeof r);
}
void gf2_square(Gf2m &m) {
    Gf2m t;
    for (int i = 0; i < 160; ++i) gf2_apply(m, m.col[i], t.col[i]);
    m = t;
}
std::vector<uint32_t> make_jump_tables() {
    Gf2m t;
    for (int i = 0; i < 160; ++i) {
        uint32_t v[5] = {0, 0, 0, 0, 0};
        v[i / 32] = 1u << (i % 32);
        const uint32_t x = v[0] ^ (v[0] >> 2);           // one xorshift step of XORWOW
        const uint32_t n4 = (v[4] ^ (v[4] << 4)) ^ (x ^ (x << 1));
        t.col[i][0] = v[1]; t.col[i][1] = v[2]; t.col[i][2] = v[3]; t.col[i][3] = v[4]; t.col[i][4] = n4;
    }
    for (int k = 0; k < 67; ++k) gf2_square(t);
    std::vector<uint32_t> out(32 * 800);
    for (int k = 0; k < 32; ++k) {
        std::memcpy(&out[(size_t)k * 800], t.col, sizeof t.col);
        gf2_square(t);
    }
    return out;
}

// Device arrays that share one capacity grow on demand: all freed and the capacity cleared before any is allocated anew, so that a failed
// hipMalloc leaves a consistent context (no dangling pointer, no capacity that promises memory).
int grow_device_arrays(HrtContext *ctx, std::initializer_list<DeviceArray> arrays, uint32_t &capacity, uint32_t need) {
    if (need <= capacity) return HRT_OK;
    for (const DeviceArray &a : arrays) { if (*a.p) (void)hipFree(*a.p); *a.p = nullptr; }
    capacity = 0;
    for (const DeviceArray &a : arrays) HIP_TRY(ctx, hipMalloc(a.p, a.elem * (size_t)need));
    capacity = need;
    return HRT_OK;
}

int ensure_workspace(HrtContext *ctx, uint32_t n, uint32_t height) {
    Workspace &w = ctx->ws;
    SampleSet &s0 = w.set[0], &s1 = w.set[1];
    int rc = grow_device_arrays(ctx, {s0.rays[0], s0.rays[1], s0.hit_tuvp, s0.hit_inst, {s0.bin_items, sizeof(uint32_t) * kNumBins}, {s0.chain, sizeof(uint32_t) * 4}, s0.result,
                                      s1.rays[0], s1.rays[1], s1.hit_tuvp, s1.hit_inst, {s1.bin_items, sizeof(uint32_t) * kNumBins}, {s1.chain, sizeof(uint32_t) * 4}, s1.result,
                                      w.accum}, w.capacity, n);
    if (rc == HRT_OK) rc = grow_device_arrays(ctx, {w.rows}, w.rows_capacity, height);
    if (rc != HRT_OK) return rc;
    for (SampleSet &st : w.set)
        if (!st.stages) { HIP_TRY(ctx, hipMalloc((void **)&st.stages, sizeof(StageCounters) * (kRayTraceDepth + 1) * kMaxSubTiles)); ctx->fused_counters_clean = false; }
    return HRT_OK;
}

void drain_spans(HrtContext *ctx) {
    for (const TimedSpan &sp : ctx->spans) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, sp.a, sp.b) == hipSuccess) { ctx->kernel_ms[sp.kind] += ms; ctx->kernel_launches[sp.kind]++; }
    }
    ctx->spans.clear();
    ctx->events_used = 0;
}

}  // namespace hrt


// ======================================================================================
extern "C" {

const char *hrt_version(void) { return "hrt 0.1 (gfx950 wavefront path tracer)"; }

const char *hrt_last_error(const HrtContext *ctx) { return ctx ? hrt::last_error_of(ctx) : hrt::create_error(); }

int hrt_ctx_create(int device_id, uint32_t flags, HrtContext **out_ctx) {
    if (!out_ctx) return fail(nullptr, HRT_ERR_INVALID, "out_ctx is NULL");
    *out_ctx = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(nullptr, HRT_ERR_NO_DEVICE, "no HIP device visible: libhrt has no CPU path");
    if (device_id < 0 || device_id >= n) return fail(nullptr, HRT_ERR_INVALID, "device %d out of range (%d devices)", device_id, n);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) != hipSuccess) return fail(nullptr, HRT_ERR_HIP, "hipGetDeviceProperties failed");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, HRT_ERR_NO_DEVICE, "device %d is %s; libhrt carries gfx950 code only", device_id, prop.gcnArchName);
    if (hipSetDevice(device_id) != hipSuccess) return fail(nullptr, HRT_ERR_HIP, "hipSetDevice(%d) failed", device_id);
    std::unique_ptr<HrtContext> ctx(new HrtContext());
    ctx->device = device_id; ctx->flags = flags; ctx->keep_splits = (flags & HRT_CTX_KEEP_SPLITS) != 0u; ctx->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    const std::vector<uint32_t> jump = make_jump_tables();
    if (hipMalloc((void **)&ctx->d_jump, jump.size() * sizeof(uint32_t)) != hipSuccess ||
        hipMemcpy(ctx->d_jump, jump.data(), jump.size() * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess ||
        hipMalloc((void **)&ctx->d_stats, sizeof(DeviceStats)) != hipSuccess ||
        hipMemset(ctx->d_stats, 0, sizeof(DeviceStats)) != hipSuccess)
        return fail(nullptr, HRT_ERR_HIP, "context allocation failed: %s", hipGetErrorString(hipGetLastError()));
    // the tuning knobs: one list (knobs.def), parsed here, documented from there (tools/knob_table.py)
#define HRT_KNOB(NAME, DEFAULT, DOC, ...) if (const char *e = std::getenv(NAME)) { __VA_ARGS__; }
#define HRT_HOST_KNOB(NAME, DEFAULT, DOC)
#include "knobs.def"
#undef HRT_KNOB
#undef HRT_HOST_KNOB
    *out_ctx = ctx.release();
    return HRT_OK;
}

int hrt_ctx_set_flags(HrtContext *ctx, uint32_t flags) {
    if (!ctx) return HRT_ERR_INVALID;
    (void)hipSetDevice(ctx->device);
    HIP_TRY(ctx, hipDeviceSynchronize());
    drain_spans(ctx);
    ctx->flags = flags;
    ctx->capture.valid = false;      // (what a capture may stand in for depends on the flags: a two-level tree is not traced under HRT_CTX_COUNT)
    return HRT_OK;
}

int hrt_ctx_destroy(HrtContext *ctx) {
    if (!ctx) return HRT_ERR_INVALID;
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    for (auto &kv : ctx->tlas) { free_tlas_device(ctx, *kv.second); free_tlas_host(*kv.second); }
    pool_drain(ctx);
    Workspace &w = ctx->ws;
    for (SampleSet &st : w.set) {
        void *sp[] = {st.rays[0], st.rays[1], st.hit_tuvp, st.hit_inst, st.bin_items, st.chain, st.result, st.stages};
        for (void *p : sp) if (p) (void)hipFree(p);
    }
    free_denoise_work(ctx);
    free_denoise_history(ctx);
    if (ctx->pin_stage) (void)hipHostFree(ctx->pin_stage);
    void *ptrs[] = {w.accum, w.slice_cost, w.slice_order, w.block_progress, w.primary_cache, w.rows, ctx->d_jump, ctx->d_stats, ctx->d_hitgroups, ctx->d_inst_program,
                    ctx->capture.tuvp, ctx->capture.inst};
    for (void *p : ptrs) if (p) (void)hipFree(p);
    for (const ScratchArena &a : ctx->scratch_free) (void)hipFree(a.p);
    for (hipEvent_t e : ctx->event_pool) (void)hipEventDestroy(e);
    for (hipEvent_t e : ctx->sub_done) (void)hipEventDestroy(e);
    for (hipStream_t st : ctx->sub_streams) (void)hipStreamDestroy(st);
    if (ctx->ev_begin) (void)hipEventDestroy(ctx->ev_begin);
    if (ctx->ev_graph_done) (void)hipEventDestroy(ctx->ev_graph_done);
    if (ctx->graph_stream) (void)hipStreamDestroy(ctx->graph_stream);
    delete ctx;
    return HRT_OK;
}

// ---- SBT ------------------------------------------------------------------------------
int hrt_sbt_record_pack_header(HrtProgram program, void *record_header) {
    if (!record_header || (int)program < 0 || (int)program >= (int)HRT_PROGRAM_COUNT) return HRT_ERR_INVALID;
    unsigned char *h = (unsigned char *)record_header;
    std::memset(h, 0, HRT_SBT_RECORD_HEADER_SIZE);
    h[0] = 'H'; h[1] = 'R'; h[2] = 'T'; h[3] = (unsigned char)program;
    return HRT_OK;
}

int hrt_materials_set(HrtContext *ctx, const HrtSbtRecord *h_records, uint32_t n_records) {
    if (!ctx || (n_records && !h_records)) return HRT_ERR_INVALID;
    for (uint32_t i = 0; i < n_records; ++i) {
        const unsigned char *h = h_records[i].header;
        if (h[0] != 'H' || h[1] != 'R' || h[2] != 'T' || h[3] >= HRT_PROGRAM_COUNT)
            return fail(ctx, HRT_ERR_INVALID, "SBT record %u: header not packed by hrt_sbt_record_pack_header", i);
    }
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->records.assign(h_records, h_records + n_records);
    ctx->have_records = true;
    ctx->materials_generation++;
    return HRT_OK;
}

int hrt_miss_set(HrtContext *ctx, const HrtMissParams *h_miss) {
    if (!ctx || !h_miss) return HRT_ERR_INVALID;
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->miss = *h_miss;
    return HRT_OK;
}

// ---- RNG ------------------------------------------------------------------------------
int hrt_rng_init(HrtContext *ctx, uint32_t width, uint32_t height, uint64_t seed_salt, void *stream, HrtRngState **out_d_states) {
    if (!ctx || !out_d_states) return HRT_ERR_INVALID;
    const uint64_t n64 = (uint64_t)width * height;
    if (n64 == 0 || n64 > 0xffffffffull) return fail(ctx, HRT_ERR_INVALID, "frame %ux%u is empty or exceeds 2^32 pixels", width, height);
    (void)hipSetDevice(ctx->device);
    RngState *d = nullptr;
    HIP_TRY(ctx, hipMalloc((void **)&d, sizeof(RngState) * n64));
    launch_rng_init(d, (uint32_t)n64, seed_salt, ctx->d_jump, (hipStream_t)stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize((hipStream_t)stream));      // reference: cudaStreamSynchronize, HostFunctions.cu:135
    *out_d_states = reinterpret_cast<HrtRngState *>(d);
    return HRT_OK;
}

int hrt_rng_free(HrtContext *ctx, HrtRngState *d_states, void *stream) {
    if (!ctx) return HRT_ERR_INVALID;
    (void)hipSetDevice(ctx->device);
    HIP_TRY(ctx, hipStreamSynchronize((hipStream_t)stream));
    if (d_states && ctx->capture.states == d_states) ctx->capture.valid = false;      // (the frame the capture is of ends with its RNG states)
    HIP_TRY(ctx, hipFree(d_states));
    return HRT_OK;
}

// ---- the launch -----------------------------------------------------------------------
// k_fused (fused.hip) keeps one sibling group per tree level in LDS without an overflow path and addresses the records with
// 32-bit byte offsets; a tree outside either limit takes round 1's fused kernel (kernels.hip), which has neither.
static bool fits_fused_kernel(const HrtContext *ctx, const Tlas &t) {
    return t.max_depth <= (uint32_t)ctx->fused_max_depth && (uint64_t)t.n_nodes * t.node_stride < ctx->fused_max_bytes &&
           (uint64_t)std::max(t.n_prims, 1u) * t.prim_stride < ctx->fused_max_bytes;
}
// A two-level tree is traced by k_fused's instanced form only: not by the counting build, not outside HRT_FUSED=1, not when it does not fit.
static bool two_level_admitted(const HrtContext *ctx, const Tlas &t, bool count) {
    return !t.two_level || (!count && ctx->fused == 1 && fits_fused_kernel(ctx, t));
}
// How many leaf groups a lane may queue before its node work waits for primitive tests.  A queued group is tested whatever has been hit
// meanwhile, so the more primitive tests a ray makes per node visit the sooner they should follow their node: soups (7 tests per 21 visits)
// run the stack full, scenes of many bodies (19 per 22 in a dense cloud) want 2, two-level trees (30 per 28, all of them inside instances) 1 --
// profiles/r04_leaf_hold.txt: +2 % / +7 %, C4 unchanged; the shipped sample's 25 particles (1.4 tests per 5.4 visits) are a soup in this respect.
static int leaf_hold_for(const HrtContext *ctx, const Tlas &t) {
    return ctx->leaf_hold > 0 ? ctx->leaf_hold : t.two_level ? 1 : (t.scene_of_bodies && t.n_instances >= 256u) ? 2 : 4;
}
// The fields of a traversal launch that do not depend on the kernel or the call site.
static TraverseArgs traverse_args(const HrtContext *ctx, const Tlas &t, float tmin, float tmax) {
    TraverseArgs ta{};
    ta.nodes = t.dev.d_nodes; ta.prims = t.dev.d_prims; ta.node_stride = t.node_stride; ta.prim_stride = t.prim_stride;
    ta.inst_inv = t.dev.d_inst_inv; ta.inst_identity = t.dev.d_inst_identity;
    ta.tmin = tmin; ta.tmax = tmax;
    ta.leaf_quorum = ctx->leaf_quorum; ta.tail_regen = ctx->fused_tail_regen; ta.seed_primary = ctx->seed_primary;
    ta.tail_split = t.two_level ? 0 : ctx->tail_split;      // (the pieces of a split ray would have to carry the instance they are in)
    return ta;
}
// The path kernel of a tree (path_plan.h: tree_path_kernel); a launch on round 1's kernel is counted in fused_fallback_launches.
static PathKernelChoice choose_path_kernel(HrtContext *ctx, const Tlas &t) {
    const PathKernelChoice pk = tree_path_kernel(fits_fused_kernel(ctx, t), t.two_level, ctx->fused_blocks_per_cu);
    if (pk.kernel == PathKernel::Round1) ctx->fused_fallback_launches++;
    return pk;
}
static PathScene path_scene(const Tlas &t) { return {!t.two_level, t.n_instances, t.has_spheres, t.dev.d_leaf_parent}; }
// A launch counts for its kernel and for every kernel that one is built on (device_types.h: path_ladder_rung).
static void count_ladder_launch(HrtContext *ctx, PathKernel kernel) {
    uint64_t *const rungs[] = {&ctx->one_group_launches, &ctx->restart_launches, &ctx->mask_idle_launches, &ctx->direct_launches};
    for (int r = 0; r < path_ladder_rung(kernel); ++r) ++*rungs[r];
}
extern "C++" {      // (helpers of hrt_internal.hpp, shared with hrt_denoise.cpp)
namespace hrt {
int refresh_tables(HrtContext *ctx, uint64_t handle, Tlas *t, hipStream_t s) {
    if (ctx->table_tlas == handle && ctx->table_tlas_gen == t->generation && ctx->table_mat_gen == ctx->materials_generation) return HRT_OK;
    const uint32_t n = std::max(t->n_instances, 1u);
    std::vector<HitGroup> hg(n); std::vector<uint32_t> prog(n, 0);
    for (auto &p : ctx->program_present) p = false;
    for (uint32_t i = 0; i < t->n_instances; ++i) {
        const uint32_t off = t->sbt_offset[i];
        if (off >= ctx->records.size()) return fail(ctx, HRT_ERR_STATE, "instance %u: sbtOffset %u has no SBT record (%zu set)", i, off, ctx->records.size());
        const HrtSbtRecord &r = ctx->records[off];
        const uint32_t program = r.header[3];
        const bool sphere_prog = program == HRT_PROGRAM_SPHERE_ROUGH || program == HRT_PROGRAM_SPHERE_METAL;
        if (sphere_prog != (t->kind[i] == kPrimKindSphere))
            return fail(ctx, HRT_ERR_STATE, "instance %u: program %u does not match its geometry", i, program);
        std::memcpy(&hg[i], &r.data, sizeof(HitGroup));
        prog[i] = program;
        ctx->program_present[program] = true;
    }
    const int rc = grow_device_arrays(ctx, {ctx->d_hitgroups, ctx->d_inst_program}, ctx->table_capacity, n);
    if (rc != HRT_OK) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_hitgroups, hg.data(), sizeof(HitGroup) * n, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_inst_program, prog.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    ctx->table_tlas = handle; ctx->table_tlas_gen = t->generation; ctx->table_mat_gen = ctx->materials_generation;
    return HRT_OK;
}

// The traversal of hrt_trace_rays (and of the denoiser's guide pass, hrt_denoise.cpp): n_rays rays already in RayRec form through the
// kernel hrt_render_launch runs in the context's configuration, hit records into tuvp / inst (t = tmax, inst = kMissPrim on a miss).
// fetch: 8 x 32 slice counters, zeroed here.  Enqueued only.
int trace_records(HrtContext *ctx, const Tlas &t, const RayRec *rays, uint32_t n_rays, float tmin, float tmax, bool any_hit,
                  float4 *tuvp, uint32_t *inst, uint32_t *fetch, hipStream_t s) {
    HIP_TRY(ctx, hipMemsetAsync(fetch, 0, sizeof(uint32_t) * 8 * 32, s));
    TraverseArgs ta = traverse_args(ctx, t, tmin, tmax);
    ta.fetch_counter = fetch; ta.leaf_hold = leaf_hold_for(ctx, t);
    const bool count = (ctx->flags & HRT_CTX_COUNT) != 0;
    if (!two_level_admitted(ctx, t, count)) return fail(ctx, HRT_ERR_STATE, "a two-level TLAS is traced by the default path kernel only");
    if (!count && ctx->fused > 0) {
        // the production configuration: the rays go through the very kernel hrt_render_launch runs (fused path kernel, v_rcp_f32
        // slab test, regeneration thresholds), each ray standing in for a pixel that is traced once and not shaded
        ta.refill_threshold = ctx->fused_refill_threshold; ta.fetch_chunk = (uint32_t)ctx->fused_fetch_chunk;
        PathArgs &pa = ta.path;
        pa.n_tile_pixels = n_rays; pa.first_pixel = 0; pa.width = n_rays; pa.height = 1; pa.spp = 1;
        pa.trace_rays = rays; pa.trace_tuvp = tuvp; pa.trace_inst = inst; pa.trace_any = any_hit ? 1u : 0u;
        pa.rays_closest = &ctx->d_stats->rays_closest; pa.rays_any = &ctx->d_stats->rays_any;
        const PathKernelChoice pk = choose_path_kernel(ctx, t);
        ta.postpone_pct = pk.kernel != PathKernel::Round1 ? ctx->fused_postpone_pct : ctx->postpone_pct;
        const uint32_t grid = std::min<uint32_t>((uint32_t)ctx->n_cu * pk.blocks_per_cu, (n_rays + 63u) / 64u);
        Timer tm(ctx, s, HRT_K_PATHS);
        // An empty interval (tmax <= tmin, or a NaN): every ray misses.  The path kernels' node step divides by bt - tmin (trav_common.h), so
        // they are not launched on one: the records are filled and the rays counted as the kernel would have.  (k_traverse, below, has no
        // such limit and takes every interval.)
        if (pk.kernel != PathKernel::Round1 && !(tmax > tmin)) launch_fill_misses(tuvp, inst, n_rays, tmax, any_hit ? pa.rays_any : pa.rays_closest, s);
        else if (!launch_path_kernel(pk.kernel, ta, path_scene(t), grid, s)) return fail(ctx, HRT_ERR_STATE, "the path kernel refused the launch (sample blocks with callers' rays)");
    } else {
        ta.seg[0].rays = rays; ta.seg[0].n_ptr = nullptr; ta.seg[0].n = n_rays; ta.seg[0].any_hit = any_hit ? 1u : 0u;
        ta.seg[0].hit_tuvp = tuvp; ta.seg[0].hit_inst = inst;
        ta.seg[0].count_nodes = any_hit ? &ctx->d_stats->nodes_any : &ctx->d_stats->nodes_closest;
        ta.seg[0].count_prims = any_hit ? &ctx->d_stats->prims_any : &ctx->d_stats->prims_closest;
        ta.refill_threshold = ctx->refill_threshold; ta.postpone_pct = ctx->postpone_pct; ta.fetch_chunk = (uint32_t)ctx->fetch_chunk;
        const uint32_t grid = std::min<uint32_t>((uint32_t)ctx->n_cu * (uint32_t)ctx->traverse_blocks_per_cu, (n_rays + 63u) / 64u);
        Timer tm(ctx, s, any_hit ? HRT_K_TRAVERSE_ANY : HRT_K_TRAVERSE);
        launch_traverse(ta, count, t.has_spheres, grid, s);
    }
    HIP_TRY(ctx, hipGetLastError());
    return HRT_OK;
}

}  // namespace hrt
}  // extern "C++"

// What both execution modes of a launch work from (hrt_render_launch has checked the arguments, found the tree, refreshed the material
// tables and uploaded the tile's row list).
struct LaunchFrame {
    HrtContext *ctx; Tlas *t; const HrtGlobalParams *h_params; const HrtRayGenParams *rg;
    uint32_t spp, n;               // samples per pixel, pixels of the tile
    hipStream_t s;
};

// ---- fused path mode: ONE launch, every lane owns a pixel and runs all its samples (generate, traverse, shade, accumulate in place).
//      No stage barriers.  The default (HRT_FUSED=1); trees outside k_fused's limits take round 1's path kernel. ----
// What every launch of a path kernel over a tile's pixels starts from (render_fused, hrt_render_accumulate): the tree, the regeneration's
// thresholds, the slice counters, the tile, the camera, the miss colour, the RNG states, the material tables, the ray counters.
static TraverseArgs fused_render_args(const LaunchFrame &f) {
    HrtContext *ctx = f.ctx; const Tlas *t = f.t; const HrtRayGenParams *rg = f.rg;
    Workspace &w = ctx->ws;
    TraverseArgs ta = traverse_args(ctx, *t, kFloatZero, kFloatInfinity);
    ta.fetch_counter = w.set[0].stages[0].fetch;
    ta.refill_threshold = ctx->fused_refill_threshold; ta.fetch_chunk = (uint32_t)ctx->fused_fetch_chunk;
    ta.leaf_hold = leaf_hold_for(ctx, *t);
    if (ctx->refill_auto && t->two_level) ta.refill_threshold = 12;      // (a two-level ray is long and its lanes finish far apart: 12 against 20 is +1.4-2.3 %, flattened trees lose 4 %)
    PathArgs &pa = ta.path;
    pa.rows = w.rows; pa.first_pixel = 0; pa.n_tile_pixels = f.n; pa.width = rg->width; pa.height = rg->height; pa.spp = f.spp;
    std::memcpy(pa.center, &rg->cameraCenter, 12); std::memcpy(pa.U, &rg->cameraU, 12);
    std::memcpy(pa.V, &rg->cameraV, 12); std::memcpy(pa.W, &rg->cameraW, 12);
    pa.bg[0] = ctx->miss.backgroundColor.x; pa.bg[1] = ctx->miss.backgroundColor.y; pa.bg[2] = ctx->miss.backgroundColor.z;
    pa.states = reinterpret_cast<RngState *>(f.h_params->stateArray);
    pa.hitgroups = ctx->d_hitgroups; pa.inst_program = ctx->d_inst_program; pa.accum = w.accum;
    pa.rays_closest = &ctx->d_stats->rays_closest; pa.rays_any = &ctx->d_stats->rays_any;
    return ta;
}
// ... and what the plan of such a render reads (path_plan.h), by value
static RenderPlanInput plan_input(const LaunchFrame &f) {
    const HrtContext *ctx = f.ctx; const Tlas &t = *f.t;
    RenderPlanInput in{};
    in.n_cu = ctx->n_cu;
    in.fits_fused = fits_fused_kernel(ctx, t); in.two_level = t.two_level; in.n_instances = t.n_instances; in.has_spheres = t.has_spheres;
    in.has_records = t.n_prims != 0u && t.n_nodes != 0u;      // (what ensure_leaf_parent makes a table of)
    in.n = f.n; in.full_frame = (uint64_t)f.n == (uint64_t)f.rg->width * f.rg->height; in.spp = f.spp;      // (the tile's rows are distinct: every row of the frame)
    in.reuse_primary = (ctx->flags & HRT_CTX_REUSE_PRIMARY) != 0u || ctx->reuse_primary;
    in.capture_primary = (ctx->flags & HRT_CTX_CAPTURE_PRIMARY) != 0u || ctx->capture_primary;
    in.fused_blocks_per_cu = ctx->fused_blocks_per_cu; in.traverse_blocks_auto = ctx->traverse_blocks_auto; in.fused_fetch_chunk = ctx->fused_fetch_chunk;
    in.fused_lpt = ctx->fused_lpt; in.sample_block = ctx->sample_block; in.taper_big = ctx->taper_big; in.taper_min = ctx->taper_min; in.taper_forced = ctx->taper_forced;
    in.fused_max_spp = ctx->fused_max_spp; in.seed_primary = ctx->seed_primary;
    in.knobs = PathKnobs{ctx->one_group, ctx->primary_restart, ctx->mask_idle, ctx->primary_direct};
    return in;
}
// The slice counters' protocol of those launches: zero on entry -- left so by the previous launch's finalize kernel, or set here -- ...
static int enter_slice_counters(HrtContext *ctx, hipStream_t s) {
    if (!ctx->fused_counters_clean) HIP_TRY(ctx, hipMemsetAsync(ctx->ws.set[0].stages, 0, sizeof(StageCounters), s));
    ctx->fused_counters_clean = false;
    return HRT_OK;
}
extern "C++" {
// What FinalizeArgs and FinalizeCountsArgs share: the tile's rows, its pixels, the frame's width, the samples, the four output buffers.
template <class Args>
static void fill_finalize(Args &fa, const LaunchFrame &f) {
    const HrtRayGenParams *rg = f.rg;
    fa.rows = f.ctx->ws.rows; fa.n_tile_pixels = f.n; fa.width = rg->width; fa.spp = f.spp;
    fa.color = reinterpret_cast<float4 *>(rg->colorBuffer); fa.albedo = reinterpret_cast<float4 *>(rg->albedoBuffer);
    fa.normal = reinterpret_cast<float4 *>(rg->normalBuffer); fa.linear = f.ctx->d_linear;
}
// ... and zeroed again by the frame's finalize kernel (launch_finalize, launch_finalize_counts) for whichever launch comes next, where that
// kernel has a thread per counter word; a smaller tile leaves them to the next entry.
template <class Args, class Launch>
static int finalize_and_reset_counters(const LaunchFrame &f, Args &fa, Launch launch) {
    HrtContext *ctx = f.ctx;
    fill_finalize(fa, f);
    constexpr uint32_t kCounterWords = (uint32_t)(sizeof(StageCounters) / sizeof(uint32_t));
    if (f.n >= kCounterWords) { fa.reset_counters = reinterpret_cast<uint32_t *>(ctx->ws.set[0].stages); fa.n_reset = kCounterWords; }
    { Timer tm(ctx, f.s, HRT_K_FINALIZE); launch(fa, f.s); }
    HIP_TRY(ctx, hipGetLastError());
    ctx->fused_counters_clean = fa.reset_counters != nullptr;
    return HRT_OK;
}
}  // extern "C++"

// The executor of a render's plan (path_plan.h says what is decided, and why): plan, size what the plan needs, run the probe if there is
// one, then launch by launch fill the arguments, make the table if wanted, launch and count; finalize.
static int render_fused(const LaunchFrame &f) {
    HrtContext *ctx = f.ctx; Tlas *t = f.t; const HrtGlobalParams *h_params = f.h_params; const HrtRayGenParams *rg = f.rg;
    const uint32_t n = f.n; hipStream_t s = f.s;
    Workspace &w = ctx->ws;
    const RenderPlanInput in = plan_input(f);
    const RenderPlan plan = plan_fused_render(in);
    const uint32_t grid = plan.grid, n_slices = plan.n_slices;
    if (plan.round1) ctx->fused_fallback_launches++;
    TraverseArgs ta = fused_render_args(f);
    PathArgs &pa = ta.path;
    ta.postpone_pct = plan.round1 ? ctx->postpone_pct : ctx->fused_postpone_pct;
    // what the plan needs: the primary-hit cache, the capture's arrays, the probe's cost and order, the blocks' progress words
    if (plan.primary_cache) {
        RC_TRY(grow_device_arrays(ctx, {{w.primary_cache, 2u * sizeof(float4)}}, w.primary_cache_lanes, grid * 64u));
        pa.primary_cache = w.primary_cache;
    }
    if (plan.capture) {
        PrimaryCapture &c = ctx->capture;
        if (n > c.capacity) HIP_TRY(ctx, hipStreamSynchronize(s));      // (a guide pass that reads the arrays may be under way)
        RC_TRY(grow_device_arrays(ctx, {c.tuvp, c.inst}, c.capacity, n));
    }
    if (plan.probe_spp) RC_TRY(grow_device_arrays(ctx, {w.slice_cost, w.slice_order}, w.slice_capacity, n_slices));
    if (plan.want_blocks) RC_TRY(grow_device_arrays(ctx, {w.block_progress}, w.block_capacity, n_slices));
    // the probe: a launch of its own that records each slice's cost; the slices are then handed out slowest first
    if (plan.probe_spp) {
        HIP_TRY(ctx, hipMemsetAsync(w.slice_cost, 0, sizeof(uint32_t) * n_slices, s));
        HIP_TRY(ctx, hipMemsetAsync(w.set[0].stages, 0, sizeof(StageCounters), s));
        pa.spp = plan.probe_spp; pa.continue_sum = 0u; pa.slice_cost = w.slice_cost; pa.slice_order = nullptr;
        { Timer tm(ctx, s, HRT_K_PATHS); (void)launch_path_kernel(plan.tree_kernel, ta, path_scene(*t), grid, s); }       // (sample_block is still 0: nothing to refuse)
        ctx->fused_counters_clean = false;
        ctx->h_slice_cost.resize(n_slices); ctx->h_slice_order.resize(n_slices);
        HIP_TRY(ctx, hipMemcpyAsync(ctx->h_slice_cost.data(), w.slice_cost, sizeof(uint32_t) * n_slices, hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipStreamSynchronize(s));
        for (uint32_t i = 0; i < n_slices; ++i) ctx->h_slice_order[i] = i;
        std::stable_sort(ctx->h_slice_order.begin(), ctx->h_slice_order.end(),
                         [&](uint32_t x, uint32_t y) { return ctx->h_slice_cost[x] > ctx->h_slice_cost[y]; });
        HIP_TRY(ctx, hipMemcpyAsync(w.slice_order, ctx->h_slice_order.data(), sizeof(uint32_t) * n_slices, hipMemcpyHostToDevice, s));
        pa.slice_cost = nullptr; pa.slice_order = w.slice_order;
    }
    bool captured = false;
    const int render_refill = ta.refill_threshold;
    for (uint32_t done_spp = plan.probe_spp; done_spp < f.spp;) {
        const LaunchPlan l = plan_fused_launch(plan, in, done_spp);
        ta.refill_threshold = launch_refill_threshold(l.kernel, render_refill, ctx->refill_auto);       // (k_path_direct's own, path_plan.h)
        pa.spp = l.now; pa.continue_sum = l.continue_sum;
        pa.sample_block = l.sample_block; pa.block_magic = l.block_magic; pa.block_min = l.block_min; pa.block_taper_end = l.block_taper_end;
        pa.block_slices = l.block_slices; pa.block_slices_magic = l.block_slices_magic; pa.block_chunk_magic = l.block_chunk_magic; pa.block_items = l.block_items;
        pa.block_progress = l.blocks ? w.block_progress : nullptr;
        if (l.blocks) {
            HIP_TRY(ctx, hipMemsetAsync(w.block_progress, 0, sizeof(uint32_t) * n_slices, s));
            ctx->sample_block_launches++;
            ctx->last_schedule[0] = l.sc.k_big; ctx->last_schedule[1] = l.sc.k_min; ctx->last_schedule[2] = l.block_taper_end; ctx->last_schedule[3] = l.sc.passes;
        }
        RC_TRY(enter_slice_counters(ctx, s));
        if (l.wants_table) RC_TRY(ensure_leaf_parent(ctx, *t, s));      // (made here the first time)
        const bool capturing = l.kernel == PathKernel::Capture;
        if (capturing) { pa.trace_tuvp = ctx->capture.tuvp; pa.trace_inst = ctx->capture.inst; }
        // HRT_MISS_BLOCK travels in trace_any, which only a launch over callers' rays reads otherwise (path_lane.h: path_finish, kDirect)
        pa.trace_any = l.kernel == PathKernel::Direct && ctx->miss_block ? 1u : 0u;
        bool admitted;
        { Timer tm(ctx, s, HRT_K_PATHS); admitted = launch_path_kernel(l.kernel, ta, path_scene(*t), grid, s); }
        if (!admitted) return fail(ctx, HRT_ERR_STATE, "the path kernel refused a launch in sample blocks (callers' rays, cost probe or slice order set; fewer waves than slice counters, no progress array, no items, or a schedule neither uniform nor tapered)");
        if (capturing) { pa.trace_tuvp = nullptr; pa.trace_inst = nullptr; ctx->primary_capture_launches++; captured = true; }
        count_ladder_launch(ctx, l.kernel);
        done_spp += l.now;
    }
    FinalizeArgs fa{};
    fa.accum = w.accum;
    RC_TRY(finalize_and_reset_counters(f, fa, launch_finalize));
    ctx->paths += (uint64_t)n * f.spp;
    ctx->last_tlas = h_params->handle;
    if (captured) {
        PrimaryCapture &c = ctx->capture;
        c.tlas = h_params->handle; c.generation = t->generation; c.width = rg->width; c.height = rg->height; c.states = h_params->stateArray;
        std::memcpy(c.camera, &rg->cameraCenter, 12); std::memcpy(c.camera + 12, &rg->cameraU, 12);
        std::memcpy(c.camera + 24, &rg->cameraV, 12); std::memcpy(c.camera + 36, &rg->cameraW, 12);
        c.valid = true;
    }
    return HRT_OK;
}

// ---- wavefront mode (HRT_FUSED=0, and always under HRT_CTX_COUNT): the north-star pipeline with separate kernels -- generate, traverse,
//      bin by material, shade per program, accumulate -- every kernel reading its input count from device memory, so a launch is a
//      fixed sequence of enqueues with no host synchronisation ----
static int render_wavefront(const LaunchFrame &f, bool count) {
    HrtContext *ctx = f.ctx; Tlas *t = f.t; const HrtGlobalParams *h_params = f.h_params; const HrtRayGenParams *rg = f.rg;
    const uint32_t spp = f.spp, n = f.n; hipStream_t s = f.s;
    Workspace &w = ctx->ws;
    int rc = HRT_OK;

    ctx->fused_counters_clean = false;      // (the wavefront schedule below shares the counters' memory)
    // ---- sub-tiles: contiguous ranges of the tile's pixels, each on its own stream.  A traverse
    //      launch ends with a tail (the longest rays, ~0.3 ms) during which most CUs idle; with
    //      2-3 independent sub-tiles in flight one sub-tile's tail overlaps another's bulk. ----
    // 0 = automatic: a full frame keeps one stream (clean per-kernel timing, the GPU is full anyway);
    // the smaller tiles of the multi-GPU split are latency-bound per stage and gain from 2-3 sub-tiles
    // in flight (measured on the 1/8 tile: 41.4 -> 37.6 ms per 32 spp with 3).
    uint32_t S = ctx->substreams > 0 ? (uint32_t)ctx->substreams : (n >= 1200000u ? 1u : (n >= 600000u ? 2u : 3u));
    while (S > 1 && n / S < (uint32_t)ctx->substream_min_pixels) --S;
    if (S > 1) {
        while (ctx->sub_streams.size() < S) {
            hipStream_t st; HIP_TRY(ctx, hipStreamCreateWithFlags(&st, hipStreamNonBlocking)); ctx->sub_streams.push_back(st);
            hipEvent_t ev; HIP_TRY(ctx, hipEventCreateWithFlags(&ev, hipEventDisableTiming)); ctx->sub_done.push_back(ev);
        }
        if (!ctx->ev_begin) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_begin, hipEventDisableTiming));
        HIP_TRY(ctx, hipEventRecord(ctx->ev_begin, s));
        for (uint32_t k = 0; k < S; ++k) HIP_TRY(ctx, hipStreamWaitEvent(ctx->sub_streams[k], ctx->ev_begin, 0));
    }
    struct Sub { uint32_t j0, n; hipStream_t st; uint32_t index; uint32_t grid_wide, grid_trav; };
    if (S > (uint32_t)kMaxSubTiles) S = kMaxSubTiles;
    // hipGraph replay of the per-sample launch sequence (below).  A capture cannot run on the legacy null stream -- the one the
    // reference, and a caller that passes NULL, uses -- so the pipeline then runs on a stream of the context's own, ordered after
    // the caller's work by an event and joined back before the finalize kernel.
    const bool want_graph = ctx->wavefront_graph && S == 1 && (ctx->flags & HRT_CTX_TIMING) == 0 && spp >= 5u;
    hipStream_t ws = s;
    if (want_graph && s == nullptr) {
        if (!ctx->graph_stream) HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->graph_stream, hipStreamNonBlocking));
        if (!ctx->ev_begin) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_begin, hipEventDisableTiming));
        if (!ctx->ev_graph_done) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_graph_done, hipEventDisableTiming));
        ws = ctx->graph_stream;
        HIP_TRY(ctx, hipEventRecord(ctx->ev_begin, s));
        HIP_TRY(ctx, hipStreamWaitEvent(ws, ctx->ev_begin, 0));
    }
    std::vector<Sub> subs(S);
    for (uint32_t k = 0; k < S; ++k) {
        const uint32_t j0 = (uint32_t)((uint64_t)n * k / S), j1 = (uint32_t)((uint64_t)n * (k + 1) / S);
        subs[k].j0 = j0; subs[k].n = j1 - j0; subs[k].st = S > 1 ? ctx->sub_streams[k] : ws; subs[k].index = k;
        subs[k].grid_wide = std::min<uint32_t>((uint32_t)ctx->n_cu * 8u, (subs[k].n + 255u) / 256u);
        subs[k].grid_trav = std::min<uint32_t>((uint32_t)ctx->n_cu * (uint32_t)ctx->traverse_blocks_per_cu, (2u * subs[k].n + 63u) / 64u);
    }

    // ---- schedule.  Class (s, d) = the rays of sample s at depth d.  Samples are sequential per pixel
    //      (one persistent RNG stream), but two things are off that chain: the primary rays of sample
    //      s+1 draw no random numbers, and the depth-5 rays of sample s only decide black / background.
    //      They ride along with the launches of the chain:
    //          T{(s,2),(s-1,5)}   T{(s,3)}   T{(s,4),(s+1,1)}
    //      so a sample costs three traversal launches instead of five, and the under-filled depth-5
    //      launch disappears.  Shading order (RNG) and the order of the per-sample sums stay sequential. ----
    auto stages_of = [&](uint32_t sample, const Sub &sb) { return w.set[sample & 1u].stages + (size_t)sb.index * (kRayTraceDepth + 1); };
    auto seg_of = [&](uint32_t sample, uint32_t depth, const Sub &sb) {
        SampleSet &st = w.set[sample & 1u];
        TraverseSeg g{};
        g.rays = st.rays[(depth - 1u) & 1u] + sb.j0;
        g.n_ptr = depth == 1 ? nullptr : &stages_of(sample, sb)[depth - 1].bin_count[1];
        g.n = sb.n;
        g.any_hit = depth >= kRayTraceDepth ? 1u : 0u;      // a hit at the depth limit is black whatever it is (Shader.cu:102-107)
        g.hit_tuvp = st.hit_tuvp + sb.j0; g.hit_inst = st.hit_inst + sb.j0;
        g.count_nodes = g.any_hit ? &ctx->d_stats->nodes_any : &ctx->d_stats->nodes_closest;
        g.count_prims = g.any_hit ? &ctx->d_stats->prims_any : &ctx->d_stats->prims_closest;
        return g;
    };
    auto do_generate = [&](uint32_t sample, const Sub &sb) -> int {
        HIP_TRY(ctx, hipMemsetAsync(stages_of(sample, sb), 0, sizeof(StageCounters) * (kRayTraceDepth + 1), sb.st));
        GenerateArgs ga{};
        ga.rays = w.set[sample & 1u].rays[0] + sb.j0; ga.rows = w.rows; ga.first_pixel = sb.j0; ga.n_tile_pixels = sb.n;
        ga.width = rg->width; ga.height = rg->height;
        std::memcpy(ga.center, &rg->cameraCenter, 12); std::memcpy(ga.U, &rg->cameraU, 12);
        std::memcpy(ga.V, &rg->cameraV, 12); std::memcpy(ga.W, &rg->cameraW, 12);
        Timer tm(ctx, sb.st, HRT_K_GENERATE); launch_generate(ga, sb.st);
        return HRT_OK;
    };
    // one traverse launch over class (sa, da) and, optionally, class (sb_, db)
    auto do_traverse = [&](const Sub &sb, uint32_t sa, uint32_t da, bool second, uint32_t sb_, uint32_t db) {
        TraverseArgs ta = traverse_args(ctx, *t, kFloatZero, kFloatInfinity);      // Shader.cu:232, :266
        ta.seg[0] = seg_of(sa, da, sb);
        if (second) ta.seg[1] = seg_of(sb_, db, sb);
        ta.fetch_counter = stages_of(sa, sb)[da].fetch;
        ta.leaf_hold = 4; ta.fetch_chunk = (uint32_t)ctx->fetch_chunk;
        Timer tm(ctx, sb.st, (da >= kRayTraceDepth && !second) ? HRT_K_TRAVERSE_ANY : HRT_K_TRAVERSE);
        // production traversal: k_fused's traversal over the ray queues (k_trace_queue); the counting build and trees that do not fit
        // k_fused's stacks / offsets keep round 1's k_traverse
        if (!count && fits_fused_kernel(ctx, *t)) {
            ta.postpone_pct = ctx->fused_postpone_pct; ta.refill_threshold = ctx->fused_refill_threshold;
            const uint32_t grid = std::min<uint32_t>((uint32_t)ctx->n_cu * (uint32_t)std::min(ctx->traverse_blocks_per_cu, kFusedBlocksPerCu), (2u * sb.n + 63u) / 64u);
            launch_trace_queue(ta, t->has_spheres, grid, sb.st);
        } else {
            ta.postpone_pct = ctx->postpone_pct; ta.refill_threshold = ctx->refill_threshold;
            launch_traverse(ta, count, t->has_spheres, sb.grid_trav, sb.st);
        }
    };
    // everything that follows the traversal of class (sample, depth): binning, shading, path ends
    auto do_after = [&](const Sub &sb, uint32_t sample, uint32_t depth) {
        SampleSet &st = w.set[sample & 1u];
        StageCounters *stg = stages_of(sample, sb);
        hipStream_t strm = sb.st;
        uint32_t *bin_items = st.bin_items + (size_t)sb.j0 * kNumBins;
        const RayRec *rays_in = st.rays[(depth - 1u) & 1u] + sb.j0;
        BinArgs ba{};
        ba.n_rays_ptr = depth == 1 ? nullptr : &stg[depth - 1].bin_count[1]; ba.n_rays = sb.n;
        ba.hit_inst = st.hit_inst + sb.j0; ba.inst_program = ctx->d_inst_program; ba.depth = depth;
        ba.bin_count = stg[depth].bin_count; ba.bin_items = bin_items; ba.bin_stride = sb.n;
        ba.total_rays = depth >= kRayTraceDepth ? &ctx->d_stats->rays_any : &ctx->d_stats->rays_closest;
        { Timer tm(ctx, strm, HRT_K_BIN); launch_bin(ba, sb.grid_wide, strm); }
        if (depth < kRayTraceDepth) {
            ShadeArgs sa{};
            sa.bin_count = stg[depth].bin_count; sa.bin_items = bin_items; sa.bin_stride = sb.n;
            sa.rays_in = rays_in; sa.rays_out = st.rays[depth & 1u] + sb.j0;
            sa.hit_tuvp = st.hit_tuvp + sb.j0; sa.hit_inst = st.hit_inst + sb.j0; sa.hitgroups = ctx->d_hitgroups;
            sa.states = reinterpret_cast<RngState *>(h_params->stateArray);
            sa.chain = st.chain; sa.depth = depth;
            for (int p = 0; p < (int)kNumPrograms; ++p)
                if (ctx->program_present[p]) { Timer tm(ctx, strm, HRT_K_SHADE); launch_shade(sa, p, sb.grid_wide, strm); }
        }
        AccumArgs aa{};
        aa.bin_count = stg[depth].bin_count; aa.bin_items = bin_items; aa.rays_in = rays_in; aa.hit_inst = st.hit_inst + sb.j0;
        aa.hitgroups = ctx->d_hitgroups; aa.chain = st.chain; aa.result = st.result;
        aa.bg[0] = ctx->miss.backgroundColor.x; aa.bg[1] = ctx->miss.backgroundColor.y; aa.bg[2] = ctx->miss.backgroundColor.z;
        aa.depth = depth;
        { Timer tm(ctx, strm, HRT_K_ACCUMULATE); launch_accumulate(aa, sb.grid_wide, strm); }
        if (depth >= kRayTraceDepth) {       // the sample is complete: add it, in sample order
            Timer tm(ctx, strm, HRT_K_ACCUMULATE);
            launch_sum(w.accum + sb.j0, st.result + sb.j0, sb.n, sample == 0 ? 1u : 0u, strm);
        }
    };

    for (const Sub &sb : subs) { rc = do_generate(0, sb); if (rc != HRT_OK) return rc; }
    for (const Sub &sb : subs) do_traverse(sb, 0, 1, false, 0, 0);
    auto sample_body = [&](uint32_t sample) -> int {
        const bool prev = sample > 0, next = sample + 1 < spp;
        for (const Sub &sb : subs) do_after(sb, sample, 1);
        for (const Sub &sb : subs) do_traverse(sb, sample, 2, prev, sample - 1, kRayTraceDepth);
        if (prev) for (const Sub &sb : subs) do_after(sb, sample - 1, kRayTraceDepth);
        for (const Sub &sb : subs) do_after(sb, sample, 2);
        for (const Sub &sb : subs) do_traverse(sb, sample, 3, false, 0, 0);
        for (const Sub &sb : subs) do_after(sb, sample, 3);
        if (next) for (const Sub &sb : subs) { const int r = do_generate(sample + 1, sb); if (r != HRT_OK) return r; }
        for (const Sub &sb : subs) do_traverse(sb, sample, 4, next, sample + 1, 1);
        for (const Sub &sb : subs) do_after(sb, sample, 4);
        return HRT_OK;
    };
    uint32_t sample = 0;
    rc = sample_body(sample++);
    if (rc != HRT_OK) return rc;
    // Samples 2 .. spp - 2 enqueue the same ~45 operations on the same buffers, alternating between the two workspace sets:
    // a pair of them is captured once as a hipGraph and replayed (HRT_WAVEFRONT_GRAPH=1; one stream, no per-kernel event
    // timers inside a graph, so not under HRT_CTX_TIMING).  Every kernel reads its ray count from device memory, so the
    // replayed launches are the eager ones, and the image is the same bits.  (Sample 1 is not like the others: its launches
    // add sample 0 to the running sum with the "initialise" flag set.)
    if (want_graph) {
        rc = sample_body(sample++);
        if (rc != HRT_OK) return rc;
        const uint32_t pairs = (spp - 3u) / 2u;
        hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr;
        HIP_TRY(ctx, hipStreamBeginCapture(ws, hipStreamCaptureModeThreadLocal));
        int rc1 = sample_body(2u);
        if (rc1 == HRT_OK) rc1 = sample_body(3u);
        const hipError_t ce = hipStreamEndCapture(ws, &graph);
        if (rc1 != HRT_OK) { if (graph) (void)hipGraphDestroy(graph); return rc1; }
        HIP_TRY(ctx, ce);
        hipError_t ge = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        for (uint32_t k = 0; k < pairs && ge == hipSuccess; ++k) ge = hipGraphLaunch(exec, ws);
        // (the executable graph must outlive its launches: the stream is drained before it is destroyed)
        if (ge == hipSuccess) ge = hipStreamSynchronize(ws);
        if (exec) (void)hipGraphExecDestroy(exec);
        (void)hipGraphDestroy(graph);
        HIP_TRY(ctx, ge);
        sample += 2u * pairs;
        ctx->graph_replays += pairs;
    }
    for (; sample < spp; ++sample) { rc = sample_body(sample); if (rc != HRT_OK) return rc; }
    for (const Sub &sb : subs) do_traverse(sb, spp - 1, kRayTraceDepth, false, 0, 0);
    for (const Sub &sb : subs) do_after(sb, spp - 1, kRayTraceDepth);
    if (ws != s) {
        HIP_TRY(ctx, hipEventRecord(ctx->ev_graph_done, ws));
        HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->ev_graph_done, 0));
    }
    if (S > 1) {
        for (uint32_t k = 0; k < S; ++k) {
            HIP_TRY(ctx, hipEventRecord(ctx->sub_done[k], ctx->sub_streams[k]));
            HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->sub_done[k], 0));
        }
    }
    FinalizeArgs fa{};
    fa.accum = w.accum; fill_finalize(fa, f);
    { Timer tm(ctx, s, HRT_K_FINALIZE); launch_finalize(fa, s); }
    HIP_TRY(ctx, hipGetLastError());
    ctx->paths += (uint64_t)n * spp;
    ctx->last_tlas = h_params->handle;
    return HRT_OK;
}

// The tile of a launch (NULL: the whole frame): its rows uploaded -- the list of the previous launch is kept while frame and tile are the
// same --, the workspace sized.  n: the tile's pixels; 0: an empty tile, nothing to do.
static int prepare_tile(HrtContext *ctx, const HrtRayGenParams *rg, const HrtTile *tile, hipStream_t s, uint32_t &n) {
    n = 0;
    HrtTile tl = tile ? *tile : HrtTile{0, rg->height, 1, 1, 0};
    if (tl.stripe_rows == 0 || tl.stripe_period == 0 || tl.stripe_phase >= tl.stripe_period || tl.y_begin > tl.y_end || tl.y_end > rg->height)
        return fail(ctx, HRT_ERR_INVALID, "bad tile");
    const bool same_rows = ctx->rows_w == rg->width && ctx->rows_h == rg->height && std::memcmp(&ctx->rows_tile, &tl, sizeof tl) == 0 && ctx->ws.rows;
    if (!same_rows) {
        ctx->rows_w = ctx->rows_h = 0;       // the cached row list is being replaced: its key is valid again only once the upload below has succeeded
        ctx->h_rows.clear();
        for (uint32_t y = tl.y_begin; y < tl.y_end; ++y)
            if ((y / tl.stripe_rows) % tl.stripe_period == tl.stripe_phase) ctx->h_rows.push_back(y);
    }
    const uint32_t n_rows = (uint32_t)ctx->h_rows.size();
    const uint64_t n64 = (uint64_t)n_rows * rg->width;
    if (n64 == 0) return HRT_OK;
    const int rc = ensure_workspace(ctx, (uint32_t)n64, rg->height);
    if (rc != HRT_OK) return rc;
    Workspace &w = ctx->ws;
    if (!same_rows) {
        HIP_TRY(ctx, hipMemcpyAsync(w.rows, ctx->h_rows.data(), sizeof(uint32_t) * n_rows, hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipStreamSynchronize(s));
        ctx->rows_tile = tl; ctx->rows_w = rg->width; ctx->rows_h = rg->height;
    }
    n = (uint32_t)n64;
    return HRT_OK;
}

// The frame of a launch (hrt_render_launch, hrt_render_accumulate): its size, the colour buffer, the RNG states.  Touches nothing.
static int check_frame(HrtContext *ctx, const HrtGlobalParams *h_params, const HrtRayGenParams *rg) {
    if (rg->width == 0 || rg->height == 0 || (uint64_t)rg->width * rg->height > 0xffffffffull) return fail(ctx, HRT_ERR_INVALID, "bad frame size %ux%u", rg->width, rg->height);
    if (!rg->colorBuffer) return fail(ctx, HRT_ERR_INVALID, "RayGenParams.colorBuffer is NULL");
    if (!h_params->stateArray) return fail(ctx, HRT_ERR_INVALID, "GlobalParams.stateArray is NULL");
    return HRT_OK;
}

int hrt_render_launch(HrtContext *ctx, const HrtGlobalParams *h_params, const HrtRayGenParams *rg, uint32_t spp,
                      const HrtTile *tile, void *stream) {
    if (!ctx || !h_params || !rg) return HRT_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    (void)hipSetDevice(ctx->device);
    ctx->capture.valid = false;      // (whatever this launch does: only a complete capture of its own makes it valid again, render_fused)
    if (spp == 0) return fail(ctx, HRT_ERR_INVALID, "spp must be >= 1");
    RC_TRY(check_frame(ctx, h_params, rg));
    if (!ctx->have_records) return fail(ctx, HRT_ERR_STATE, "hrt_materials_set has not been called");
    Tlas *t;
    int rc = find_tlas(ctx, h_params->handle, t);
    if (rc == HRT_OK) rc = refresh_tables(ctx, h_params->handle, t, s);
    if (rc != HRT_OK) return rc;

    uint32_t n;
    rc = prepare_tile(ctx, rg, tile, s, n);
    if (rc != HRT_OK || n == 0u) return rc;

    const bool count = (ctx->flags & HRT_CTX_COUNT) != 0;
    if (!two_level_admitted(ctx, *t, count)) return fail(ctx, HRT_ERR_STATE, "a two-level TLAS is traced by the default path kernel only (not under HRT_CTX_COUNT / HRT_FUSED != 1, and not beyond its limits)");
    const LaunchFrame frame{ctx, t, h_params, rg, spp, n, s};
    const bool use_fused = !count && (ctx->fused > 0 || (ctx->fused < 0 && n <= (uint32_t)ctx->fused_max_pixels));
    return use_fused ? render_fused(frame) : render_wavefront(frame, count);
}

// ---- adaptive sampling (include/hrt.h): one launch of k_path_counts over the caller's sums, then its finalize kernel.  Every refusal comes
//      before anything of the context or the caller's is touched. ----
int hrt_render_accumulate(HrtContext *ctx, const HrtGlobalParams *h_params, const HrtRayGenParams *rg, uint32_t spp, const uint32_t *d_counts,
                          HrtFloat4 *d_sum, uint32_t *d_taken, const HrtTile *tile, void *stream) {
    if (!ctx || !h_params || !rg) return HRT_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    (void)hipSetDevice(ctx->device);
    if (spp == 0 || spp > 65536u) return fail(ctx, HRT_ERR_INVALID, "spp must be 1..65536 (got %u)", spp);
    if (!d_sum || !d_taken) return fail(ctx, HRT_ERR_INVALID, "d_sum / d_taken is NULL");
    RC_TRY(check_frame(ctx, h_params, rg));
    if ((ctx->flags & HRT_CTX_COUNT) != 0u) return fail(ctx, HRT_ERR_STATE, "hrt_render_accumulate runs the path kernel k_path_counts: not under HRT_CTX_COUNT");
    if (ctx->fused != 1) return fail(ctx, HRT_ERR_STATE, "hrt_render_accumulate runs the path kernel k_path_counts: not with HRT_FUSED != 1");
    if (!ctx->have_records) return fail(ctx, HRT_ERR_STATE, "hrt_materials_set has not been called");
    Tlas *t;
    int rc = find_tlas(ctx, h_params->handle, t);
    if (rc != HRT_OK) return rc;
    if (!fits_fused_kernel(ctx, *t)) return fail(ctx, HRT_ERR_STATE, "hrt_render_accumulate: the tree is outside k_fused's limits (depth %u, HRT_FUSED_MAX_DEPTH / HRT_FUSED_MAX_BYTES)", t->max_depth);
    rc = refresh_tables(ctx, h_params->handle, t, s);
    if (rc != HRT_OK) return rc;
    uint32_t n;
    rc = prepare_tile(ctx, rg, tile, s, n);
    if (rc != HRT_OK) return rc;
    ctx->capture.valid = false;
    if (n == 0u) return HRT_OK;

    const LaunchFrame frame{ctx, t, h_params, rg, spp, n, s};
    TraverseArgs ta = fused_render_args(frame);
    ta.postpone_pct = ctx->fused_postpone_pct;
    PathArgs &pa = ta.path;
    // (the fields that are free in this launch carry the caller's arrays, all in frame order: path_lane.h, kCounts)
    pa.accum = reinterpret_cast<float4 *>(d_sum); pa.trace_inst = d_taken; pa.slice_order = d_counts;
    const PathKernelChoice pk = choose_path_kernel(ctx, *t);
    const uint32_t grid = fused_render_grid(ctx->n_cu, ctx->traverse_blocks_auto, pk.blocks_per_cu, n);
    RC_TRY(enter_slice_counters(ctx, s));
    bool admitted;
    { Timer tm(ctx, s, HRT_K_PATHS); admitted = launch_path_kernel(PathKernel::Counts, ta, path_scene(*t), grid, s); }
    if (!admitted) return fail(ctx, HRT_ERR_STATE, "the path kernel refused the counts launch");
    FinalizeCountsArgs fa{};
    fa.sum = pa.accum; fa.taken = d_taken; fa.counts = d_counts;
    // HrtStats.paths: a uniform launch's samples are known here, a map's are summed by the finalize kernel (read in hrt_stats_get)
    if (d_counts) fa.paths = reinterpret_cast<unsigned long long *>(&ctx->d_stats->paths);
    else ctx->paths += (uint64_t)n * spp;
    RC_TRY(finalize_and_reset_counters(frame, fa, launch_finalize_counts));
    ctx->last_tlas = h_params->handle;
    return HRT_OK;
}

int hrt_sample_counts_default_params(HrtSampleCountParams *out) {
    if (!out) return HRT_ERR_INVALID;
    *out = HrtSampleCountParams{0.05f, 1u, 64u, 1u, {0u, 0u}};
    return HRT_OK;
}

int hrt_sample_counts(HrtContext *ctx, const HrtFloat4 *d_sum, const uint32_t *d_taken, uint32_t width, uint32_t height,
                      const HrtSampleCountParams *h_params, uint32_t *d_counts, void *stream) {
    if (!ctx || !d_sum || !d_taken || !d_counts) return HRT_ERR_INVALID;
    if ((uint64_t)width * height > 0xffffffffull) return fail(ctx, HRT_ERR_INVALID, "frame too large");
    HrtSampleCountParams p;
    (void)hrt_sample_counts_default_params(&p);
    if (h_params) p = *h_params;
    if (!(p.target_sigma > 0.0f) || !std::isfinite(p.target_sigma)) return fail(ctx, HRT_ERR_INVALID, "HrtSampleCountParams.target_sigma must be > 0 and finite");
    if (p.min_total < 1u || p.min_total > 65536u || p.max_total < p.min_total || p.max_total > 65536u)
        return fail(ctx, HRT_ERR_INVALID, "HrtSampleCountParams: 1 <= min_total <= max_total <= 65536 (got %u, %u)", p.min_total, p.max_total);
    if (p.radius > 2u) return fail(ctx, HRT_ERR_INVALID, "HrtSampleCountParams.radius must be 0..2 (got %u)", p.radius);
    if (p.reserved[0] != 0u || p.reserved[1] != 0u) return fail(ctx, HRT_ERR_INVALID, "HrtSampleCountParams.reserved must be 0");
    (void)hipSetDevice(ctx->device);
    SampleCountArgs a{};
    a.sum = reinterpret_cast<const float4 *>(d_sum); a.taken = d_taken; a.counts = d_counts;
    a.width = width; a.height = height; a.radius = p.radius; a.min_total = p.min_total; a.max_total = p.max_total; a.target_sigma = p.target_sigma;
    launch_sample_counts(a, (hipStream_t)stream);
    HIP_TRY(ctx, hipGetLastError());
    return HRT_OK;
}


int hrt_sync(HrtContext *ctx, void *stream) {
    if (!ctx) return HRT_ERR_INVALID;
    (void)hipSetDevice(ctx->device);
    HIP_TRY(ctx, hipStreamSynchronize((hipStream_t)stream));
    return HRT_OK;
}

int hrt_to_rgba8(HrtContext *ctx, const HrtFloat4 *d_src, HrtUchar4 *d_dst, uint32_t width, uint32_t height, void *stream) {
    if (!ctx || !d_src || !d_dst) return HRT_ERR_INVALID;
    const uint64_t n = (uint64_t)width * height;
    if (n > 0xffffffffull) return fail(ctx, HRT_ERR_INVALID, "frame too large");
    (void)hipSetDevice(ctx->device);
    launch_to_rgba8(reinterpret_cast<const float4 *>(d_src), reinterpret_cast<uchar4 *>(d_dst), (uint32_t)n, (hipStream_t)stream);
    HIP_TRY(ctx, hipGetLastError());
    return HRT_OK;
}

int hrt_color_to_float4(HrtContext *ctx, const HrtFloat4 *d_src, HrtFloat4 *d_dst, uint32_t n, void *stream) {
    if (!ctx || (n && (!d_src || !d_dst))) return HRT_ERR_INVALID;
    (void)hipSetDevice(ctx->device);
    launch_color_to_float4(reinterpret_cast<const float4 *>(d_src), reinterpret_cast<float4 *>(d_dst), n, (hipStream_t)stream);
    HIP_TRY(ctx, hipGetLastError());
    return HRT_OK;
}

// ---- measurement ----------------------------------------------------------------------
int hrt_sample_schedule(uint32_t spp, uint32_t block_big, uint32_t block_min, uint32_t *first, uint32_t capacity, uint32_t *n_passes) {
    const bool tapered = block_min != 0u;
    if (!first || !n_passes || spp == 0u || block_big == 0u || block_min > block_big) return HRT_ERR_INVALID;
    if (tapered && ((block_big & (block_big - 1u)) != 0u || (block_min & (block_min - 1u)) != 0u || !taper_fits(spp, block_big))) return HRT_ERR_INVALID;
    const SampleSchedule sc = tapered ? sample_schedule(spp, block_big, block_min) : uniform_schedule(spp, block_big);
    if (sc.passes >= capacity) return HRT_ERR_INVALID;
    for (uint32_t b = 0; b < sc.passes; ++b) first[b] = schedule_first(sc, b);
    first[sc.passes] = spp;
    // what the kernel's lanes see: a boundary behind sample p exactly where a pass starts (block_ends is path_finish's test)
    if (tapered)
        for (uint32_t p = 1, b = 1; p < spp; ++p) {
            const bool starts = b < sc.passes && first[b] == p;
            if (block_ends(sc.k_big, sc.k_min, sc.taper_end, p) != starts) return HRT_ERR_STATE;
            if (starts) ++b;
        }
    // ... and what k_path_direct's miss block steps with (device_types.h: hold_ends), uniform blocks too: a lane's hold ends behind sample p - 1
    // exactly where a pass starts or the launch's samples end, with the block fields a launch of this schedule gets (path_plan.h)
    const uint32_t magic = tapered ? 0u : (uint32_t)std::min<uint64_t>((1ull << 32) / sc.k_big, 0xffffffffull);
    for (uint32_t p = 1, b = 1; p <= spp; ++p) {
        const bool starts = b < sc.passes && first[b] == p;
        if (hold_ends(spp, sc.k_big, magic, tapered ? sc.k_min : 0u, tapered ? sc.taper_end : 0u, p) != (starts || p == spp)) return HRT_ERR_STATE;
        if (starts) ++b;
    }
    *n_passes = sc.passes;
    return HRT_OK;
}

int hrt_stats_reset(HrtContext *ctx) {
    if (!ctx) return HRT_ERR_INVALID;
    (void)hipSetDevice(ctx->device);
    HIP_TRY(ctx, hipDeviceSynchronize());
    HIP_TRY(ctx, hipMemset(ctx->d_stats, 0, sizeof(DeviceStats)));
    drain_spans(ctx);
    for (int k = 0; k < HRT_K_COUNT; ++k) { ctx->kernel_ms[k] = 0.0; ctx->kernel_launches[k] = 0; }
    ctx->paths = 0;
    return HRT_OK;
}

int hrt_stats_get(HrtContext *ctx, HrtStats *out) {
    if (!ctx || !out) return HRT_ERR_INVALID;
    (void)hipSetDevice(ctx->device);
    HIP_TRY(ctx, hipDeviceSynchronize());
    drain_spans(ctx);
    DeviceStats ds;
    HIP_TRY(ctx, hipMemcpy(&ds, ctx->d_stats, sizeof ds, hipMemcpyDeviceToHost));
    std::memset(out, 0, sizeof *out);
    out->rays_closest = ds.rays_closest; out->rays_any = ds.rays_any; out->rays = ds.rays_closest + ds.rays_any;
    out->paths = ctx->paths + ds.paths; out->node_visits = ds.nodes_closest + ds.nodes_any; out->prim_tests = ds.prims_closest + ds.prims_any;
    out->node_visits_closest = ds.nodes_closest; out->prim_tests_closest = ds.prims_closest;
    for (int k = 0; k < 4; ++k) out->debug[k] = ds.debug[k];
    for (int k = 0; k < 8; ++k) out->tail[k] = ds.tail[k];
    for (int k = 0; k < 60; ++k) out->wave_clock[k] = ds.wave_clock[k];
    out->tlas_refits = ctx->tlas_refits; out->tlas_rebuilds = ctx->tlas_rebuilds; out->tlas_refit_ratio = ctx->tlas_refit_ratio;
    for (int k = 0; k < HRT_K_COUNT; ++k) { out->kernel_ms[k] = ctx->kernel_ms[k]; out->kernel_launches[k] = ctx->kernel_launches[k]; }
    std::lock_guard<std::mutex> lk(ctx->mu);
    auto it = ctx->tlas.find(ctx->last_tlas);
    if (it != ctx->tlas.end()) {
        const Tlas &tl = *it->second;
        out->bvh_nodes = tl.n_nodes; out->bvh_triangles = tl.n_triangles; out->bvh_spheres = tl.n_spheres; out->bvh_depth = tl.max_depth;
        out->bvh_bytes = (uint64_t)tl.n_nodes * sizeof(Bvh8Node) + (uint64_t)tl.n_prims * sizeof(PrimRecord);
        out->bvh_alloc_bytes = tl.alloc_bytes;
    }
    out->fused_fallback_launches = ctx->fused_fallback_launches; out->graph_replays = ctx->graph_replays;
    out->sample_block_launches = ctx->sample_block_launches;
    for (int i = 0; i < 4; ++i) out->sample_block_schedule[i] = ctx->last_schedule[i];
    out->primary_capture_launches = ctx->primary_capture_launches;
    out->guide_passes_traced = ctx->guide_passes_traced; out->guide_passes_captured = ctx->guide_passes_captured;
    out->denoise_history_rebinds = ctx->denoise_history_rebinds;
    out->denoise_by_primitive_links = ctx->denoise_by_primitive_links;
    out->one_group_launches = ctx->one_group_launches; out->restart_launches = ctx->restart_launches; out->mask_idle_launches = ctx->mask_idle_launches; out->direct_launches = ctx->direct_launches;
    return HRT_OK;
}

int hrt_primary_hits_get(HrtContext *ctx, float *d_t, float *d_u, float *d_v, uint32_t *d_prim, uint32_t *d_inst, void *stream) {
    if (!ctx) return HRT_ERR_INVALID;
    (void)hipSetDevice(ctx->device);
    const PrimaryCapture &c = ctx->capture;
    if (!c.valid) return fail(ctx, HRT_ERR_STATE, "no valid primary-hit capture: the last hrt_render_launch did not capture the whole frame (HRT_CTX_CAPTURE_PRIMARY), or the scene, the flags or the frame have changed since");
    launch_unpack_hits(c.tuvp, c.inst, c.width * c.height, d_t, d_u, d_v, d_prim, d_inst, (hipStream_t)stream);
    HIP_TRY(ctx, hipGetLastError());
    return HRT_OK;
}

// ---- introspection for the parity tests -----------------------------------------------
int hrt_trace_rays(HrtContext *ctx, HrtTraversable tlas, const HrtFloat3 *d_origins, const HrtFloat3 *d_directions, uint32_t n_rays,
                   float tmin, float tmax, int any_hit, float *d_t, float *d_u, float *d_v, uint32_t *d_prim, uint32_t *d_inst, void *stream) {
    if (!ctx || !d_origins || !d_directions || !d_t || !d_u || !d_v || !d_prim || !d_inst) return HRT_ERR_INVALID;
    if (n_rays == 0) return HRT_OK;
    hipStream_t s = (hipStream_t)stream;
    (void)hipSetDevice(ctx->device);
    Tlas *t;
    { std::lock_guard<std::mutex> lk(ctx->mu); auto it = ctx->tlas.find(tlas); if (it == ctx->tlas.end()) return fail(ctx, HRT_ERR_INVALID, "unknown TLAS handle"); t = it->second.get(); }
    RayRec *rays = nullptr; float4 *tuvp = nullptr; uint32_t *inst = nullptr, *fetch = nullptr;
    struct Scratch { void **p[4]; ~Scratch() { for (void **q : p) if (*q) (void)hipFree(*q); } }
        scratch{{(void **)&rays, (void **)&tuvp, (void **)&inst, (void **)&fetch}};     // freed on every way out
    HIP_TRY(ctx, hipMalloc((void **)&rays, sizeof(RayRec) * (size_t)n_rays));
    HIP_TRY(ctx, hipMalloc((void **)&tuvp, sizeof(float4) * (size_t)n_rays));
    HIP_TRY(ctx, hipMalloc((void **)&inst, sizeof(uint32_t) * (size_t)n_rays));
    HIP_TRY(ctx, hipMalloc((void **)&fetch, sizeof(uint32_t) * 8 * 32));
    launch_pack_rays(reinterpret_cast<const float *>(d_origins), reinterpret_cast<const float *>(d_directions), n_rays, rays, s);
    const int rc = trace_records(ctx, *t, rays, n_rays, tmin, tmax, any_hit != 0, tuvp, inst, fetch, s);
    if (rc != HRT_OK) return rc;
    launch_unpack_hits(tuvp, inst, n_rays, d_t, d_u, d_v, d_prim, d_inst, s);
    hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(ctx, HRT_ERR_HIP, "hrt_trace_rays: %s", hipGetErrorString(e));
    ctx->last_tlas = tlas;
    return HRT_OK;
}

int hrt_debug_set_linear_output(HrtContext *ctx, HrtFloat4 *d_linear) {
    if (!ctx) return HRT_ERR_INVALID;
    ctx->d_linear = reinterpret_cast<float4 *>(d_linear);
    return HRT_OK;
}

}  // extern "C"
