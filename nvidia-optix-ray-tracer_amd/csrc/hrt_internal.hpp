// hrt_internal.hpp -- what the translation units of libhrt.so share: the objects behind the opaque handles of
// include/hrt.h (context, BLAS, TLAS, workspace), error plumbing and the helpers that cross file boundaries.
// hrt_api.cpp: context, materials, RNG, the launch, measurement.  hrt_accel.cpp: acceleration structures
// (build, per-frame refit, trees over instances, poses, download).  hrt_mem.cpp: the device memory a context keeps between builds.
#pragma once
#include "../../include/hrt.h"
#include "bvh8.h"
#include "bvh8_geom.h"
#include "device_types.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <vector>


namespace hrt {

// An object-space tree of a BLAS on the device, as a two-level TLAS copies it in: topology in packed 80 / 48 byte records, stored breadth
// first (nodes of level l: [level_begin[l], level_begin[l + 1])).  d_clip: a tree with spatial splits has the box of every record's part of
// its primitive (6 floats per record: what the pack's refit takes instead of the primitive's own box); NULL otherwise.  Written once, under
// Blas::tmpl_mu, and not changed afterwards -- hrt_blas_update_triangles drops it whole (the next build that wants it makes a new one); the
// BLAS owns the three blocks (hipMalloc).
struct BlasTree {
    unsigned char *d_nodes = nullptr, *d_prims = nullptr; float *d_clip = nullptr;
    uint32_t n_nodes = 0, n_records = 0, n_triangles = 0, n_spheres = 0, max_depth = 0;
    std::vector<uint32_t> level_begin;
};

struct Blas {
    uint32_t kind = kPrimKindTriangle;
    uint32_t n_prims = 0;
    // host copies of the geometry: only filled when the HOST builder is asked for (HRT_BUILD=host), from d_verts
    std::vector<float> verts;        // triangles: 9 floats each (object space)
    std::vector<float> centers;      // spheres: 3 floats each
    std::vector<float> radii;
    bool host_geometry = false;
    float *d_verts = nullptr;        // device copy of the geometry (triangles: 9 floats each; spheres: {cx, cy, cz, r}): the device
                                     // build and every refit derive the world-space records from it
                                     // (the caller may free its vertex buffer after the build, RendererMesh.cu:116)
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};   // object-space bounds
    uint64_t geometry_epoch = 0;     // bumped by hrt_blas_update_triangles / _spheres: a TLAS whose Tlas::blas_epoch differs still holds the geometry as it was
    // object-space BVH8 of this geometry alone: the per-instance subtree of the trees over instances (built on first use)
    std::mutex tmpl_mu; bool tmpl_built = false; Bvh8 tmpl;
    BlasTree tmpl_dev;               // ... and its device copy: what a two-level TLAS copies in behind its top level
    float bsphere[4] = {0, 0, 0, -1.0f}; bool bsphere_ready = false;      // bounding sphere (centre of the box, largest vertex distance): the instances' tight bound
    // A SECOND object-space tree, with spatial splits: what the two-level trees of a HRT_CTX_FAST_TRACE context copy in instead of `tmpl` (the
    // geometry moves relative to these boxes only in hrt_blas_update_triangles, which drops the tree with its clip boxes).  Device only.
    // Built once per geometry (tmpl_mu) and shared by every TLAS that instances the BLAS; `tmpl` stays what it is.
    BlasTree split;
    bool split_decided = false;      // `split` is there, or this BLAS is known to go without (4096 primitives or fewer; the top-down phase gave up)
    ~Blas() {
        if (d_verts) (void)hipFree(d_verts);
        for (BlasTree *t : {&tmpl_dev, &split}) for (void *p : {(void *)t->d_nodes, (void *)t->d_prims, (void *)t->d_clip}) if (p) (void)hipFree(p);
    }
};

// The device memory of a TLAS: every member is a block from the context's pool (pool_alloc) and nothing else, so that free_tlas_device
// can hand them all back by walking the struct and reset them by value.  A new table is declared here and nowhere else.
struct TlasDevice {
    void *d_nodes = nullptr, *d_prims = nullptr;
    float *d_inst_inv = nullptr;
    uint32_t *d_inst_identity = nullptr;
    // refit (hrt_tlas_update): the device tables the refit kernel reads
    float *d_node_box = nullptr, *d_node_ref = nullptr;
    uint32_t *d_order = nullptr;                         // trees over instances: refit order (NULL: breadth-first index ranges)
    float *d_inst_xf = nullptr, *d_area = nullptr;
    const void **d_inst_src = nullptr;
    uint32_t *d_inst_first = nullptr, *d_inst_kind = nullptr;   // device build: global number of each instance's first primitive; geometry kind
    uint32_t *d_inst_root = nullptr;                     // two-level trees, per instance: node index of its BLAS's root
    float *d_blas_bound = nullptr;                       // two-level trees, per instance, 10 floats: its BLAS's object-space box and bounding sphere (the top level's "geometry")
    // asynchronous updates (HRT_CTX_ASYNC_UPDATE): what the tree was built with, for the device-side tables kernel, and its verdict
    unsigned long long *d_sig_handle = nullptr; uint32_t *d_sig_visibility = nullptr, *d_sig_sbt = nullptr; float *d_blas_box = nullptr;
    uint32_t *d_update_flags = nullptr;                  // [0] scene scale (float bits), [1] bit 0: handle / visibility changed, bit 1: an sbtOffset changed
    float *d_rec_box = nullptr;                          // small trees: 6 floats per record, the refit's per-record pass (refit.hip k_refit_records)
    // two-level trees, for the refit of a BLAS's subtree after hrt_blas_update_triangles (the pack's refit of build_two_level): per unique
    // BLAS the object -> "world" (identity), identity flag and geometry source; per BLAS node the walk order (Tlas::pack has the phases)
    float *d_pack_xf = nullptr; uint32_t *d_pack_identity = nullptr; const void **d_pack_src = nullptr; uint32_t *d_pack_order = nullptr;
    uint32_t *d_leaf_parent = nullptr;                   // one-level trees of triangles: per record, the node whose leaf slot covers it (ensure_leaf_parent: made at the first launch that wants
                                                         // it; a refit keeps topology and record order, hence the table; a rebuild is a new Tlas and starts without one)
    // a flattened tree that keeps its spatial splits through updates (HRT_CTX_KEEP_SPLITS; Tlas::keeps_splits): per record the as-built world
    // clip box and the barycentric ranges of its part of its triangle (6 floats each), per instance the build's transform (12 floats) and the
    // word "changed since the build" (RefitArgs::inst_changed)
    float *d_keep_clip = nullptr, *d_keep_bary = nullptr, *d_build_xf = nullptr; uint32_t *d_inst_changed = nullptr;
};
static_assert(std::is_standard_layout<TlasDevice>::value && std::is_trivially_copyable<TlasDevice>::value && sizeof(TlasDevice) % sizeof(void *) == 0,
              "TlasDevice holds pool blocks only: free_tlas_device walks it as an array of pointers");

// One unique BLAS of a two-level tree: its subtree's records and, as ranges of TlasDevice::d_pack_order, its levels from the bottom up.
struct PackSlice {
    const Blas *blas = nullptr;             // (kept alive by Tlas::blas_refs)
    uint32_t n_records = 0; bool split = false;      // split: the subtree is the BLAS's tree with spatial splits (its clip boxes are not kept: a changed geometry rebuilds)
    std::vector<std::pair<uint32_t, uint32_t>> phases;
};

struct Tlas {
    uint32_t n_instances = 0;
    std::vector<uint32_t> sbt_offset;      // per instance
    std::vector<uint32_t> kind;            // per instance: triangle / sphere BLAS
    Bvh8 bvh;                               // host copy of a HOST-built tree (empty for device builds)
    uint32_t n_nodes = 0, n_prims = 0, n_triangles = 0, n_spheres = 0, max_depth = 0;
    float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    TlasDevice dev;                         // nodes, records and every per-instance table on the device
    bool has_spheres = false;
    uint32_t node_stride = 80, prim_stride = 48;
    uint64_t alloc_bytes = 0;               // device memory of nodes + node boxes / reference areas + records, as allocated
    uint64_t generation = 0;
    // refit (hrt_tlas_update): what must stay the same (the device tables the refit kernel reads: TlasDevice)
    std::vector<std::shared_ptr<Blas>> blas_refs;       // keeps the source geometry alive
    std::vector<uint64_t> sig_handle; std::vector<uint32_t> sig_visibility;
    std::vector<uint64_t> blas_epoch;                   // per instance: Blas::geometry_epoch the tree was last built or refitted for
    std::vector<float> h_blas_box, h_blas_bound;        // host copies of d_blas_box (made when a geometry has changed) / d_blas_bound (two-level trees: kept since the build)
    std::vector<PackSlice> pack;                        // two-level trees: per unique BLAS
    std::vector<float> h_xf, h_inv; std::vector<uint32_t> h_ident;   // staging of the per-instance uploads
    // asynchronous updates (HRT_CTX_ASYNC_UPDATE)
    bool built_posed = false;                           // built by an update, for the poses of that frame (not the reference's identity-posed load-time build): asynchronous updates may follow at once
    bool async_words_ready = false;                      // d_update_flags / d_area are in their initial state (the asynchronous update's epilogue leaves them so)
    uint32_t *h_update_flags = nullptr;                  // pinned: [0..1] copy of the above after the last update, [2..3] their initial values
    std::vector<std::pair<uint32_t, uint32_t>> phases;   // (first, count) in processing order, children before parents
    bool instanced = false;
    // TWO-LEVEL tree (bvh8.h: transform nodes; the reference's IAS over shared GASes): nodes [0, n_top_nodes) are the top level -- box nodes and
    // one transform node per visible instance, what an update refits --, behind them one object-space tree per UNIQUE BLAS; d_prims holds those
    // trees' records only.  Memory and update cost: instances + unique primitives.
    bool two_level = false; uint32_t n_top_nodes = 0, n_unique_blas = 0;
    bool scene_of_bodies = false;        // at least 4 visible instances of fewer than 20 000 primitives each on average (the reference's kind of scene)
    float built_reach = 1.0f;                            // the largest object-space |coordinate| a ray origin was assumed to have when the BLAS trees were padded
    bool has_split_refs = false;                         // a FLATTENED tree built with spatial splits (HRT_CTX_FAST_TRACE): a refit would recompute the leaf boxes from whole primitives, so the first update rebuilds instead
                                                         // (never a two-level tree: its updates do not touch the BLAS trees, split or not)
    bool keeps_splits = false;                           // ... built under HRT_CTX_KEEP_SPLITS: the tree has the tables (TlasDevice::d_keep_*) with which a refit keeps the split references' boxes, and is
                                                         // refitted like any other; a rebuild inside an update is a split build again
    uint32_t build_dropped = 0;                          // merged device builds: non-finite primitives the build left out
    std::vector<float> h_build_xf; std::vector<uint32_t> h_inst_changed;      // keeps_splits: host copies of d_build_xf / d_inst_changed (synchronous updates fill bit 0 here)
    bool fast_trace = false;                             // what hrt_tlas_build was asked for: a rebuild inside hrt_tlas_update of a two-level tree asks for the same (the BLASes' split trees are reused)
    float *h_area = nullptr;                             // pinned: area sum of the last refit
    hipEvent_t area_ready = nullptr; bool area_pending = false;
    uint64_t refits = 0, rebuilds = 0, refits_since_build = 0;
};

// per-depth counters, zeroed once per sample: bin sizes + 8 slice counters on 128-byte lines of their own
struct StageCounters { uint32_t bin_count[32]; uint32_t fetch[8 * 32]; };
static_assert(sizeof(StageCounters) == 128 + 8 * 128, "stage counters layout");

struct DeviceStats {
    uint64_t rays_closest, rays_any, nodes_closest, prims_closest, nodes_any, prims_any; uint64_t debug[4]; uint64_t tail[8];
    uint64_t paths;      // samples taken by hrt_render_accumulate launches with a count map: known on the device only (HrtStats.paths adds it to the host's count)
    uint64_t wave_clock[60];      // instrumented build only (trav_common.h: LaneStats::report, which addresses it as word 19 of this structure)
};
static_assert(offsetof(DeviceStats, wave_clock) == 19 * sizeof(uint64_t), "LaneStats::report writes the waves' clocks behind `paths`");

// Everything one sample needs besides the per-pixel state.  Two sets (sample parity): the stages of
// two consecutive samples overlap in time (hrt_render_launch), never more.
struct SampleSet {
    RayRec *rays[2] = {nullptr, nullptr};  // depth d reads rays[(d-1)&1], shade writes rays[d&1]
    float4 *hit_tuvp = nullptr; uint32_t *hit_inst = nullptr;
    uint32_t *bin_items = nullptr;          // kNumBins x n ray indices
    uint32_t *chain = nullptr;              // 4 instance indices per tile pixel
    float4 *result = nullptr;               // the sample's linear radiance per tile pixel
    StageCounters *stages = nullptr;        // [sub-tile][kRayTraceDepth + 1]
};
struct Workspace {
    uint32_t capacity = 0, rows_capacity = 0;
    SampleSet set[2];
    float4 *accum = nullptr;
    uint32_t *rows = nullptr;
    uint32_t *slice_cost = nullptr, *slice_order = nullptr; uint32_t slice_capacity = 0;   // fused mode: cost-ordered slices
    uint32_t *block_progress = nullptr; uint32_t block_capacity = 0;                         // fused mode, sample blocks: per slice, the blocks its pixels have ended
    float4 *primary_cache = nullptr; uint32_t primary_cache_lanes = 0;                     // HRT_CTX_REUSE_PRIMARY: two float4 per lane of the path kernel's grid
};

// the denoiser's working memory (hrt_denoise.cpp), grown on demand: the guide pass's rays and hit records, the guides of hrt_denoise_launch,
// the filter's two ping-pong frames, the variance-guided filter's two variance frames
struct DenoiseWork {
    uint32_t capacity = 0;                  // pixels each of the per-pixel arrays below holds
    RayRec *rays = nullptr; float4 *tuvp = nullptr; uint32_t *inst = nullptr;
    uint4 *guides = nullptr;
    float4 *frame[2] = {nullptr, nullptr};
    float *var[2] = {nullptr, nullptr};
    uint32_t *fetch = nullptr;              // 8 x 32 slice counters of the traversal
    const float4 *hit_tuvp = nullptr; const uint32_t *hit_inst = nullptr;      // the hit records the last guide pass took: tuvp / inst (traced) or the context's primary capture
};

// HRT_CTX_CAPTURE_PRIMARY: every pixel's primary hit as the path kernel of the last hrt_render_launch found it (k_path_capture), in frame
// order and hrt_trace_rays' form, and what it is the hit of.  The denoiser's guide pass takes it instead of tracing when its call asks
// for exactly that (capture_matches); hrt_primary_hits_get hands it out.
struct PrimaryCapture {
    float4 *tuvp = nullptr; uint32_t *inst = nullptr; uint32_t capacity = 0;      // pixels the two arrays hold
    bool valid = false;                     // a launch that captured covered every row of the frame, and nothing has changed since
    uint64_t tlas = 0, generation = 0;      // the tree: handle and Tlas::generation (updates of the handle clear `valid` themselves: a refit keeps the generation)
    uint32_t width = 0, height = 0;
    unsigned char camera[48];               // cameraCenter, U, V, W as the launch had them, compared bitwise
    const void *states = nullptr;           // the launch's RNG states: hrt_rng_free of them ends the frame the capture is of
};

// the temporal mode's history (hrt_denoise.cpp): two sets, the last call's and the one this call writes, swapped per call; each holds the
// accumulated colour, the history length, the guides and (instance, primitive) of every pixel, the object -> world table and the camera
struct DenoiseHistorySet {
    float4 *accum = nullptr; float *length = nullptr; uint4 *guides = nullptr; uint2 *id = nullptr;
    float2 *moments = nullptr;              // the variance-guided mode's (m1, m2), allocated by its first call
    float *xf = nullptr; uint32_t xf_capacity = 0;      // instances the table holds: each set's own, so that a call on a TLAS of another
                                                        // instance count (a linked one) grows the set it writes and keeps the last call's
    float center[3], U[3], V[3], W[3];
};
struct DenoiseHistory {
    uint32_t pixels = 0;                    // pixels of every per-pixel array
    DenoiseHistorySet set[2];
    float2 *motion = nullptr;               // the last call's (x', y')
    uint32_t cur = 0;                       // set[cur] is the last call's; a call writes set[cur ^ 1], then flips cur
    bool valid = false;                     // a history to blend with exists
    bool called = false;                    // the intermediates of a call exist (hrt_debug_denoise_temporal_state)
    enum Mode : uint32_t { kNone = 0, kTemporal, kVariance };
    Mode mode = kNone;                      // whose history it is: a call of the other mode starts afresh
    float *variance = nullptr;              // the variance-guided mode: what k_denoise_variance wrote and the filter took
    bool variance_called = false;           // hrt_debug_denoise_variance_state: set[variance_set].moments and `variance` are a call's
    uint32_t variance_set = 0;
    uint64_t tlas = 0; uint32_t width = 0, height = 0, n_instances = 0;     // what it was made for
    // hrt_denoise_temporal_rebind: one pending link from the history's TLAS to link_tlas.  link[i], i < link_n, is the index instance i
    // of link_tlas had in the history's TLAS, or HRT_NO_INSTANCE.  The next temporal / variance call takes it if it is on link_tlas (and
    // in the history's mode and frame size); that call, any other one, a reset, hrt_tlas_destroy of link_tlas or another rebind ends it.
    uint32_t *link = nullptr; uint32_t link_capacity = 0;      // device table, grown on demand
    std::vector<uint32_t> h_link;                               // its staging
    bool link_pending = false; uint64_t link_tlas = 0; uint32_t link_n = 0;
    // hrt_denoise_temporal_rebind_geometry: next to `link`, per instance of link_tlas the device vertices (Blas::d_verts) of the BLAS its
    // predecessor had where the instance is linked by primitive, NULL elsewhere.  link_blas owns those BLASes from the rebind until the
    // link is consumed, replaced or dropped (drop_link), so that hrt_blas_destroy / hrt_tlas_destroy of the old file's objects in
    // between is harmless.  Releasing the last reference runs ~Blas, whose hipFree waits for the device: the kernel that read the
    // vertices has finished by then.  link_by_prim: entries linked by primitive (0: the call runs k_denoise_temporal_linked).
    const float **link_verts = nullptr; uint32_t link_verts_capacity = 0;
    std::vector<const float *> h_link_verts;
    std::vector<std::shared_ptr<Blas>> link_blas;
    uint32_t link_by_prim = 0;
    void drop_link() { link_pending = false; link_by_prim = 0; link_blas.clear(); }
};

struct TimedSpan { int kind; hipEvent_t a, b; };

// working memory of the device builds, kept by the context between builds (a few arenas: builds may run on several loader threads)
struct ScratchArena { void *p = nullptr; size_t bytes = 0; };

}  // namespace hrt

namespace hrt { extern int g_instance_table_threads; }      // host threads that derive the per-instance tables of 32768 instances and more (HRT_TABLE_THREADS)
using namespace hrt;

struct HrtContext {
    int device = 0;
    uint32_t flags = 0;
    int n_cu = 256;
    std::string error;                          // last failure of any thread (under the error lock of hrt_api.cpp); a thread asks for its own first
    std::mutex mu;
    std::unordered_map<uint64_t, std::shared_ptr<hrt::Blas>> blas;
    std::unordered_map<uint64_t, std::unique_ptr<hrt::Tlas>> tlas;
    uint64_t next_handle = 0x1000;
    std::mutex pin_mu; void *pin_stage = nullptr; size_t pin_bytes = 0;      // pinned staging for the instance array of large synchronous updates (hrt_accel.cpp download_instances)
    std::mutex scratch_mu; std::vector<hrt::ScratchArena> scratch_free;      // scratch_acquire / scratch_release (hrt_mem.cpp)
    std::mutex pool_mu; std::vector<hrt::ScratchArena> pool_free; std::unordered_map<void *, size_t> pool_live; size_t pool_bytes = 0;   // pool_alloc / pool_release: the trees' device memory
    // materials
    std::vector<HrtSbtRecord> records;
    HrtMissParams miss{{0.7f, 0.8f, 0.9f}};      // reference default, src/Global/RendererMesh.cu:262
    bool have_records = false;
    uint64_t materials_generation = 0;
    // per-launch device tables derived from (tlas, records)
    HitGroup *d_hitgroups = nullptr; uint32_t *d_inst_program = nullptr; uint32_t table_capacity = 0;
    uint64_t table_tlas = 0, table_tlas_gen = 0, table_mat_gen = ~0ull;
    bool program_present[kNumPrograms] = {false, false, false, false};
    // rng
    uint32_t *d_jump = nullptr;
    // workspace + stats
    Workspace ws;
    std::vector<uint32_t> h_slice_cost, h_slice_order;
    std::vector<uint32_t> h_rows; HrtTile rows_tile{0, 0, 0, 0, 0}; uint32_t rows_w = 0, rows_h = 0;
    DeviceStats *d_stats = nullptr;
    uint64_t paths = 0;
    uint64_t last_tlas = 0;
    std::vector<TimedSpan> spans; std::vector<hipEvent_t> event_pool; size_t events_used = 0;
    double kernel_ms[HRT_K_COUNT] = {0}; uint64_t kernel_launches[HRT_K_COUNT] = {0};
    float4 *d_linear = nullptr;
    int refill_threshold = 16;                  // round 1's kernels (k_traverse); k_fused and k_trace_queue: fused_refill_threshold
    int fused_refill_threshold = 20, fused_fetch_chunk = 16;   // measured optimum of the fused path mode (profiles/r01_sweep_fused_*.txt, r02_sweep_fused_knobs.txt, r03_sweep_fused_knobs.txt: 20 is 1 % ahead of 16)
    int traverse_blocks_per_cu = 16;            // one-wave workgroups of the wavefront traverse kernel per CU
    int fused_blocks_per_cu = 20;               // ... of the fused path kernels: round 1's takes 5 waves per SIMD (96 VGPRs), k_fused is capped at kFusedBlocksPerCu
    bool traverse_blocks_auto = true;           // fused mode: fewer of them for small tiles (not when the env knob is set)
    int postpone_pct = 25;                      // round 1's kernels (k_traverse); k_fused and k_trace_queue: fused_postpone_pct
    int fused_postpone_pct = 40;                // (r02_sweep_lanes_active.txt: same speed as 25, 65 % of the lanes active instead of 63.4 %)
    int fused_max_depth = kFusedMaxDepth;       // deeper trees take round 1's fused kernel (HRT_FUSED_MAX_DEPTH lowers it: tests)
    uint64_t fused_max_bytes = 1ull << 32;      // k_fused addresses nodes and records by 32-bit byte offsets: larger arrays take round 1's kernel (HRT_FUSED_MAX_BYTES lowers it: tests)
    bool fused_counters_clean = false;          // the path kernel's slice counters are zero (the previous launch's finalize kernel left them so)
    uint64_t fused_fallback_launches = 0;       // launches that took round 1's path kernel because the tree did not fit k_fused
    int wavefront_graph = 0;                    // wavefront mode: 1 = replay a captured pair of samples as a hipGraph; 0 (default) = enqueue every launch: the launches
                                                // are not what limits the mode (traversal is 85 % of its GPU time), profiles/r03_wavefront.txt
    uint64_t graph_replays = 0;
    int fused_tail_regen = 12;                  // k_fused, tile used up: finished rays that wait before a regeneration (HRT_TAIL_REGEN; 1/8 of C4: 142 ms with 1, 129 with 8..16)
    bool refill_auto = true;                    // HRT_REFILL_THRESHOLD not set: two-level launches regenerate at 12 waiting lanes (profiles/r04_leaf_hold.txt)
    int leaf_hold = 0;                          // HRT_LEAF_HOLD: leaf groups a lane may queue before its node work waits for primitive tests; 0 = by scene (render_fused)
    int seed_primary = 2;                       // HRT_SEED_PRIMARY: a pixel's repeat primary rays start with the culling bound at the hit its previous sample found (path_lane.h): 1 = from above, 2 = from below too (a window under the hit), 0 = off
    int leaf_quorum = 1;                        // k_fused: lanes with nothing but leaf work wait until this many of them have gathered (HRT_LEAF_QUORUM)
    int tail_split = 1;
    int node_stride = 80, prim_stride = 64;     // bytes between records in HBM (80/48 packed; 128/64 = one cache line each)
    bool node_stride_auto = true;               // no HRT_NODE_STRIDE given: trees beyond the Infinity Cache (> 3.5 M primitives) get 128-byte nodes -- a packed
                                                // 80-byte node straddles two 128-byte lines two times in five, which only costs once the lines come from HBM
                                                // (32 M triangles: +3.4 %, 8 M: +1 %, C4: -3 %; profiles/r03_large_scenes_node_stride.txt)
    int fused = 1;                              // 1: fused persistent path kernel k_fused (default), 0: wavefront kernels, -1: fused only for small tiles
    int fused_max_pixels = 700000;
    bool reuse_primary = false;                 // HRT_REUSE_PRIMARY: every launch as under HRT_CTX_REUSE_PRIMARY
    bool capture_primary = false;               // HRT_CAPTURE_PRIMARY: every launch as under HRT_CTX_CAPTURE_PRIMARY
    hrt::PrimaryCapture capture;
    uint64_t primary_capture_launches = 0;      // path-kernel launches that ran k_path_capture
    uint64_t guide_passes_traced = 0, guide_passes_captured = 0;      // the denoiser's guide passes: traced / served from the capture
    uint64_t denoise_by_primitive_links = 0;    // instances hrt_denoise_temporal_rebind_geometry has linked by primitive
    uint64_t denoise_history_rebinds = 0;       // temporal / variance calls that began from a linked history (hrt_denoise_temporal_rebind)
    int fused_lpt = 2;                          // samples of the probe launch that orders the slices by cost for the rest of the render (0: off)
    int sample_block = -1;                      // samples a lane takes of a pixel before it gives it back (-1: kSampleBlockAuto where the frame is large enough; 0: off)
    uint64_t sample_block_launches = 0;         // path-kernel launches that handed pixels out in sample blocks
    bool one_group = true;                      // HRT_ONE_GROUP: a launch in sample blocks of a one-level tree of triangles over exactly one instance runs k_path_one (fused_one.hip)
    uint64_t one_group_launches = 0;            // ... and how many did
    bool primary_restart = true;                // HRT_PRIMARY_RESTART: ... of those, the launches with the seed window (seed_primary == 2) run k_path_restart (fused_restart.hip) over the tree's leaf_parent table
    uint64_t restart_launches = 0;              // ... and how many did
    bool mask_idle = true;                      // HRT_MASK_IDLE: ... of those, k_path_idle (fused_idle.hip) instead: idle lanes off in the loop's primitive test and node step
    uint64_t mask_idle_launches = 0;            // ... and how many did
    bool primary_direct = true;                 // HRT_PRIMARY_DIRECT: ... of those, k_path_direct (fused_direct.hip) instead: repeat primary rays test their known hit's record in the regeneration
    uint64_t direct_launches = 0;               // ... and how many did
    bool miss_block = true;                     // HRT_MISS_BLOCK: k_path_direct's regeneration lets a primary ray that left the scene take the rest of its sample block (path_lane.h: path_finish)
    int taper_big = kSampleTaperBig, taper_min = kSampleTaperMin;      // HRT_SAMPLE_TAPER: what `auto` hands out -- blocks that start at taper_big samples and end on taper_min (0: uniform blocks of kSampleBlockAuto)
    bool taper_forced = false;                  // ... whatever the tile, like HRT_SAMPLE_BLOCK=N (tests)
    uint32_t last_schedule[4] = {0u, 0u, 0u, 0u};      // the last launch in sample blocks: largest block, smallest block, end of the halvings (0: uniform), passes
    int fused_max_spp = 512;                    // samples per fused launch
    int fetch_chunk = 64;
    int substream_min_pixels = 32768;
    int two_level = 0;                          // hrt_tlas_build: 1 = two-level trees (transform nodes over shared BLASes) whenever the path kernel can take them,
                                                // -1 = never, 0 = when flattening would leave the caches: more than two_level_min_prims flattened primitives,
                                                // at least two_level_min_share times the unique ones (HRT_TWO_LEVEL, HRT_CTX_TWO_LEVEL)
    uint64_t two_level_min_prims = 4000000ull; float two_level_min_share = 4.0f;
    int tlas_instanced = 0;                     // 1: hrt_tlas_build makes trees over instances too, 0: only rebuilds during updates do, -1: never
    int build_on_device = 1;                    // 1: PLOC build on the GPU (build.hip), 0: binned-SAH build on the host (HRT_BUILD=host; needs a host copy of the geometry)
    float quant_guard = 1.25f;                  // device builds (HRT_QUANT_GUARD; 0: off): see build.hip emit_item
    int build_topdown = 1;                      // device builds of more than 4096 primitives start with the top-down phase of build_split.hip (object splits; HRT_BUILD_TOPDOWN=0: PLOC alone)
    int reinsert_rounds = kReinsertRounds;      // fast-trace builds: rounds of the reinsertion pass over the finished BVH2 (HRT_REINSERT; 0: none)
    int fast_trace_on_device = 1;               // HRT_CTX_FAST_TRACE builds: 1 = on the device with spatial splits (build_split.hip), 0 = the host builder (HRT_FAST_TRACE_BUILD=device|host)
    float split_budget = 1.0f, split_alpha = 1e-5f, split_bias = 0.95f, split_cut_bias = 1.0f; int split_cell_refs = 16;      // the device's spatial splits (HRT_SBVH_BUDGET / _ALPHA / _BIAS / _CELL_REFS)
    int ploc_radius = 2;                        // device build: nearest-neighbour search radius of the PLOC rounds (positions in Morton order); 2 traces fastest
                                                // on the soup scenes (C4: 24.1 node visits per ray, 16: 28.3, 64: 36.6 -- profiles/r02_build_bench.txt)
    int build_width = 8;                        // children per node at most (HRT_BVH_WIDTH)
    float build_c_node = 1.0f, build_c_prim = 0.45f;   // collapse costs (bvh8_build.cpp has the same defaults)
    // ... and the primitive's cost for scenes of BODIES (several instances of small meshes: the reference's kind): their rays test as many primitives as they
    // visit nodes, a lane tests one primitive per iteration, and the collapse's 0.45 -- right for a soup, whose rays visit three nodes per test -- makes leaves too
    // fat: 2.0 is 10-12 % faster on 2000 particles, 5-10 % on 25, 3 % on the shipped sample's loop, 8 % on two-level trees, and 1 % SLOWER on C4
    // (profiles/r04_cprim_sweep.txt).  HRT_BVH_CPRIM sets both.
    float build_c_prim_bodies = 2.0f;
    bool build_verbose = false;                 // HRT_BUILD_VERBOSE: builds and updates report on stderr
    bool keep_splits = false;                   // HRT_CTX_KEEP_SPLITS at hrt_ctx_create, or HRT_KEEP_SPLITS=1: flattened device split builds keep their splits through updates
    int refit = 1;                              // hrt_tlas_update: 1 = device refit when only transforms changed, 0 = always rebuild
    int refit_moved_far_check = 1;              // the first update after a build rebuilds without refitting first when most instances have moved further than their size (HRT_REFIT_MOVED_FAR=0: always refit first)
    float refit_rebuild_ratio = 1.5f;           // rebuild when the refitted tree's weighted mean node area has grown by this factor
    std::atomic<uint64_t> tlas_refits{0}, tlas_rebuilds{0}; std::atomic<double> tlas_refit_ratio{1.0};   // (builds run on several loader threads)
    int substreams = 0;                         // sub-tiles rendered on their own HIP streams so that one's tail overlaps another's bulk
    std::vector<hipStream_t> sub_streams; std::vector<hipEvent_t> sub_done; hipEvent_t ev_begin = nullptr;
    hipStream_t graph_stream = nullptr; hipEvent_t ev_graph_done = nullptr;     // wavefront mode's graph capture when the caller's stream is the null stream
    hrt::DenoiseWork denoise;                   // hrt_denoise_* (hrt_denoise.cpp)
    hrt::DenoiseHistory denoise_history;        // hrt_denoise_temporal_* (hrt_denoise.cpp)
};

namespace hrt {

// formats the message into ctx->error (or the creating thread's error when ctx is NULL) and returns code
int fail(HrtContext *ctx, int code, const char *fmt, ...);
const char *create_error();
const char *last_error_of(const HrtContext *ctx);

#define HIP_TRY(ctx, expr)                                                                   \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess)                                                                \
            return fail(ctx, _e == hipErrorOutOfMemory ? HRT_ERR_OOM : HRT_ERR_HIP,          \
                        "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

// ... and for a step that has reported its own failure: pass its code on
#define RC_TRY(expr) do { const int _rc = (expr); if (_rc != HRT_OK) return _rc; } while (0)

// the TLAS that a launch's GlobalParams.handle names
inline int find_tlas(HrtContext *ctx, uint64_t handle, Tlas *&t) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    auto it = ctx->tlas.find(handle);
    if (it == ctx->tlas.end()) return fail(ctx, HRT_ERR_INVALID, "GlobalParams.handle 0x%llx is not a TLAS", (unsigned long long)handle);
    t = it->second.get();
    return HRT_OK;
}

// the capture is the primary hits of exactly this call's rays: same tree (handle and generation), frame size and camera bits
inline bool capture_matches(const HrtContext *ctx, uint64_t handle, const Tlas &t, const HrtRayGenParams *rg) {
    const PrimaryCapture &c = ctx->capture;
    static_assert(sizeof(rg->cameraCenter) == 12 && sizeof(c.camera) == 48, "four float3");
    return c.valid && c.tlas == handle && c.generation == t.generation && c.width == rg->width && c.height == rg->height &&
           std::memcmp(c.camera, &rg->cameraCenter, 12) == 0 && std::memcmp(c.camera + 12, &rg->cameraU, 12) == 0 &&
           std::memcmp(c.camera + 24, &rg->cameraV, 12) == 0 && std::memcmp(c.camera + 36, &rg->cameraW, 12) == 0;
}

constexpr int kMaxSubTiles = 8;

struct Timer {
    HrtContext *ctx; hipStream_t s; bool on; TimedSpan span{};
    Timer(HrtContext *c, hipStream_t st, int kind) : ctx(c), s(st), on((c->flags & HRT_CTX_TIMING) != 0) {
        if (!on) { ctx->kernel_launches[kind]++; return; }
        span.kind = kind; span.a = next(); span.b = next();
        (void)hipEventRecord(span.a, s);
    }
    ~Timer() { if (on) { (void)hipEventRecord(span.b, s); ctx->spans.push_back(span); } }
    hipEvent_t next() {
        if (ctx->events_used == ctx->event_pool.size()) { hipEvent_t e; (void)hipEventCreate(&e); ctx->event_pool.push_back(e); }
        return ctx->event_pool[ctx->events_used++];
    }
};

void drain_spans(HrtContext *ctx);

// hrt_api.cpp: device arrays of one capacity, grown on demand (need <= capacity: nothing happens).  Freed, nulled and the capacity cleared before
// anything is allocated, so a failed hipMalloc leaves the context consistent.  An array: its pointer and the bytes it holds per unit of capacity.
struct DeviceArray {
    void **p; size_t elem;
    template <class T> DeviceArray(T *&array, size_t bytes_per_unit = sizeof(T)) : p((void **)&array), elem(bytes_per_unit) {}
};
int grow_device_arrays(HrtContext *ctx, std::initializer_list<DeviceArray> arrays, uint32_t &capacity, uint32_t need);

// hrt_api.cpp: the launch's material tables for a TLAS, and hrt_trace_rays' traversal of rays in RayRec form (enqueued only)
int refresh_tables(HrtContext *ctx, uint64_t handle, Tlas *t, hipStream_t s);
int trace_records(HrtContext *ctx, const Tlas &t, const RayRec *rays, uint32_t n_rays, float tmin, float tmax, bool any_hit,
                  float4 *tuvp, uint32_t *inst, uint32_t *fetch, hipStream_t s);
// hrt_denoise.cpp
void free_denoise_work(HrtContext *ctx);
void free_denoise_history(HrtContext *ctx);

// hrt_mem.cpp
hrt::ScratchArena scratch_acquire(HrtContext *ctx, size_t bytes);      // {nullptr, 0} when the device is out of memory
void scratch_release(HrtContext *ctx, hrt::ScratchArena a);
hipError_t pool_alloc(HrtContext *ctx, void **p, size_t bytes);
void pool_release(HrtContext *ctx, void *p);
void pool_drain(HrtContext *ctx);
// hrt_accel.cpp
void free_tlas_device(HrtContext *ctx, Tlas &t);
void free_tlas_host(Tlas &t);
int ensure_leaf_parent(HrtContext *ctx, Tlas &t, hipStream_t s);      // Tlas::dev.d_leaf_parent, made on `s` if the tree has none yet (enqueued only)

}  // namespace hrt
