// device_types.h -- records and kernel argument blocks shared by the kernels' translation units and the host API, and the path kernels'
// launch path: the list of kernels, the choice of a launch's kernel and the admission rule.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

namespace hrt {

constexpr float    kFloatZero     = 1e-6f;    // FLOAT_ZERO_VALUE, include/Global/DeviceFunctions.cuh:18
constexpr float    kFloatInfinity = 1e16f;    // FLOAT_INFINITY_VALUE, :19
constexpr uint32_t kRayTraceDepth = 5u;       // rayTraceDepth, include/Global/Shader.cuh:8
constexpr uint32_t kMissPrim      = 0xffffffffu;

constexpr int kProgramSphereRough = 0, kProgramSphereMetal = 1, kProgramTriangleRough = 2, kProgramTriangleMetal = 3;
constexpr uint32_t kNumPrograms = 4;
constexpr uint32_t kNumBins = 1 + kNumPrograms;      // bin 0: path ends; bin 1+P: closest-hit program P

// curandStateXORWOW_t layout (48 B); only d and v[] are live for curand_uniform.
struct RngState {
    uint32_t d, v[5];
    int32_t  boxmuller_flag, boxmuller_flag_double;
    float    boxmuller_extra, _pad;
    double   boxmuller_extra_double;
};
static_assert(sizeof(RngState) == 48, "curandState is 48 bytes");

// One queued ray (32 B, two 16-byte accesses).  o.w = tile-local pixel index (bits),
// d.w = global pixel index y*W+x (bits) = RNG stream index (shader/Shader.cu:97).
struct alignas(16) RayRec { float4 o, d; };

// HitGroupParams as the shader reads it (include/Global/Shader.cuh:43-70), 32 B.
struct alignas(8) HitGroup {
    const void *ptr0;      // sphere.centers | triangles.vertexNormals
    const void *ptr1;      // sphere.radii
    float albedo[3];
    float fuzz;
};
static_assert(sizeof(HitGroup) == 32, "HitGroupParams is 32 bytes");

struct GenerateArgs {
    RayRec *rays;
    const uint32_t *rows;          // tile rows -> frame rows
    uint32_t first_pixel;          // tile-local index of rays[0] (sub-tiles)
    uint32_t n_tile_pixels, width, height;
    float center[3], U[3], V[3], W[3];
};

// one input queue of a traverse launch and where its hit records go
struct TraverseSeg {
    const RayRec *rays;            // NULL: segment unused
    const uint32_t *n_ptr;         // 4 device counters whose sum is the queue length, or NULL
    uint32_t n;                    // used when n_ptr == NULL
    uint32_t any_hit;              // 1: the rays only need hit / no hit (depth >= rayTraceDepth)
    float4 *hit_tuvp;              // t, u, v, primitive index (bits); t = tmax on miss
    uint32_t *hit_inst;            // instance index, kMissPrim on miss
    uint64_t *count_nodes, *count_prims;   // COUNT builds
};

// fused path modes (k_fused, k_traverse<..., FUSED>): what generate / shade / accumulate need, in one launch
struct PathArgs {
    const uint32_t *rows; uint32_t first_pixel, n_tile_pixels, width, height;
    uint32_t spp;                  // samples taken by THIS launch
    uint32_t continue_sum;         // 1: accum already holds the sum of earlier samples of this render
    uint32_t *slice_cost;          // probe launch: per slice of fetch_chunk pixels, the time its pixels' samples took (clock / 16); else NULL
    const uint32_t *slice_order;   // order in which the slices are handed out (most expensive first); NULL: as they lie
                                   // (k_path_restart, a block render, which has no slice order: the tree's leaf_parent table, one word per record --
                                   // put here by the restart launch, fused_restart.hip, never by the caller)
                                   // (k_path_counts, which has no slice order either: the per-pixel sample counts in frame order, or NULL; its sums, also in
                                   // frame order, ride in accum and the samples they hold in trace_inst -- put there by hrt_render_accumulate, path_lane.h: kCounts)
    float center[3], U[3], V[3], W[3], bg[3];
    uint32_t block_min;            // sample blocks, tapered: the smallest block (below; in what was padding: the offsets of everything else are as before)
    RngState *states;
    const HitGroup *hitgroups; const uint32_t *inst_program;
    float4 *accum;                 // per tile pixel: sum of the samples' linear radiance
    uint64_t *rays_closest, *rays_any;
    const RayRec *trace_rays;      // fused kernel as hrt_trace_rays: the "pixels" are these rays, traced once; results below (else NULL)
    float4 *trace_tuvp; uint32_t *trace_inst; uint32_t trace_any;
                                   // (trace_any in a launch of k_path_direct, a block render, which has no callers' rays: HRT_MISS_BLOCK, path_lane.h: path_finish)
    uint32_t block_taper_end;      // sample blocks, tapered: the sample at which the halving blocks end (below; in what was padding)
    float4 *primary_cache;         // k_fused<.., REUSE>: two float4 per lane of the grid, the primary hit of the lane's pixel (else NULL)
    // sample blocks (path_lane.h; k_fused's one-level instantiations without REUSE): 0 = a lane keeps its pixel for all samples of the launch
    // The launch's samples are cut into blocks by a schedule (block_first, block_ends below), one of two kinds:
    //   uniform   block_magic != 0: blocks of K = sample_block samples, any K >= 1 (HRT_SAMPLE_BLOCK=N)
    //   tapered   block_magic == 0: powers of two that never grow -- blocks of sample_block = K_big up to T = block_taper_end - K_big (a
    //             multiple of K_big), then K_big / 2, K_big / 4, ... block_min, block_min, which end at block_taper_end, then block_min
    //             for as long as the launch lasts (HRT_SAMPLE_TAPER); the launch's last block is cut short where its samples end
    uint32_t sample_block;         // K, K_big: samples a lane takes of a pixel before it gives it back
    uint32_t block_magic;          // min(2^32 / K, 2^32 - 1): path_finish's test for a multiple of K (0: tapered, or K = 0)
    uint32_t block_slices;         // slices of the tile
    uint32_t block_slices_magic, block_chunk_magic;   // min(2^32 / d, 2^32 - 1) for d = block_slices, fetch_chunk (path_lane.h: div_magic)
    uint32_t block_items;          // passes x slices: what the slice counters hand out (x fetch_chunk below 2^32)
    uint32_t *block_progress;      // per slice: blocks ended by its pixels, zeroed before the launch
};

static_assert(sizeof(PathArgs) == 232 && offsetof(PathArgs, states) == 112 && offsetof(PathArgs, primary_cache) == 192 && offsetof(PathArgs, block_progress) == 224,
              "block_min and block_taper_end sit in what was padding: nothing else has moved");

// The block schedule in closed form, for the kernel (path_lane.h) and the host (path_plan.h: sample_schedule) alike.
// block_first: the first sample of pass b.
__host__ __device__ inline uint32_t block_first(uint32_t k_big, uint32_t k_min, uint32_t taper_end, bool tapered, uint32_t pass) {
    if (!tapered) return pass * k_big;
    const uint32_t log_big = (uint32_t)__builtin_ctz(k_big), n_big = (taper_end - k_big) >> log_big;      // passes of K_big in front of the halvings
    if (pass <= n_big) return pass << log_big;
    const uint32_t j = pass - n_big, halvings = log_big - (uint32_t)__builtin_ctz(k_min);
    const uint32_t h = j < halvings ? j : halvings;                          // pass n_big + j starts where K_big >> j samples are left of the window ...
    return taper_end - (k_big >> h) + (j - h) * k_min;                       // ... and K_min later for every pass after the last halving
}
// block_ends: a tapered schedule has a boundary at sample p >= 1.  With q = taper_end - p: a multiple of K_big in front of the window
// (q >= K_big), a power of two that is at least K_min, or 0, inside it, a multiple of K_min behind it (q < 0) -- that is, q has no bit in
// common with min(q - 1, K_big - 1) | (K_min - 1), behind the window q modulo K_min.  All three K = 0 (no blocks): never.
__host__ __device__ inline bool block_ends(uint32_t k_big, uint32_t k_min, uint32_t taper_end, uint32_t p) {
    uint32_t q = taper_end - p;
    if ((int32_t)q < 0) q &= k_min - 1u;
    const uint32_t below = q - 1u < k_big - 1u ? q - 1u : k_big - 1u;
    return (q & (below | (k_min - 1u))) == 0u;
}
// hold_ends: a lane that has taken sample p - 1 of its pixel gives the pixel back -- the launch's `spp` samples are taken, or the schedule
// (magic != 0: uniform blocks of k_big, magic = min(2^32 / k_big, 2^32 - 1); else tapered) has a boundary at p.  path_finish's test
// (path_lane.h), word for word, as a function: k_path_direct's miss block steps through a block's samples with it, and
// hrt_sample_schedule holds it to the passes of every schedule it makes.
__host__ __device__ inline bool hold_ends(uint32_t spp, uint32_t k_big, uint32_t magic, uint32_t k_min, uint32_t taper_end, uint32_t p) {
    bool ends = p >= spp;
    if (magic != 0u) {
        const uint32_t rem = p - (uint32_t)(((uint64_t)p * magic) >> 32) * k_big;
        ends = ends || rem == 0u || rem == k_big;
    } else {
        ends = ends || block_ends(k_big, k_min, taper_end, p);
    }
    return ends;
}

struct TraverseArgs {
    const void *nodes;             // Bvh8Node[]
    const void *prims;             // PrimRecord[]
    uint32_t node_stride, prim_stride;   // bytes between consecutive records (80 / 48 when packed)
    TraverseSeg seg[2];
    uint32_t *fetch_counter;       // 8 slice counters on 128-byte lines, zeroed before the launch
    const float *inst_inv;         // 12 floats per instance: world->object (spheres)
    const uint32_t *inst_identity;
    float tmin, tmax;
    int refill_threshold;          // refill when at least this many lanes are idle
    uint32_t fetch_chunk;          // rays per slice a wave takes from the queue
    int tail_split;                // split long rays across idle lanes once the queue is drained
    int postpone_pct;              // the leaf pass is skipped while fewer than this % of the alive lanes have leaf work and none needs it
    int leaf_quorum;               // k_fused: ... and fewer than this many lanes have nothing but leaf work (they wait; >= 1)
    int leaf_hold;                 // k_fused: a lane with this many leaf groups queued takes no new node until some are tested (2 .. 4 = the leaf stack's depth)
    int tail_regen;                // k_fused, tile used up: regenerate once this many finished rays wait (>= 1)
    int seed_primary;              // k_fused / k_path_blocks: a pixel's repeat primary rays start bounded at its known hit -- 1 = from above, 2 = and in a window under it (fused_body.h: s_seed, kSeedWindow)
    PathArgs path;                 // FUSED only
};

struct BinArgs {
    const uint32_t *n_rays_ptr; uint32_t n_rays;
    const uint32_t *hit_inst;
    const uint32_t *inst_program;
    uint32_t depth;
    uint32_t *bin_count;           // kNumBins counters of this stage (zeroed)
    uint32_t *bin_items;           // kNumBins arrays of bin_stride ray indices
    uint32_t bin_stride;
    uint64_t *total_rays;
};

struct ShadeArgs {
    const uint32_t *bin_count; const uint32_t *bin_items; uint32_t bin_stride;
    const RayRec *rays_in; RayRec *rays_out;
    const float4 *hit_tuvp; const uint32_t *hit_inst;
    const HitGroup *hitgroups;
    RngState *states;
    uint32_t *chain;               // 4 instance indices per tile pixel
    uint32_t depth;
};

struct AccumArgs {
    const uint32_t *bin_count; const uint32_t *bin_items;
    const RayRec *rays_in; const uint32_t *hit_inst;
    const HitGroup *hitgroups;
    const uint32_t *chain;
    float4 *result;                // per tile pixel: linear radiance of this sample
    float bg[3];
    uint32_t depth;
};

struct FinalizeArgs {
    const float4 *accum; const uint32_t *rows;
    uint32_t n_tile_pixels, width, spp;
    float4 *color, *albedo, *normal, *linear;
    uint32_t *reset_counters; uint32_t n_reset;      // when set: n_reset words (< the launch's threads) zeroed on the way
};

// one level of the bottom-up refit (refit.hip)
struct RefitArgs {
    unsigned char *nodes; uint32_t node_stride;
    unsigned char *prims; uint32_t prim_stride;
    float *node_box;               // 6 floats per node: padded bounds of everything below it
    uint32_t first_node, n_nodes;  // the phase: nodes first_node .. first_node + n_nodes (positions in `order` when it is set)
    const uint32_t *order;         // NULL: node index = position (trees stored breadth first)
    const float *inst_xf;          // 12 floats per instance: object -> world
    const uint32_t *inst_identity;
    const void *const *inst_src;   // per instance: the object-space geometry of its BLAS where the BLAS keeps it (Blas::d_verts) -- 9 floats per
                                   // triangle, {cx, cy, cz, r} per sphere (16-byte aligned) -- which every record is derived from anew; the
                                   // top level of a two-level tree: the BLAS's object-space box and bounding sphere (10 floats)
    const float *inst_inv;         // two-level trees: 12 floats per instance, world -> object (written into the transform nodes)
    const uint32_t *inst_root;     // two-level trees: per instance, the node index of its BLAS's root
    float pad;
    const uint32_t *scale_bits;    // when set: pad = 4e-6 * max(1, scene scale) with the scale read from here (float bits; written by
                                   // k_instance_tables on the same stream), instead of the host's `pad`
    float *node_ref;               // 2 floats per node: {weight, 1 / half area as built}
    uint32_t write_reference;      // 1: this refit completes a build -- record the areas instead of comparing with them
    float *area_sum;               // weighted mean of area now / area as built (quality after the refit), may be NULL
    float *rec_box; uint32_t n_records;   // when set (small trees): 6 floats per record, the record's padded box, written by k_refit_records before the levels
                                   // are walked -- the records' arithmetic then runs one thread per record instead of inside the walk up the tree
    const float *clip;             // when set (the refit that completes a device build with spatial splits, flattened or of a two-level tree's BLASes): 6 floats per
                                   // record, the box of the part of the primitive this record stands for, taken instead of the primitive's own
    // A flattened tree that keeps its spatial splits through updates (HRT_CTX_KEEP_SPLITS).  bary set: the launches take the kernels'
    // <true> instantiations, `clip` is the tree's own copy of the as-built boxes and inst_changed is set.  A record of an instance whose
    // word is 0 takes its as-built box; of any other, a triangle the box of its barycentric hexagon under the new vertices
    // (bvh8_geom.h: bary_hexagon_box) within the primitive's own, a sphere the primitive's own.
    const float *bary;             // 6 floats per record: {u0, u1, v0, v1, w0, w1} (clip_triangle_barycentric; spheres: unused)
    const uint32_t *inst_changed;  // per instance: bit 0 the transform differs from the build's, bit 1 its BLAS has had new vertices since
};
constexpr uint32_t kRefitTopLevels = 16, kRefitTopLevelNodes = 128;      // (one pass of the 1024-thread workgroup per level; wider levels are quicker as launches of their own: 95 -> ~45 us for the reference's sample)
struct RefitLevels { uint32_t n_levels; uint32_t first[kRefitTopLevels], count[kRefitTopLevels]; };   // phases in processing order, each at most kRefitTopLevelNodes wide
// two-level trees: copy of one BLAS's template tree (packed: 80-byte nodes, 48-byte records) into a TLAS's arrays
struct PackBlasArgs {
    const unsigned char *src_nodes, *src_prims; uint32_t n_nodes, n_prims;
    unsigned char *dst_nodes, *dst_prims; uint32_t node_stride, prim_stride;
    uint32_t node_off, prim_off;   // where the tree lands: index of its root in the TLAS's node array, of its first record
    uint32_t slot;                 // the BLAS's number in the tables of the pack's refit (written to the records' instance field)
    // a TLAS that holds a BLAS tree with spatial splits: the pack's refit takes every record's box from ONE array over all records (RefitArgs::clip)
    float *dst_clip;               // 6 floats per record of the TLAS (NULL: no BLAS of this TLAS has split references)
    const float *src_clip;         // this BLAS's own clip boxes; NULL: it has none, its records get their primitives' own boxes ...
    const float *src_geom;         // ... from its object-space geometry (9 floats per triangle; spheres are in their records)
};
void launch_pack_blas(const PackBlasArgs &a, hipStream_t s);
void launch_refit_level(const RefitArgs &a, hipStream_t s);
void launch_refit_records(const RefitArgs &a, hipStream_t s);
// per-instance tables of an update derived on the device from the caller's instance array (asynchronous updates)
struct InstanceTableArgs {
    const void *instances;         // HrtInstance[] (80 B each): transform[12], instanceId, sbtOffset, visibilityMask, flags, handle (u64), pad
    uint32_t n;
    const unsigned long long *sig_handle; const uint32_t *sig_visibility;   // what the tree was built with
    const uint32_t *sig_sbt;       // the sbtOffsets the material tables were derived from
    const float *blas_box;         // 6 floats per instance: object-space bounds of its BLAS (lo > hi: empty)
    float *inst_xf, *inst_inv; uint32_t *inst_identity;
    uint32_t *flags;               // [0]: scene scale (float bits, starts at 1.0f); [1]: bit 0 set when a handle or visibility bit differs (-> rebuild), bit 1 when an sbtOffset does (-> synchronous update)
    const float *build_xf; uint32_t *inst_changed;      // trees that keep their splits (RefitArgs::inst_changed), else NULL: the transforms of the build; bit 0 is set here, bit 1 kept
};
void launch_instance_tables(const InstanceTableArgs &a, hipStream_t s);
// the end of an asynchronous update, one launch instead of two copies to the host, one from it and a fill: the refit's area sum and the
// tables kernel's verdict go to pinned host memory, the device words are set up for the next update
struct UpdateEpilogueArgs { float *d_area; uint32_t *d_flags; float *h_area; uint32_t *h_flags; uint32_t flags_init0, flags_init1; };
void launch_update_epilogue(const UpdateEpilogueArgs &a, hipStream_t s);
void launch_refit_top(const RefitArgs &a, const RefitLevels &lv, hipStream_t s);
// after a flattened build with spatial splits under HRT_CTX_KEEP_SPLITS, one thread per record: a triangle record's part of its triangle -- the
// world clip box the build gave it -- as ranges of the triangle's barycentrics (bvh8_geom.h: clip_triangle_barycentric), the triangle
// taken through triangle_world from the source vertices and the build's transform, as the builder took it
struct BaryClipArgs {
    const unsigned char *prims; uint32_t prim_stride, n_records;
    const float *inst_xf; const uint32_t *inst_identity; const void *const *inst_src;
    const float *clip; float *bary;
};
void launch_bary_clip(const BaryClipArgs &a, hipStream_t s);

// particle pose update (pose.hip)
struct PoseArgs {
    void *instances;               // HrtInstance[] (80 B each, transform first)
    uint32_t first_instance, n;
    const float4 *current, *next;  // HrtParticleState[] as 3 float4 each
    float duration; uint32_t frame, frame_count;
    float offset[3], scale[3];
    uint32_t mesh_mode;            // RendererMesh's drift-only update (no rotation, position not added)
};
void launch_pose_instances(const PoseArgs &a, hipStream_t s);
void launch_debug_trig(int which, const float *a, const float *b, uint32_t first, uint32_t stride, uint64_t n, int force_slow, float *out, hipStream_t s);

// denoiser (denoise.hip): the guide pass -- primary rays of a full frame, then their hits turned into HrtDenoiseGuide records (16 B,
// uint4 here) -- and one a-trous pass of the filter, which in the variance-guided mode (DESIGN.md 3e "Variance-guided mode") carries a
// variance frame along with the colour
struct DenoiseRayArgs {
    RayRec *rays; uint32_t width, height;
    float center[3], U[3], V[3], W[3];
};
struct DenoiseGuideArgs {
    const RayRec *rays; const float4 *tuvp; const uint32_t *inst; uint32_t n;
    const HitGroup *hitgroups; const uint32_t *inst_program;
    uint4 *guides;
};
struct DenoisePassArgs {
    const float4 *src; const uint4 *guides; float4 *dst;
    uint32_t width, height, step;  // taps step pixels apart
    float k_color, k_albedo;       // 1 / sigma_color_i^2, 1 / sigma_albedo^2
    float sigma_depth_step;        // sigma_depth * step
    uint32_t normal_squarings;
    const float *var_src; float *var_dst;      // the variance-guided form (var_src == NULL: the plain one, which reads none of these)
    float k_luminance, variance_floor;         // sigma_luminance^2; k_color is not read by this form
};
// the temporal mode's reprojection and blend: one thread per pixel of the frame; prev_* are the last call's history (has_history == 0:
// none), cur_* this call's
struct DenoiseTemporalArgs {
    const RayRec *rays; const float4 *tuvp; const uint32_t *inst; const float4 *color;
    const float *inst_inv;                                   // this frame's world -> object table (Tlas::d_inst_inv)
    const float *prev_xf;                                    // the last call's object -> world table
    const float4 *prev_accum; const float *prev_length; const uint4 *prev_guides; const uint2 *prev_id;
    float4 *accum; float *length; uint2 *id; float2 *motion;
    uint32_t width, height, has_history;
    float prev_center[3], prev_U[3], prev_V[3], prev_W[3];
    float alpha_min, max_history, depth_tolerance;
    const float2 *prev_moments; float2 *moments;             // the variance-guided mode's luminance moments (moments == NULL: not carried)
};
// ... of the first call after hrt_denoise_temporal_rebind (denoise_link.hip): the history is another TLAS's, prev_index[i] the index
// instance i had there (kNoInstance: none).  The table rides behind the unlinked kernels' arguments, not among them: their kernel-argument
// segment, and with it the offsets of the hidden arguments their code reads, stays what it was.
constexpr uint32_t kNoInstance = 0xffffffffu;               // HRT_NO_INSTANCE
struct DenoiseTemporalLinkedArgs {
    DenoiseTemporalArgs t;
    const uint32_t *prev_index;
};
// ... of the first call after hrt_denoise_temporal_rebind_geometry when the link has by-primitive entries (denoise_link_prim.hip):
// prev_verts[i] is the object-space vertex array (9 floats per triangle, Blas::d_verts) of the BLAS instance i had in the history's TLAS
// where the two BLASes differ, NULL where instance i takes the rigid path or has no predecessor.  Behind the unlinked arguments too.
struct DenoiseTemporalByPrimArgs {
    DenoiseTemporalArgs t;
    const uint32_t *prev_index;
    const float *const *prev_verts;
};
// the variance-guided mode: the per-pixel variance from the moments
struct DenoiseVarianceArgs {
    const float2 *moments; const float *length; const uint2 *id; float *variance;
    uint32_t width, height;
    float history_min;                                       // L below it: the spatial estimate
};
// the accumulated mode (denoise_accum.hip; DESIGN.md 3e "Accumulated mode"): hrt_render_accumulate's sums and totals and the frame's
// guides -> the linear mean, the variance of that mean and the guides the filter takes (a pixel without a sample: background)
struct DenoiseAccumArgs {
    const float4 *sum; const uint32_t *taken; const uint4 *guides;
    float4 *mean; float *variance; uint4 *guides_out;        // (guides_out is not guides: a young pixel's taps read their neighbours' depths)
    uint32_t width, height;
    uint32_t believed;                                       // max(history_min, 2): a hit with fewer samples takes the 5x5 estimate
};
void launch_denoise_accumulated(const DenoiseAccumArgs &a, hipStream_t s);     // denoise_accum.hip
void launch_denoise_variance(const DenoiseVarianceArgs &a, hipStream_t s);
void launch_denoise_temporal(const DenoiseTemporalArgs &a, hipStream_t s);
void launch_denoise_temporal_linked(const DenoiseTemporalLinkedArgs &a, hipStream_t s);      // denoise_link.hip
void launch_denoise_temporal_by_prim(const DenoiseTemporalByPrimArgs &a, hipStream_t s);     // denoise_link_prim.hip
void launch_denoise_rays(const DenoiseRayArgs &a, hipStream_t s);
void launch_denoise_guides(const DenoiseGuideArgs &a, hipStream_t s);
void launch_denoise_pass(const DenoisePassArgs &a, hipStream_t s);

// host-callable launchers (defined in kernels.hip)
void launch_rng_init(RngState *states, uint32_t n, uint64_t salt, const uint32_t *d_jump, hipStream_t s);
void launch_generate(const GenerateArgs &a, hipStream_t s);
void launch_traverse(const TraverseArgs &a, bool count, bool has_spheres, uint32_t grid_blocks, hipStream_t s);
constexpr int kSampleBlockAuto = 32;   // HRT_SAMPLE_BLOCK=auto with HRT_SAMPLE_TAPER=0: samples per block (profiles/r13_sample_blocks.txt); with a taper: `auto` wants 2 x this many samples in a launch
constexpr int kSampleTaperBig = 64, kSampleTaperMin = 8;   // HRT_SAMPLE_TAPER: the largest and the smallest block of the tapered schedule (profiles/r19_sample_taper.txt)
constexpr int kFusedBlocksPerCu = 16;  // k_fused is compiled for 4 waves per SIMD (125 VGPRs, nothing spilled): more workgroups per CU would only queue
constexpr int kFusedInstancedBlocksPerCu = 12;   // k_fused<.., INSTANCED> is compiled for 3 waves per SIMD (fused.hip)
constexpr uint32_t kFetchShards = 8;         // slice counters (one per XCD-group of blocks)
constexpr uint32_t kFetchShardStride = 32;   // u32s between counters: one 128-byte line each
constexpr int kFusedMaxDepth = 12;     // deepest tree (levels below the root) k_fused takes: its per-lane node stack in LDS (trav_lean.h: kNodeStackLds)
constexpr uint32_t kTraversalStackEntries = 64;   // per-lane stack of round 1's kernels, which take what k_fused cannot (trav_common.h: kLdsStack + kSpillStack); a tree of
                                                  // depth d needs 2 d + 2 of them, and a build that comes out deeper fails (hrt_accel.cpp)
// ---- the path kernels: one launch renders every sample of every pixel of a tile (or traces callers' rays, PathArgs::trace_rays) ----
// Every kernel is an enumerator; which one a launch gets (choose_path_launch), what it takes for granted (path_launch_admitted) and the one
// entry that launches it (launch_path_kernel) follow, the first two as plain host code that tests/test_path_launch_cpu.py runs without a device.
// What a render decides before that choice -- grid, cache, probe, capture, the sample-block gate, the schedule -- is path_plan.h's, host code likewise.
enum class PathKernel {
    Fused,              // k_fused (fused.hip): one-level trees; with PathArgs::primary_cache, its primary-reuse instantiation
    FusedInstanced,     // k_fused<.., INSTANCED> (fused.hip): two-level trees (transform nodes, bvh8.h)
    Capture,            // k_path_capture (fused_capture.hip): k_fused<S, I, false> that also keeps every pixel's primary hit
    Blocks,             // k_path_blocks (fused_blocks.hip): pixels handed out in sample blocks
    OneGroup,           // k_path_one (fused_one.hip): the block render of a scene with one hit group
    Restart,            // k_path_restart (fused_restart.hip): k_path_one whose repeat primary rays start at the node of their known hit
    Round1,             // k_traverse<.., FUSED> (kernels.hip): round 1's fused kernel, for the trees k_fused cannot take
    Counts,             // k_path_counts (fused_counts.hip): k_fused<S, I, false> over a caller's sums, every pixel with a sample count of its own (hrt_render_accumulate)
    MaskIdle,           // k_path_idle (fused_idle.hip): k_path_restart whose loop switches idle lanes off for the primitive test and the node step
    Direct              // k_path_direct (fused_direct.hip): k_path_idle whose repeat primary rays test their known hit's record in the regeneration
};
struct PathScene { bool one_level; uint32_t n_instances; bool has_spheres; const uint32_t *leaf_parent; };      // what the TraverseArgs do not say about the tree (leaf_parent: below, or NULL)
// The ladder of the one-group block kernels, each the one before it plus one thing: k_path_one (1), k_path_restart (2), k_path_idle (3),
// k_path_direct (4); every other kernel 0.  A kernel takes for granted what every rung up to its own does, and a launch of it counts for each
// of them (HrtStats: one_group_launches >= restart_launches >= mask_idle_launches >= direct_launches).
inline int path_ladder_rung(PathKernel kernel) {
    switch (kernel) {
        case PathKernel::OneGroup: return 1;
        case PathKernel::Restart: return 2;
        case PathKernel::MaskIdle: return 3;
        case PathKernel::Direct: return 4;
        default: return 0;
    }
}
// What each kernel takes for granted, in one place: its regeneration does not look at the fields it is compiled without, so a launch that
// contradicts the kernel it names is refused instead of rendering something else -- and a launch in blocks that could wait for ever is
// refused instead of taking the GPU away.  Plain host code: no device, nothing launched.
inline bool path_launch_admitted(PathKernel kernel, const TraverseArgs &a, const PathScene &scene, uint32_t grid_blocks) {
    const PathArgs &p = a.path;
    auto pow2 = [](uint32_t v) { return v != 0u && (v & (v - 1u)) == 0u; };
    // the schedule is one of the two kinds PathArgs names, not a mixture: uniform blocks, or a taper of powers of two whose halvings end at or behind the first block
    const bool uniform = p.block_magic != 0u && p.block_min == 0u && p.block_taper_end == 0u;
    const bool tapered = p.block_magic == 0u && p.block_min != 0u && p.block_taper_end >= p.sample_block && pow2(p.sample_block) && pow2(p.block_min);
    // a render in sample blocks: a one-level tree, no callers' rays, no cost probe, no slice order; the hand-over's memory -- the slices' progress words, and items
    // to hand out; every slice counter some wave's home (fewer waves than counters: a held item's predecessor can sit behind a counter nobody visits, fused_body.h);
    // ... of triangles over exactly one instance, whose table entries exist
    const bool in_blocks = scene.one_level && p.sample_block != 0u && p.trace_rays == nullptr && p.slice_cost == nullptr && p.slice_order == nullptr &&
                           grid_blocks >= kFetchShards && p.block_progress != nullptr && p.block_items != 0u && (uniform || tapered);
    const bool one_group = in_blocks && scene.n_instances == 1u && !scene.has_spheres && p.hitgroups != nullptr && p.inst_program != nullptr;
    // the ladder: one hit group; from the restart on the table, and the window its rays start in (k_path_idle and k_path_direct: the same launch, the kernel alone differs)
    if (const int rung = path_ladder_rung(kernel)) return one_group && (rung < 2 || (scene.leaf_parent != nullptr && a.seed_primary >= 2));
    switch (kernel) {
        case PathKernel::Fused: return scene.one_level && p.sample_block == 0u;           // (the caller names the block kernels: nothing forwards)
        case PathKernel::FusedInstanced: return !scene.one_level && p.sample_block == 0u;
        case PathKernel::Capture: return p.sample_block == 0u && p.trace_rays == nullptr && p.primary_cache == nullptr;      // (trace_tuvp / trace_inst carry its arrays)
        case PathKernel::Blocks: return in_blocks;
        case PathKernel::Round1: return true;
        // (accum: the caller's sums, trace_inst: the samples they hold, slice_order: the counts or NULL -- so no callers' rays, no cost probe, no order)
        case PathKernel::Counts: return p.sample_block == 0u && p.trace_rays == nullptr && p.primary_cache == nullptr && p.slice_cost == nullptr &&
                                        p.accum != nullptr && p.trace_inst != nullptr && p.spp != 0u;
        default: return false;
    }
}
// The kernel of ONE launch of a render (path_plan.h: plan_fused_launch), from what is decided by then: the tree's kernel (Fused, FusedInstanced or
// Round1), whether the render captures primary hits -- of a render cut into several launches the first one does, and never one in blocks: the
// primary ray of a pixel's first sample is every sample's --, whether this launch goes in sample blocks, and how many samples earlier launches
// have taken; has_table: the tree has its leaf_parent table, or will by the time the launch runs (it has records and nodes).  A launch in blocks of a scene with ONE hit group -- a one-level tree of triangles over exactly one instance, any single-mesh
// render -- climbs the ladder as far as the knobs let it: k_path_one (HRT_ONE_GROUP=0: k_path_blocks like everything else); where its repeat
// primary rays get their window (HRT_SEED_PRIMARY=2) and the tree has its leaf_parent table, k_path_restart (HRT_PRIMARY_RESTART=0: k_path_one);
// k_path_idle (HRT_MASK_IDLE); k_path_direct (HRT_PRIMARY_DIRECT).  Decided per launch, from the tree that is launched: an update that adds an
// instance sends the next launch back to k_path_blocks.  Plain host code like the rule above, which admits whatever this returns.
struct PathKnobs { bool one_group, primary_restart, mask_idle, primary_direct; };
inline PathKernel choose_path_launch(PathKernel tree_kernel, bool capture, bool blocks, uint32_t done_spp, int seed_primary, const PathKnobs &knobs, const PathScene &scene, bool has_table) {
    if (!blocks) return capture && done_spp == 0u ? PathKernel::Capture : tree_kernel;
    if (!(knobs.one_group && scene.one_level && scene.n_instances == 1u && !scene.has_spheres)) return PathKernel::Blocks;
    if (!(knobs.primary_restart && seed_primary == 2 && has_table)) return PathKernel::OneGroup;      // (a tree without records has no table)
    return !knobs.mask_idle ? PathKernel::Restart : knobs.primary_direct ? PathKernel::Direct : PathKernel::MaskIdle;
}
// The one launch entry of the path kernels (fused.hip).  false: refused (path_launch_admitted), nothing launched.
bool launch_path_kernel(PathKernel kernel, const TraverseArgs &a, const PathScene &scene, uint32_t grid_blocks, hipStream_t s);
using PathLauncher = void(const TraverseArgs &a, const PathScene &scene, uint32_t grid_blocks, hipStream_t s);      // (its halves in the other kernels' translation units: each launches its own kernel)
PathLauncher launch_path_capture, launch_path_blocks, launch_path_one, launch_path_restart, launch_path_idle, launch_path_direct, launch_path_round1, launch_path_counts;
// leaf_parent[record] = index of the node whose leaf slot covers that record, for every record of a finished one-level tree (refit.hip; the host's
// counterpart, over a blob: hrt_host_leaf_parent).  A leaf slot's meta byte holds the unary count in bits 7..5 and the offset from the node's
// primitive base in bits 4..0 (bvh8.h); split references have a record each, so every record has exactly one slot.
struct LeafParentArgs { const unsigned char *nodes; uint32_t node_stride, n_nodes, n_records; uint32_t *leaf_parent; };
void launch_leaf_parent(const LeafParentArgs &a, hipStream_t s);
void launch_trace_queue(const TraverseArgs &a, bool has_spheres, uint32_t grid_blocks, hipStream_t s);   // k_trace_queue (fused_queue.hip): wavefront mode's traverse kernel, k_fused's traversal over ray queues
void launch_sum(float4 *accum, const float4 *result, uint32_t n, uint32_t first_sample, hipStream_t s);
void launch_bin(const BinArgs &a, uint32_t grid_blocks, hipStream_t s);
void launch_shade(const ShadeArgs &a, int program, uint32_t grid_blocks, hipStream_t s);
void launch_accumulate(const AccumArgs &a, uint32_t grid_blocks, hipStream_t s);
void launch_finalize(const FinalizeArgs &a, hipStream_t s);
// hrt_render_accumulate's finalize (sample_counts.hip): per tile pixel taken += c, colour from sum / taken where that is not 0; c = counts ?
// min(counts[p], spp) : spp as the path kernel took it.  The slice counters are zeroed as by k_finalize; with counts set the launch's samples are added to *paths.
struct FinalizeCountsArgs {
    const float4 *sum; uint32_t *taken; const uint32_t *counts; const uint32_t *rows;
    uint32_t n_tile_pixels, width, spp;
    float4 *color, *albedo, *normal, *linear;
    uint32_t *reset_counters; uint32_t n_reset;
    unsigned long long *paths;
};
void launch_finalize_counts(const FinalizeCountsArgs &a, hipStream_t s);
// hrt_sample_counts (sample_counts.hip): how many more samples each pixel of a frame takes, from its sums (include/hrt.h)
struct SampleCountArgs {
    const float4 *sum; const uint32_t *taken; uint32_t *counts;
    uint32_t width, height, radius, min_total, max_total;
    float target_sigma;
};
void launch_sample_counts(const SampleCountArgs &a, hipStream_t s);
void launch_to_rgba8(const float4 *src, uchar4 *dst, uint32_t n, hipStream_t s);
void launch_color_to_float4(const float4 *src, float4 *dst, uint32_t n, hipStream_t s);
void launch_pack_rays(const float *o, const float *d, uint32_t n, RayRec *rays, hipStream_t s);
void launch_unpack_hits(const float4 *tuvp, const uint32_t *inst, uint32_t n, float *t, float *u, float *v,
                        uint32_t *prim, uint32_t *oinst, hipStream_t s);
void launch_fill_misses(float4 *tuvp, uint32_t *inst, uint32_t n, float tmax, uint64_t *rays, hipStream_t s);

}  // namespace hrt
