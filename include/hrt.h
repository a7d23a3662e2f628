/*
 * hrt.h -- C ABI of the MI355X wavefront path tracer (libhrt.so).
 *
 * Drop-in boundary for ONE path of the reference: the per-frame ray-tracing
 * launch and the acceleration-structure calls that feed it.  Every entry point
 * names the reference call site it replaces (paths relative to the reference
 * tree).  Plain pointers and sizes only; "stream" is a hipStream_t passed as
 * void* (NULL = the null stream, which is what the reference uses).
 *
 * Conventions
 *   - every function returns HRT_OK (0) or a negative HrtStatus; the message of
 *     the last failure on a context is hrt_last_error(ctx).  (The reference
 *     logs and exit()s through its check macros, include/Global/HostFunctions.cuh:147-166;
 *     a library cannot, so the caller re-wraps.)
 *   - d_* parameters are DEVICE pointers owned by the caller, h_* are host pointers.
 *   - acceleration-structure memory is owned by the handle (reference:
 *     cleanupAccelerationStructure, src/Global/RendererImpl.cu:244-266).
 *   - *_build calls are thread-safe per context (reference builds from several
 *     loader threads, src/Global/RendererMesh.cu:93-100); hrt_render_launch is
 *     called from one thread at a time per context.
 *   - there is NO CPU fallback: without a gfx950 device every compute entry
 *     point fails with HRT_ERR_NO_DEVICE.
 */
#ifndef HRT_H
#define HRT_H

#include <stdint.h>
#include "hrt_params.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum HrtStatus {
    HRT_OK               =  0,
    HRT_ERR_INVALID      = -1,   /* bad argument                                 */
    HRT_ERR_NO_DEVICE    = -2,   /* no HIP device / wrong architecture           */
    HRT_ERR_HIP          = -3,   /* a HIP runtime call failed                    */
    HRT_ERR_OOM          = -4,
    HRT_ERR_STATE        = -5    /* call order (e.g. launch before materials_set)*/
} HrtStatus;

typedef struct HrtContext HrtContext;

/* context flags */
#define HRT_CTX_TIMING   0x1u    /* bracket every kernel with HIP events (hrt_get_stats) */
#define HRT_CTX_COUNT    0x2u    /* traverse kernel counts node visits / primitive tests */
#define HRT_CTX_ASYNC_UPDATE 0x8u /* hrt_tlas_update never reads the instance array back: the per-instance tables (object->world, its inverse, the
                                    scene scale) are derived on the device and the refit is only enqueued -- the whole Time-mode frame (pose kernel,
                                    update, launch) then runs without a host synchronisation.  The caller promises what updateIAS requires anyway
                                    (OPTIX_BUILD_OPERATION_UPDATE, RendererImpl.cu:210-242): same BLAS handles, visibility bits and sbtOffsets as
                                    at the build.  A broken promise and a tree that has degraded past the rebuild ratio are both detected on the
                                    device and acted on at the NEXT update (one frame late), which then takes the synchronous path: a changed handle /
                                    visibility bit or a degraded tree rebuilds, a changed sbtOffset refreshes the material tables.  The FIRST update
                                    after a build is synchronous in either mode (one small read-back per build): the reference builds every file's IAS
                                    with identity transforms and poses it afterwards, so that update is the one that has to rebuild. */
#define HRT_CTX_TWO_LEVEL 0x10u  /* hrt_tlas_build keeps the reference's structure, an IAS over shared GASes (RendererImpl.cu:174-206; GAS by shapeID,
                                    RendererTime.cu:116-130): a top level over the instances whose leaves are TRANSFORM NODES, one object-space tree per
                                    unique BLAS behind it -- memory, build and update cost grow with instances + unique primitives instead of
                                    instances x primitives; a ray entering an instance is transformed into its object space (csrc/bvh8.h, fused.hip).
                                    Without the flag such a tree is built when the flattened one would leave the caches (more than 4 M flattened
                                    primitives, at least 4 per unique one; HRT_TWO_LEVEL=1 / -1: always / never).  Hits of such a tree are pinned to the
                                    oracle's INSTANCED mode (object-space triangle test), those of a flattened tree to its FLATTENED mode: the two
                                    differ in rounding, not in geometry.  Trees too deep for the path kernel's stack, and contexts that count
                                    (HRT_CTX_COUNT) or run another execution mode (HRT_FUSED != 1), flatten.  Together with HRT_CTX_FAST_TRACE the
                                    shared BLAS trees are built with spatial splits (see there).  The flag asks for two levels whatever the
                                    environment says: it wins over HRT_TWO_LEVEL=-1. */
#define HRT_CTX_REUSE_PRIMARY 0x20u /* hrt_render_launch with spp > 1: the reference's raygen has no pixel jitter (shader/Shader.cu:249-261), so a pixel's
                                    primary ray hits the same thing in every sample.  With this flag (or HRT_REUSE_PRIMARY=1) the path kernel traverses it for
                                    the first sample a launch takes of the pixel and shades the later samples from that hit record: the same image bit
                                    for bit, a third fewer rays on the reference's scenes.  HrtStats.rays counts TRAVERSED rays only, so Mrays/s figures
                                    with and without the flag are not comparable -- compare times.  Off by default (all published figures are without);
                                    ignored by the other execution modes (HRT_FUSED != 1, HRT_CTX_COUNT). */
#define HRT_CTX_CAPTURE_PRIMARY 0x40u /* hrt_render_launch keeps every pixel's PRIMARY HIT -- (t, u, v, primitive, instance) of the first primary ray the path
                                    kernel traces for the pixel, hrt_trace_rays' record, a miss as (tmax, ., ., 0xffffffff) -- in the context.  The denoiser's
                                    guide pass (hrt_denoise_guides, hrt_denoise_launch, hrt_denoise_temporal_launch, hrt_denoise_variance_launch) traces exactly
                                    those rays again; while the capture is valid for its call -- same TLAS handle, no update, rebuild or destruction of it
                                    since, same frame size, the same camera bit for bit -- it takes the capture instead: the same guides and output bit for
                                    bit, one traversal of the frame less, and its rays are not counted in HrtStats.rays.  hrt_primary_hits_get hands the
                                    records out (picking, depth / id AOVs).  The image, the RNG states and the launch's ray counts are what they are
                                    without the flag.  A launch captures when it renders the whole frame (tile == NULL or every row) with the plain path
                                    kernel: not with HRT_CTX_REUSE_PRIMARY at spp > 1, sample blocks (HRT_SAMPLE_BLOCK: by themselves from 64 samples on),
                                    the cost-order probe of small tiles, round 1's path kernel, HRT_FUSED != 1 or HRT_CTX_COUNT -- renders of many
                                    samples, where one more traversal does not count; higher-spp captures are deliberately left out.  Of a render cut
                                    into several launches (HRT_FUSED_MAX_SPP) the first captures.  Every other hrt_render_launch, hrt_tlas_update /
                                    hrt_tlas_destroy of the handle, hrt_ctx_set_flags, hrt_rng_free of the launch's states and a guide pass for another
                                    frame (camera, size, tree) leave the context without a capture, and the guide pass traces as ever.  The capture is ordered like the colour buffer: enqueue the render and the
                                    denoiser on the same stream, or synchronise between them.  HRT_CAPTURE_PRIMARY=1: every context.  32 B per pixel. */
#define HRT_CTX_FAST_TRACE 0x4u  /* hrt_tlas_build prefers trace speed to build speed: the reference's OPTIX_BUILD_FLAG_PREFER_FAST_TRACE
                                    (its GAS builds, RendererImpl.cu:94,118,144).  The tree is then built WITH SPATIAL SPLITS: on the device
                                    (csrc/build_split.hip: top-down SAH splits of references level by level, PLOC within the cells that
                                    remain; 1 M triangles: ~15 ms against ~9 ms for the default build -- the same phase with object splits only,
                                    which keeps the tree refittable --, 9.5 % fewer node visits per ray,
                                    1.46 records per triangle, ~1.2 KB of working memory per triangle), or -- environment
                                    HRT_FAST_TRACE_BUILD=host -- by the host's binned-SAH builder from a host copy of the geometry (the same
                                    rules, ~1.3 s).  Such a tree is for static scenes: the first hrt_tlas_update replaces it by a
                                    default-built one (a plain refit cannot keep the split references' boxes), and rebuilds inside hrt_tlas_update
                                    are always default builds (the reference's IAS flags: ALLOW_UPDATE | PREFER_FAST_BUILD, RendererImpl.cu:180)
                                    -- unless the context also has HRT_CTX_KEEP_SPLITS (below), under which the device-built tree is refitted
                                    and keeps its splits.
                                    A split build whose tree comes out deeper than any kernel's stack (a geometric chain of primitives) is built
                                    again by position, without splits, like the default build; it used to fail with HRT_ERR_INVALID.
                                    TOGETHER WITH HRT_CTX_TWO_LEVEL (or HRT_TWO_LEVEL=1: two levels asked for, not chosen by size) -- the
                                    reference's own pairing, fast-trace GASes under an IAS it updates every frame -- hrt_tlas_build makes a
                                    two-level tree whose BLAS trees carry the splits: every BLAS of more than 4096 primitives gets a second
                                    object-space tree with spatial splits, built once on the device and shared by every TLAS that instances
                                    it (records and a 24-byte clip box each on top of the unsplit template's memory).  Geometry does not move
                                    relative to the boxes of its own object space, so such a tree is REFITTED by hrt_tlas_update like any
                                    two-level tree (the top level only) and keeps its splits for ever; a rebuild inside an update copies the
                                    cached split trees in again.  Smaller BLASes, a split phase that gives up and a split build that does not
                                    fit in memory leave that BLAS the unsplit tree, byte for byte as under HRT_CTX_TWO_LEVEL alone.  Where no
                                    two-level tree can be had -- HRT_CTX_COUNT, HRT_FUSED != 1, HRT_FAST_TRACE_BUILD=host, top + 1 + deepest
                                    BLAS levels beyond the path kernel's stack (split trees are deeper) -- the flattened split tree above is
                                    built, as with HRT_CTX_FAST_TRACE alone. */

#define HRT_CTX_KEEP_SPLITS 0x80u /* together with HRT_CTX_FAST_TRACE: the FLATTENED tree the device builds with spatial splits keeps them through
                                    hrt_tlas_update -- the reference's own configuration, PREFER_FAST_TRACE GASes under an IAS that updateIAS refits
                                    every frame.  The tree is the one built without the flag, byte for byte; it also keeps, per record, the as-built
                                    world clip box and the record's part of its triangle as ranges of the triangle's own barycentric coordinates
                                    (48 B per record in all), and per instance the build's transform.  An update then REFITS it (tlas_refits), synchronous and
                                    HRT_CTX_ASYNC_UPDATE alike: records of an instance whose transform is the build's bit for bit and whose BLAS has
                                    had no hrt_blas_update_triangles since keep their as-built boxes (an update that moves nothing leaves the tree
                                    byte-identical); a triangle record of any other instance takes the box of its barycentric hexagon under the new
                                    vertices -- an affine map preserves barycentrics, so it holds under rotation, any scale, a singular matrix and
                                    after hrt_blas_update_triangles, which such a tree follows by a refit too (unless the build left a non-finite
                                    primitive out); a sphere record of a moved instance, or of a BLAS that has had hrt_blas_update_spheres (which
                                    such a tree follows by a refit too), takes the sphere's whole box under every one of its
                                    records (correct; the limitation).  The refit stands under the usual quality verdict
                                    (HRT_REFIT_REBUILD_RATIO) and the first update's moved-far check; a rebuild inside an update -- a changed
                                    handle or visibility bit, a verdict, moved far, HRT_REFIT=0 -- is a device split build again, not a default
                                    build.  Read at hrt_ctx_create only (hrt_ctx_set_flags does not switch it); HRT_KEEP_SPLITS=1: every context.
                                    No effect on HRT_FAST_TRACE_BUILD=host trees, two-level trees (which keep their splits anyway), trees built
                                    again by position, and builds of 4096 primitives or fewer, which have no splits -- a rebuild under the flag
                                    that comes out as one of these too (the visible primitives have fallen to 4096 or fewer, the tree is too
                                    deep) leaves a tree without the tables, and from then on this TLAS is updated and rebuilt by the unflagged
                                    rules: the flag acts on the tree a TLAS has, not on the context's intent.  Off by default, and not
                                    for scenes that turn as a whole: measured with every instance moving, the kept splits trace 4-6 % slower
                                    than the default tree after a rotation and level with it after a translation; what is saved is the
                                    first update's rebuild. */

/* replaces createContext / destroyContext, src/Global/RendererImpl.cu:6-27 */
int  hrt_ctx_create(int device_id, uint32_t flags, HrtContext **out_ctx);
int  hrt_ctx_destroy(HrtContext *ctx);
int  hrt_ctx_set_flags(HrtContext *ctx, uint32_t flags);   /* switch HRT_CTX_TIMING / HRT_CTX_COUNT / HRT_CTX_REUSE_PRIMARY / HRT_CTX_CAPTURE_PRIMARY at run time; forgets the primary-hit capture */
const char *hrt_last_error(const HrtContext *ctx);        /* ctx may be NULL: creation errors */
const char *hrt_version(void);

/* replaces buildGASForTriangles / buildGASForParticle, src/Global/RendererImpl.cu:89-111,139-172.
 * d_vertices: float3, stride 12, every 3 consecutive vertices are one triangle (no index
 * buffer, as the reference).  n_vertices must be a multiple of 3.  The caller may free
 * d_vertices after the call returns (Mesh mode does, src/Global/RendererMesh.cu:116). */
int  hrt_blas_build_triangles(HrtContext *ctx, const HrtFloat3 *d_vertices, uint32_t n_vertices,
                              void *stream, HrtTraversable *out_blas);
/* replaces buildGASForSpheres, src/Global/RendererImpl.cu:113-138 */
int  hrt_blas_build_spheres(HrtContext *ctx, const HrtFloat3 *d_centers, const float *d_radii,
                            uint32_t n_spheres, void *stream, HrtTraversable *out_blas);
int  hrt_blas_destroy(HrtContext *ctx, HrtTraversable blas);
/* OPTIX_BUILD_OPERATION_UPDATE for a triangle GAS: the same triangles at new object-space positions (a deforming mesh), without a new
 * handle and without a rebuild.  `blas` is a live triangle BLAS of the context and n_vertices exactly what it was built with: triangle k
 * stays triangle k.  HRT_ERR_INVALID for an unknown handle, a sphere BLAS, another count, or NULL d_vertices with a non-zero count; a
 * refused call changes nothing.  A BLAS of zero primitives with n_vertices == 0: HRT_OK.
 * The vertices are written into the BLAS's own copy on `stream` and the object-space bounds recomputed in the same pass
 * (csrc/blas_update.hip; by the build's rule, so an updated BLAS has the bounds a BLAS built from these vertices has; non-finite
 * vertices contribute nothing and their triangles are never hit).  Like the build, the call synchronises `stream` once for the bounds'
 * read-back, and the caller may free d_vertices when it returns.  The BLAS's cached object-space trees (two-level TLASes, rebuilds
 * during updates) are dropped and built again by the next build that wants them.
 * Every TLAS that instances the BLAS is STALE until its next hrt_tlas_update, which picks the change up: a refit where the tree holds
 * every primitive of the BLAS as a record of its own -- the default flattened build, trees over instances, two-level trees with
 * unsplit BLAS trees (the BLAS's subtree is refitted in place, then the top level), synchronous and HRT_CTX_ASYNC_UPDATE alike,
 * counted in HrtStats.tlas_refits, under the same quality verdict as moved instances (the two-level subtree's own degradation is
 * not part of it) -- and a rebuild, counted in tlas_rebuilds, everywhere else: HRT_CTX_FAST_TRACE trees with split references
 * (but for the flattened tree built under HRT_CTX_KEEP_SPLITS, which refits: a triangle's barycentric ranges hold wherever it goes),
 * two-level trees in which the BLAS carries a split tree, trees built while a primitive of the BLAS was non-finite, HRT_REFIT=0.
 * Tracing or rendering a stale TLAS is well defined: its records hold world-space (two-level: object-space) vertices of their own, so
 * it sees the OLD geometry, bit for bit, until that update.  Shading normals are not the library's: they live in the caller's buffer
 * (HrtSbtRecord.data.triangles.vertexNormals), which the caller rewrites, ordered on its stream against the launches that read it.
 * The denoiser: a PENDING by-primitive link (hrt_denoise_temporal_rebind_geometry) that reads this BLAS as its old geometry is dropped,
 * as hrt_tlas_destroy drops a link; an existing history is left alone -- it reprojects the instance as if rigid, the id and depth tests
 * vet the taps: an approximation.  Not thread-safe against a concurrent build or update of a TLAS that instances the same BLAS;
 * otherwise like the build calls.  Sphere BLASes: hrt_blas_update_spheres, below. */
int  hrt_blas_update_triangles(HrtContext *ctx, HrtTraversable blas, const HrtFloat3 *d_vertices, uint32_t n_vertices, void *stream);
/* OPTIX_BUILD_OPERATION_UPDATE for a sphere GAS: the same spheres at new object-space centres and with new radii (a moving particle
 * cloud), without a new handle and without a rebuild.  `blas` is a live sphere BLAS of the context and n_spheres exactly what it was
 * built with: sphere k stays sphere k.  HRT_ERR_INVALID for a NULL context, an unknown handle, a triangle BLAS, another count, NULL
 * d_centers or d_radii with a non-zero count, or a pointer that is not aligned for a float; a refused call changes nothing.  A BLAS of
 * zero primitives with n_spheres == 0: HRT_OK.
 * The centres and radii are written into the BLAS's own copy on `stream` (the radius verbatim, sign included, as the build stores it)
 * and the object-space bounds recomputed in the same pass (csrc/blas_update.hip; by the build's rule, so an updated BLAS has the bounds
 * a BLAS built from these arrays has; a sphere with a non-finite centre or radius contributes nothing and is never hit).  Like the
 * build, the call synchronises `stream` once for the bounds' read-back, and the caller may free d_centers and d_radii when it returns.
 * The BLAS's host copy, its bounding sphere and its cached object-space trees (two-level TLASes, rebuilds during updates) are dropped
 * and made again by the next build that wants them, exactly as hrt_blas_update_triangles drops them.
 * Every TLAS that instances the BLAS is STALE until its next hrt_tlas_update, which picks the change up: a refit where the tree holds
 * every primitive of the BLAS as a record of its own -- the default flattened build, trees over instances, two-level trees with
 * unsplit BLAS trees (the BLAS's subtree is refitted in place, then the top level), synchronous and HRT_CTX_ASYNC_UPDATE alike,
 * counted in HrtStats.tlas_refits, under the same quality verdict as moved instances (the two-level subtree's own degradation is
 * not part of it) -- and a rebuild, counted in tlas_rebuilds, everywhere else: HRT_CTX_FAST_TRACE trees with split references
 * (but for the flattened tree built under HRT_CTX_KEEP_SPLITS, which refits: every record of a changed sphere takes the sphere's whole
 * box at its new place, as under a moved instance), two-level trees in which the BLAS carries a split tree, trees built while a
 * primitive of the BLAS was non-finite, HRT_REFIT=0.
 * Tracing or rendering a stale TLAS is well defined: its records hold a centre and radius of their own, so it sees the OLD spheres,
 * bit for bit, until that update.  Shading data is not the library's: HrtSbtRecord.data.sphere.centers / radii are the caller's
 * buffers, which the caller rewrites, ordered on its stream against the launches that shade with them.
 * The denoiser: sphere BLASes never link by primitive, so no pending link (hrt_denoise_temporal_rebind_geometry) can read one; an
 * existing history is left alone -- it reprojects the instance as if rigid, the id and depth tests vet the taps: an approximation.
 * Not thread-safe against a concurrent build or update of a TLAS that instances the same BLAS; otherwise like the build calls. */
int  hrt_blas_update_spheres(HrtContext *ctx, HrtTraversable blas, const HrtFloat3 *d_centers, const float *d_radii,
                             uint32_t n_spheres, void *stream);

/* replaces buildIAS / updateIAS, src/Global/RendererImpl.cu:174-242.  d_instances lives in
 * device memory (reference: cudaMemcpy H2D then build, src/Global/RendererMesh.cu:151-160).
 * hrt_tlas_build flattens the instances into one world-space BVH8, built on the device (top-down SAH object splits down to
 * cells of a few references, csrc/build_split.hip -- with spatial splits under HRT_CTX_FAST_TRACE --, then Morton sort, PLOC
 * within the cells and the optimal 8-wide collapse, csrc/build.hip; scenes of at most 4096 primitives: PLOC alone).  hrt_tlas_update takes
 * the same number of instances: when only transforms (and sbtOffsets) changed, the tree is refitted on the
 * device, asynchronously on `stream` after one small read-back of the instance array; a changed BLAS handle
 * or visibility mask, or a refitted tree whose boxes have grown too far, rebuilds it (as a tree over
 * instances, which costs milliseconds).  A BLAS may be destroyed while a TLAS still instances it. */
int  hrt_tlas_build(HrtContext *ctx, const HrtInstance *d_instances, uint32_t n_instances,
                    void *stream, HrtTraversable *out_tlas);
int  hrt_tlas_update(HrtContext *ctx, HrtTraversable tlas, const HrtInstance *d_instances,
                     uint32_t n_instances, void *stream);
int  hrt_tlas_destroy(HrtContext *ctx, HrtTraversable tlas);

/* replaces the per-frame host loop of Time mode, src/Global/RendererTime.cu:436-472: for particle i,
 * slerp(cur.quat, next.quat, factor) (:296-340) -> quatToEuler (:343-370) -> constructTransformMatrix(offset + shift,
 * rotate, scale) (include/Global/DeviceFunctions.cuh:133-148), written to d_instances[first_instance + i].transform
 * on the device -- no host loop, no H2D copy of the instance array.  Follow with hrt_tlas_update. */
int  hrt_pose_instances(HrtContext *ctx, HrtInstance *d_instances, uint32_t first_instance, uint32_t n_particles,
                        const HrtParticleState *d_current, const HrtParticleState *d_next,
                        const HrtPoseParams *h_params, void *stream);

/* replaces optixSbtRecordPackHeader as used at src/Global/RendererImpl.cu:514-560 */
int  hrt_sbt_record_pack_header(HrtProgram program, void *record_header);
/* replaces the hit-group SBT upload, src/Global/RendererMesh.cu:283-305: record i belongs
 * to the instance whose sbtOffset is i.  h_records is host memory; it is copied. */
int  hrt_materials_set(HrtContext *ctx, const HrtSbtRecord *h_records, uint32_t n_records);
/* replaces the miss record of createRaygenMissSBTRecord, src/Global/RendererImpl.cu:472-492 */
int  hrt_miss_set(HrtContext *ctx, const HrtMissParams *h_miss);

/* replaces RandomGenerator::initDeviceRandomGenerators / freeDeviceRandomGenerators,
 * src/Global/HostFunctions.cu:122-140: allocates W*H states and initialises state i with
 * curand_init(seed = i ^ seed_salt, subsequence = i, offset = 0).  seed_salt pins the
 * reference's clock64() term (quirk Q8); the kernel is bounds-checked and indexes by the
 * frame width (fixes quirk Q9). */
int  hrt_rng_init(HrtContext *ctx, uint32_t width, uint32_t height, uint64_t seed_salt,
                  void *stream, HrtRngState **out_d_states);
int  hrt_rng_free(HrtContext *ctx, HrtRngState *d_states, void *stream);

/* replaces optixLaunch(pipeline, stream, dev_params, sizeof(GlobalParams), &sbt, W, H, 1)
 * + cudaDeviceSynchronize, src/Global/RendererMesh.cu:416-419 / RendererTime.cu:497-500.
 * h_params / h_raygen are HOST copies of the two blocks the reference uploads each frame
 * (RendererMesh.cu:403-413).  spp successive samples are taken on the persistent per-pixel
 * RNG streams; the colour written is colorToFloat4(mean of the samples), which for spp = 1
 * is exactly the reference's frame.  tile == NULL renders the whole frame; rows outside the
 * tile are left untouched.  The call returns after the work has been ENQUEUED on stream;
 * hrt_sync (or any stream sync) completes it.  (Renders of >= 16 samples on small tiles synchronise
 * the stream once in the middle: a probe launch orders the pixel slices by cost for the rest.)
 * With spp > 1 the path kernels start a pixel's repeat primary rays bounded at the hit its previous sample found,
 * from above and, in a window under it, from below (HRT_SEED_PRIMARY, level 2 by default): the same image, the same
 * ray counts, fewer node steps. */
int  hrt_render_launch(HrtContext *ctx, const HrtGlobalParams *h_params,
                       const HrtRayGenParams *h_raygen, uint32_t spp,
                       const HrtTile *tile, void *stream);
int  hrt_sync(HrtContext *ctx, void *stream);
/* HRT_CTX_CAPTURE_PRIMARY: the primary hits the last hrt_render_launch captured, width * height of each in frame order, in
 * hrt_trace_rays' output form (on a miss t = tmax, the shader's FLOAT_INFINITY_VALUE 1e16, and prim = inst = 0xffffffff); a NULL pointer skips its array.
 * HRT_ERR_STATE when the context holds no valid capture (see the flag).  Enqueued only, behind the launch on the same stream. */
int  hrt_primary_hits_get(HrtContext *ctx, float *d_t, float *d_u, float *d_v, uint32_t *d_prim, uint32_t *d_inst, void *stream);

/* ---- adaptive sampling: per-pixel sample counts ----
 * hrt_render_accumulate is hrt_render_launch over sums the CALLER keeps, every pixel with a sample count of its own.
 *   d_sum, d_taken   in and out, width * height entries each in frame order (p = y * width + x).  d_sum[p].xyz is the sum of the linear
 *                    radiance of the samples pixel p has taken so far, d_sum[p].w the sum of l * l over them, l = (0.2126 r.x + 0.7152 r.y)
 *                    + 0.0722 r.z the luminance of one sample's radiance r; d_taken[p] is how many samples that is.  A frame starts with
 *                    d_taken zeroed; d_sum need not be.
 *   d_counts         frame order, may be NULL: pixel p takes c = d_counts ? min(d_counts[p], spp) : spp more samples.  spp is 1 .. 65536.
 * Per pixel of the tile: the c samples are taken in order on the pixel's RNG stream, exactly as hrt_render_launch takes them, and added to
 * the sum in that order -- where d_taken[p] is 0 on entry the first one is assigned, not added, .w included; d_taken[p] += c; the RNG state
 * is stored.  c == 0: sum, count and state are untouched and no ray is traced.  Then every tile pixel with d_taken[p] > 0 gets colorBuffer[p] =
 * colorToFloat4(sum.xyz / (float)d_taken[p]) (alpha 1; the linear debug output likewise; albedoBuffer / normalBuffer zeroed), hrt_render_launch's
 * arithmetic; a tile pixel whose d_taken[p] is still 0 keeps whatever it had.  Rows outside the tile are neither read nor written.
 * THE INVARIANT: after any sequence of these calls on a frame, pixel p's sum.xyz / taken, colour, linear output and RNG state are bit for bit
 * those of ONE hrt_render_launch(spp = d_taken[p]) from the same initial states.  The caller keeps every total below 2^24 (float sums of counts).
 * One launch of one kernel (k_path_counts): no sample blocks, no cost-order probe, no cutting into launches of HRT_FUSED_MAX_SPP;
 * HRT_CTX_REUSE_PRIMARY and HRT_CTX_CAPTURE_PRIMARY are ignored and a capture the context holds is invalidated, as by any other launch;
 * HRT_SEED_PRIMARY applies.  HrtStats.rays* count the traced rays, HrtStats.paths grows by the samples taken.
 * HRT_ERR_STATE: a context under HRT_CTX_COUNT, HRT_FUSED != 1, a tree outside k_fused's limits (HRT_FUSED_MAX_DEPTH, HRT_FUSED_MAX_BYTES), a
 * call before hrt_materials_set.  HRT_ERR_INVALID: NULL d_sum / d_taken / colorBuffer, spp out of range.  A refused call touches nothing.
 * Enqueued only. */
int  hrt_render_accumulate(HrtContext *ctx, const HrtGlobalParams *h_params, const HrtRayGenParams *h_raygen,
                           uint32_t spp, const uint32_t *d_counts,
                           HrtFloat4 *d_sum, uint32_t *d_taken,
                           const HrtTile *tile, void *stream);

/* hrt_sample_counts: from a frame's sums (above), how many MORE samples each pixel should take -- d_counts for the next hrt_render_accumulate.
 * Per pixel, in float32 without contraction, in this order: n = (float)taken; taken < 2: v = +inf (nothing known yet), else m1 = l(sum.xyz) / n,
 * m2 = sum.w / n, v = fmaxf(0, m2 - m1 * m1) (a NaN gives 0); V = the fmaxf of v over the pixels of the (2 radius + 1)^2 window that lie
 * inside the frame; x = V / (target_sigma * target_sigma); total = x >= (float)max_total ? max_total : (uint32_t)ceilf(x) (a NaN x: 0), then
 * total = max(total, min_total); d_counts[p] = total > taken ? total - taken : 0.  No global reduction: the result does not depend on the
 * launch's geometry.  NULL h_params: the defaults.  HRT_ERR_INVALID for parameters out of range; nothing is written then.  Enqueued only. */
typedef struct HrtSampleCountParams {
    float    target_sigma;   /* wanted standard deviation of a pixel's mean luminance (linear), > 0, finite   (default 0.05) */
    uint32_t min_total;      /* every pixel ends with at least this many samples in total, 1..65536           (default 1)    */
    uint32_t max_total;      /* ... and at most this many, min_total..65536                                   (default 64)   */
    uint32_t radius;         /* a pixel takes the largest variance within this many pixels, 0..2              (default 1)    */
    uint32_t reserved[2];    /* must be 0 */
} HrtSampleCountParams;
int  hrt_sample_counts_default_params(HrtSampleCountParams *out);
int  hrt_sample_counts(HrtContext *ctx, const HrtFloat4 *d_sum, const uint32_t *d_taken, uint32_t width, uint32_t height,
                       const HrtSampleCountParams *h_params, uint32_t *d_counts, void *stream);

/* replaces convertFloat4ToUchar4Kernel, src/Global/RendererImpl.cu:672-678 (second sRGB
 * encode: quirk Q7) */
int  hrt_to_rgba8(HrtContext *ctx, const HrtFloat4 *d_src, HrtUchar4 *d_dst,
                  uint32_t width, uint32_t height, void *stream);

/* colorToFloat4 (include/Global/DeviceFunctions.cuh:188-209) over n colours: the conversion raygen applies to its
 * result (shader/Shader.cu:270), as a call of its own.  Both conversions pin the shader's powf(c, 1/2.4f) as the
 * correctly rounded float of c^y, y = (double)(1.0f/2.4f) (csrc/srgb_pow.h), so the float image and the byte image are
 * bit-exact against the oracle. */
int  hrt_color_to_float4(HrtContext *ctx, const HrtFloat4 *d_src, HrtFloat4 *d_dst, uint32_t n, void *stream);

/* ---- denoiser: what stands in for denoiseOutput (src/Global/RendererImpl.cu:680-710) --------------------------------------
 * The reference hands its sRGB-encoded colour buffer to the OptiX denoiser, whose network cannot be reproduced.  In its slot:
 * an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) guided by the buffers the reference MEANT to give OptiX --
 * the depth-1 albedo and normal AOV of Shader.cu:216-227, which quirk Q3 blanks in the reference -- recomputed from one
 * primary ray per pixel into a buffer of the denoiser's own (albedoBuffer / normalBuffer stay zero).  Deterministic, defined
 * with + - * / only (DESIGN.md "Denoiser" has the definition and tests/denoise_ref.py restates it), no CPU path.
 * Non-finite colour is not removed: in a pass, a pixel with a NaN among its taps' colours (its own included, and an infinite pixel's
 * own inf - inf) has a NaN weight sum and keeps its colour unfiltered; otherwise an infinite tap turns the channels it is infinite in
 * to NaN; later passes carry this at most 2 (2^iterations - 1) pixels far.  The alpha channel is always the centre pixel's bits. */

/* one pixel's guide: the primary hit of the ray the path kernel traces first for the pixel (same origin, direction, tmin, tmax) --
 * traced by the guide pass, or, under HRT_CTX_CAPTURE_PRIMARY, taken from what the render launch itself found (the same bits) */
typedef struct HrtDenoiseGuide {
    uint16_t normal[3];            /* IEEE half, round to nearest even: normalize(normalVector) as Shader.cu:224-226 (front-face flipped) */
    uint16_t albedo[3];            /* IEEE half, round to nearest even: the hit material's albedo                                          */
    float    depth;                /* hit distance t; +inf on a miss (normal and albedo then 0).  The filter takes a pixel of depth
                                      0 < depth < +inf as a hit, every other one as background                                          */
} HrtDenoiseGuide;                 /* 16 B */

typedef struct HrtDenoiseParams {
    uint32_t iterations;           /* filter passes, 1..16; pass i takes taps 2^i pixels apart                              (default 5)    */
    float    sigma_color;          /* colour edge stop of pass 0, halved every pass: wc = 1/(1 + |c_p - c_q|^2 / sigma_i^2)  (default 0.5)  */
    float    sigma_albedo;         /* wa = 1/(1 + |a_p - a_q|^2 / sigma_albedo^2)                                            (default 0.1)  */
    float    sigma_depth;          /* wz = 1/(1 + ((z_p - z_q) / (sigma_depth * z_p * 2^i))^2)                              (default 0.02) */
    uint32_t normal_power_log2;    /* wn = max(0, n_p . n_q)^(2^k), k squarings, 0..8                                      (default 3)    */
    uint32_t reserved;             /* must be 0 */
} HrtDenoiseParams;

int  hrt_denoise_default_params(HrtDenoiseParams *out);
/* the primary-hit guides of the full frame h_raygen describes (width x height, camera; its buffers are not read or written) through
 * the TLAS h_params->handle, into d_guides (width * height records).  Needs hrt_materials_set; a two-level tree is refused under
 * HRT_CTX_COUNT (HRT_ERR_STATE), as by hrt_trace_rays.  Enqueued only. */
int  hrt_denoise_guides(HrtContext *ctx, const HrtGlobalParams *h_params, const HrtRayGenParams *h_raygen,
                        HrtDenoiseGuide *d_guides, void *stream);
/* the filter alone over caller-given guides: d_color (width * height float4) -> d_out, which may be d_color itself.
 * h_dparams == NULL: the defaults.  Enqueued only. */
int  hrt_denoise_filter(HrtContext *ctx, const HrtFloat4 *d_color, const HrtDenoiseGuide *d_guides, HrtFloat4 *d_out,
                        uint32_t width, uint32_t height, const HrtDenoiseParams *h_dparams, void *stream);
/* replaces denoiseOutput, src/Global/RendererImpl.cu:680-710: the guides of the frame (in memory the context owns) and the filter
 * of h_raygen->colorBuffer into d_out (may be the colour buffer).  Follow with hrt_to_rgba8 as the reference follows with
 * convertFloat4ToUchar4Kernel; its skipDenoise path is hrt_to_rgba8 of the colour buffer alone.  Enqueued only. */
int  hrt_denoise_launch(HrtContext *ctx, const HrtGlobalParams *h_params, const HrtRayGenParams *h_raygen,
                        const HrtDenoiseParams *h_dparams, HrtFloat4 *d_out, void *stream);

/* Temporal mode: the frames of an animation reuse the samples of the frames before them (DESIGN.md 3e "Temporal mode";
 * tests/denoise_temporal_ref.py restates it).  Each call traces the guides as hrt_denoise_launch does, reprojects every hit pixel into
 * the previous frame (through the instance's object space: this frame's world->object table, the last call's object->world table, the
 * last call's camera), blends the colour buffer into the bilinearly fetched history of the same instance and primitive at the expected
 * depth -- A = H + alpha (C - H), alpha = max(1 / L, alpha_min), L the history length, at most max_history -- and filters A as
 * hrt_denoise_launch filters the colour buffer.  A call without history (the first, after hrt_denoise_temporal_reset, or after a
 * change of frame size, of instance count, or of TLAS handle that hrt_denoise_temporal_rebind has not announced) starts it afresh
 * and returns hrt_denoise_launch's result bit for bit.  The history (about 100 B per pixel) lives in the context. */
typedef struct HrtDenoiseTemporalParams {
    float    alpha_min;            /* smallest blend weight of the current frame, 0 < alpha_min <= 1                      (default 0.8)  */
    uint32_t max_history;          /* cap of the history length L, 1..65536                                                 (default 32)   */
    float    depth_tolerance;      /* a history tap counts if |z_prev - z'| <= depth_tolerance * z', > 0                   (default 0.02) */
    uint32_t reserved;             /* must be 0 */
} HrtDenoiseTemporalParams;

int  hrt_denoise_temporal_default_params(HrtDenoiseTemporalParams *out);
/* one frame of the temporal mode into d_out (may be h_raygen->colorBuffer).  NULL parameters: the defaults.  Two-level trees and
 * counting contexts as in hrt_denoise_guides.  Enqueued only. */
int  hrt_denoise_temporal_launch(HrtContext *ctx, const HrtGlobalParams *h_params, const HrtRayGenParams *h_raygen,
                                 const HrtDenoiseParams *h_dparams, const HrtDenoiseTemporalParams *h_tparams,
                                 HrtFloat4 *d_out, void *stream);
/* forget the history (and a pending hrt_denoise_temporal_rebind): the next hrt_denoise_temporal_launch (or hrt_denoise_variance_launch)
 * starts afresh */
int  hrt_denoise_temporal_reset(HrtContext *ctx);
/* Hand the history over to another TLAS of the same scene (DESIGN.md 3e "History across TLAS handles"; tests/denoise_handoff_ref.py
 * restates it): the caller declares that next_tlas continues the scene of the TLAS the context's history was made for -- the next
 * file's IAS of a Time-mode loop (RendererTime.cu:443-447), whose instance k is the body instance k was.
 * h_prev_instance[i] (host memory, copied; n_instances entries) is the index, in the history's TLAS, of the body that is instance i of
 * next_tlas, or HRT_NO_INSTANCE for a body that was not there.  NULL: the identity over the first min(n_prev, n_next) instances, every
 * further instance new.  n_instances must be next_tlas's count; the two counts may differ; an index may appear more than once.  An
 * instance whose BLAS handle differs from its predecessor's is treated as HRT_NO_INSTANCE (another geometry's primitive ids mean
 * nothing), compared at this call: both TLASes must be alive.  A caller whose BLASes are rebuilt with the same triangles -- Mesh
 * mode's program flow, which builds a new GAS per particle and file -- declares that with hrt_denoise_temporal_rebind_geometry below.
 * The map is uploaded on `stream` (4 B per instance, kept by the context) and forms one pending link.  The next
 * hrt_denoise_temporal_launch / hrt_denoise_variance_launch takes it if it is on next_tlas, in the history's mode and frame size, and
 * the history is valid: a hit pixel of instance i with pi = map[i] reprojects by P' = X_prev(pi) (X_inv(i) P) and takes the taps
 * that hold (pi, primitive); pi == HRT_NO_INSTANCE: A = C, L = 1, no motion.  After that call the history is next_tlas's and the link
 * is gone.  hrt_tlas_update of next_tlas in between keeps the link (rebind, pose, update, launch is the normal order; instance
 * indices persist through refits and rebuilds).  The link is dropped by hrt_denoise_temporal_reset, by a temporal or variance call on
 * any other handle, frame size or mode (which starts afresh as ever), by hrt_tlas_destroy of next_tlas, and by another rebind, which
 * replaces it.  With no valid history, or the history's TLAS destroyed, the call returns HRT_OK and links nothing.  HRT_ERR_INVALID:
 * next_tlas unknown, n_instances not its count, an entry neither below the history's instance count nor HRT_NO_INSTANCE. */
#define HRT_NO_INSTANCE 0xffffffffu
int  hrt_denoise_temporal_rebind(HrtContext *ctx, HrtTraversable next_tlas, const uint32_t *h_prev_instance, uint32_t n_instances,
                                 void *stream);
/* ... across rebuilt BLASes as well (DESIGN.md 3e "History across rebuilt BLASes"; tests/denoise_by_primitive_ref.py restates it):
 * hrt_denoise_temporal_rebind in everything -- the map, NULL, the checks, the one pending link and what keeps and drops it, HRT_OK
 * with nothing linked when there is no valid history -- except for an instance i whose BLAS handle differs from its predecessor pi's.
 * If both BLASes are triangle BLASes with the same, non-zero primitive count, the instance is linked BY PRIMITIVE: the caller declares
 * that primitive k at barycentrics (u, v) of the new BLAS is the material point (k, u, v) of the old one -- a mesh uploaded again,
 * deformed, or baked at other world positions (RendererMesh.cu's GAS per particle and file), its triangles in the same order.  A hit
 * pixel of such an instance reprojects from Po = (a w + b u) + c v, w = (1 - u) - v, with a, b, c primitive k's vertices in the OLD
 * BLAS in the caller's order (u weighs the second vertex, v the third, as in the shading normal), P' = X_prev(pi) Po; this frame's
 * X_inv(i) is not used for it.  The taps, the (pi, k) id test, the depth test and the blend are the rigid path's.  A sphere BLAS on
 * either side, differing counts, or triangles against spheres: HRT_NO_INSTANCE as above.  Instances whose handle is unchanged take the
 * rigid path, and a link without a by-primitive entry is hrt_denoise_temporal_rebind's bit for bit.
 * The link keeps every old BLAS it reads alive (its device vertices, 36 B per triangle) until it is consumed, replaced or dropped:
 * hrt_blas_destroy / hrt_tlas_destroy of the old objects between this call and the launch is allowed.  Uploads 4 + 8 B per instance
 * on `stream`.  HrtStats.denoise_by_primitive_links counts the instances linked by primitive, at this call. */
int  hrt_denoise_temporal_rebind_geometry(HrtContext *ctx, HrtTraversable next_tlas, const uint32_t *h_prev_instance, uint32_t n_instances,
                                          void *stream);
/* the last hrt_denoise_temporal_launch's intermediates, width * height each (a NULL pointer skips its buffer): the accumulated colour
 * A (float4, what the filter took), the history length L (float; 0 on background), and the reprojected position (x', y') in the
 * previous frame's pixel coordinates (float2; NaN where no projection was made).  HRT_ERR_STATE before the first call.  Enqueued only. */
int  hrt_debug_denoise_temporal_state(HrtContext *ctx, HrtFloat4 *d_accum, float *d_length, float *d_motion, void *stream);

/* Variance-guided mode: the temporal mode with the filter's colour edge stop following the accumulated frame's variance (SVGF,
 * Schied et al. 2017; DESIGN.md 3e "Variance-guided mode"; tests/denoise_variance_ref.py restates it).  Next to the colour, the history
 * carries the first two moments M = (m1, m2) of the luminance l(c) = (0.2126 c.x + 0.7152 c.y) + 0.0722 c.z through the same
 * reprojection and blend (8 B per pixel and set more).  The per-pixel variance is max(0, m2 - m1^2) where the history length L has
 * reached history_min, and the variance of the moments over the 5x5 block's pixels of the same instance where it has not.  Every
 * filter pass weighs a tap's luminance difference against the 3x3-smoothed variance, 1 / (1 + dl^2 / (sigma_luminance^2 var +
 * variance_floor)), in place of the colour stop, and filters the variance as that of the weighted mean.  sigma_color is not used,
 * but is still refused (HRT_ERR_INVALID) unless it is > 0 and finite, like every other field of HrtDenoiseParams.
 * The history is the temporal mode's: a call whose predecessor was hrt_denoise_temporal_launch (or the reverse) starts afresh, as
 * after hrt_denoise_temporal_reset or a change of frame size, instance count or (without hrt_denoise_temporal_rebind) TLAS handle.  A call that starts afresh is NOT
 * hrt_denoise_launch's result: it is the definition with L = 1 on every hit pixel, so the 5x5 variance applies everywhere. */
typedef struct HrtDenoiseVarianceParams {
    float    sigma_luminance;      /* luminance edge stop in standard deviations, > 0                                       (default 4.0)  */
    uint32_t history_min;          /* 1..65536: a hit pixel with L below it takes the 5x5 variance                          (default 4)    */
                                   /* (accumulated mode: the samples a pixel needs before its own moments are believed, 2 at least)        */
    float    variance_floor;       /* added to sigma_luminance^2 var, > 0                                                   (default 1e-6) */
    uint32_t reserved;             /* must be 0 */
} HrtDenoiseVarianceParams;

int  hrt_denoise_variance_default_params(HrtDenoiseVarianceParams *out);
/* the variance-guided filter alone over caller-given colour, guides and variance (width * height floats): -> d_out (may be d_color)
 * and the filtered variance -> d_var_out (may be d_variance, or NULL).  NULL parameters: the defaults.  Enqueued only. */
int  hrt_denoise_filter_variance(HrtContext *ctx, const HrtFloat4 *d_color, const HrtDenoiseGuide *d_guides, const float *d_variance,
                                 HrtFloat4 *d_out, float *d_var_out, uint32_t width, uint32_t height,
                                 const HrtDenoiseParams *h_dparams, const HrtDenoiseVarianceParams *h_vparams, void *stream);
/* one frame of the variance-guided mode into d_out (may be h_raygen->colorBuffer): guides, reprojection and blend with the moments,
 * variance, variance-guided filter.  NULL parameters: the defaults.  Enqueued only. */
int  hrt_denoise_variance_launch(HrtContext *ctx, const HrtGlobalParams *h_params, const HrtRayGenParams *h_raygen,
                                 const HrtDenoiseParams *h_dparams, const HrtDenoiseTemporalParams *h_tparams,
                                 const HrtDenoiseVarianceParams *h_vparams, HrtFloat4 *d_out, void *stream);
/* the last hrt_denoise_variance_launch's moments (width * height float2) and the variance its filter took (width * height float); a
 * NULL pointer skips its buffer.  hrt_debug_denoise_temporal_state gives its A, L and motion.  HRT_ERR_STATE before the first call.
 * Enqueued only. */
int  hrt_debug_denoise_variance_state(HrtContext *ctx, float *d_moments, float *d_variance, void *stream);

/* Accumulated mode: the variance-guided filter over a still frame that hrt_render_accumulate has sampled, its edge stop taken from the
 * frame's own sums instead of a temporal history (DESIGN.md 3e "Accumulated mode"; tests/denoise_accumulated_ref.py restates it).
 * Inputs: d_sum and d_taken as hrt_render_accumulate leaves them (width * height, frame order), and the frame's guides.  Per pixel with
 * n = d_taken[p] samples: the linear mean m = sum.xyz / n (k_finalize_counts' arithmetic; (0, 0, 0) for n = 0; alpha 1); the guides
 * with the depth of a pixel without a sample set to +inf, so that it is background to the filter -- never a tap, never filtered,
 * black in the result: a frame of which only a tile has been accumulated is a valid input; and the variance of the mean's luminance:
 * 0 on background, max(0, m2 - m1^2) / n with m1 = l(sum.xyz) / n, m2 = sum.w / n (hrt_sample_counts' estimator over n) on a hit with
 * n >= max(history_min, 2), and on every other hit the variance of l(m) over the 5x5 block's hits.  These three go through
 * hrt_denoise_filter_variance's passes, on LINEAR radiance (the other modes filter the encoded buffer: the moments are linear), and
 * d_out receives colorToFloat4 of the result.  Parameters as for hrt_denoise_filter_variance (NULL: the defaults), with the same
 * refusals.  HRT_ERR_INVALID also for a NULL d_sum, d_taken, d_guides or d_out, for d_out or d_linear_out equal to d_sum, and for
 * d_linear_out equal to d_out; a refused call writes nothing.  The sums, the totals, the caller's guides and the RNG states are never
 * written; neither is the temporal history read or forgotten: a still between two frames of a sequence leaves it alone.
 * Enqueued only.
 * ... over caller-given guides (no scene needed): the encoded result -> d_out, the filtered linear frame -> d_linear_out (may be
 * NULL), the filtered variance -> d_var_out (may be NULL) */
int  hrt_denoise_accumulated_filter(HrtContext *ctx, const HrtFloat4 *d_sum, const uint32_t *d_taken, const HrtDenoiseGuide *d_guides,
                                    HrtFloat4 *d_out, HrtFloat4 *d_linear_out, float *d_var_out, uint32_t width, uint32_t height,
                                    const HrtDenoiseParams *h_dparams, const HrtDenoiseVarianceParams *h_vparams, void *stream);
/* ... over the guides of the frame h_raygen describes (traced, or the primary capture where it is the hits of exactly these rays, as
 * in hrt_denoise_launch; HRT_ERR_STATE as there) into d_out, which may be h_raygen->colorBuffer: the colour buffer is not read, and
 * not written unless it is d_out. */
int  hrt_denoise_accumulated_launch(HrtContext *ctx, const HrtGlobalParams *h_params, const HrtRayGenParams *h_raygen,
                                    const HrtFloat4 *d_sum, const uint32_t *d_taken, const HrtDenoiseParams *h_dparams,
                                    const HrtDenoiseVarianceParams *h_vparams, HrtFloat4 *d_out, void *stream);

/* ---- measurement (no reference counterpart: the reference has no timers) ------------- */
enum { HRT_K_GENERATE = 0, HRT_K_TRAVERSE, HRT_K_TRAVERSE_ANY, HRT_K_BIN, HRT_K_SHADE,
       HRT_K_ACCUMULATE, HRT_K_FINALIZE, HRT_K_PATHS /* fused path mode */, HRT_K_REFIT /* hrt_tlas_update */, HRT_K_COUNT };

typedef struct HrtStats {
    uint64_t rays;                         /* trace calls since the last reset (1..5 per pixel-sample) */
    uint64_t rays_closest, rays_any;       /* split by traverse kernel                                 */
    uint64_t paths;                        /* pixel-samples                                            */
    uint64_t node_visits, prim_tests;      /* HRT_CTX_COUNT only, closest+any                          */
    uint64_t node_visits_closest, prim_tests_closest;   /* the closest-hit kernel's share            */
    double   kernel_ms[HRT_K_COUNT];       /* HRT_CTX_TIMING only: summed HIP-event time per kernel    */
    uint64_t kernel_launches[HRT_K_COUNT];
    uint64_t bvh_nodes, bvh_triangles, bvh_spheres;   /* of the TLAS last launched               */
    uint64_t bvh_bytes;
    uint64_t debug[4];                     /* HRT_CTX_COUNT, closest-hit kernel: wave iterations, wave leaf passes,
                                              sum of alive lanes over iterations, reserved                     */
    uint64_t tlas_refits, tlas_rebuilds;   /* hrt_tlas_update calls served by the device refit / builds + rebuilds    */
    double   tlas_refit_ratio;             /* quality sum of the last refitted tree checked / that of the built tree  */
    uint64_t bvh_depth;                    /* levels below the root of the TLAS last launched (trees deeper than 12 take round 1's path kernel) */
    uint64_t fused_fallback_launches;      /* launches since the context was created that took round 1's path kernel because the tree did not
                                              fit k_fused (deeper than 12 levels, or node / record arrays beyond 4 GiB = 32-bit byte offsets) */
    uint64_t graph_replays;                /* wavefront mode: sample pairs replayed from a captured hipGraph since the context was created */
    uint64_t bvh_alloc_bytes;              /* device memory the TLAS last launched holds for nodes, node boxes and records (bvh_bytes: the packed payload) */
    uint64_t sample_block_launches;        /* path-kernel launches since the context was created that handed pixels out in sample blocks (HRT_SAMPLE_BLOCK) */
    uint64_t tail[8];                      /* instrumented build only (make stats, tools/tail_profile.py): the path kernel's drained phase --
                                              wave iterations, alive lanes over them, clock base, ~first drained clock, last exit clock,
                                              sum of exit clocks, idle lane-ticks between draining and exit, waves (100 MHz ticks)        */
    uint64_t sample_block_schedule[4];     /* the last launch that handed pixels out in sample blocks: largest block, smallest block, the sample
                                              at which the halving blocks end (0: uniform blocks), passes (hrt_sample_schedule) */
    uint64_t wave_clock[60];               /* instrumented build only (make stats, tools/wave_clock.py): the clock the path kernel's waves ran at, from the shader
                                              clock's counter and the 100 MHz one read at a wave's first regeneration and at its exit -- waves, sum of
                                              their cycles, sum of their ticks, reserved, then 56 bins of 16 MHz from 1600 MHz (the ends take what lies
                                              beyond).  Added with mask_idle_launches: rebuild against this header */
    uint64_t direct_launches;              /* of mask_idle_launches: those that ran k_path_direct, k_path_idle whose repeat primary rays test their known hit's
                                              record in the regeneration and never enter the traversal loop (HRT_PRIMARY_DIRECT).  Added ahead of
                                              mask_idle_launches, which tests/test_mask_idle_cpu.py pins in front of restart_launches: rebuild against this header */
    uint64_t mask_idle_launches;           /* of restart_launches: those that ran k_path_idle, k_path_restart with idle lanes switched off in the loop's
                                              primitive test and node step (HRT_MASK_IDLE).  Added ahead of restart_launches, which
                                              tests/test_primary_restart_cpu.py pins in front of one_group_launches: rebuild against this header */
    uint64_t restart_launches;             /* of one_group_launches: those that ran k_path_restart, whose repeat primary rays start at the node of their
                                              known hit (HRT_PRIMARY_RESTART).  Added ahead of one_group_launches, which
                                              tests/test_denoise_by_primitive_cpu.py pins in front of the counters below: rebuild against this header */
    uint64_t one_group_launches;           /* of sample_block_launches: those that ran k_path_one (or k_path_restart, above), the kernel for a scene with one hit group -- a one-level
                                              tree of triangles over exactly one instance (HRT_ONE_GROUP).  Added ahead of the counters below, like
                                              denoise_history_rebinds: rebuild against this header */
    uint64_t denoise_by_primitive_links;   /* instances that hrt_denoise_temporal_rebind_geometry calls since the context was created have linked by
                                              primitive (counted at the call).  Added ahead of denoise_history_rebinds, which
                                              tests/test_denoise_handoff_cpu.py pins in front of the last three: rebuild against this header */
    uint64_t denoise_history_rebinds;      /* temporal / variance denoiser calls since the context was created that began from a history handed over
                                              from another TLAS (hrt_denoise_temporal_rebind).  Added ahead of the three counters below, which
                                              tests/test_primary_capture_cpu.py pins as the structure's last: rebuild against this header */
    uint64_t primary_capture_launches;     /* path-kernel launches since the context was created that captured primary hits (HRT_CTX_CAPTURE_PRIMARY) */
    uint64_t guide_passes_traced;          /* denoiser guide passes since the context was created that traced their rays ...                          */
    uint64_t guide_passes_captured;        /* ... and that took the render launch's capture instead (they add nothing to `rays`)                      */
} HrtStats;

/* The sample blocks a path-kernel launch of spp samples is cut into (host only, no context, no GPU): block_big = N, block_min = 0 -- uniform
 * blocks of N, HRT_SAMPLE_BLOCK=N; block_big : block_min, powers of two -- the tapered schedule, HRT_SAMPLE_TAPER.  Writes the first sample
 * of every pass and, behind the last, spp into first[0 .. *n_passes] (capacity: entries of first; HRT_ERR_INVALID when too small or
 * the sizes are not as above).  Pass b is samples first[b] .. first[b + 1]; the last block ends where the samples do, short if need be. */
int  hrt_sample_schedule(uint32_t spp, uint32_t block_big, uint32_t block_min, uint32_t *first, uint32_t capacity, uint32_t *n_passes);

int  hrt_stats_reset(HrtContext *ctx);
int  hrt_stats_get(HrtContext *ctx, HrtStats *out);       /* synchronises the device */

/* ---- introspection used by the parity tests ------------------------------------------ */
/* Trace n rays (origin/direction float3 arrays on the device, tmin/tmax as in the shader)
 * through a TLAS and write t,u,v (float) and prim,inst (u32; 0xffffffff on miss) per ray.
 * The rays go through the kernel hrt_render_launch itself runs in the context's configuration: the
 * fused path kernel by default (each ray stands in for a pixel that is traced once and not shaded),
 * the wavefront traverse kernel under HRT_CTX_COUNT or HRT_FUSED=0. */
int  hrt_trace_rays(HrtContext *ctx, HrtTraversable tlas, const HrtFloat3 *d_origins,
                    const HrtFloat3 *d_directions, uint32_t n_rays, float tmin, float tmax,
                    int any_hit, float *d_t, float *d_u, float *d_v,
                    uint32_t *d_prim, uint32_t *d_inst, void *stream);

/* When set (non-NULL), every following launch also writes the linear mean radiance (the value
 * colorToFloat4 is applied to, shader/Shader.cu:270) as W*H float4, so that tests can compare
 * it bit-for-bit with the oracle.  Pass NULL to switch it off. */
int  hrt_debug_set_linear_output(HrtContext *ctx, HrtFloat4 *d_linear);

/* sinf (0) / cosf (1) / acosf (2) / asinf (3) / atan2f (4) as hrt_pose_instances evaluates them (csrc/cr_trig.h: the correctly
 * rounded float of the exact value, the pin shared with the oracle), over n arguments: d_a[i] (atan2: y = d_a[i], x = d_b[i]), or,
 * when d_a is NULL, the floats whose bit patterns are first_bits + i * stride_bits.  force_slow != 0 decides every value in
 * double-double arithmetic (the path one call in ~500 000 takes). */
int  hrt_debug_trig(HrtContext *ctx, int function, const float *d_a, const float *d_b, uint32_t first_bits, uint32_t stride_bits,
                    uint64_t n, int force_slow, float *d_out, void *stream);

/* Host-only BVH8 build over triangles given as 9 floats each (no GPU needed): returns the
 * packed node and primitive blobs the device kernels traverse.  Free with hrt_host_free. */
typedef struct HrtBvhBlob {
    void    *nodes;      uint64_t n_nodes;      /* 80-byte packed BVH8 nodes             */
    void    *triangles;  uint64_t n_triangles;  /* 48-byte triangle records, leaf order  */
    float    bounds[6];
} HrtBvhBlob;
int  hrt_host_build_bvh8(const float *h_triangles, uint32_t n_triangles, HrtBvhBlob *out);
/* Host only (tests): the part of the triangle tri9 (three vertices) inside the box box6 (lo, hi) as ranges of the triangle's own
 * barycentric coordinates, out6 = {u0, u1, v0, v1, w0, w1} with p = v0 + u (v1 - v0) + v (v2 - v0), w = 1 - u - v: what a tree
 * under HRT_CTX_KEEP_SPLITS keeps per record (csrc/bvh8_geom.h: clip_triangle_barycentric).  Full ranges [0, 1] where the part is empty. */
int  hrt_host_clip_barycentric(const float tri9[9], const float box6[6], float out6[6]);
/* Copy the flattened world-space BVH of a TLAS, as it is in device memory now (after any refit), back to
 * the host (same blob format). */
int  hrt_tlas_download(HrtContext *ctx, HrtTraversable tlas, HrtBvhBlob *out);
/* The table record -> node of a blob (host only): out[r] = index of the node whose leaf slot covers record r, for the blob's
 * n_triangles records (capacity: entries of out).  HRT_ERR_STATE when a record is covered by no slot or by two.  It is what the
 * path kernel's repeat primary rays start from (HRT_PRIMARY_RESTART). */
int  hrt_host_leaf_parent(const HrtBvhBlob *blob, uint32_t *out, uint64_t capacity);
/* ... and the same table as the device made it for a TLAS (a one-level tree of triangles; made now if no launch has asked for it yet),
 * copied to the host: h_out holds capacity entries, *n_records says how many the tree has.  Synchronises the device. */
int  hrt_tlas_leaf_parent(HrtContext *ctx, HrtTraversable tlas, uint32_t *h_out, uint64_t capacity, uint64_t *n_records);
void hrt_host_free(HrtBvhBlob *blob);

#ifdef __cplusplus
}
static_assert(sizeof(HrtDenoiseGuide) == 16, "HrtDenoiseGuide is 16 B");
static_assert(sizeof(HrtDenoiseTemporalParams) == 16, "HrtDenoiseTemporalParams is 16 B");
static_assert(sizeof(HrtDenoiseParams) == 24, "HrtDenoiseParams is 24 B");
static_assert(sizeof(HrtDenoiseVarianceParams) == 16, "HrtDenoiseVarianceParams is 16 B");
#endif
#endif /* HRT_H */
