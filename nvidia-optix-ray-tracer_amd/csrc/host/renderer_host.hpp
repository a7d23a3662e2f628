// renderer_host.hpp -- C++ host-side mirror of the reference's renderer-implementation layer
// over the C ABI (include/hrt.h).  Same function names and argument meaning as the reference's
// include/Global/RendererImpl.cuh:153-253 for the path that was rebuilt; errors follow the
// reference's convention (log + exit, include/Global/HostFunctions.cuh:147-166), which is what a
// reference-side caller expects from these helpers.  Header-only; link against libhrt.so.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <tuple>
#include <utility>
#include <vector>

#include "hrt.h"

namespace project {

constexpr int HRT_ERROR_EXIT_CODE = -200;   // the reference's OptiX error exit code (HostFunctions.cu:30-50)

#define hrtCheckError(ctx, call)                                                                  \
    do {                                                                                          \
        const int _rc = (call);                                                                   \
        if (_rc != HRT_OK) {                                                                      \
            std::fprintf(stderr, "[hrt] %s failed (%d): %s\n", #call, _rc, hrt_last_error(ctx)); \
            std::exit(project::HRT_ERROR_EXIT_CODE);                                              \
        }                                                                                         \
    } while (0)

typedef std::pair<HrtTraversable, void *> GAS;                 // (handle, unused) -- RendererImpl.cuh:20
typedef std::tuple<HrtTraversable, void *, size_t> IAS;        // RendererImpl.cuh:21

struct RendererSphere { int materialType; size_t materialIndex; HrtFloat3 *dev_centers; float *dev_radii; size_t count; };
struct RendererTriangle { int materialType; size_t materialIndex; HrtFloat3 *dev_vertices; HrtFloat3 *dev_normals; size_t count; };

// createContext / destroyContext, src/Global/RendererImpl.cu:6-27
inline HrtContext *createContext(int device = 0, bool isDebugMode = false) {
    HrtContext *ctx = nullptr;
    const int rc = hrt_ctx_create(device, isDebugMode ? (HRT_CTX_TIMING | HRT_CTX_COUNT) : 0u, &ctx);
    if (rc != HRT_OK) { std::fprintf(stderr, "[hrt] createContext: %s\n", hrt_last_error(nullptr)); std::exit(HRT_ERROR_EXIT_CODE); }
    return ctx;
}
inline void destroyContext(HrtContext *&ctx) { hrt_ctx_destroy(ctx); ctx = nullptr; }

// buildGASForSpheres / buildGASForTriangles, src/Global/RendererImpl.cu:113-172 (count = triangles, Q6 fixed: 3 vertices each)
inline GAS buildGASForSpheres(HrtContext *ctx, const RendererSphere &s, hipStream_t stream = nullptr) {
    HrtTraversable h = 0;
    hrtCheckError(ctx, hrt_blas_build_spheres(ctx, s.dev_centers, s.dev_radii, (uint32_t)s.count, stream, &h));
    return {h, nullptr};
}
inline GAS buildGASForTriangles(HrtContext *ctx, const RendererTriangle &t, hipStream_t stream = nullptr) {
    HrtTraversable h = 0;
    hrtCheckError(ctx, hrt_blas_build_triangles(ctx, t.dev_vertices, (uint32_t)(3 * t.count), stream, &h));
    return {h, nullptr};
}
// optixAccelBuild with OPTIX_BUILD_OPERATION_UPDATE on a triangle GAS (no call site in the reference, whose meshes are rigid): the same
// triangles at new positions, triangle.count as at the build.  triangle.dev_normals is the caller's to rewrite; follow with updateIAS.
inline void updateGASForTriangles(HrtContext *ctx, const GAS &gas, const RendererTriangle &t, hipStream_t stream = nullptr) {
    hrtCheckError(ctx, hrt_blas_update_triangles(ctx, gas.first, t.dev_vertices, (uint32_t)(3 * t.count), stream));
}
// ... and on a sphere GAS (a moving particle cloud): the same spheres at new centres and with new radii, sphere.count as at the build.  The
// record's centers / radii are the caller's buffers (sphere.dev_centers / dev_radii where they are the ones it shades with); follow with updateIAS.
inline void updateGASForSpheres(HrtContext *ctx, const GAS &gas, const RendererSphere &s, hipStream_t stream = nullptr) {
    hrtCheckError(ctx, hrt_blas_update_spheres(ctx, gas.first, s.dev_centers, s.dev_radii, (uint32_t)s.count, stream));
}
// buildIAS / updateIAS, src/Global/RendererImpl.cu:174-242
inline IAS buildIAS(HrtContext *ctx, const HrtInstance *dev_instances, size_t instanceCount, hipStream_t stream = nullptr) {
    HrtTraversable h = 0;
    hrtCheckError(ctx, hrt_tlas_build(ctx, dev_instances, (uint32_t)instanceCount, stream, &h));
    return {h, nullptr, instanceCount};
}
inline void updateIAS(HrtContext *ctx, IAS &ias, const HrtInstance *dev_instances, size_t instanceCount, hipStream_t stream = nullptr) {
    hrtCheckError(ctx, hrt_tlas_update(ctx, std::get<0>(ias), dev_instances, (uint32_t)instanceCount, stream));
}
inline void cleanupAccelerationStructure(HrtContext *ctx, GAS &g) { hrt_blas_destroy(ctx, g.first); g = {}; }
inline void cleanupAccelerationStructure(HrtContext *ctx, IAS &i) { hrt_tlas_destroy(ctx, std::get<0>(i)); i = {}; }

// SBT records, src/Global/RendererImpl.cu:472-575.  The four OptixProgramGroup arguments of the reference become the
// HrtProgram ids hrt_sbt_record_pack_header takes; the records keep their layout and are handed to hrt_materials_set
// (record i <-> instance with sbtOffset i) where the reference copies them to the device (RendererMesh.cu:283-305).
enum MaterialType { ROUGH = 0, METAL = 1 };                                   // include/Global/Shader.cuh:16-18
struct RendererMaterial { std::vector<HrtFloat3> roughs; std::vector<std::pair<HrtFloat3, float>> metals; };   // RendererImpl.cuh:109-112
typedef HrtSbtRecord HitGroupSbtRecord;

inline void packMaterial(HrtContext *ctx, HitGroupSbtRecord &record, bool sphere, int materialType, size_t materialIndex,
                         const RendererMaterial &globalMaterials) {
    if (materialType == ROUGH) {
        hrtCheckError(ctx, hrt_sbt_record_pack_header(sphere ? HRT_PROGRAM_SPHERE_ROUGH : HRT_PROGRAM_TRIANGLE_ROUGH, &record));
        record.data.rough.albedo = globalMaterials.roughs.at(materialIndex);
    } else {
        hrtCheckError(ctx, hrt_sbt_record_pack_header(sphere ? HRT_PROGRAM_SPHERE_METAL : HRT_PROGRAM_TRIANGLE_METAL, &record));
        record.data.metal.albedo = globalMaterials.metals.at(materialIndex).first;
        record.data.metal.fuzz = globalMaterials.metals.at(materialIndex).second;
    }
}
// createAddSphereTriangleSBTRecord, RendererImpl.cu:494-552: spheres first, then triangles
inline std::vector<HitGroupSbtRecord> createAddSphereTriangleSBTRecord(HrtContext *ctx, const std::vector<RendererSphere> &spheres,
                                                                       const std::vector<RendererTriangle> &triangles,
                                                                       const RendererMaterial &globalMaterials) {
    std::vector<HitGroupSbtRecord> records;
    records.reserve(spheres.size() + triangles.size());
    for (const auto &sphere : spheres) {
        HitGroupSbtRecord record = {};
        record.data.sphere.centers = sphere.dev_centers; record.data.sphere.radii = sphere.dev_radii;
        packMaterial(ctx, record, true, sphere.materialType, sphere.materialIndex, globalMaterials);
        records.push_back(record);
    }
    for (const auto &triangle : triangles) {
        HitGroupSbtRecord record = {};
        record.data.triangles.vertexNormals = triangle.dev_normals;
        packMaterial(ctx, record, false, triangle.materialType, triangle.materialIndex, globalMaterials);
        records.push_back(record);
    }
    return records;
}
// createVTKParticleSBTRecord, RendererImpl.cu:554-575: (rough material index, vertex normals) per particle, all ROUGH
inline std::vector<HitGroupSbtRecord> createVTKParticleSBTRecord(HrtContext *ctx, const std::vector<std::pair<size_t, HrtFloat3 *>> &particles,
                                                                 const RendererMaterial &globalMaterials) {
    std::vector<HitGroupSbtRecord> records;
    records.reserve(particles.size());
    for (const auto &particle : particles) {
        HitGroupSbtRecord record = {};
        record.data.triangles.vertexNormals = particle.second;
        packMaterial(ctx, record, false, ROUGH, particle.first, globalMaterials);
        records.push_back(record);
    }
    return records;
}
// the miss half of createRaygenMissSBTRecord, RendererImpl.cu:472-492 (the raygen record's payload is HrtRayGenParams, passed per launch)
inline void createMissSBTRecord(HrtContext *ctx, const HrtFloat3 &backgroundColor) {
    const HrtMissParams miss{backgroundColor};
    hrtCheckError(ctx, hrt_miss_set(ctx, &miss));
}

// RandomGenerator::initDeviceRandomGenerators, src/Global/HostFunctions.cu:128-140 (seedSalt pins clock64())
struct RandomGenerator {
    static void initDeviceRandomGenerators(HrtContext *ctx, HrtRngState *&dev_stateArray, size_t x, size_t y,
                                           unsigned long long seedSalt, hipStream_t stream = nullptr) {
        hrtCheckError(ctx, hrt_rng_init(ctx, (uint32_t)x, (uint32_t)y, seedSalt, stream, &dev_stateArray));
    }
    static void freeDeviceRandomGenerators(HrtContext *ctx, HrtRngState *&dev_stateArray, hipStream_t stream = nullptr) {
        hrtCheckError(ctx, hrt_rng_free(ctx, dev_stateArray, stream));
        dev_stateArray = nullptr;
    }
};

// SDL_GraphicsWindowConfigureCamera, src/GraphicsAPI/SDL_GraphicsWindow.cu:4-14
struct SDL_GraphicsWindowCamera { HrtFloat3 upDirection, cameraCenter, cameraTarget, cameraU, cameraV, cameraW; };
inline HrtFloat3 hostNormalize(HrtFloat3 v) {
    const float len2 = v.x * v.x + v.y * v.y + v.z * v.z;
    if (len2 <= HRT_FLOAT_ZERO_VALUE * HRT_FLOAT_ZERO_VALUE) return {0.0f, 0.0f, 1.0f};
    const float inv = 1.0f / std::sqrt(len2);
    return {v.x * inv, v.y * inv, v.z * inv};
}
inline HrtFloat3 hostCross(HrtFloat3 a, HrtFloat3 b) {
    return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
inline SDL_GraphicsWindowCamera SDL_GraphicsWindowConfigureCamera(const HrtFloat3 &center, const HrtFloat3 &target, const HrtFloat3 &up, bool isOpenGL) {
    SDL_GraphicsWindowCamera camera{};
    camera.upDirection = hostNormalize(up); camera.cameraCenter = center; camera.cameraTarget = target;
    if (!isOpenGL) camera.upDirection = {-camera.upDirection.x, -camera.upDirection.y, -camera.upDirection.z};
    camera.cameraW = {target.x - center.x, target.y - center.y, target.z - center.z};
    camera.cameraU = hostNormalize(hostCross(camera.cameraW, camera.upDirection));
    camera.cameraV = hostNormalize(hostCross(camera.cameraU, camera.cameraW));
    return camera;
}

// the launch: optixLaunch + cudaDeviceSynchronize, src/Global/RendererMesh.cu:416-419
inline void launch(HrtContext *ctx, const HrtGlobalParams &params, const HrtRayGenParams &raygen, unsigned int spp = 1,
                   const HrtTile *tile = nullptr, hipStream_t stream = nullptr) {
    hrtCheckError(ctx, hrt_render_launch(ctx, &params, &raygen, spp, tile, stream));
    hrtCheckError(ctx, hrt_sync(ctx, stream));
}

// HRT_CTX_CAPTURE_PRIMARY (include/hrt.h; no reference counterpart): the primary hit of every pixel as the last full-frame launch found
// it, width * height of each in frame order (a NULL pointer skips its array) -- picking, depth and id buffers without a second trace.
// false when the context holds no valid capture.  With the flag set, the three denoiseOutput calls below take the capture for their
// guides instead of tracing the frame's primary rays again (launch and denoiser on the same stream).
inline bool primaryHits(HrtContext *ctx, float *dev_t, float *dev_u, float *dev_v, uint32_t *dev_prim, uint32_t *dev_inst, hipStream_t stream = nullptr) {
    const int rc = hrt_primary_hits_get(ctx, dev_t, dev_u, dev_v, dev_prim, dev_inst, stream);
    if (rc == HRT_ERR_STATE) return false;
    hrtCheckError(ctx, rc);
    return true;
}

// denoiseOutput, src/Global/RendererImpl.cu:680-710: the OptiX denoiser's slot, filled by the library's guided a-trous filter (include/hrt.h);
// like the reference it reads the frame's colour buffer and leaves the result for convertFloat4ToUchar4Kernel (hrt_to_rgba8).  The
// skipDenoise branch (Tab held) converts the colour buffer directly.
inline void denoiseOutput(HrtContext *ctx, const HrtGlobalParams &params, const HrtRayGenParams &raygen, HrtFloat4 *output,
                          const HrtDenoiseParams *denoiseParams = nullptr, hipStream_t stream = nullptr) {
    hrtCheckError(ctx, hrt_denoise_launch(ctx, &params, &raygen, denoiseParams, output, stream));
}

// denoiseOutput's temporal mode (include/hrt.h): the same slot, for a frame loop at a few samples per pixel -- each frame is blended into
// the reprojected history of the frames before it, then filtered.  The history lives in the context; the first frame is denoiseOutput's.
inline void denoiseOutputTemporal(HrtContext *ctx, const HrtGlobalParams &params, const HrtRayGenParams &raygen, HrtFloat4 *output,
                                  const HrtDenoiseParams *denoiseParams = nullptr, const HrtDenoiseTemporalParams *temporalParams = nullptr,
                                  hipStream_t stream = nullptr) {
    hrtCheckError(ctx, hrt_denoise_temporal_launch(ctx, &params, &raygen, denoiseParams, temporalParams, output, stream));
}

// denoiseOutput's variance-guided mode (include/hrt.h): the temporal mode with the luminance moments carried through the history and the
// filter's colour edge stop following the accumulated frame's variance.  It shares the context's history with the temporal mode.
inline void denoiseOutputVariance(HrtContext *ctx, const HrtGlobalParams &params, const HrtRayGenParams &raygen, HrtFloat4 *output,
                                  const HrtDenoiseParams *denoiseParams = nullptr, const HrtDenoiseTemporalParams *temporalParams = nullptr,
                                  const HrtDenoiseVarianceParams *varianceParams = nullptr, hipStream_t stream = nullptr) {
    hrtCheckError(ctx, hrt_denoise_variance_launch(ctx, &params, &raygen, denoiseParams, temporalParams, varianceParams, output, stream));
}

// The frame loop moves on to another IAS of the same scene (the next file's, RendererTime.cu:443-447): the history of the two calls
// above goes with it (hrt_denoise_temporal_rebind, include/hrt.h).  previousInstance[i]: the index instance i of `next` had in the IAS
// the history was made for, HRT_NO_INSTANCE for a new body; NULL: the same index.  Call it before the first denoiseOutputTemporal /
// denoiseOutputVariance on `next`, before or after that frame's pose step and updateIAS.
inline void rebindDenoiseHistory(HrtContext *ctx, HrtTraversable next, size_t instanceCount, const uint32_t *previousInstance = nullptr,
                                 hipStream_t stream = nullptr) {
    hrtCheckError(ctx, hrt_denoise_temporal_rebind(ctx, next, previousInstance, (uint32_t)instanceCount, stream));
}

// ... on to an IAS whose GASes were built anew from the same triangles (Mesh mode: a GAS per particle and file, RendererMesh.cu:93-157):
// an instance whose GAS differs from its predecessor's keeps its history primitive by primitive, through the previous GAS's vertices
// (hrt_denoise_temporal_rebind_geometry).  The previous file's GASes and IAS may be cleaned up right after this call.
inline void rebindDenoiseHistoryGeometry(HrtContext *ctx, HrtTraversable next, size_t instanceCount, const uint32_t *previousInstance = nullptr,
                                         hipStream_t stream = nullptr) {
    hrtCheckError(ctx, hrt_denoise_temporal_rebind_geometry(ctx, next, previousInstance, (uint32_t)instanceCount, stream));
}

}  // namespace project
