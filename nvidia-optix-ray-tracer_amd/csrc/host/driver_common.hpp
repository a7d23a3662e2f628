// driver_common.hpp -- what the headless drivers of the reference's two program flows (hrt_time_render.cpp, hrt_mesh_render.cpp) have in
// common beyond renderer_host.hpp's mirror of the reference's API: their error checks, the denoiser's command-line switches and its
// slot in the frame loop, the material table and frame buffers made from the config, the run's summary and the PPM file at its end.
#pragma once
#include "renderer_host.hpp"
#include "hrt_io.h"

#include <algorithm>
#include <cstring>
#include <string>

#define hipCheck(x) do { hipError_t e = (x); if (e != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e)); std::exit(-100); } } while (0)
#define ioCheck(x) do { if ((x) != 0) { std::fprintf(stderr, "%s\n", hrt_io_last_error()); std::exit(-1); } } while (0)   // VTK_READER_ERROR_EXIT_CODE

namespace driver {
using namespace project;

inline std::string join(const std::string &base, const std::string &p) { return (!p.empty() && p[0] == '/') ? p : base + "/" + p; }

// --denoise (anywhere): every frame goes through denoiseOutput before the conversion, as the reference's default display does
// (RendererTime.cu / RendererMesh.cu: launch -> denoiseOutput -> convertFloat4ToUchar4Kernel); without it the raw frame is shown, skipDenoise
// --denoise-temporal (anywhere): the same slot in the library's temporal mode, each frame blended into the history of the ones before
// --denoise-variance (anywhere): the temporal mode with variance-guided edge stops (denoiseOutputVariance)
enum class DenoiseMode { kNone, kSpatial, kTemporal, kVariance };
constexpr const char *kDenoiseUsage = "[--denoise | --denoise-temporal | --denoise-variance] [--no-capture]";

// takes the switches out of argv; two different ones end the program with status 2
inline DenoiseMode parseDenoiseMode(int &argc, char **argv) {
    static const struct { const char *flag; DenoiseMode mode; } kFlags[] = {
        {"--denoise", DenoiseMode::kSpatial}, {"--denoise-temporal", DenoiseMode::kTemporal}, {"--denoise-variance", DenoiseMode::kVariance}};
    DenoiseMode mode = DenoiseMode::kNone;
    bool clash = false;
    int k = 1;
    for (int i = 1; i < argc; ++i) {
        const auto *f = std::find_if(std::begin(kFlags), std::end(kFlags), [&](const auto &c) { return std::strcmp(argv[i], c.flag) == 0; });
        if (f == std::end(kFlags)) { argv[k++] = argv[i]; continue; }
        clash = clash || (mode != DenoiseMode::kNone && mode != f->mode);
        mode = f->mode;
    }
    argc = k;
    if (clash) { std::fprintf(stderr, "--denoise, --denoise-temporal and --denoise-variance exclude each other\n"); std::exit(2); }
    return mode;
}

// What a driver adds to its context's flags for the denoiser: HRT_CTX_CAPTURE_PRIMARY, so that the guide pass of every frame takes the
// primary hits the render launch has just found instead of tracing them again (the same image bit for bit; include/hrt.h).
// --no-capture (anywhere, taken out of argv): the guide pass traces, as it does in a context without the flag.
inline uint32_t denoiseContextFlags(DenoiseMode mode, int &argc, char **argv) {
    bool capture = mode != DenoiseMode::kNone;
    int k = 1;
    for (int i = 1; i < argc; ++i) {
        if (std::strcmp(argv[i], "--no-capture") == 0) capture = false;
        else argv[k++] = argv[i];
    }
    argc = k;
    return capture ? HRT_CTX_CAPTURE_PRIMARY : 0u;
}

// Whether a frame loop that changes IAS (Time mode: one per particle file) hands the denoiser's history over to the next one
// (rebindDenoiseHistory): under --denoise-temporal and --denoise-variance, unless --no-history-handoff (anywhere, taken out of argv)
// keeps every file's first frame a fresh start.
constexpr const char *kHandoffUsage = "[--no-history-handoff]";
inline bool denoiseHistoryHandoff(DenoiseMode mode, int &argc, char **argv) {
    bool handoff = mode == DenoiseMode::kTemporal || mode == DenoiseMode::kVariance;
    int k = 1;
    for (int i = 1; i < argc; ++i) {
        if (std::strcmp(argv[i], "--no-history-handoff") == 0) handoff = false;
        else argv[k++] = argv[i];
    }
    argc = k;
    return handoff;
}

// the denoiser's slot of a frame, in place: the colour buffer is not read again
inline void denoiseFrame(DenoiseMode mode, HrtContext *ctx, const HrtGlobalParams &params, const HrtRayGenParams &raygen, HrtFloat4 *color) {
    switch (mode) {
    case DenoiseMode::kNone: break;
    case DenoiseMode::kSpatial: denoiseOutput(ctx, params, raygen, color); break;
    case DenoiseMode::kTemporal: denoiseOutputTemporal(ctx, params, raygen, color); break;
    case DenoiseMode::kVariance: denoiseOutputVariance(ctx, params, raygen, color); break;
    }
}

// materials: the config's roughs and metals, then the baked ramp of rampCount colours as roughs from materialOffset on
// (RendererTime.cu:246-256, RendererMesh.cu:222-232)
struct MaterialTable { RendererMaterial materials; size_t materialOffset; };
inline MaterialTable materialsFromConfig(const HrtIoConfig &cfg, uint64_t rampCount) {
    std::vector<float> ramp(3 * rampCount);
    ioCheck(hrt_io_bake_color_ramp(cfg.particle_material_preset, rampCount, ramp.data()));
    MaterialTable t;
    for (uint64_t i = 0; i < cfg.n_roughs; ++i) t.materials.roughs.push_back({cfg.roughs[3 * i], cfg.roughs[3 * i + 1], cfg.roughs[3 * i + 2]});
    for (uint64_t i = 0; i < cfg.n_metals; ++i) t.materials.metals.push_back({{cfg.metals[4 * i], cfg.metals[4 * i + 1], cfg.metals[4 * i + 2]}, cfg.metals[4 * i + 3]});
    t.materialOffset = t.materials.roughs.size();
    for (uint64_t i = 0; i < rampCount; ++i) t.materials.roughs.push_back({ramp[3 * i], ramp[3 * i + 1], ramp[3 * i + 2]});
    return t;
}

// the config's camera, a W x H colour buffer and its 8-bit twin on the device
struct Frame { HrtRayGenParams raygen; HrtFloat4 *color; HrtUchar4 *rgba; };
inline Frame frameFromConfig(const HrtIoConfig &cfg, uint32_t W, uint32_t H) {
    const auto camera = SDL_GraphicsWindowConfigureCamera({cfg.camera_center[0], cfg.camera_center[1], cfg.camera_center[2]},
                                                          {cfg.camera_target[0], cfg.camera_target[1], cfg.camera_target[2]},
                                                          {cfg.up_direction[0], cfg.up_direction[1], cfg.up_direction[2]}, cfg.api_is_opengl != 0);
    Frame f{};
    hipCheck(hipMalloc((void **)&f.color, sizeof(HrtFloat4) * (size_t)W * H));
    hipCheck(hipMalloc((void **)&f.rgba, sizeof(HrtUchar4) * (size_t)W * H));
    f.raygen.width = W; f.raygen.height = H; f.raygen.colorBuffer = f.color;
    f.raygen.cameraCenter = camera.cameraCenter; f.raygen.cameraU = camera.cameraU; f.raygen.cameraV = camera.cameraV; f.raygen.cameraW = camera.cameraW;
    return f;
}

// the kernel classes' times (under HRT_CTX_TIMING) and the frame rate of `frames` frames rendered in `ms`
inline void printSummary(HrtContext *ctx, long frames, uint32_t W, uint32_t H, double ms) {
    HrtStats st{};
    hrtCheckError(ctx, hrt_stats_get(ctx, &st));
    for (int k = 0; k < HRT_K_COUNT; ++k)
        if (st.kernel_launches[k] && st.kernel_ms[k] > 0.0) std::printf("  kernel class %d: %.3f ms in %llu launches\n", k, st.kernel_ms[k], (unsigned long long)st.kernel_launches[k]);
    std::printf("%ld frames %ux%u: %.3f ms/frame (%.0f frames/s), %.1f Mrays/s, refits %llu rebuilds %llu\n", frames, W, H, ms / std::max(1l, frames),
                frames / ms * 1e3, st.rays / ms * 1e-3, (unsigned long long)st.tlas_refits, (unsigned long long)st.tlas_rebuilds);
}

inline void writePpm(const std::string &path, const HrtUchar4 *dev_rgba, uint32_t W, uint32_t H) {
    std::vector<HrtUchar4> host((size_t)W * H);
    hipCheck(hipMemcpy(host.data(), dev_rgba, host.size() * sizeof(HrtUchar4), hipMemcpyDeviceToHost));
    if (FILE *fp = std::fopen(path.c_str(), "wb")) {
        std::fprintf(fp, "P6\n%u %u\n255\n", W, H);
        for (uint32_t y = 0; y < H; ++y) for (uint32_t x = 0; x < W; ++x) std::fwrite(&host[(size_t)y * W + x], 1, 3, fp);
        std::fclose(fp);
    }
}

}  // namespace driver
