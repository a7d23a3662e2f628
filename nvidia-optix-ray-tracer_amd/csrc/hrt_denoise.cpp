// hrt_denoise.cpp -- C ABI of the denoiser (include/hrt.h "denoiser"): what stands in for denoiseOutput, src/Global/RendererImpl.cu:680-710.
// Guide pass: the primary rays of the frame (denoise.hip k_denoise_rays) through hrt_trace_rays' traversal (hrt_api.cpp trace_records: the
// path kernel in the context's configuration, flattened and two-level trees alike), their hits turned into HrtDenoiseGuide records with
// the material tables of the launch.  Filter: `iterations` a-trous passes, one launch each, ping-ponging between two frames the context
// owns; the variance-guided filter is the same path (pass_constants, run_filter) with a variance frame ping-ponged next to the colour.
// The accumulated mode (accumulated_filter) feeds that filter from hrt_render_accumulate's sums and encodes what it returns.
// The temporal and the variance-guided mode share the reprojection step (run_temporal), the history and everything around their filter
// (temporal_launch).  Every call only enqueues work (the material tables' upload after hrt_materials_set synchronises once, as in
// hrt_render_launch).
#include "hrt_internal.hpp"

namespace hrt {

void free_denoise_work(HrtContext *ctx) {
    DenoiseWork &d = ctx->denoise;
    void *ptrs[] = {d.rays, d.tuvp, d.inst, d.guides, d.frame[0], d.frame[1], d.var[0], d.var[1], d.fetch};
    for (void *p : ptrs) if (p) (void)hipFree(p);
    d = DenoiseWork{};
}

void free_denoise_history(HrtContext *ctx) {
    DenoiseHistory &h = ctx->denoise_history;
    for (DenoiseHistorySet &s : h.set) {
        void *ptrs[] = {s.accum, s.length, s.guides, s.id, s.moments, s.xf};
        for (void *p : ptrs) if (p) (void)hipFree(p);
    }
    if (h.motion) (void)hipFree(h.motion);
    if (h.variance) (void)hipFree(h.variance);
    if (h.link) (void)hipFree(h.link);
    if (h.link_verts) (void)hipFree((void *)h.link_verts);
    h = DenoiseHistory{};
}

namespace {

constexpr uint32_t kMaxDenoiseSide = 1u << 16;       // (the filter's pixel arithmetic is in int: sides plus 2 * 2^15 stay far from overflow)

int check_frame(HrtContext *ctx, uint32_t width, uint32_t height) {
    if (width == 0 || height == 0 || width > kMaxDenoiseSide || height > kMaxDenoiseSide || (uint64_t)width * height > 0xffffffffull)
        return fail(ctx, HRT_ERR_INVALID, "bad frame size %ux%u", width, height);
    return HRT_OK;
}

// the per-pixel arrays for n pixels: the guide pass's, the filter's two frames, or those and the variance-guided filter's two variance
// frames.  All are sized by d.capacity: free_denoise_work, called before the capacity grows, frees every one of them, so a non-NULL one
// is large enough.
enum Work { kTrace, kFilter, kFilterVariance };
int ensure_work(HrtContext *ctx, uint32_t n, Work work) {
    DenoiseWork &d = ctx->denoise;
    if (n > d.capacity) {
        free_denoise_work(ctx);
        HIP_TRY(ctx, hipMalloc((void **)&d.fetch, sizeof(uint32_t) * 8 * 32));
        d.capacity = n;
    }
    if (work == kTrace && !d.rays) {
        HIP_TRY(ctx, hipMalloc((void **)&d.rays, sizeof(RayRec) * (size_t)d.capacity));
        HIP_TRY(ctx, hipMalloc((void **)&d.tuvp, sizeof(float4) * (size_t)d.capacity));
        HIP_TRY(ctx, hipMalloc((void **)&d.inst, sizeof(uint32_t) * (size_t)d.capacity));
        HIP_TRY(ctx, hipMalloc((void **)&d.guides, sizeof(uint4) * (size_t)d.capacity));
    }
    if (work != kTrace && !d.frame[0]) {
        HIP_TRY(ctx, hipMalloc((void **)&d.frame[0], sizeof(float4) * (size_t)d.capacity));
        HIP_TRY(ctx, hipMalloc((void **)&d.frame[1], sizeof(float4) * (size_t)d.capacity));
    }
    if (work == kFilterVariance)
        for (float *&v : d.var)
            if (!v) HIP_TRY(ctx, hipMalloc((void **)&v, sizeof(float) * (size_t)d.capacity));
    return HRT_OK;
}

bool positive_finite(float x) { return std::isfinite(x) && x > 0.0f; }

// the filter's parameters (NULL: the defaults), validated; HRT_ERR_INVALID when one is out of range
int filter_params(HrtContext *ctx, const HrtDenoiseParams *h_dparams, HrtDenoiseParams &p) {
    hrt_denoise_default_params(&p);
    if (h_dparams) p = *h_dparams;
    if (p.iterations < 1 || p.iterations > 16 || p.normal_power_log2 > 8 || p.reserved != 0 ||
        !positive_finite(p.sigma_color) || !positive_finite(p.sigma_albedo) || !positive_finite(p.sigma_depth))
        return fail(ctx, HRT_ERR_INVALID, "denoise parameters out of range (iterations 1..16, sigmas > 0 and finite, normal_power_log2 <= 8, reserved 0)");
    return HRT_OK;
}

// the variance-guided mode's parameters (NULL: the defaults), not yet validated: pass_constants does that
HrtDenoiseVarianceParams variance_params(const HrtDenoiseVarianceParams *h_vparams) {
    HrtDenoiseVarianceParams vp;
    hrt_denoise_variance_default_params(&vp);
    if (h_vparams) vp = *h_vparams;
    return vp;
}

// ... and the constants of every pass.  vp != NULL: the variance-guided filter's, which does not use sigma_color beyond filter_params'
// range check; the other fields of HrtDenoiseParams it does
int pass_constants(HrtContext *ctx, const HrtDenoiseParams *h_dparams, const HrtDenoiseVarianceParams *vp, std::vector<DenoisePassArgs> &passes) {
    HrtDenoiseParams p;
    int rc = filter_params(ctx, h_dparams, p);
    if (rc != HRT_OK) return rc;
    const float k_luminance = vp ? vp->sigma_luminance * vp->sigma_luminance : 0.0f;
    if (vp && (!positive_finite(vp->sigma_luminance) || !positive_finite(k_luminance) || vp->history_min < 1 || vp->history_min > 65536 ||
               !positive_finite(vp->variance_floor) || vp->reserved != 0))
        return fail(ctx, HRT_ERR_INVALID, "variance denoise parameters out of range (sigma_luminance > 0 with a finite, non-zero square, history_min 1..65536, variance_floor > 0 and finite, reserved 0)");
    passes.assign(p.iterations, DenoisePassArgs{});
    for (uint32_t i = 0; i < p.iterations; ++i) {
        DenoisePassArgs &a = passes[i];
        a.step = 1u << i;
        a.k_albedo = 1.0f / (p.sigma_albedo * p.sigma_albedo);
        a.sigma_depth_step = p.sigma_depth * (float)a.step;
        a.normal_squarings = p.normal_power_log2;
        bool finite = positive_finite(a.k_albedo) && positive_finite(a.sigma_depth_step);
        if (vp) { a.k_luminance = k_luminance; a.variance_floor = vp->variance_floor; }
        else {
            const float sc = std::ldexp(p.sigma_color, -(int)i);                      // sigma_color * 2^-i, exact above the subnormals
            a.k_color = 1.0f / (sc * sc);
            finite = finite && positive_finite(a.k_color);
        }
        if (!finite) return fail(ctx, HRT_ERR_INVALID, "denoise parameters out of range: pass %u's constants are not finite", i);
    }
    return HRT_OK;
}

// variance == NULL: the plain filter.  Else a variance frame goes through the passes next to the colour, and into var_out if given.
// out == NULL (with `last`): the result stays in the context's frame the last pass wrote, which *last receives.
int run_filter(HrtContext *ctx, const float4 *color, const uint4 *guides, const float *variance, float4 *out, float *var_out,
               uint32_t width, uint32_t height, std::vector<DenoisePassArgs> &passes, hipStream_t s, const float4 **last = nullptr) {
    int rc = ensure_work(ctx, width * height, variance ? kFilterVariance : kFilter);
    if (rc != HRT_OK) return rc;
    const float4 *src = color;
    const float *vsrc = variance;
    const size_t n = passes.size();
    for (size_t i = 0; i < n; ++i) {
        DenoisePassArgs &a = passes[i];
        // the last pass writes what the caller gave -- unless that is its source (one pass in place), which goes through a frame of the
        // context's, as every other pass does
        auto target = [&](auto *given, const auto *source, auto *own) { return i + 1 < n || !given || given == source ? own : given; };
        float4 *dst = target(out, src, ctx->denoise.frame[i & 1]);
        float *vdst = variance ? target(var_out, vsrc, ctx->denoise.var[i & 1]) : nullptr;
        a.src = src; a.var_src = vsrc; a.guides = guides; a.dst = dst; a.var_dst = vdst; a.width = width; a.height = height;
        launch_denoise_pass(a, s);
        src = dst; vsrc = vdst;
    }
    if (last) *last = src;
    if (out && src != out) HIP_TRY(ctx, hipMemcpyAsync(out, src, sizeof(float4) * (size_t)width * height, hipMemcpyDeviceToDevice, s));
    if (var_out && vsrc != var_out) HIP_TRY(ctx, hipMemcpyAsync(var_out, vsrc, sizeof(float) * (size_t)width * height, hipMemcpyDeviceToDevice, s));
    HIP_TRY(ctx, hipGetLastError());
    return HRT_OK;
}

// guides == NULL: into the context's own (hrt_denoise_launch)
int run_guides(HrtContext *ctx, const HrtGlobalParams *h_params, const HrtRayGenParams *rg, uint4 *guides, hipStream_t s) {
    if (!ctx->have_records) return fail(ctx, HRT_ERR_STATE, "hrt_materials_set has not been called");
    Tlas *t;
    int rc = find_tlas(ctx, h_params->handle, t);
    if (rc != HRT_OK) return rc;
    const uint32_t n = rg->width * rg->height;
    rc = refresh_tables(ctx, h_params->handle, t, s);
    if (rc == HRT_OK) rc = ensure_work(ctx, n, kTrace);
    if (rc != HRT_OK) return rc;
    DenoiseWork &d = ctx->denoise;
    DenoiseRayArgs ra{};
    ra.rays = d.rays; ra.width = rg->width; ra.height = rg->height;
    std::memcpy(ra.center, &rg->cameraCenter, 12); std::memcpy(ra.U, &rg->cameraU, 12); std::memcpy(ra.V, &rg->cameraV, 12); std::memcpy(ra.W, &rg->cameraW, 12);
    launch_denoise_rays(ra, s);
    // The hit records: what the last hrt_render_launch captured (HRT_CTX_CAPTURE_PRIMARY) when that is the hits of exactly these rays --
    // the path kernel has just traced them as every pixel's first primary ray -- and a traversal of them otherwise.  Ordered after the
    // capturing launch by the stream, as the colour buffer is.
    if (capture_matches(ctx, h_params->handle, *t, rg)) {
        d.hit_tuvp = ctx->capture.tuvp; d.hit_inst = ctx->capture.inst;
        ctx->guide_passes_captured++;
    } else {
        ctx->capture.valid = false;      // (asked for another frame -- camera, size, tree -- than the one it holds, the context keeps no capture)
        rc = trace_records(ctx, *t, d.rays, n, kFloatZero, kFloatInfinity, false, d.tuvp, d.inst, d.fetch, s);      // Shader.cu:266
        if (rc != HRT_OK) return rc;
        d.hit_tuvp = d.tuvp; d.hit_inst = d.inst;
        ctx->guide_passes_traced++;
    }
    DenoiseGuideArgs ga{};
    ga.rays = d.rays; ga.tuvp = d.hit_tuvp; ga.inst = d.hit_inst; ga.n = n;
    ga.hitgroups = ctx->d_hitgroups; ga.inst_program = ctx->d_inst_program; ga.guides = guides ? guides : d.guides;
    launch_denoise_guides(ga, s);
    HIP_TRY(ctx, hipGetLastError());
    ctx->last_tlas = h_params->handle;
    return HRT_OK;
}

// hrt_denoise_accumulated_filter, and hrt_denoise_accumulated_launch after its guide pass: sums, totals and guides -> mean, variance of
// the mean and guides' (k_denoise_accumulated), the variance-guided filter over them, colorToFloat4 of its result.  The mean and its
// variance go into the frames the first pass reads and the second writes (frame[1], var[1]), guides' into the context's guide buffer;
// `guides` is the caller's, or the launch's in frame[0], which the first pass overwrites once the kernel has read it.
int accumulated_filter(HrtContext *ctx, const float4 *sum, const uint32_t *taken, const uint4 *guides, float4 *out, float4 *linear_out,
                       float *var_out, uint32_t width, uint32_t height, const HrtDenoiseVarianceParams &vp,
                       std::vector<DenoisePassArgs> &passes, hipStream_t s) {
    const uint32_t n = width * height;
    int rc = ensure_work(ctx, n, kFilterVariance);
    if (rc == HRT_OK) rc = ensure_work(ctx, n, kTrace);
    if (rc != HRT_OK) return rc;
    DenoiseWork &d = ctx->denoise;
    DenoiseAccumArgs aa{};
    aa.sum = sum; aa.taken = taken; aa.guides = guides;
    aa.mean = d.frame[1]; aa.variance = d.var[1]; aa.guides_out = d.guides;
    aa.width = width; aa.height = height; aa.believed = std::max(vp.history_min, 2u);
    launch_denoise_accumulated(aa, s);
    const float4 *filtered = nullptr;
    rc = run_filter(ctx, d.frame[1], d.guides, d.var[1], linear_out, var_out, width, height, passes, s, &filtered);
    if (rc != HRT_OK) return rc;
    launch_color_to_float4(linear_out ? linear_out : filtered, out, n, s);
    HIP_TRY(ctx, hipGetLastError());
    return HRT_OK;
}

// what both accumulated calls check before anything is enqueued (the context and the host pointers are the caller's to have checked)
int accumulated_checks(HrtContext *ctx, const void *d_sum, const void *d_taken, const void *d_out, const void *d_linear_out,
                       uint32_t width, uint32_t height, const HrtDenoiseParams *h_dparams, const HrtDenoiseVarianceParams &vp,
                       std::vector<DenoisePassArgs> &passes) {
    if (!d_sum || !d_taken || !d_out) return fail(ctx, HRT_ERR_INVALID, "accumulated denoise: d_sum, d_taken or d_out is NULL");
    if (d_out == d_sum || d_linear_out == d_sum) return fail(ctx, HRT_ERR_INVALID, "accumulated denoise: the sums are not written: d_out and d_linear_out must not be d_sum");
    if (d_linear_out && d_linear_out == d_out) return fail(ctx, HRT_ERR_INVALID, "accumulated denoise: d_linear_out is d_out");
    int rc = check_frame(ctx, width, height);
    if (rc == HRT_OK) rc = pass_constants(ctx, h_dparams, &vp, passes);
    return rc;
}

// the temporal parameters (NULL: the defaults); HRT_ERR_INVALID when one is out of range
int temporal_constants(HrtContext *ctx, const HrtDenoiseTemporalParams *h_tparams, HrtDenoiseTemporalParams &p) {
    hrt_denoise_temporal_default_params(&p);
    if (h_tparams) p = *h_tparams;
    if (!positive_finite(p.alpha_min) || p.alpha_min > 1.0f || p.max_history < 1 || p.max_history > 65536 ||
        !positive_finite(p.depth_tolerance) || p.reserved != 0)
        return fail(ctx, HRT_ERR_INVALID, "temporal denoise parameters out of range (0 < alpha_min <= 1, max_history 1..65536, depth_tolerance > 0 and finite, reserved 0)");
    return HRT_OK;
}

// the history's arrays for n pixels, and room for n_inst instances in the object -> world table of the set the next call writes; a new
// frame size forgets the history (and a pending link).  The last call's set keeps its table, sized for its own instance count: a linked
// call reads it through the link.  moments: the variance-guided mode's arrays too
int ensure_history(HrtContext *ctx, uint32_t n, uint32_t n_inst, bool moments) {
    DenoiseHistory &h = ctx->denoise_history;
    if (h.pixels != n) {
        free_denoise_history(ctx);
        for (DenoiseHistorySet &s : h.set) {
            HIP_TRY(ctx, hipMalloc((void **)&s.accum, sizeof(float4) * (size_t)n));
            HIP_TRY(ctx, hipMalloc((void **)&s.length, sizeof(float) * (size_t)n));
            HIP_TRY(ctx, hipMalloc((void **)&s.guides, sizeof(uint4) * (size_t)n));
            HIP_TRY(ctx, hipMalloc((void **)&s.id, sizeof(uint2) * (size_t)n));
        }
        HIP_TRY(ctx, hipMalloc((void **)&h.motion, sizeof(float2) * (size_t)n));
        h.pixels = n;
    }
    if (moments && !h.variance) {
        for (DenoiseHistorySet &s : h.set)
            if (!s.moments) HIP_TRY(ctx, hipMalloc((void **)&s.moments, sizeof(float2) * (size_t)n));
        HIP_TRY(ctx, hipMalloc((void **)&h.variance, sizeof(float) * (size_t)n));
    }
    const uint32_t need = std::max(n_inst, 1u);
    DenoiseHistorySet &next = h.set[h.cur ^ 1u];
    if (need > next.xf_capacity) {
        if (next.xf) (void)hipFree(next.xf);      // (hipFree waits for the device: the call that read this table two calls ago is done)
        next.xf = nullptr; next.xf_capacity = 0;
        HIP_TRY(ctx, hipMalloc((void **)&next.xf, sizeof(float) * 12 * (size_t)need));
        next.xf_capacity = need;
    }
    return HRT_OK;
}

// what the temporal and the variance-guided mode share: the guides of the frame into the history set this call writes, the reprojection
// and blend (with the luminance moments in the variance-guided mode), the object -> world table and camera kept for the next call.
// Leaves the history invalid and h.set[h.cur] the set just written: the caller enqueues its filter, then sets h.valid.
int run_temporal(HrtContext *ctx, const HrtGlobalParams *h_params, const HrtRayGenParams *h_raygen, const HrtDenoiseTemporalParams &tp,
                 DenoiseHistory::Mode mode, hipStream_t s) {
    const uint32_t width = h_raygen->width, height = h_raygen->height, n = width * height;
    const bool moments = mode == DenoiseHistory::kVariance;
    Tlas *t;
    int rc = find_tlas(ctx, h_params->handle, t);
    if (rc == HRT_OK) rc = ensure_history(ctx, n, t->n_instances, moments);
    if (rc != HRT_OK) return rc;
    DenoiseHistory &h = ctx->denoise_history;
    const bool same_frames = h.valid && h.mode == mode && h.width == width && h.height == height;
    // a pending link (hrt_denoise_temporal_rebind) to this call's TLAS: the history is blended through it.  Whatever this call is, the
    // link ends with it (below)
    const bool linked = same_frames && h.link_pending && h.link_tlas == h_params->handle && h.link_n == t->n_instances;
    const bool has_history = linked || (same_frames && h.tlas == h_params->handle && h.n_instances == t->n_instances);
    const DenoiseHistorySet &prev = h.set[h.cur];
    DenoiseHistorySet &next = h.set[h.cur ^ 1u];
    rc = run_guides(ctx, h_params, h_raygen, next.guides, s);
    if (rc != HRT_OK) return rc;
    const DenoiseWork &d = ctx->denoise;
    DenoiseTemporalArgs ta{};
    ta.rays = d.rays; ta.tuvp = d.hit_tuvp; ta.inst = d.hit_inst; ta.color = reinterpret_cast<const float4 *>(h_raygen->colorBuffer);
    ta.inst_inv = t->dev.d_inst_inv; ta.prev_xf = prev.xf;
    ta.prev_accum = prev.accum; ta.prev_length = prev.length; ta.prev_guides = prev.guides; ta.prev_id = prev.id;
    ta.accum = next.accum; ta.length = next.length; ta.id = next.id; ta.motion = h.motion;
    ta.width = width; ta.height = height; ta.has_history = has_history ? 1u : 0u;
    std::memcpy(ta.prev_center, prev.center, 12); std::memcpy(ta.prev_U, prev.U, 12); std::memcpy(ta.prev_V, prev.V, 12); std::memcpy(ta.prev_W, prev.W, 12);
    ta.alpha_min = tp.alpha_min; ta.max_history = (float)tp.max_history; ta.depth_tolerance = tp.depth_tolerance;
    if (moments) { ta.prev_moments = prev.moments; ta.moments = next.moments; }
    if (linked) {
        // (a link with no by-primitive entry is hrt_denoise_temporal_rebind's, whichever call made it)
        if (h.link_by_prim) launch_denoise_temporal_by_prim(DenoiseTemporalByPrimArgs{ta, h.link, h.link_verts}, s);
        else launch_denoise_temporal_linked(DenoiseTemporalLinkedArgs{ta, h.link}, s);
        ctx->denoise_history_rebinds++;
    } else launch_denoise_temporal(ta, s);
    HIP_TRY(ctx, hipMemcpyAsync(next.xf, t->dev.d_inst_xf, sizeof(float) * 12 * (size_t)std::max(t->n_instances, 1u), hipMemcpyDeviceToDevice, s));
    std::memcpy(next.center, &h_raygen->cameraCenter, 12); std::memcpy(next.U, &h_raygen->cameraU, 12);
    std::memcpy(next.V, &h_raygen->cameraV, 12); std::memcpy(next.W, &h_raygen->cameraW, 12);
    h.cur ^= 1u;
    h.drop_link();                    // (consumed or not.  The old BLASes it owned go here: ~Blas's hipFree waits for the kernel above)
    h.valid = false;                  // (until the caller has enqueued the filter as well)
    h.mode = mode;
    h.called = true;
    h.tlas = h_params->handle; h.width = width; h.height = height; h.n_instances = t->n_instances;
    return HRT_OK;
}

// hrt_denoise_temporal_launch, and with vp != NULL hrt_denoise_variance_launch: the checks, the reprojection and blend, the filter of the
// accumulated frame.  The variance-guided mode differs between the two by its variance kernel, whose result its filter takes.
int temporal_launch(HrtContext *ctx, const HrtGlobalParams *h_params, const HrtRayGenParams *h_raygen, const HrtDenoiseParams *h_dparams,
                    const HrtDenoiseTemporalParams *h_tparams, const HrtDenoiseVarianceParams *vp, HrtFloat4 *d_out, void *stream) {
    if (!ctx || !h_params || !h_raygen || !d_out) return HRT_ERR_INVALID;
    (void)hipSetDevice(ctx->device);
    if (!h_raygen->colorBuffer) return fail(ctx, HRT_ERR_INVALID, "RayGenParams.colorBuffer is NULL");
    const uint32_t width = h_raygen->width, height = h_raygen->height;
    int rc = check_frame(ctx, width, height);
    std::vector<DenoisePassArgs> passes;
    HrtDenoiseTemporalParams tp;
    if (rc == HRT_OK) rc = pass_constants(ctx, h_dparams, vp, passes);
    if (rc == HRT_OK) rc = temporal_constants(ctx, h_tparams, tp);
    if (rc != HRT_OK) return rc;
    const hipStream_t s = (hipStream_t)stream;
    DenoiseHistory &h = ctx->denoise_history;
    rc = run_temporal(ctx, h_params, h_raygen, tp, vp ? DenoiseHistory::kVariance : DenoiseHistory::kTemporal, s);
    if (rc != HRT_OK) return rc;
    const DenoiseHistorySet &next = h.set[h.cur];
    if (vp) {
        DenoiseVarianceArgs va{};
        va.moments = next.moments; va.length = next.length; va.id = next.id; va.variance = h.variance;
        va.width = width; va.height = height; va.history_min = (float)vp->history_min;
        launch_denoise_variance(va, s);
        h.variance_called = true;
        h.variance_set = h.cur;
    }
    rc = run_filter(ctx, next.accum, next.guides, vp ? h.variance : nullptr, reinterpret_cast<float4 *>(d_out), nullptr, width, height, passes, s);
    if (rc != HRT_OK) return rc;
    h.valid = true;
    return HRT_OK;
}

// hrt_denoise_temporal_rebind, and with by_primitive hrt_denoise_temporal_rebind_geometry (`name`: whose messages these are): the link
// from the history's TLAS to next_tlas.  An instance whose BLAS handle differs from its predecessor's has no history in the first; in
// the second it is linked by primitive where both BLASes are triangle BLASes of the same, non-zero primitive count, decided here from
// the BLAS each TLAS keeps per instance (Tlas::blas_refs, filled by every build path: build_tlas_fresh).
int rebind_history(HrtContext *ctx, const char *name, bool by_primitive, HrtTraversable next_tlas, const uint32_t *h_prev_instance,
                   uint32_t n_instances, void *stream) {
    if (!ctx) return HRT_ERR_INVALID;
    (void)hipSetDevice(ctx->device);
    DenoiseHistory &h = ctx->denoise_history;
    std::vector<uint32_t> link;
    std::vector<const float *> verts;
    std::vector<std::shared_ptr<Blas>> owned;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        const auto next = ctx->tlas.find(next_tlas);
        if (next == ctx->tlas.end()) return fail(ctx, HRT_ERR_INVALID, "%s: 0x%llx is not a TLAS", name, (unsigned long long)next_tlas);
        const Tlas &tn = *next->second;
        if (n_instances != tn.n_instances)
            return fail(ctx, HRT_ERR_INVALID, "%s: n_instances %u is not the TLAS's %u", name, n_instances, tn.n_instances);
        const auto prev = ctx->tlas.find(h.tlas);
        if (!h.valid || prev == ctx->tlas.end()) {      // nothing to hand over: the next call starts afresh, as without this one
            h.drop_link();
            return HRT_OK;
        }
        const Tlas &tp = *prev->second;
        link.assign(std::max(n_instances, 1u), HRT_NO_INSTANCE);
        if (by_primitive) verts.assign(link.size(), nullptr);
        for (uint32_t i = 0; i < n_instances; ++i) {
            uint32_t pi = h_prev_instance ? h_prev_instance[i] : (i < tp.n_instances ? i : HRT_NO_INSTANCE);
            if (pi != HRT_NO_INSTANCE && pi >= tp.n_instances)
                return fail(ctx, HRT_ERR_INVALID, "%s: h_prev_instance[%u] = %u, the history's TLAS has %u instances", name, i, pi, tp.n_instances);
            if (pi != HRT_NO_INSTANCE && tn.sig_handle[i] != tp.sig_handle[pi]) {
                // another geometry: its primitive ids mean nothing (such a body starts afresh) unless the caller has declared the
                // triangles the same ones, which two triangle BLASes of one count can be
                const std::shared_ptr<Blas> &bn = tn.blas_refs[i], &bp = tp.blas_refs[pi];
                const bool same_triangles = by_primitive && bn && bp && bn->kind == kPrimKindTriangle && bp->kind == kPrimKindTriangle &&
                                            bn->n_prims != 0 && bn->n_prims == bp->n_prims && bp->d_verts;
                if (same_triangles) { verts[i] = bp->d_verts; owned.push_back(bp); }
                else pi = HRT_NO_INSTANCE;
            }
            link[i] = pi;
        }
    }
    h.drop_link();                             // (replaced: a failed upload leaves none)
    if (link.size() > h.link_capacity) {
        if (h.link) (void)hipFree(h.link);
        h.link = nullptr; h.link_capacity = 0;
        HIP_TRY(ctx, hipMalloc((void **)&h.link, sizeof(uint32_t) * link.size()));
        h.link_capacity = (uint32_t)link.size();
    }
    const hipStream_t s = (hipStream_t)stream;
    h.h_link.swap(link);
    HIP_TRY(ctx, hipMemcpyAsync(h.link, h.h_link.data(), sizeof(uint32_t) * h.h_link.size(), hipMemcpyHostToDevice, s));
    if (!owned.empty()) {
        if (verts.size() > h.link_verts_capacity) {
            if (h.link_verts) (void)hipFree((void *)h.link_verts);
            h.link_verts = nullptr; h.link_verts_capacity = 0;
            HIP_TRY(ctx, hipMalloc((void **)&h.link_verts, sizeof(const float *) * verts.size()));
            h.link_verts_capacity = (uint32_t)verts.size();
        }
        h.h_link_verts.swap(verts);
        HIP_TRY(ctx, hipMemcpyAsync(h.link_verts, h.h_link_verts.data(), sizeof(const float *) * h.h_link_verts.size(), hipMemcpyHostToDevice, s));
        // The link owns the predecessors' BLASes from here until it is consumed, replaced or dropped (DenoiseHistory::drop_link).  The
        // last reference's ~Blas runs hipFree, which waits for the device: a kernel that reads these vertices has finished by then.
        h.link_by_prim = (uint32_t)owned.size();
        h.link_blas.swap(owned);
        ctx->denoise_by_primitive_links += h.link_by_prim;
    }
    h.link_pending = true; h.link_tlas = next_tlas; h.link_n = n_instances;
    return HRT_OK;
}

}  // namespace
}  // namespace hrt


extern "C" {

int hrt_denoise_default_params(HrtDenoiseParams *out) {
    if (!out) return HRT_ERR_INVALID;
    // (profiles/r05_denoise.txt: the sweep these come from)
    *out = HrtDenoiseParams{5u, 0.5f, 0.1f, 0.02f, 3u, 0u};
    return HRT_OK;
}

int hrt_denoise_guides(HrtContext *ctx, const HrtGlobalParams *h_params, const HrtRayGenParams *h_raygen, HrtDenoiseGuide *d_guides, void *stream) {
    if (!ctx || !h_params || !h_raygen || !d_guides) return HRT_ERR_INVALID;
    (void)hipSetDevice(ctx->device);
    int rc = check_frame(ctx, h_raygen->width, h_raygen->height);
    if (rc != HRT_OK) return rc;
    return run_guides(ctx, h_params, h_raygen, reinterpret_cast<uint4 *>(d_guides), (hipStream_t)stream);
}

int hrt_denoise_filter(HrtContext *ctx, const HrtFloat4 *d_color, const HrtDenoiseGuide *d_guides, HrtFloat4 *d_out,
                       uint32_t width, uint32_t height, const HrtDenoiseParams *h_dparams, void *stream) {
    if (!ctx || !d_color || !d_guides || !d_out) return HRT_ERR_INVALID;
    (void)hipSetDevice(ctx->device);
    int rc = check_frame(ctx, width, height);
    std::vector<DenoisePassArgs> passes;
    if (rc == HRT_OK) rc = pass_constants(ctx, h_dparams, nullptr, passes);
    if (rc != HRT_OK) return rc;
    return run_filter(ctx, reinterpret_cast<const float4 *>(d_color), reinterpret_cast<const uint4 *>(d_guides), nullptr,
                      reinterpret_cast<float4 *>(d_out), nullptr, width, height, passes, (hipStream_t)stream);
}

int hrt_denoise_launch(HrtContext *ctx, const HrtGlobalParams *h_params, const HrtRayGenParams *h_raygen, const HrtDenoiseParams *h_dparams,
                       HrtFloat4 *d_out, void *stream) {
    if (!ctx || !h_params || !h_raygen || !d_out) return HRT_ERR_INVALID;
    (void)hipSetDevice(ctx->device);
    if (!h_raygen->colorBuffer) return fail(ctx, HRT_ERR_INVALID, "RayGenParams.colorBuffer is NULL");
    int rc = check_frame(ctx, h_raygen->width, h_raygen->height);
    std::vector<DenoisePassArgs> passes;
    if (rc == HRT_OK) rc = pass_constants(ctx, h_dparams, nullptr, passes);
    const hipStream_t s = (hipStream_t)stream;
    if (rc == HRT_OK) rc = run_guides(ctx, h_params, h_raygen, nullptr, s);
    if (rc != HRT_OK) return rc;
    return run_filter(ctx, reinterpret_cast<const float4 *>(h_raygen->colorBuffer), ctx->denoise.guides, nullptr, reinterpret_cast<float4 *>(d_out),
                      nullptr, h_raygen->width, h_raygen->height, passes, s);
}

int hrt_denoise_temporal_default_params(HrtDenoiseTemporalParams *out) {
    if (!out) return HRT_ERR_INVALID;
    // (profiles/r07_denoise_temporal.txt: the sweep these come from)
    *out = HrtDenoiseTemporalParams{0.8f, 32u, 0.02f, 0u};
    return HRT_OK;
}

int hrt_denoise_temporal_launch(HrtContext *ctx, const HrtGlobalParams *h_params, const HrtRayGenParams *h_raygen, const HrtDenoiseParams *h_dparams,
                                const HrtDenoiseTemporalParams *h_tparams, HrtFloat4 *d_out, void *stream) {
    return temporal_launch(ctx, h_params, h_raygen, h_dparams, h_tparams, nullptr, d_out, stream);
}

int hrt_denoise_temporal_reset(HrtContext *ctx) {
    if (!ctx) return HRT_ERR_INVALID;
    ctx->denoise_history.valid = false;
    ctx->denoise_history.drop_link();
    return HRT_OK;
}

int hrt_denoise_temporal_rebind(HrtContext *ctx, HrtTraversable next_tlas, const uint32_t *h_prev_instance, uint32_t n_instances, void *stream) {
    return rebind_history(ctx, "hrt_denoise_temporal_rebind", false, next_tlas, h_prev_instance, n_instances, stream);
}

int hrt_denoise_temporal_rebind_geometry(HrtContext *ctx, HrtTraversable next_tlas, const uint32_t *h_prev_instance, uint32_t n_instances, void *stream) {
    return rebind_history(ctx, "hrt_denoise_temporal_rebind_geometry", true, next_tlas, h_prev_instance, n_instances, stream);
}

int hrt_debug_denoise_temporal_state(HrtContext *ctx, HrtFloat4 *d_accum, float *d_length, float *d_motion, void *stream) {
    if (!ctx) return HRT_ERR_INVALID;
    (void)hipSetDevice(ctx->device);
    const DenoiseHistory &h = ctx->denoise_history;
    if (!h.called) return fail(ctx, HRT_ERR_STATE, "hrt_denoise_temporal_launch has not been called");
    const hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)h.width * h.height;
    const DenoiseHistorySet &last = h.set[h.cur];
    if (d_accum) HIP_TRY(ctx, hipMemcpyAsync(d_accum, last.accum, sizeof(float4) * n, hipMemcpyDeviceToDevice, s));
    if (d_length) HIP_TRY(ctx, hipMemcpyAsync(d_length, last.length, sizeof(float) * n, hipMemcpyDeviceToDevice, s));
    if (d_motion) HIP_TRY(ctx, hipMemcpyAsync(d_motion, h.motion, sizeof(float2) * n, hipMemcpyDeviceToDevice, s));
    return HRT_OK;
}

int hrt_denoise_variance_default_params(HrtDenoiseVarianceParams *out) {
    if (!out) return HRT_ERR_INVALID;
    // (profiles/r12_denoise_variance.txt: the four-case sweep that picks sigma_luminance 4.0 and history_min 4)
    *out = HrtDenoiseVarianceParams{4.0f, 4u, 1e-6f, 0u};
    return HRT_OK;
}

int hrt_denoise_filter_variance(HrtContext *ctx, const HrtFloat4 *d_color, const HrtDenoiseGuide *d_guides, const float *d_variance,
                                HrtFloat4 *d_out, float *d_var_out, uint32_t width, uint32_t height, const HrtDenoiseParams *h_dparams,
                                const HrtDenoiseVarianceParams *h_vparams, void *stream) {
    if (!ctx || !d_color || !d_guides || !d_variance || !d_out) return HRT_ERR_INVALID;
    (void)hipSetDevice(ctx->device);
    int rc = check_frame(ctx, width, height);
    std::vector<DenoisePassArgs> passes;
    const HrtDenoiseVarianceParams vp = variance_params(h_vparams);
    if (rc == HRT_OK) rc = pass_constants(ctx, h_dparams, &vp, passes);
    if (rc != HRT_OK) return rc;
    return run_filter(ctx, reinterpret_cast<const float4 *>(d_color), reinterpret_cast<const uint4 *>(d_guides), d_variance,
                      reinterpret_cast<float4 *>(d_out), d_var_out, width, height, passes, (hipStream_t)stream);
}

int hrt_denoise_variance_launch(HrtContext *ctx, const HrtGlobalParams *h_params, const HrtRayGenParams *h_raygen, const HrtDenoiseParams *h_dparams,
                                const HrtDenoiseTemporalParams *h_tparams, const HrtDenoiseVarianceParams *h_vparams, HrtFloat4 *d_out,
                                void *stream) {
    const HrtDenoiseVarianceParams vp = variance_params(h_vparams);
    return temporal_launch(ctx, h_params, h_raygen, h_dparams, h_tparams, &vp, d_out, stream);
}

int hrt_denoise_accumulated_filter(HrtContext *ctx, const HrtFloat4 *d_sum, const uint32_t *d_taken, const HrtDenoiseGuide *d_guides,
                                   HrtFloat4 *d_out, HrtFloat4 *d_linear_out, float *d_var_out, uint32_t width, uint32_t height,
                                   const HrtDenoiseParams *h_dparams, const HrtDenoiseVarianceParams *h_vparams, void *stream) {
    if (!ctx) return HRT_ERR_INVALID;
    (void)hipSetDevice(ctx->device);
    if (!d_guides) return fail(ctx, HRT_ERR_INVALID, "accumulated denoise: d_guides is NULL");
    std::vector<DenoisePassArgs> passes;
    const HrtDenoiseVarianceParams vp = variance_params(h_vparams);
    int rc = accumulated_checks(ctx, d_sum, d_taken, d_out, d_linear_out, width, height, h_dparams, vp, passes);
    if (rc != HRT_OK) return rc;
    return accumulated_filter(ctx, reinterpret_cast<const float4 *>(d_sum), d_taken, reinterpret_cast<const uint4 *>(d_guides),
                              reinterpret_cast<float4 *>(d_out), reinterpret_cast<float4 *>(d_linear_out), d_var_out, width, height, vp,
                              passes, (hipStream_t)stream);
}

int hrt_denoise_accumulated_launch(HrtContext *ctx, const HrtGlobalParams *h_params, const HrtRayGenParams *h_raygen, const HrtFloat4 *d_sum,
                                   const uint32_t *d_taken, const HrtDenoiseParams *h_dparams, const HrtDenoiseVarianceParams *h_vparams,
                                   HrtFloat4 *d_out, void *stream) {
    if (!ctx || !h_params || !h_raygen) return HRT_ERR_INVALID;
    (void)hipSetDevice(ctx->device);
    const uint32_t width = h_raygen->width, height = h_raygen->height;
    std::vector<DenoisePassArgs> passes;
    const HrtDenoiseVarianceParams vp = variance_params(h_vparams);
    int rc = accumulated_checks(ctx, d_sum, d_taken, d_out, nullptr, width, height, h_dparams, vp, passes);
    // the frames first: the guides of this frame go into one of them (accumulated_filter), which a larger frame would free again
    if (rc == HRT_OK) rc = ensure_work(ctx, width * height, kFilterVariance);
    if (rc != HRT_OK) return rc;
    const hipStream_t s = (hipStream_t)stream;
    uint4 *guides = reinterpret_cast<uint4 *>(ctx->denoise.frame[0]);
    rc = run_guides(ctx, h_params, h_raygen, guides, s);
    if (rc != HRT_OK) return rc;
    return accumulated_filter(ctx, reinterpret_cast<const float4 *>(d_sum), d_taken, guides, reinterpret_cast<float4 *>(d_out), nullptr, nullptr,
                              width, height, vp, passes, s);
}

int hrt_debug_denoise_variance_state(HrtContext *ctx, float *d_moments, float *d_variance, void *stream) {
    if (!ctx) return HRT_ERR_INVALID;
    (void)hipSetDevice(ctx->device);
    const DenoiseHistory &h = ctx->denoise_history;
    if (!h.variance_called) return fail(ctx, HRT_ERR_STATE, "hrt_denoise_variance_launch has not been called");
    const hipStream_t s = (hipStream_t)stream;
    const size_t n = h.pixels;
    if (d_moments) HIP_TRY(ctx, hipMemcpyAsync(d_moments, h.set[h.variance_set].moments, sizeof(float2) * n, hipMemcpyDeviceToDevice, s));
    if (d_variance) HIP_TRY(ctx, hipMemcpyAsync(d_variance, h.variance, sizeof(float) * n, hipMemcpyDeviceToDevice, s));
    return HRT_OK;
}

}  // extern "C"
