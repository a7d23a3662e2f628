// path_plan.h -- what render_fused (hrt_api.cpp) decides before it launches anything, as plain host code: the block schedule of a launch, the
// plan of a render (the tree's kernel, the grid, the primary-hit cache, the cost-order probe, the capture, the sample-block gate) and the plan
// of each of its launches (the cut into launches of HRT_FUSED_MAX_SPP, the schedule, the block fields of PathArgs, the kernel).  Values in,
// values out: no context, no tree, no device, nothing allocated -- tests/test_render_plan_cpu.py runs it over a table of inputs, and every
// launch it plans is one that path_launch_admitted (device_types.h) admits.
#pragma once
#include "device_types.h"

#include <algorithm>

namespace hrt {

// ---- sample blocks: the schedule of one path-kernel launch (device_types.h: PathArgs, block_first, block_ends) ----
struct SampleSchedule { uint32_t k_big = 0, k_min = 0, taper_end = 0; bool tapered = false; uint32_t passes = 0; };
inline uint32_t schedule_first(const SampleSchedule &sc, uint32_t pass) { return block_first(sc.k_big, sc.k_min, sc.taper_end, sc.tapered, pass); }
// passes: the first pass that would start at or behind the launch's last sample (block_first grows with the pass, by 1 at least)
inline void count_passes(SampleSchedule &sc, uint32_t spp) {
    uint32_t lo = 0, hi = spp;
    while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2u; if (schedule_first(sc, mid) >= spp) hi = mid; else lo = mid + 1u; }
    sc.passes = lo;
}
inline SampleSchedule uniform_schedule(uint32_t spp, uint32_t k) {
    SampleSchedule sc; sc.k_big = sc.k_min = k; sc.passes = (uint32_t)(((uint64_t)spp + k - 1u) / k); return sc;
}
// The tapered schedule of a launch of spp samples: blocks of K_big = `big` (no more than the launch has samples) up to T, then the sizes
// K_big / 2, K_big / 4, ... K_min, K_min, which fill the window [T, T + K_big), and K_min behind it.  T + K_big is the last multiple of
// K_big the launch reaches: the halvings are its last whole window, what is left behind them (less than K_big samples) goes in blocks
// of K_min, and the launch's last block ends with its samples, short if need be -- every launch ends on K_min, with K_big / K_min - 1
// more hand-overs at the most than it takes to get there.  Powers of two that never grow, so every boundary is a multiple of the block
// that ends there.  256 samples, 64 : 8 -- 64, 64, 64, 32, 16, 8, 8.  (32-bit arithmetic: for launches of spp x big below 2^31, taper_fits.)
inline bool taper_fits(uint32_t spp, uint32_t big) { return (uint64_t)spp * big < (1ull << 31); }
inline SampleSchedule sample_schedule(uint32_t spp, uint32_t big, uint32_t min) {
    SampleSchedule sc; sc.tapered = true;
    sc.k_big = big; while (sc.k_big > 1u && sc.k_big > spp) sc.k_big >>= 1;
    sc.k_min = std::min(min, sc.k_big);
    sc.taper_end = spp / sc.k_big * sc.k_big;
    count_passes(sc, spp);
    return sc;
}

// ---- the tree's kernel and the grid: what every launch over a tile's pixels shares (render_fused, hrt_render_accumulate, trace_records) ----
// The path kernel of a tree: k_fused, its instanced form for two-level trees, or -- for a tree outside k_fused's limits -- round 1's
// fused kernel, counted in fused_fallback_launches.  blocks_per_cu: one-wave workgroups per CU at most.
struct PathKernelChoice { PathKernel kernel; uint32_t blocks_per_cu; };
inline PathKernelChoice tree_path_kernel(bool fits_fused, bool two_level, int fused_blocks_per_cu) {
    const uint32_t knob = (uint32_t)fused_blocks_per_cu;
    if (!fits_fused) return {PathKernel::Round1, knob};
    if (two_level) return {PathKernel::FusedInstanced, std::min<uint32_t>(knob, (uint32_t)kFusedInstancedBlocksPerCu)};
    return {PathKernel::Fused, std::min<uint32_t>(knob, (uint32_t)kFusedBlocksPerCu)};
}
// Waves per CU: a lane runs its pixel's samples one after the other, so a small tile (the multi-GPU split) ends
// with its slowest pixels; about 1.4 pixels per lane lets the lanes that drew cheap pixels take a second one
// while fewer waves share each SIMD (measured, profiles/r01_sweep_tile_waves.txt: 1/8 of the C4 frame takes
// 172 ms on 12 waves per CU, 210 ms on 16).  A full frame has many pixels per lane and keeps the maximum: 16 waves
// per CU = 4 per SIMD for k_fused (122 VGPRs, nothing spilled: 3120 Mrays/s on C4; compiled for 5 waves it spills 95
// registers around the shading: 2560), 20 = 5 per SIMD for round 1's kernel (96 VGPRs, a few spills: 2905).
// The grid: one-wave workgroups, blocks_per_cu of them per CU at most.
inline uint32_t fused_render_grid(int n_cu, bool blocks_auto, uint32_t blocks_per_cu, uint32_t n) {
    if (blocks_auto) {
        const uint32_t fit = (uint32_t)((10ull * n + 14ull * 64ull * (uint64_t)n_cu - 1ull) / (14ull * 64ull * (uint64_t)n_cu));
        blocks_per_cu = std::min(blocks_per_cu, std::max(fit, 4u));
    }
    return std::min<uint32_t>((uint32_t)n_cu * blocks_per_cu, (n + 63u) / 64u);
}

// ---- the plan ----
// Everything render_fused's decisions read, by value.
struct RenderPlanInput {
    int n_cu;
    // the tree: inside k_fused's limits; two-level; its instances; spheres; it has records and nodes, so a leaf_parent table can exist (ensure_leaf_parent)
    bool fits_fused, two_level; uint32_t n_instances; bool has_spheres, has_records;
    // the tile: its pixels, whether they are every row of the frame, and the render's samples
    uint32_t n; bool full_frame; uint32_t spp;
    // the context: HRT_CTX_REUSE_PRIMARY / HRT_REUSE_PRIMARY, HRT_CTX_CAPTURE_PRIMARY / HRT_CAPTURE_PRIMARY, and the knobs (hrt_internal.hpp: HrtContext)
    bool reuse_primary, capture_primary;
    int fused_blocks_per_cu; bool traverse_blocks_auto; int fused_fetch_chunk;
    int fused_lpt, sample_block, taper_big, taper_min; bool taper_forced;
    int fused_max_spp, seed_primary;
    PathKnobs knobs;
};
struct RenderPlan {
    PathKernel tree_kernel; bool round1;      // (round 1's kernel: a fallback launch, and round 1's postponement)
    uint32_t blocks_per_cu, grid, n_slices;
    bool primary_cache;                       // the lanes' slots for their pixels' primary hits: two float4 per lane of the grid
    uint32_t probe_spp;                       // samples of the cost-order probe launch, 0: none
    bool capture;                             // the render's first launch runs k_path_capture
    bool want_blocks, forced;                 // the sample-block gate: launches of this render may go in blocks; whatever their length
};
inline RenderPlan plan_fused_render(const RenderPlanInput &in) {
    RenderPlan r{};
    const PathKernelChoice pk = tree_path_kernel(in.fits_fused, in.two_level, in.fused_blocks_per_cu);
    r.tree_kernel = pk.kernel; r.round1 = pk.kernel == PathKernel::Round1; r.blocks_per_cu = pk.blocks_per_cu;
    const bool lean = !r.round1;
    r.grid = fused_render_grid(in.n_cu, in.traverse_blocks_auto, pk.blocks_per_cu, in.n);
    const uint32_t chunk = (uint32_t)in.fused_fetch_chunk;
    r.n_slices = (in.n + chunk - 1u) / chunk;
    // HRT_CTX_REUSE_PRIMARY: the lanes' slots for their pixels' primary hits (k_fused<.., REUSE>, fused.hip)
    r.primary_cache = lean && in.spp > 1u && in.reuse_primary;
    // Longest-processing-time-first: a pixel's samples run one after the other in one lane, so a render ends with
    // whatever pixels were started last.  For renders of many samples the first sample is a probe launch of its own
    // that records how long each slice's pixels took over their sample; the slices are then handed out slowest first,
    // and the render ends on pixels whose paths leave the scene at once.  (The image does not depend on the order.)
    // Worth it when a lane gets only a few pixels (the tiles of the multi-GPU split: 1/4 of the C4 frame 238 -> 219 ms);
    // a full frame has ~8 pixels per lane and keeps its single launch.  Its tail is not small either -- from the first wave that finds
    // the tile used up to the end of the kernel is 22 % of the kernel's time on C4, and 9 % of the kernel's lane-slots stand idle in it, at 64
    // spp as at 256 (tools/tail_profile.py, profiles/r13_sample_blocks.txt) -- but it is sample blocks, below, that shorten it.
    const bool lpt = in.fused_lpt && in.spp >= 16u && r.n_slices >= 4096u && (uint64_t)in.n < 4ull * 64ull * (uint64_t)r.grid;
    if (lpt) r.probe_spp = (uint32_t)std::min<int>(std::max(in.fused_lpt, 1), (int)in.spp / 4);
    // HRT_CTX_CAPTURE_PRIMARY: a launch that would run plain k_fused<S, I, false> over the whole frame runs k_path_capture instead, which
    // also leaves every pixel's primary hit in the context (PrimaryCapture).  Not with the primary-hit cache, the cost-order probe or
    // sample blocks (choose_path_launch), not on round 1's kernel: frames of many samples, where one more traversal for the guides does not count.
    r.capture = lean && !r.primary_cache && in.full_frame && in.capture_primary && !lpt;
    // Sample blocks (path_lane.h): a lane gives its pixel back after K samples and the slices go round pass by pass, so only the last K
    // samples of a frame run in a draining GPU.  k_fused's one-level kernels without the primary-hit cache (which wants a pixel's samples in
    // one lane) and without the cost order (which keeps precedence on the small tiles where it applies).  `auto`: only where an item's
    // predecessor was handed out at least three fills of the machine before it -- the tile has four slices per slice in flight -- so that
    // the hand-over never has to wait.
    // Never, forced or not, on a grid of fewer waves than slice counters: a wave keeps an item that is not ready until it is, and takes
    // from another counter only once its own is drained, so every counter needs a wave whose home it is -- otherwise the predecessor of
    // a held item can sit behind a counter that nobody visits and the wave waits for ever (the argument: fused_body.h; the rule refuses
    // such a launch too, path_launch_admitted).
    if (pk.kernel == PathKernel::Fused && !r.primary_cache && !lpt && in.sample_block != 0 && r.grid >= kFetchShards) {
        r.forced = in.sample_block > 0 || (in.taper_big > 0 && in.taper_forced);
        r.want_blocks = r.forced || (uint64_t)r.n_slices * chunk >= 4ull * 64ull * (uint64_t)r.grid;
    }
    return r;
}

// The regeneration threshold of one launch (TraverseArgs::refill_threshold: the lanes that are idle before a wave regenerates).  The render's
// is the context's 20, or 12 on a two-level tree (hrt_api.cpp: fused_render_args); a launch of k_path_direct gets kDirectRefillThreshold
// while nobody has set HRT_REFILL_THRESHOLD (`refill_auto`).  That kernel keeps the short rays out of the waiting pool -- a repeat primary
// ray with a record never waits, a primary miss takes its block -- so what waits are bounces, and a regeneration is worth waiting longer
// for: on C4 26 is 0.7 % above 20, every run of five alternating ones above 20's median plus twice its range, and C3 stays level; 32 is
// another 0.4 % on C4 and 0.7 % under 20 on C3, whose paths are shorter (profiles/r33_primary_miss_block.txt section 6).  Every other
// kernel keeps the render's value.
constexpr int kDirectRefillThreshold = 26;
inline int launch_refill_threshold(PathKernel kernel, int render_threshold, bool refill_auto) {
    return refill_auto && kernel == PathKernel::Direct ? kDirectRefillThreshold : render_threshold;
}

// One launch of the render, after done_spp samples (the probe's included).
struct LaunchPlan {
    uint32_t now, continue_sum;               // PathArgs::spp, continue_sum
    SampleSchedule sc; bool blocks;           // the schedule, and whether the launch goes in blocks (else every block field of PathArgs is 0 but the three divisors)
    uint32_t sample_block, block_magic, block_min, block_taper_end, block_slices, block_slices_magic, block_chunk_magic, block_items;
    PathKernel kernel; bool wants_table;      // the launch's kernel; it reads the tree's leaf_parent table (k_path_restart and above), to be made before the launch
};
inline LaunchPlan plan_fused_launch(const RenderPlan &r, const RenderPlanInput &in, uint32_t done_spp) {
    LaunchPlan l{};
    // very long renders are cut into launches of at most fused_max_spp samples (a launch should stay in the
    // range of seconds); the RNG states and the running sums carry over, so the result is the same bits
    const uint32_t now = std::min<uint32_t>(in.spp - done_spp, (uint32_t)in.fused_max_spp), chunk = (uint32_t)in.fused_fetch_chunk;
    l.now = now; l.continue_sum = done_spp > 0 ? 1u : 0u;
    // What a launch of `now` samples is cut into is a schedule (device_types.h: block_first): HRT_SAMPLE_BLOCK=N forces uniform blocks of N;
    // `auto` takes HRT_SAMPLE_TAPER's -- large blocks while the machine is full, so that a pixel changes hands seldom, halved down to small
    // ones over the last samples, so that the frame ends on a short tail (sample_schedule above) -- or, with HRT_SAMPLE_TAPER=0, uniform
    // blocks of kSampleBlockAuto.
    SampleSchedule &sc = l.sc;
    if (r.want_blocks) sc = in.sample_block > 0 ? uniform_schedule(now, (uint32_t)in.sample_block) : in.taper_big > 0 && taper_fits(now, (uint32_t)in.taper_big) ? sample_schedule(now, (uint32_t)in.taper_big, (uint32_t)in.taper_min) : uniform_schedule(now, (uint32_t)kSampleBlockAuto);
    // this launch in blocks: at least two of them (`auto`: 2 kSampleBlockAuto samples), and the counters' numbers, in pixels, within 32 bits
    const bool blocks = sc.passes >= 2u && (r.forced || now >= 2u * (uint32_t)kSampleBlockAuto) && (uint64_t)sc.passes * r.n_slices * chunk < (1ull << 32);
    auto magic = [](uint32_t d) { return d ? (uint32_t)std::min<uint64_t>((1ull << 32) / d, 0xffffffffull) : 0u; };      // (an empty tile has no slices)
    l.blocks = blocks;
    l.sample_block = blocks ? sc.k_big : 0u; l.block_magic = blocks && !sc.tapered ? magic(sc.k_big) : 0u;
    l.block_min = blocks && sc.tapered ? sc.k_min : 0u; l.block_taper_end = blocks && sc.tapered ? sc.taper_end : 0u;
    l.block_slices = r.n_slices; l.block_slices_magic = magic(r.n_slices); l.block_chunk_magic = magic(chunk);
    l.block_items = blocks ? (uint32_t)((uint64_t)sc.passes * r.n_slices) : 0u;
    // Which kernel (device_types.h: choose_path_launch, which says what decides it), chosen once: a tree with records and nodes has its
    // leaf_parent table by the time the launch runs -- from k_path_restart on a launch wants it, and render_fused makes it the first time --
    // and a tree without records has none, so its launch stays k_path_one's.
    const PathScene scene{!in.two_level, in.n_instances, in.has_spheres, nullptr};
    l.kernel = choose_path_launch(r.tree_kernel, r.capture, blocks, done_spp, in.seed_primary, in.knobs, scene, in.has_records);
    l.wants_table = path_ladder_rung(l.kernel) >= 2;
    return l;
}

}  // namespace hrt
