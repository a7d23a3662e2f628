// hrt_mem.cpp -- the device memory a context keeps between builds: the arenas the device builds work in (scratch_*) and the pool the
// trees' blocks come from and go back to (pool_*).  They share nothing with tree building (hrt_accel.cpp) but the context.
#include "hrt_internal.hpp"

namespace hrt {

// Out of memory: what the context keeps for later -- the trees' cached blocks AND the builds' arenas (up to eight) -- goes back to the
// runtime; the caller then asks once more.
static void reclaim_kept_memory(HrtContext *ctx) {
    (void)hipGetLastError();
    pool_drain(ctx);
    std::vector<ScratchArena> arenas;
    { std::lock_guard<std::mutex> lk(ctx->scratch_mu); arenas.swap(ctx->scratch_free); }
    for (const ScratchArena &a : arenas) (void)hipFree(a.p);
}

// Working memory of the device builds.  A build takes the smallest free arena that is large enough (or allocates one, a quarter
// larger than asked for) and gives it back when it is done; the context keeps up to eight of them, so loader threads building
// side by side each find one.  Without this a 1500-triangle rebuild spent most of its 2 ms in hipMalloc / hipFree.
ScratchArena scratch_acquire(HrtContext *ctx, size_t bytes) {
    {
        std::lock_guard<std::mutex> lk(ctx->scratch_mu);
        int best = -1;
        for (int i = 0; i < (int)ctx->scratch_free.size(); ++i)
            if (ctx->scratch_free[i].bytes >= bytes && (best < 0 || ctx->scratch_free[i].bytes < ctx->scratch_free[best].bytes)) best = i;
        if (best >= 0) { const ScratchArena a = ctx->scratch_free[best]; ctx->scratch_free.erase(ctx->scratch_free.begin() + best); return a; }
    }
    ScratchArena a;
    a.bytes = bytes + bytes / 4 + 4096;
    if (hipMalloc(&a.p, a.bytes) != hipSuccess) {
        // (the other arenas were each too small for this request or one would have been taken above); then exactly what was asked for
        reclaim_kept_memory(ctx);
        a.bytes = bytes;
        if (hipMalloc(&a.p, a.bytes) != hipSuccess) { (void)hipGetLastError(); a = ScratchArena(); }
    }
    return a;
}
void scratch_release(HrtContext *ctx, ScratchArena a) {
    if (!a.p) return;
    if (a.bytes > ((size_t)2 << 30)) { (void)hipFree(a.p); return; }      // the working memory of a very large build is not kept
    ScratchArena drop;
    {
        std::lock_guard<std::mutex> lk(ctx->scratch_mu);
        ctx->scratch_free.push_back(a);
        if (ctx->scratch_free.size() > 8) {                // keep the large ones
            size_t smallest = 0;
            for (size_t i = 1; i < ctx->scratch_free.size(); ++i) if (ctx->scratch_free[i].bytes < ctx->scratch_free[smallest].bytes) smallest = i;
            drop = ctx->scratch_free[smallest];
            ctx->scratch_free.erase(ctx->scratch_free.begin() + (long)smallest);
        }
    }
    if (drop.p) (void)hipFree(drop.p);
}

// Device memory of the trees (nodes, records, a dozen small per-instance tables), kept by the context when a tree is freed and handed
// out again to the next build: an update that rebuilds (every file's first frame in the reference's Time mode) otherwise spends more
// time in ~20 hipMalloc / hipFree pairs -- each hipFree waits for the device -- than in its kernels.  Eight size classes per octave;
// blocks above 64 MiB and anything beyond 1 GiB in all go back to the runtime.
static size_t pool_class(size_t bytes) {
    bytes = std::max<size_t>(bytes, 256);
    size_t p2 = 256;
    while (p2 * 2 <= bytes) p2 *= 2;
    const size_t step = p2 / 8;
    return (bytes + step - 1) / step * step;
}
hipError_t pool_alloc(HrtContext *ctx, void **p, size_t bytes) {
    const size_t cls = pool_class(bytes);
    {
        std::lock_guard<std::mutex> lk(ctx->pool_mu);
        for (size_t i = 0; i < ctx->pool_free.size(); ++i)
            if (ctx->pool_free[i].bytes == cls) {
                *p = ctx->pool_free[i].p;
                ctx->pool_free.erase(ctx->pool_free.begin() + (long)i);
                ctx->pool_bytes -= cls; ctx->pool_live[*p] = cls;
                return hipSuccess;
            }
    }
    hipError_t e = hipMalloc(p, cls);
    if (e != hipSuccess) { reclaim_kept_memory(ctx); e = hipMalloc(p, cls); }
    if (e == hipSuccess) { std::lock_guard<std::mutex> lk(ctx->pool_mu); ctx->pool_live[*p] = cls; }
    return e;
}
// (the caller has made sure the device is done with the block)
void pool_release(HrtContext *ctx, void *p) {
    if (!p) return;
    {
        std::lock_guard<std::mutex> lk(ctx->pool_mu);
        const auto it = ctx->pool_live.find(p);
        if (it != ctx->pool_live.end()) {
            const size_t bytes = it->second;
            ctx->pool_live.erase(it);
            if (bytes <= ((size_t)64 << 20) && ctx->pool_bytes + bytes <= ((size_t)1 << 30) && ctx->pool_free.size() < 512) {
                ctx->pool_free.push_back({p, bytes}); ctx->pool_bytes += bytes;
                return;
            }
        }
    }
    (void)hipFree(p);
}
void pool_drain(HrtContext *ctx) {
    std::vector<ScratchArena> blocks;
    { std::lock_guard<std::mutex> lk(ctx->pool_mu); blocks.swap(ctx->pool_free); ctx->pool_bytes = 0; }
    for (const ScratchArena &b : blocks) (void)hipFree(b.p);
}

}  // namespace hrt
