#!/usr/bin/env python3
"""A deforming mesh, or a cloud of moving spheres, per frame, on one MI355X: hrt_blas_update_triangles / _spheres + hrt_tlas_update (a)
against what the library offered before for the same frame (b): hrt_blas_build_triangles / _spheres + hrt_tlas_update with the new handle
(which rebuilds) + hrt_blas_destroy.

Scenes: C4's soup as one BLAS of 1 M triangles; the 2000-particle cloud with one of its three shapes deformed, flattened and two-level;
one sphere BLAS of 1 M spheres in the unit cube (radii 0.001 .. 0.003: a cloud, not a lump); the 2000-particle cloud with shape 0 replaced
by a cluster of 128 spheres, flattened and two-level.
The geometry alternates between two 2 % deformations (spheres: of the centres, radii scaled by up to 10 %), so the refitted tree does not drift.  Per scene five alternating runs of (a) and (b),
each a warm-up frame and --frames timed ones: host clock from the first call to a device synchronise after the last, per frame;
medians and ranges over the runs, one JSON line per scene.  (b) includes the upload of the instance array with the new handle, which
that flow needs every frame; neither includes an upload of vertices (they are on the device).
Also: the BLAS calls alone, as stream time between two events around the call -- the update's one pass (counters in, kernel, counters
out) against the build's device-to-device copy (spheres: k_pack_spheres) + bounds pass (gpu_blas_bounds) --, and the trace rate of the refitted tree against a
freshly built one after the deformation (hrt_trace_rays of --rays random rays, clock around call + synchronise).
Usage: python tools/blas_update_bench.py [--frames 10] [--runs 5] [--rays 2000000] [--only soup|cloud|cloud2|spheres|scloud|scloud2]"""
import argparse, ctypes as C, importlib, json, statistics, sys, time
from pathlib import Path
import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
hrt = importlib.import_module("nvidia-optix-ray-tracer_amd")
import torch


def deform(v, which):
    p = v.reshape(-1, 3).astype(np.float64)
    ext = float((p.max(axis=0) - p.min(axis=0)).max())
    k = np.array([[2.1, 0.7, -1.3], [-0.9, 2.4, 1.1], [1.6, -1.2, 2.2]]) * (1.0 + 0.5 * (which - 1)) / ext
    return (p + 0.02 * ext * np.sin(p @ k.T + 0.4 * which)).astype(np.float32).reshape(v.shape)


def move_spheres(c, r, which):
    p = c.reshape(-1, 3).astype(np.float64)
    return deform(c, which), (r.astype(np.float64) * (1.0 + 0.1 * np.sin(7.0 * p[:, 0] + which))).astype(np.float32)


def med(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def trace_rate(r, n_rays):
    rng = np.random.default_rng(5)
    o = rng.uniform(-1.6, 1.6, (n_rays, 3)).astype(np.float32)
    d = (rng.uniform(-0.8, 0.8, (n_rays, 3)) - o).astype(np.float32)
    o, d = r._dev(o), r._dev(d)
    out = [torch.empty(n_rays, dtype=torch.float32, device=r.device) for _ in range(5)]
    rates = []
    for k in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r._check(r.lib.hrt_trace_rays(r.ctx, r.tlas, o.data_ptr(), d.data_ptr(), n_rays, 1e-6, 1e16, 0, *[x.data_ptr() for x in out], r._stream()), "hrt_trace_rays")
        torch.cuda.synchronize()
        if k:
            rates.append(n_rays / (time.perf_counter() - t0) / 1e6)
    return med(rates), int((out[3].view(torch.int32) != -1).sum())


def run(name, scene, shape_instances, flags, a):
    """shape_instances: the instances over the BLAS that deforms"""
    lib = hrt.load_library()
    r = hrt.Renderer(0, flags)
    r.load_scene(scene)
    st = r._stream()
    n = len(scene["instances"])
    it0 = scene["instances"][shape_instances[0]]
    spheres = it0["geometry"] == "spheres"
    # the two states on the device, and the two calls on state k: update(handle, k), build(k, out_handle)
    if spheres:
        host = [move_spheres(it0["centers"], it0["radii"], w) for w in (1, 2)]
        dev = [(r._dev(c), r._dev(rad)) for c, rad in host]
        n_prims = int(dev[0][1].shape[0])
        update = lambda h, k: r._check(lib.hrt_blas_update_spheres(r.ctx, h, dev[k][0].data_ptr(), dev[k][1].data_ptr(), n_prims, st), "hrt_blas_update_spheres")      # noqa: E731
        build = lambda k, out: r._check(lib.hrt_blas_build_spheres(r.ctx, dev[k][0].data_ptr(), dev[k][1].data_ptr(), n_prims, st, C.byref(out)), "hrt_blas_build_spheres")      # noqa: E731
    else:
        host = [deform(it0["vertices"], w) for w in (1, 2)]
        dev = [r._dev(v.reshape(-1, 3)) for v in host]
        n_prims = int(dev[0].shape[0]) // 3
        update = lambda h, k: r._check(lib.hrt_blas_update_triangles(r.ctx, h, dev[k].data_ptr(), 3 * n_prims, st), "hrt_blas_update_triangles")      # noqa: E731
        build = lambda k, out: r._check(lib.hrt_blas_build_triangles(r.ctx, dev[k].data_ptr(), 3 * n_prims, st, C.byref(out)), "hrt_blas_build_triangles")      # noqa: E731
    handle = int(r._h_inst[shape_instances[0]].traversableHandle)
    h_inst = np.frombuffer(bytes(r._h_inst), dtype=np.uint8).copy().reshape(-1, 80)[:n]
    d_inst = r._d_inst
    frame = [0]

    def frame_a():
        update(handle, frame[0] & 1)
        r._check(lib.hrt_tlas_update(r.ctx, r.tlas, d_inst.data_ptr(), n, st), "hrt_tlas_update")
        frame[0] += 1

    def frame_b():
        nonlocal handle
        new = C.c_uint64()
        build(frame[0] & 1, new)
        h_inst[shape_instances, 64:72] = np.frombuffer(np.uint64(new.value).tobytes(), dtype=np.uint8)
        d_inst[: n * 80].copy_(torch.from_numpy(h_inst.reshape(-1)))
        r._check(lib.hrt_tlas_update(r.ctx, r.tlas, d_inst.data_ptr(), n, st), "hrt_tlas_update")
        r._check(lib.hrt_blas_destroy(r.ctx, handle), "hrt_blas_destroy")
        handle = new.value
        frame[0] += 1

    def timed(fn, frames):
        fn()                                              # warm-up (and, after the other mode, the first update after a build)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(frames):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / frames

    s0 = r.stats()
    ta, tb = [], []
    for _ in range(a.runs):
        ta.append(timed(frame_a, a.frames))
        tb.append(timed(frame_b, a.frames))
    s1 = r.stats()

    # the BLAS calls alone, as stream time
    def stream_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def build_alone():
        h = C.c_uint64()
        build(0, h)
        build_alone.made.append(h.value)
    build_alone.made = []
    probe = C.c_uint64()
    build(0, probe)
    upd = lambda: update(probe.value, 1)      # noqa: E731
    upd(); build_alone()
    pass_u, pass_b = [], []
    for _ in range(a.runs * 2):
        pass_u.append(stream_ms(upd)); pass_b.append(stream_ms(build_alone))
    for h in build_alone.made + [probe.value]:
        lib.hrt_blas_destroy(r.ctx, h)

    # trace rate: the refitted tree against a freshly built one, after one 2 % deformation
    frame_a(); frame_a()
    refits_before = r.stats().tlas_refits
    frame[0] = 0
    frame_a()
    was_refit = r.stats().tlas_refits == refits_before + 1
    rate_refit, hits_refit = trace_rate(r, a.rays)
    r.close()
    fresh_scene = dict(scene, instances=[dict(it) for it in scene["instances"]])
    for i in shape_instances:
        if spheres:
            fresh_scene["instances"][i]["centers"], fresh_scene["instances"][i]["radii"] = host[0]
        else:
            fresh_scene["instances"][i]["vertices"] = host[0]
            fresh_scene["instances"][i]["normals"] = hrt.scenes.face_normals(host[0])
    r = hrt.Renderer(0, flags)
    r.load_scene(fresh_scene)
    rate_fresh, hits_fresh = trace_rate(r, a.rays)
    r.close()
    below = all(x < y for x, y in zip(ta, tb))
    print(json.dumps({"scene": name, "flags": flags, "instances": n, "geometry": it0["geometry"], "deformed_triangles" if not spheres else "moved_spheres": n_prims, "deformed_instances": len(shape_instances),
                      "frames_per_run": a.frames, "runs": a.runs,
                      "a_update_ms_per_frame": med(ta), "a_runs": [round(x, 4) for x in ta],
                      "b_build_update_destroy_ms_per_frame": med(tb), "b_runs": [round(x, 4) for x in tb],
                      "a_below_b_in_every_pair": below,
                      "refits": int(s1.tlas_refits - s0.tlas_refits), "rebuilds": int(s1.tlas_rebuilds - s0.tlas_rebuilds),
                      "blas_update_stream_ms": med(pass_u), "blas_build_copy_plus_bounds_stream_ms": med(pass_b),
                      "trace_Mrays_refitted": rate_refit, "trace_Mrays_fresh": rate_fresh, "traced_tree_was_refit": was_refit,
                      "hits_refitted": hits_refit, "hits_fresh": hits_fresh}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--rays", type=int, default=2000000)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("blas_update_bench: no GPU: nothing is measured without one")
    if a.only in ("", "soup"):
        run("C4-soup-1M as one BLAS", hrt.scenes.soup_1m(64, 64, 1), [0], 0, a)
    if a.only in ("", "cloud", "cloud2"):
        sc = hrt.scenes.particle_cloud(2000, 64, 64, 1)
        shape0 = [i for i, it in enumerate(sc["instances"]) if it.get("shape") == 0]
        if a.only in ("", "cloud"):
            run("cloud-2000, shape 0 deformed, flattened", sc, shape0, 0, a)
        if a.only in ("", "cloud2"):
            run("cloud-2000, shape 0 deformed, two-level", sc, shape0, hrt.CTX_TWO_LEVEL, a)
    S = hrt.scenes
    if a.only in ("", "spheres"):
        n = 1000000
        cloud = S._sphere_instance(S.uniform_f32(7001, 3 * n, -0.5, 0.5).reshape(n, 3), S.uniform_f32(7002, n, 0.001, 0.003), S.WHITE)
        run("sphere-cloud-1M as one BLAS", dict(S.soup_1m(64, 64, 1), instances=[cloud]), [0], 0, a)
    if a.only in ("", "scloud", "scloud2"):
        sc = S.particle_cloud(2000, 64, 64, 1)
        shape0 = [i for i, it in enumerate(sc["instances"]) if it.get("shape") == 0]
        c, rad = S.uniform_f32(7003, 3 * 128, -0.04, 0.04).reshape(128, 3), S.uniform_f32(7004, 128, 0.008, 0.015)
        for i in shape0:                                  # (one BLAS for all of them: "shape" is what load_scene shares by)
            old = sc["instances"][i]
            sc["instances"][i] = dict(S._sphere_instance(c, rad, old["albedo"], old["material"], old["fuzz"], old["transform"]), shape=0)
        if a.only in ("", "scloud"):
            run("cloud-2000, shape 0 a 128-sphere cluster that moves, flattened", sc, shape0, 0, a)
        if a.only in ("", "scloud2"):
            run("cloud-2000, shape 0 a 128-sphere cluster that moves, two-level", sc, shape0, hrt.CTX_TWO_LEVEL, a)


if __name__ == "__main__":
    main()
