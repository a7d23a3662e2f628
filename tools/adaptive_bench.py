#!/usr/bin/env python3
"""Adaptive sampling measured (hrt_render_accumulate / hrt_sample_counts; DESIGN.md section 2.1 "Per-pixel sample counts"):
  (a) what the variant costs: C4 at 1920 x 1080, accumulate with a uniform map of 64 against hrt_render_launch(64), both in a context created
      under HRT_SAMPLE_BLOCK=0 -- the plain k_fused that k_path_counts is a variant of; legs alternated, --runs each, median and range;
  (b) what it buys: C4 and the shipped 25-particle sample, render_adaptive(pilot 16, max_total 256) over four target sigmas against a uniform
      render at the spp nearest to the adaptive mean: MSE of the linear frame against a 4096-spp render of the same seed, samples taken, time.
  (c) --denoise (off by default): the denoiser's accumulated mode (hrt_denoise_accumulated_launch; DESIGN.md 3e "Accumulated mode") on the
      adaptive frames of (b) -- MSE against the 4096-spp frame of the adaptive frame as it is, filtered by this mode, filtered by
      hrt_denoise_launch, and of this mode over a uniform render of the same mean samples -- and the call's time at 1920 x 1080 against
      hrt_denoise_variance_launch starting afresh on the same frame, legs alternated, --runs runs of 20 calls each.
tools/adaptive_bench.py [--runs 5] [--reference-spp 4096] [--skip-cost] [--skip-gain]      -> profiles/r28_adaptive.txt
tools/adaptive_bench.py --skip-cost --skip-gain --denoise                                  -> profiles/r34_denoise_accumulated.txt"""
import argparse, importlib, os, statistics, sys, time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch
hrt = importlib.import_module("nvidia-optix-ray-tracer_amd")
ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=5); ap.add_argument("--reference-spp", type=int, default=4096)
ap.add_argument("--skip-cost", action="store_true"); ap.add_argument("--skip-gain", action="store_true")
ap.add_argument("--denoise", action="store_true")
a = ap.parse_args()


def renderer(scene, flags, env=None):
    """a context created under `env` (the knobs are read when the context is created)"""
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        r = hrt.Renderer(0, flags)
    finally:
        for k, v in old.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v
    r.load_scene(scene)
    r.set_frame(scene["width"], scene["height"], hrt.scenes.SEED_SALT, aov=False, linear=True)
    return r


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def spread(ms):
    return f"median {statistics.median(ms):8.2f} ms, range {min(ms):8.2f} .. {max(ms):8.2f} ({len(ms)} runs)"


if not a.skip_cost:
    scene = hrt.scenes.BASELINE_CONFIGS["C4"]()
    w, h, spp = scene["width"], scene["height"], 64
    r = renderer(scene, hrt.CTX_FAST_TRACE, {"HRT_SAMPLE_BLOCK": "0"})
    full = torch.full((h, w), spp, dtype=torch.int32, device=r.device)

    def leg_accumulate():
        r.taken.zero_(); r.accumulate(spp, counts=full, sync=False)

    def leg_launch():
        r.render(spp, sync=False)
    leg_accumulate(); leg_launch()                         # warm-up
    acc, plain = [], []
    for _ in range(a.runs):
        acc.append(timed(leg_accumulate)); plain.append(timed(leg_launch))
    print(f"(a) C4 {w} x {h}, {spp} spp, HRT_SAMPLE_BLOCK=0, legs alternated")
    print(f"    hrt_render_launch({spp})               k_fused          {spread(plain)}")
    print(f"    hrt_render_accumulate(map of {spp})    k_path_counts    {spread(acc)}")
    print(f"    ratio of the medians: {statistics.median(acc) / statistics.median(plain):.4f}", flush=True)
    r.close()

if not a.skip_gain:
    for name, scene in (("C4", hrt.scenes.BASELINE_CONFIGS["C4"]()), ("shipped sample (25 particles)", hrt.scenes.particle_scene(25, 1200, 800, 1))):
        w, h = scene["width"], scene["height"]
        r = renderer(scene, hrt.CTX_FAST_TRACE)
        r.render(a.reference_spp)
        reference = r.linear[..., :3].clone()
        mse = lambda: float(((r.linear[..., :3] - reference).double() ** 2).mean())
        print(f"(b) {name}, {w} x {h}: pilot 16, max_total 256, radius 1; MSE of the linear frame against {a.reference_spp} spp of the same seed")
        print("    target_sigma   adaptive: samples/pixel  zero-count share        MSE    time ms |  uniform: spp        MSE    time ms")
        for sigma in (0.07, 0.05, 0.035, 0.025):
            params = dict(target_sigma=sigma, max_total=256)
            fresh = lambda: r.set_frame(w, h, hrt.scenes.SEED_SALT, aov=False, linear=True)
            fresh(); r.render_adaptive(16, params)             # warm-up
            t_ad = []
            for _ in range(3):
                fresh(); r.reset_stats()
                t_ad.append(timed(lambda: r.render_adaptive(16, params)))
            mean_spp = r.stats().paths / (w * h)
            zero = float((r.counts == 0).float().mean())
            mse_ad = mse()
            u = max(1, round(mean_spp))
            t_un = []
            for _ in range(3):
                fresh()
                t_un.append(timed(lambda: r.render(u, sync=False)))
            print(f"    {sigma:12.3f}   {mean_spp:23.2f}  {zero:16.3f}  {mse_ad:9.3e}  {statistics.median(t_ad):9.2f} |  {u:12d}  {mse():9.3e}  {statistics.median(t_un):9.2f}", flush=True)
        r.close()

if a.denoise:
    def encode(r, linear):
        """colorToFloat4 of an (H, W, 4) linear frame"""
        src = torch.ones((linear.shape[0], linear.shape[1], 4), dtype=torch.float32, device=r.device)
        src[..., :3] = linear[..., :3]
        dst = torch.empty_like(src)
        r._check(r.lib.hrt_color_to_float4(r.ctx, src.data_ptr(), dst.data_ptr(), src.shape[0] * src.shape[1], r._stream()), "hrt_color_to_float4")
        torch.cuda.synchronize()
        return dst

    for name, scene in (("C4", hrt.scenes.BASELINE_CONFIGS["C4"]()), ("shipped sample (25 particles)", hrt.scenes.particle_scene(25, 1200, 800, 1))):
        w, h = scene["width"], scene["height"]
        r = renderer(scene, hrt.CTX_FAST_TRACE)
        r.render(a.reference_spp)
        reference = r.linear[..., :3].clone()
        reference_enc = encode(r, r.linear)[..., :3]
        mse = lambda x: float(((x[..., :3] - reference).double() ** 2).mean())
        mse_enc = lambda x: float(((x[..., :3] - reference_enc).double() ** 2).mean())
        fresh = lambda: r.set_frame(w, h, hrt.scenes.SEED_SALT, aov=False, linear=True)
        print(f"(c) {name}, {w} x {h}: pilot 16, max_total 256, radius 1, the denoisers' default parameters; MSE against {a.reference_spp} spp of the same seed,")
        print("    of the linear frame (lin) and of the colorToFloat4-encoded frame (enc; hrt_denoise_launch filters the encoded buffer and has no linear frame)")
        print("    target_sigma  samples/pixel | adaptive frame: lin       enc | accumulated mode: lin       enc | hrt_denoise_launch: enc | uniform spp  accumulated mode: lin       enc")
        for sigma in (0.05, 0.035, 0.025):
            fresh(); r.reset_stats()
            r.render_adaptive(16, dict(target_sigma=sigma, max_total=256))
            mean_spp = r.stats().paths / (w * h)
            raw = (mse(r.linear), mse_enc(r.color))
            guides = r.denoise_guides()
            out, lin, _ = r.denoise_accumulated_filter(r.sum, r.taken, guides, var_out=False)
            mode = (mse(lin), mse_enc(out))
            plain = mse_enc(r.denoise())
            u = max(1, round(mean_spp))
            fresh(); r.accumulation_reset(); r.accumulate(u)
            out, lin, _ = r.denoise_accumulated_filter(r.sum, r.taken, guides, var_out=False)
            print(f"    {sigma:12.3f}  {mean_spp:13.2f} | {raw[0]:19.3e} {raw[1]:9.3e} | {mode[0]:21.3e} {mode[1]:9.3e} | {plain:23.3e} | {u:11d}  {mse(lin):21.3e} {mse_enc(out):9.3e}", flush=True)
        if (w, h) == (1920, 1080):
            # the call's time on the last adaptive frame's sums: both legs trace the guides and run the same five passes
            fresh(); r.render_adaptive(16, dict(target_sigma=0.035, max_total=256))
            out = torch.empty_like(r.color)

            calls = 20                                                           # per timed run: a single call is a millisecond

            def leg_accumulated():
                for _ in range(calls):
                    r.denoise_accumulated(out=out)

            def leg_variance():
                for _ in range(calls):
                    r.denoise_temporal_reset()                                   # (a flag on the host: the call starts afresh every time)
                    r.denoise_variance(out=out)
            leg_accumulated(); leg_variance()                                    # warm-up
            acc, var = [], []
            for _ in range(a.runs):
                acc.append(timed(leg_accumulated) / calls); var.append(timed(leg_variance) / calls)
            print(f"    the call at {w} x {h}, target_sigma 0.035, default parameters (5 passes); enqueue + sync, {calls} calls per run, ms per call, legs alternated")
            fine = lambda ms: f"median {statistics.median(ms):7.3f} ms, range {min(ms):7.3f} .. {max(ms):7.3f} ({len(ms)} runs)"
            print(f"    hrt_denoise_accumulated_launch                       {fine(acc)}")
            print(f"    hrt_denoise_variance_launch, afresh every time       {fine(var)}")
            print(f"    ratio of the medians: {statistics.median(acc) / statistics.median(var):.4f}", flush=True)
        r.close()
