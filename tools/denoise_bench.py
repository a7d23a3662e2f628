"""What the denoiser costs at 1080p next to the 1-spp frame it cleans: C4 (bench.py's scene) and the shipped sample (tests/golden/files,
first frame of Time mode).  Per scene: a 1-spp render, hrt_denoise_guides, hrt_denoise_filter and hrt_denoise_launch, each the median
of --reps timed repetitions (HIP events around the Renderer method, after a warm-up: the figure includes the method's argument checks
and its hrt_sync, so it is a whole-call time, not a sum of kernel times).  Under `rocprofv3 --kernel-trace --stats` the per-kernel
split is k_fused (render and guide rays), k_denoise_rays, k_denoise_guides, k_denoise_pass<3, false> (one launch per filter pass).
--temporal adds hrt_denoise_temporal_launch (the frame repeated, so that every call after the first blends with a history): its own
kernel is k_denoise_temporal.  --variance adds hrt_denoise_variance_launch in the same way (k_denoise_temporal<true>,
k_denoise_variance, k_denoise_pass<3, true>: the same pass kernel's variance form) and hrt_denoise_filter_variance over the frame's guides and a constant variance.
--handoff (with --temporal) adds the same call begun from a history handed over from another TLAS every time (hrt_denoise_temporal_rebind
between two identical trees, alternating): its kernel is k_denoise_temporal_linked, to be set against k_denoise_temporal in the same
trace; the whole-call figure also pays hrt_materials_set and the material tables of the other tree.
--by-primitive (with --temporal --handoff) adds the call begun from a history handed over across REBUILT BLASes every time
(hrt_denoise_temporal_rebind_geometry between two trees in which every second triangle instance -- the only one, in a one-mesh scene --
has a BLAS of its own, from the scene's vertices): its kernel is k_denoise_temporal_by_prim, with lanes on the rigid and on the
by-primitive path in the same waves where the scene has both, to be set against k_denoise_temporal_linked in the same trace; with
--variance as well, both hand-overs are repeated in the variance-guided mode (the kernels' <true> instantiations).
--capture sets HRT_CTX_CAPTURE_PRIMARY: the render launch runs k_path_capture and the guide pass of every denoise call takes its
primary hits instead of tracing (guides_ms is then the pass without its traversal).  With or without it, frame_ms is what the switch is
about -- a 1-spp render and hrt_denoise_launch enqueued back to back, one synchronisation --, and path_kernel_ms the path kernel of
the render alone, from the context's own HIP events (HRT_CTX_TIMING), so that k_path_capture can be set against k_fused.

    python tools/denoise_bench.py [--reps 20] [--width 1920 --height 1080] [--scenes c4,sample] [--temporal [--handoff [--by-primitive]]] [--variance] [--capture]
"""
from __future__ import annotations

import argparse
import importlib
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def median_ms(torch, fn, reps):
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--scenes", default="c4,sample")
    ap.add_argument("--temporal", action="store_true")
    ap.add_argument("--variance", action="store_true")
    ap.add_argument("--handoff", action="store_true")
    ap.add_argument("--by-primitive", action="store_true")
    ap.add_argument("--capture", action="store_true")
    args = ap.parse_args()
    import torch
    hrt = importlib.import_module("nvidia-optix-ray-tracer_amd")
    io = importlib.import_module("nvidia-optix-ray-tracer_amd.io")
    w, h = args.width, args.height
    for name in args.scenes.split(","):
        flags = hrt.CTX_CAPTURE_PRIMARY if args.capture else 0
        r = hrt.Renderer(0, flags)
        if name == "c4":
            scene = hrt.scenes.BASELINE_CONFIGS["C4"]()
            r.load_scene(scene)
            r.set_frame(w, h, hrt.scenes.SEED_SALT, aov=False)
        else:
            tm = io.time_mode_scene(ROOT / "tests" / "golden" / "files" / "config.json", width=w, height=h)
            cfg, scene = tm["config"], tm["scene"]
            r.load_scene(scene)
            r.set_frame(w, h, hrt.scenes.SEED_SALT, aov=False)
            r.pose_instances(tm["states"][0], tm["states"][min(1, len(tm["states"]) - 1)], float(tm["durations"][0]), 0,
                             tm["frame_counts"][0], first_instance=tm["n_extra"], offset=cfg["particle-shift"], scale=cfg["particle-scale"])
        out = torch.empty_like(r.color)
        dp = hrt.DenoiseParams()
        r.lib.hrt_denoise_default_params(dp)
        r.render(1)
        guides = r.denoise_guides()
        r.denoise_filter(r.color, guides, out=out)
        r.denoise(out=out)
        def frame():
            r.render(1, sync=False)
            r.denoise(out=out)

        res = {"scene": name, "width": w, "height": h, "capture": bool(args.capture),
               "frame_ms": median_ms(torch, frame, args.reps),
               "render_1spp_ms": median_ms(torch, lambda: r.render(1, sync=False), args.reps),
               "guides_ms": median_ms(torch, r.denoise_guides, args.reps),
               "filter_ms": median_ms(torch, lambda: r.denoise_filter(r.color, guides, out=out), args.reps),
               "denoise_launch_ms": median_ms(torch, lambda: r.denoise(out=out), args.reps)}
        res["filter_per_pass_ms"] = res["filter_ms"] / dp.iterations
        if args.temporal:
            r.denoise_temporal(out=out)
            res["denoise_temporal_ms"] = median_ms(torch, lambda: r.denoise_temporal(out=out), args.reps)
            if args.handoff:
                trees = [r.tlas, r.build_tlas(None, r.instance_transforms())]

                def linked():
                    trees.reverse()
                    r.denoise_temporal_rebind(trees[0])
                    r.use_tlas(trees[0])
                    r.denoise_temporal(out=out)

                linked()
                res["denoise_temporal_linked_ms"] = median_ms(torch, linked, args.reps)
                res["history_rebinds"] = r.stats().denoise_history_rebinds
                if args.by_primitive:
                    tri = [j for j, it in enumerate(scene["instances"]) if it["geometry"] == "triangles"]
                    own = {j: scene["instances"][j]["vertices"] for j in (tri[1::2] if len(tri) > 1 else tri)}
                    normals = {j: scene["instances"][j]["normals"] for j in own}
                    rebuilt = [r.build_tlas(None, r.instance_transforms(), vertices=own, normals=normals) for _ in range(2)]

                    def by_primitive():
                        rebuilt.reverse()
                        r.denoise_temporal_rebind(rebuilt[0], by_primitive=True)
                        r.use_tlas(rebuilt[0])
                        r.denoise_temporal(out=out)

                    by_primitive()
                    by_primitive()
                    res["denoise_temporal_by_primitive_ms"] = median_ms(torch, by_primitive, args.reps)
                    res["by_primitive_instances"] = len(own)
                    res["by_primitive_links"] = r.stats().denoise_by_primitive_links
                    if args.variance:      # the same two hand-overs in the variance-guided mode: the kernels' <true> instantiations
                        def handed_variance(pair, by_prim):
                            pair.reverse()
                            r.denoise_temporal_rebind(pair[0], by_primitive=by_prim)
                            r.use_tlas(pair[0])
                            r.denoise_variance(out=out)

                        for pair, by_prim, key in ((trees, False, "denoise_variance_linked_ms"), (rebuilt, True, "denoise_variance_by_primitive_ms")):
                            r.use_tlas(pair[0])
                            r.denoise_variance(out=out)
                            handed_variance(pair, by_prim)
                            res[key] = median_ms(torch, lambda: handed_variance(pair, by_prim), args.reps)
                    r.use_tlas(trees[0])
        if args.variance:
            var = torch.full((h, w), 1e-3, dtype=torch.float32, device=r.device)
            var_out = torch.empty_like(var)
            r.denoise_temporal_reset()
            r.denoise_variance(out=out)
            res["denoise_variance_ms"] = median_ms(torch, lambda: r.denoise_variance(out=out), args.reps)
            r.denoise_filter_variance(r.color, guides, var, out=out, var_out=var_out)
            res["filter_variance_ms"] = median_ms(torch, lambda: r.denoise_filter_variance(r.color, guides, var, out=out, var_out=var_out), args.reps)
            res["filter_variance_per_pass_ms"] = res["filter_variance_ms"] / dp.iterations
        r.set_flags(flags | hrt.CTX_TIMING)
        r.reset_stats()
        for _ in range(args.reps):
            r.render(1)
        st = r.stats()
        res["path_kernel_ms"] = st.kernel_ms[hrt.K_PATHS] / max(1, st.kernel_launches[hrt.K_PATHS])
        res["guide_passes"] = {"captured": st.guide_passes_captured, "traced": st.guide_passes_traced}
        print(json.dumps(res), flush=True)
        r.close()


if __name__ == "__main__":
    main()
