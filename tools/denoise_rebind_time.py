#!/usr/bin/env python3
"""What hrt_denoise_temporal_rebind itself costs -- a host loop over the instances and one upload per file boundary -- at DEM-sized
instance counts: scenes.particle_cloud(n), two identical TLASes, the NULL map (Time mode's case), the median of --reps calls with the
stream synchronised after each.  Figures: profiles/r21_denoise_handoff.txt.
--by-primitive K: hrt_denoise_temporal_rebind_geometry instead, between two trees whose first K particles have BLASes of their own
(the same vertices): those K entries are linked by primitive -- a BLAS reference and a pointer each, and the 8-byte-per-instance
table's upload on top of the map's.  Figures: profiles/r25_denoise_by_primitive.txt.

    python tools/denoise_rebind_time.py [--counts 2000,100000] [--reps 9] [--by-primitive K]
"""
import argparse
import importlib
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", default="2000,100000")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--by-primitive", type=int, default=0)
    args = ap.parse_args()
    import torch
    hrt = importlib.import_module("nvidia-optix-ray-tracer_amd")
    w, h = 96, 64
    for n in (int(x) for x in args.counts.split(",")):
        r = hrt.Renderer(0, hrt.CTX_TWO_LEVEL)
        scene = hrt.scenes.particle_cloud(n, w, h, 1)
        r.load_scene(scene)
        r.set_frame(w, h, hrt.scenes.SEED_SALT, aov=False)
        k = min(args.by_primitive, n)
        if k:
            own = {j: scene["instances"][j]["vertices"] for j in range(1, k + 1)}
            normals = {j: scene["instances"][j]["normals"] for j in own}
            trees = [r.build_tlas(None, None, vertices=own, normals=normals) for _ in range(2)]
            r.use_tlas(trees[0])
        else:
            trees = [r.tlas, r.build_tlas()]
        r.render(1)
        r.denoise_temporal()
        times = []
        for _ in range(args.reps):
            trees.reverse()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r.denoise_temporal_rebind(trees[0], by_primitive=bool(k))
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
            r.use_tlas(trees[0])
            r.denoise_temporal()
        times.sort()
        print(json.dumps({"instances": n + 1, "rebind_ms_median": times[len(times) // 2], "rebind_ms_min": times[0], "rebind_ms_max": times[-1],
                          "history_rebinds": r.stats().denoise_history_rebinds, "by_primitive_links": r.stats().denoise_by_primitive_links}), flush=True)
        r.close()


if __name__ == "__main__":
    main()
