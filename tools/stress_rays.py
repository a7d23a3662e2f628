#!/usr/bin/env python3
"""Adversarial rays against brute force: the rays of tests/ray_cases.py (through vertices and along edges of the scene's triangles, tangent to its spheres, from origins
on the surfaces, with direction components that are signed zeros, denormals, tiny, huge; odd [tmin, tmax] windows) over random scenes -- and, unlike the tests, from origins
50 and a million units away (reported, not required; STRESS_FAR=1: where does the envelope end?).  Closest and any-hit.
    tools/stress_rays.py [n_scenes=10] [seed=1] [configurations=flat,two-level]
configurations: a comma-separated choice of the names below (the execution modes tests/test_adversarial_rays_gpu.py pins on its fixed scenes)."""
import importlib, os, sys, time
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))

# name -> (context flags, environment, the oracle's instanced mode)
CONFIGURATIONS = {
    "flat": ((), {}, False),
    "two-level": (("CTX_TWO_LEVEL",), {}, True),
    "counting": (("CTX_COUNT",), {}, False),
    "wavefront": ((), {"HRT_FUSED": "0"}, False),
    "round-1-path-kernel": ((), {"HRT_FUSED_MAX_DEPTH": "1"}, False),
    "round-1-traverse-kernel": ((), {"HRT_FUSED": "0", "HRT_FUSED_MAX_DEPTH": "1"}, False),
    "host-build": ((), {"HRT_BUILD": "host"}, False),
    "aligned-records": ((), {"HRT_NODE_STRIDE": "128", "HRT_PRIM_STRIDE": "64"}, False),
    "fast-trace": (("CTX_FAST_TRACE",), {"HRT_FAST_TRACE_BUILD": "device"}, False),
    "fast-trace-host": (("CTX_FAST_TRACE",), {"HRT_FAST_TRACE_BUILD": "host"}, False),
    "two-level-fast-trace": (("CTX_TWO_LEVEL", "CTX_FAST_TRACE"), {}, True),
}


def main():
    import torch  # noqa: F401
    hrt = importlib.import_module("nvidia-optix-ray-tracer_amd")
    import oracle_py as oracle
    import ray_cases as rc
    n_scenes = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
    chosen = sys.argv[3].split(",") if len(sys.argv) > 3 else ["flat", "two-level"]
    far_run = bool(os.environ.get("STRESS_FAR"))
    # (origins up to ~10 scene extents from the scene are what the boxes' padding is made for, DESIGN.md section 3: the 50 and the 10^6 here are
    # reported, not required -- at 10^6 a float of the origin resolves 0.06 units.  In units of extent / 2, as in the generator.)
    distances = (10.0, 20.0, 50.0, 100.0, 300.0, 1000.0, 1e4) if far_run else rc.DISTANCES + (50.0, 1e6)
    bad = 0
    for k in range(n_scenes):
        kind = rng.integers(0, 4)
        if kind == 0: scene = hrt.scenes.mixed_test_scene(int(rng.integers(10, 3000)), int(rng.integers(1, 40)), int(rng.integers(1, 1000)), 64, 64, 1)
        elif kind == 1: scene = hrt.scenes.particle_cloud(int(rng.integers(4, 300)), 64, 64, 1, seed=int(rng.integers(1, 100)))
        elif kind == 2: scene = hrt.scenes.cornell_box(64, 64, 1)
        else: scene = hrt.scenes.random_soup(int(rng.integers(1, 20000)), float(rng.uniform(0.01, 0.3)), int(rng.integers(1, 1000)), 64, 64, 1)
        o, d, cls, info = rc.adversarial_rays(scene, 60000, int(rng.integers(1, 1 << 31)), 2.0, distances=distances, details=True)      # (extent 2: distances in scene units, as ever)
        dist, scale = info["dist"], info["scale"]
        tmin, tmax = rc.WINDOWS[int(rng.integers(0, 4))]
        for name in chosen:
            flags, env, instanced = CONFIGURATIONS[name]
            saved = {key: os.environ.get(key) for key in env}
            os.environ.update(env)
            value = 0
            for f in flags: value |= getattr(hrt, f)
            r = hrt.Renderer(0, value)
            try:
                r.load_scene(scene)
                want = oracle.OracleScene(scene, force_brute=True, instanced=instanced).trace(o, d, tmin=tmin, tmax=tmax)
                got = r.trace_rays(o, d, tmin=tmin, tmax=tmax)
                any_g = r.trace_rays(o, d, tmin=tmin, tmax=tmax, any_hit=True)
                diff = rc.records_differ(got, want)
                adiff = (any_g[3] != rc.MISS) != (want[3] != rc.MISS)
                far = dist > 10.0
                if far_run:
                    print("   differing rays by the origin's distance:", {float(v): (int(((diff | adiff) & (dist == v)).sum()), int((dist == v).sum())) for v in np.unique(dist)}, flush=True)
                elif (diff | adiff)[far].any():
                    print("   (beyond the envelope: origins 50 units off", int(((diff | adiff) & (dist == 50.0)).sum()), "of", int((dist == 50.0).sum()), "rays differ; 10^6 units off", int(((diff | adiff) & (dist == 1e6)).sum()), "of", int((dist == 1e6).sum()), ")", flush=True)
                diff &= ~far; adiff &= ~far
                if diff.any() or adiff.any():
                    bad += 1
                    print("   mismatches by the origin's distance from its target:", {float(v): int(((diff | adiff) & (dist == v)).sum()) for v in np.unique(dist)},
                          "by direction scale:", {float(v): int(((diff | adiff) & (scale == v)).sum()) for v in np.unique(scale)}, "with a replaced component:", int(((diff | adiff) & info["replaced"]).sum()),
                          "by class:", {rc.CLASS_NAMES[c]: int(((diff | adiff) & (cls == c)).sum()) for c in range(7)}, flush=True)
                    j = int(np.argmax(diff | adiff))
                    print("MISMATCH", scene["name"], name, "window", (tmin, tmax), int(diff.sum()), "closest,", int(adiff.sum()), "any-hit; first: o", o[j], "d", d[j],
                          "gpu", (got[0][j], got[3][j], got[4][j]), "oracle", (want[0][j], want[3][j], want[4][j]), "any", any_g[3][j], flush=True)
            finally:
                r.close()
                for key, v in saved.items():
                    if v is None: os.environ.pop(key, None)
                    else: os.environ[key] = v
        print(time.strftime("%H:%M:%S"), k, scene["name"], "window", (tmin, tmax), "ok" if not bad else f"{bad} bad so far", flush=True)
    print("stress:", "all hit records bit-exact" if not bad else f"{bad} FAILURES")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
