"""tools/denoise_variance_sweep.py without a GPU: the same four cases, grid and output lines, from the numpy specification
(tests/denoise_variance_ref.py) over frames the CPU oracle renders.  The oracle's frames and the specification's outputs are the
renderer's and the kernels' bit for bit (tests/test_gpu_parity.py, tests/test_denoise_variance_gpu.py), so the figures are the GPU
sweep's.  The filter's output is not fed back into the history, so A, L and M of the last frame depend on alpha_min alone: per
alpha_min the sequence runs once through moments_step, and every (sigma_luminance, history_min) filters that last frame.

    python tools/denoise_variance_sweep_spec.py [--jobs 8] > sweep.jsonl
"""
import argparse
import copy
import importlib
import itertools
import json
import math
import sys
from concurrent.futures import ProcessPoolExecutor
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
hrt = importlib.import_module("nvidia-optix-ray-tracer_amd")
io = importlib.import_module("nvidia-optix-ray-tracer_amd.io")
import denoise_ref as ref  # noqa: E402
import denoise_temporal_ref as tref  # noqa: E402
import denoise_variance_ref as vref  # noqa: E402
import oracle_py as oracle  # noqa: E402

SAMPLE = ROOT / "tests" / "golden" / "files" / "config.json"
SIGMAS = (1.0, 2.0, 3.0, 4.0, 6.0, 8.0)
HISTORY_MINS = (1, 2, 4, 8)
ALPHAS = (0.05, 0.1, 0.2, 0.4, 0.6, 0.8)
REFERENCE_SPP = 4096


def frame_scenes(name, w, h, frames):
    """The scene of every frame: C1 static; the sample with the oracle's pose_transforms of frames 0.. of its first step interval."""
    if name == "c1":
        return [hrt.scenes.cornell_box(w, h, 1)] * frames
    tm = io.time_mode_scene(SAMPLE, width=w, height=h)
    cfg, out = tm["config"], []
    for f in range(frames):
        scene = copy.deepcopy(tm["scene"])
        xf = oracle.pose_transforms(tm["states"][0], tm["states"][1], float(tm["durations"][0]), f, tm["frame_counts"][0],
                                    cfg["particle-shift"], cfg["particle-scale"])
        for it, m in zip(scene["instances"][tm["n_extra"]:], xf):
            it["transform"] = m.copy()
        out.append(scene)
    return out


def cam_of(scene):
    c = scene["camera"]
    u, v, w = hrt.configure_camera(c["center"], c["target"], c["up"], c.get("opengl", True))
    return (np.asarray(c["center"], np.float32), u, v, w)


def case(args):
    name, w, h, frames, spp = args
    scenes = frame_scenes(name, w, h, frames)
    cam = cam_of(scenes[0])
    center, U, V, W = cam
    dirs = ref.primary_directions(w, h, U, V, W)
    origins = np.broadcast_to(center, dirs.shape).copy()
    osc = oracle.OracleScene(scenes[-1])
    conv = osc.render(w, h, oracle.rng_init(w, h, hrt.scenes.SEED_SALT), REFERENCE_SPP)["color"][..., :3].astype(np.float64)
    osc.close()
    mse = lambda x: float(((x[..., :3].astype(np.float64) - conv) ** 2).mean())      # noqa: E731
    states = oracle.rng_init(w, h, hrt.scenes.SEED_SALT)
    per_frame = []
    for scene in scenes:
        osc = oracle.OracleScene(scene)
        raw = osc.render(w, h, states, spp)["color"].copy()
        hits = osc.trace(origins, dirs)
        xf = np.array([np.asarray(it["transform"], np.float32).reshape(12) for it in scene["instances"]], np.float32).reshape(-1, 12)
        per_frame.append((raw, hits, tref.world_to_object(osc), xf))
        osc.close()
    raw, hits = per_frame[-1][0], per_frame[-1][1]
    guides = ref.guides_from_hits(scenes[-1], center, dirs, *hits, w, h)
    mse_raw, mse_spatial, mse_temporal = mse(raw), mse(ref.atrous(raw, guides)), None
    out = []
    for alpha in sorted(set(ALPHAS) | {tref.DEFAULTS["alpha_min"]}):
        hist = None
        for color, fh, inv, xf in per_frame:
            A, L, _, M, hist = vref.moments_step(hist, color, fh, cam, inv, xf, w, h, {"alpha_min": alpha})
        if alpha == tref.DEFAULTS["alpha_min"]:
            mse_temporal = mse(ref.atrous(A, guides))                              # the temporal mode at its defaults: the same A
        if alpha not in ALPHAS:
            continue
        for hmin in HISTORY_MINS:
            var = vref.variance(M, L, hist["inst"], hmin)
            for sigma in SIGMAS:
                res, _ = vref.filter_variance(A, guides, var, None, {"sigma_luminance": sigma, "history_min": hmin})
                out.append({"scene": name, "spp": spp, "sigma_luminance": sigma, "history_min": hmin, "alpha_min": alpha, "mse_variance": mse(res)})
    for r in out:
        r.update(mse_raw=mse_raw, mse_spatial=mse_spatial, mse_temporal=mse_temporal, ratio_spatial=r["mse_variance"] / mse_spatial,
                 ratio_temporal=r["mse_variance"] / mse_temporal)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=4)
    args = ap.parse_args()
    assert tref.DEFAULTS["alpha_min"] == max(ALPHAS)                                # (sorted: the default's A comes before its use above)
    cases = [(name, w, h, frames, spp) for name, w, h, frames in (("c1", 256, 256, 16), ("sample", 300, 200, 8)) for spp in (1, 4)]
    grid = list(itertools.product(SIGMAS, HISTORY_MINS, ALPHAS))
    ratios, ratios_t = {g: [] for g in grid}, {g: [] for g in grid}
    out = sys.stdout
    with ProcessPoolExecutor(min(args.jobs, len(cases))) as pool:
        for recs in pool.map(case, cases):
            for r in recs:
                g = (r["sigma_luminance"], r["history_min"], r["alpha_min"])
                ratios[g].append(r["ratio_spatial"])
                ratios_t[g].append(r["ratio_temporal"])
                out.write(json.dumps(r) + "\n")
            out.flush()
    geo = lambda v: math.exp(sum(math.log(x) for x in v) / len(v))      # noqa: E731
    for g in grid:
        out.write(json.dumps({"summary": g, "worst_spatial": max(ratios[g]), "geomean_spatial": geo(ratios[g]),
                              "ratios_spatial": ratios[g], "ratios_temporal": ratios_t[g]}) + "\n")
    at_default = [g for g in grid if g[2] == tref.DEFAULTS["alpha_min"]]
    for key, cands in (("chosen_defaults", at_default), ("chosen", grid)):
        best = min(max(ratios[g]) for g in cands)
        chosen = min((g for g in cands if max(ratios[g]) <= best + 0.001), key=lambda g: geo(ratios[g]))
        out.write(json.dumps({key: chosen, "worst_spatial": max(ratios[chosen]), "geomean_spatial": geo(ratios[chosen]),
                              "ratios_spatial": ratios[chosen], "ratios_temporal": ratios_t[chosen]}) + "\n")


if __name__ == "__main__":
    main()
