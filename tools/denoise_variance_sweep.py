"""Sweep of the denoiser's variance-guided mode (profiles/r12_denoise_variance.txt) over the four cases of
tools/denoise_temporal_sweep.py: C1 static (16 frames) and the shipped sample's Time-mode animation (frames 0..7 of the first step
interval), at 1 and 4 spp, against 4096-spp frames of the last pose.  The raw frames of a case are rendered once and every setting
denoises the same ones.  One JSON line per (scene, spp, setting) on stdout: the MSE of the variance-guided output, of the spatial
filter alone on the last raw frame and of the temporal mode at its defaults, and the two ratios; then one "summary" line per
setting over the four cases, and two lines by r07's rule -- the smallest worst-case ratio to the spatial filter, ties within 0.001
going to the better geometric mean: "chosen_defaults" over (sigma_luminance, history_min) at the temporal parameters' default
alpha_min, which is what a call with every parameter at its default runs and so what hrt_denoise_variance_default_params follows, and
"chosen" over the whole grid, alpha_min included.

    python tools/denoise_variance_sweep.py > sweep.jsonl
"""
import itertools
import json
import math
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tools")]
from denoise_temporal_sweep import hrt, pose, reference, setup  # noqa: E402

SIGMAS = (1.0, 2.0, 3.0, 4.0, 6.0, 8.0)
HISTORY_MINS = (1, 2, 4, 8)
ALPHAS = (0.05, 0.1, 0.2, 0.4, 0.6, 0.8)


def main():
    out = sys.stdout
    grid = list(itertools.product(SIGMAS, HISTORY_MINS, ALPHAS))
    ratios = {g: [] for g in grid}
    ratios_t = {g: [] for g in grid}
    for name, w, h, frames in (("c1", 256, 256, 16), ("sample", 300, 200, 8)):
        conv = reference(name, frames, w, h)
        mse = lambda x: float(((x.cpu().numpy()[..., :3].astype(np.float64) - conv) ** 2).mean())      # noqa: E731
        for spp in (1, 4):
            r = hrt.Renderer(0, 0)
            try:
                tm = setup(name, r, w, h)
                raws = []
                for f in range(frames):
                    pose(name, r, tm, f)
                    r.render(spp)
                    raws.append(r.color.clone())
                    temporal = r.denoise_temporal()
                mse_raw, mse_spatial, mse_temporal = mse(r.color), mse(r.denoise()), mse(temporal)
                for g in grid:
                    sigma, hmin, alpha = g
                    r.denoise_temporal_reset()
                    for f in range(frames):
                        pose(name, r, tm, f)
                        r.color.copy_(raws[f])
                        res = r.denoise_variance(tparams={"alpha_min": alpha}, vparams={"sigma_luminance": sigma, "history_min": hmin})
                    m = mse(res)
                    ratios[g].append(m / mse_spatial)
                    ratios_t[g].append(m / mse_temporal)
                    out.write(json.dumps({"scene": name, "spp": spp, "sigma_luminance": sigma, "history_min": hmin, "alpha_min": alpha,
                                          "mse_raw": mse_raw, "mse_spatial": mse_spatial, "mse_temporal": mse_temporal, "mse_variance": m,
                                          "ratio_spatial": m / mse_spatial, "ratio_temporal": m / mse_temporal}) + "\n")
                    out.flush()
            finally:
                r.close()
    geo = lambda v: math.exp(sum(math.log(x) for x in v) / len(v))      # noqa: E731
    for g in grid:
        out.write(json.dumps({"summary": g, "worst_spatial": max(ratios[g]), "geomean_spatial": geo(ratios[g]),
                              "ratios_spatial": ratios[g], "ratios_temporal": ratios_t[g]}) + "\n")
    tp = hrt.DenoiseTemporalParams()
    hrt.load_library().hrt_denoise_temporal_default_params(tp)
    at_default = [g for g in grid if abs(g[2] - tp.alpha_min) < 1e-6]
    for key, cands in (("chosen_defaults", at_default), ("chosen", grid)):
        best = min(max(ratios[g]) for g in cands)
        chosen = min((g for g in cands if max(ratios[g]) <= best + 0.001), key=lambda g: geo(ratios[g]))
        out.write(json.dumps({key: chosen, "worst_spatial": max(ratios[chosen]), "geomean_spatial": geo(ratios[chosen]),
                              "ratios_spatial": ratios[chosen], "ratios_temporal": ratios_t[chosen]}) + "\n")


if __name__ == "__main__":
    main()
