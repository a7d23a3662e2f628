"""Sweep of the denoiser's temporal parameters (profiles/r07_denoise_temporal.txt): C1 static (16 frames) and the shipped sample's
Time-mode animation (frames 0..7 of the first step interval), at 1 and 4 spp, against 4096-spp frames of the last pose.  Every setting
runs in a fresh renderer with the same seed, so all see the same frames.  One JSON line per (scene, spp, setting) on stdout;
ratio = MSE(temporal output) / MSE(spatial filter alone on the same raw frame).

    python tools/denoise_temporal_sweep.py > sweep.jsonl
"""
import importlib
import itertools
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
hrt = importlib.import_module("nvidia-optix-ray-tracer_amd")
io = importlib.import_module("nvidia-optix-ray-tracer_amd.io")
SAMPLE = ROOT / "tests" / "golden" / "files" / "config.json"
from test_denoise_temporal_gpu import _edge_pixels  # noqa: E402


def setup(name, r, w, h):
    if name == "c1":
        r.load_scene(hrt.scenes.cornell_box(w, h, 1))
        r.set_frame(w, h, hrt.scenes.SEED_SALT)
        return None
    tm = io.time_mode_scene(SAMPLE, width=w, height=h)
    r.load_scene(tm["scene"])
    r.set_frame(w, h, hrt.scenes.SEED_SALT)
    return tm


def pose(name, r, tm, f):
    if name == "c1":
        return
    cfg = tm["config"]
    r.pose_instances(tm["states"][0], tm["states"][1], float(tm["durations"][0]), f, tm["frame_counts"][0], first_instance=tm["n_extra"],
                     offset=cfg["particle-shift"], scale=cfg["particle-scale"])


def run(name, spp, frames, w, h, tparams):
    r = hrt.Renderer(0, 0)
    try:
        tm = setup(name, r, w, h)
        shares = []
        for f in range(frames):
            pose(name, r, tm, f)
            r.render(spp)
            out = r.denoise_temporal(tparams=tparams)
            if f > 0:
                L = r.denoise_temporal_state()[1].cpu().numpy()
                shares.append(float((L > 1).sum() / max((L > 0).sum(), 1)))
        raw = r.color.cpu().numpy()[..., :3].astype(np.float64)
        temporal = out.cpu().numpy()[..., :3].astype(np.float64)
        spatial = r.denoise().cpu().numpy()[..., :3].astype(np.float64)
        edge = _edge_pixels(r.denoise_guides().cpu().numpy().view(np.uint16))
    finally:
        r.close()
    return raw, temporal, spatial, edge, shares


def reference(name, frames, w, h):
    r = hrt.Renderer(0, 0)
    try:
        tm = setup(name, r, w, h)
        pose(name, r, tm, frames - 1)
        r.render(4096)
        return r.color.cpu().numpy()[..., :3].astype(np.float64)
    finally:
        r.close()


def main():
    f = sys.stdout
    grid = list(itertools.product([0.05, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.75, 0.8, 0.85, 0.9, 0.95], [8, 32], [0.01, 0.02, 0.05]))
    for name, w, h, frames in (("c1", 256, 256, 16), ("sample", 300, 200, 8)):
        t0 = time.time()
        conv = reference(name, frames, w, h)
        print(f"{name}: reference {time.time() - t0:.1f} s", file=sys.stderr, flush=True)
        for spp in (1, 4):
            for a, m, d in grid:
                raw, tmp, spa, edge, shares = run(name, spp, frames, w, h, {"alpha_min": a, "max_history": m, "depth_tolerance": d})
                mse = lambda x: float(((x - conv) ** 2).mean())      # noqa: E731
                emse = lambda x: float(((x - conv) ** 2)[edge].mean())  # noqa: E731
                rec = {"scene": name, "spp": spp, "alpha_min": a, "max_history": m, "depth_tolerance": d,
                       "mse_raw": mse(raw), "mse_spatial": mse(spa), "mse_temporal": mse(tmp), "ratio": mse(tmp) / mse(spa),
                       "edge_raw": emse(raw), "edge_temporal": emse(tmp), "min_share": min(shares)}
                f.write(json.dumps(rec) + "\n")
                f.flush()
            print(f"{name} {spp} spp done {time.time() - t0:.1f} s", file=sys.stderr, flush=True)


if __name__ == "__main__":
    main()
