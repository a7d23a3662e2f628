#!/usr/bin/env python3
"""The history hand-over at Time mode's file boundary, measured on the specification alone -- no GPU: the CPU oracle renders the frames
(its colour buffer is the library's bit for bit) and tests/denoise_handoff_ref.py, denoise_temporal_ref.py denoise them over the
oracle's primary hits.  Figures for profiles/r21_denoise_handoff.txt and the bound of
tests/test_denoise_handoff_gpu.py::test_handoff_quality_at_the_file_boundary.

  python3 tools/denoise_handoff_spec.py [--spp 4096] [--width 120 --height 80]

1. The shipped sample, hrt_time_render's loop at 1 spp: the untimed launch, the 9 frames of file 0, the first frame of file 1 -- that
   one denoised with the hand-over (identity link) and as a fresh start -- against --spp samples of the same pose: MSE of both, of the
   spatial filter and of the raw frame, overall and next to guide edges.
2. The history length over the sample's three files with and without the hand-over (geometry only: the colour plays no part)."""
import argparse
import copy
import importlib
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import denoise_handoff_ref as href      # noqa: E402
import denoise_ref as ref               # noqa: E402
import denoise_temporal_ref as tref     # noqa: E402
import oracle_py                        # noqa: E402
from test_denoise_temporal_gpu import _edge_pixels      # noqa: E402  (the existing quality test's mask)

SAMPLE = ROOT / "tests" / "golden" / "files" / "config.json"


def posed(tm, f, frame):
    """The sample's scene at frame `frame` of file f (None: the identity-posed scene of the untimed launch)."""
    sc = copy.copy(tm["scene"])
    sc["instances"] = [dict(it) for it in tm["scene"]["instances"]]
    if f is not None:
        cfg = tm["config"]
        nxt = tm["states"][min(f + 1, len(tm["states"]) - 1)]
        xf = oracle_py.pose_transforms(tm["states"][f], nxt, float(tm["durations"][f]), frame, tm["frame_counts"][f],
                                       cfg["particle-shift"], cfg["particle-scale"])
        for it, m in zip(sc["instances"][tm["n_extra"]:], xf):
            it["transform"] = m
    return sc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=4096)
    ap.add_argument("--width", type=int, default=120)
    ap.add_argument("--height", type=int, default=80)
    a = ap.parse_args()
    w, h = a.width, a.height
    hrt = importlib.import_module("nvidia-optix-ray-tracer_amd")
    io = importlib.import_module("nvidia-optix-ray-tracer_amd.io")
    tm = io.time_mode_scene(SAMPLE, width=w, height=h)
    c = tm["scene"]["camera"]
    cam = (np.asarray(c["center"], np.float32), *hrt.configure_camera(c["center"], c["target"], c["up"], c.get("opengl", True)))
    per_file = tm["frame_counts"]
    ids = href.blas_ids(tm["scene"])
    link = href.make_link(ids, ids)

    # 1. the boundary frame
    states = oracle_py.rng_init(w, h, hrt.scenes.SEED_SALT)
    hist = None
    steps = [(None, 0)] + [(0, k) for k in range(per_file[0])] + [(1, 0)]
    for f, frame in steps:
        sc = posed(tm, f, frame)
        osc = oracle_py.OracleScene(sc)
        color = osc.render(w, h, states, 1, want_linear=False)["color"]
        if (f, frame) == (1, 0):
            handed, _, L_h, _, _ = href.handoff_temporal_frame(hist, link, color, osc, sc, cam, w, h)
            reset, _, L_r, _, _ = tref.temporal_frame(None, color, osc, sc, cam, w, h)
            guides = ref.primary_guides(osc, sc, cam, w, h)
            t0 = time.time()
            conv = osc.render(w, h, oracle_py.rng_init(w, h, hrt.scenes.SEED_SALT), a.spp, want_linear=False)["color"]
            print(f"({a.spp} spp reference: {time.time() - t0:.0f} s)")
        else:
            _, _, _, _, hist = tref.temporal_frame(hist, color, osc, sc, cam, w, h)
        osc.close()
    spatial = ref.atrous(color, guides)
    assert np.array_equal(spatial.view(np.uint32), reset.view(np.uint32))           # a fresh start IS the spatial filter
    edge = _edge_pixels(guides)
    d = lambda x: ((x[..., :3].astype(np.float64) - conv[..., :3].astype(np.float64)) ** 2)      # noqa: E731
    mse = {k: d(v).mean() for k, v in (("raw", color), ("reset", reset), ("handover", handed))}
    emse = {k: d(v)[edge].mean() for k, v in (("raw", color), ("reset", reset), ("handover", handed))}
    hit = L_h > 0
    print(f"sample {w}x{h}, 1 spp, first frame of file 1 against {a.spp} spp:")
    print(f"  MSE raw {mse['raw']:.6g}  reset (= spatial filter) {mse['reset']:.6g}  hand-over {mse['handover']:.6g}"
          f"  ratio hand-over / reset {mse['handover'] / mse['reset']:.4f}")
    print(f"  next to guide edges ({edge.sum()} px): raw {emse['raw']:.6g}  reset {emse['reset']:.6g}  hand-over {emse['handover']:.6g}"
          f"  hand-over / raw {emse['handover'] / emse['raw']:.4f}")
    print(f"  hit pixels {hit.sum()}, with history (L > 1) {(L_h > 1).sum() / hit.sum():.4f}, mean L {L_h[hit].mean():.2f} (reset: {L_r[hit].mean():.2f})")
    ratio = mse["handover"] / mse["reset"]
    print(f"  bound of the test, halfway between the ratio and 1: {(ratio + 1) / 2:.4f}")

    # 2. the history length over the three files
    zero = np.zeros((h, w, 4), np.float32)
    for handoff in (True, False):
        hist, rows = None, []
        for f in range(len(per_file)):
            for frame in range(per_file[f]):
                sc = posed(tm, f, frame)
                osc = oracle_py.OracleScene(sc)
                dirs = ref.primary_directions(w, h, *cam[1:])
                hits = osc.trace(np.broadcast_to(cam[0], dirs.shape).copy(), dirs)
                xf = np.array([np.asarray(it["transform"], np.float32).reshape(12) for it in sc["instances"]], np.float32)
                inv = tref.world_to_object(osc)
                if frame == 0 and f > 0 and handoff:
                    _, L, _, _, hist = href.handoff_step(hist, link, zero, hits, cam, inv, xf, w, h)
                else:
                    _, L, _, hist = tref.temporal_step(None if frame == 0 and f > 0 else hist, zero, hits, cam, inv, xf, w, h)
                osc.close()
                rows.append((f, frame, L[L > 0].mean(), L.max()))
        print(f"history length L over the sample's files, {'with' if handoff else 'without'} the hand-over (max_history 32): "
              f"longest {max(r[3] for r in rows):.0f}")
        print("   " + "  ".join(f"{f}.{frame}: {m:.1f}" for f, frame, m, _ in rows) + "   (file.frame: mean L of the hit pixels)")


if __name__ == "__main__":
    main()
