#!/usr/bin/env python3
"""The by-primitive history hand-over at Mesh mode's file boundary, measured on the specification alone -- no GPU: the CPU oracle
renders the frames (its colour buffer is the library's bit for bit) and tests/denoise_by_primitive_ref.py, denoise_temporal_ref.py
denoise them over the oracle's primary hits.  Figures for profiles/r25_denoise_by_primitive.txt and the bound of
tests/test_denoise_by_primitive_gpu.py::test_by_primitive_quality_at_the_file_boundary.

  python3 tools/denoise_by_primitive_spec.py [--spp 4096] [--width 120 --height 80]

io.write_mesh_mode_sample's data set (3 files, 12 particles, ids permuted per file), hrt_mesh_render's loop at 1 spp: the frames of
file 0, then the first frame of file 1 -- that one denoised with the hand-over (by particle id, every particle by primitive, the
ground sphere rigid) and as a fresh start -- against --spp samples of the same pose: MSE of both and of the raw frame, overall and
next to guide edges."""
import argparse
import importlib
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import denoise_by_primitive_ref as pref  # noqa: E402
import denoise_ref as ref               # noqa: E402
import denoise_temporal_ref as tref     # noqa: E402
import oracle_py                        # noqa: E402
from test_denoise_temporal_gpu import _edge_pixels      # noqa: E402  (the existing quality test's mask)


def mesh_transforms(velocities, dur, frame, count, off, sc):
    """Mesh mode's per-frame update (RendererMesh.cu:379-391): shift = offset + (velocity * duration / frames) * frame, no rotation."""
    f = np.float32
    out = np.zeros((len(velocities), 12), np.float32)
    for i, vel in enumerate(np.asarray(velocities, np.float32)):
        per_frame = ((vel * f(dur)).astype(f) / f(count)).astype(f)
        out[i] = oracle_py.construct_transform((np.asarray(off, f) + (per_frame * f(frame)).astype(f)).astype(f), (0, 0, 0), sc)
    return out


def posed(mm, f, frame):
    cfg, n_extra = mm["config"], mm["n_extra"]
    sc = {k: v for k, v in mm["scenes"][f].items() if k != "instances"}
    sc["instances"] = [dict(it) for it in mm["scenes"][f]["instances"]]
    xf = mesh_transforms(mm["velocities"][f], float(mm["durations"][f]), frame, mm["frame_counts"][f], cfg["particle-shift"], cfg["particle-scale"])
    for it, m in zip(sc["instances"][n_extra:], xf):
        it["transform"] = m
    return sc


def file_link(mm, ids, f):
    """(link, by_prim) of hrt_mesh_render's rebind at the boundary into file f: the extra spheres share their BLAS, every particle has
    one of its own per file and is the particle of file f - 1 with its id."""
    n_extra = mm["n_extra"]
    info = lambda k: ([(("extra", i), pref.SPHERES, 1) for i in range(n_extra)] +                                     # noqa: E731
                      [(("file", k, p), pref.TRIANGLES, len(it["vertices"])) for p, it in enumerate(mm["scenes"][k]["instances"][n_extra:])])
    last = {pid: n_extra + p for p, pid in enumerate(ids[f - 1])}
    prev_instance = list(range(n_extra)) + [last.get(pid, int(pref.NO_INSTANCE)) for pid in ids[f]]
    return pref.make_link(info(f - 1), info(f), prev_instance)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=4096)
    ap.add_argument("--width", type=int, default=120)
    ap.add_argument("--height", type=int, default=80)
    a = ap.parse_args()
    w, h = a.width, a.height
    hrt = importlib.import_module("nvidia-optix-ray-tracer_amd")
    io = importlib.import_module("nvidia-optix-ray-tracer_amd.io")
    with tempfile.TemporaryDirectory() as tmp:
        cfg_path = io.write_mesh_mode_sample(tmp, n_files=3, n_particles=12, width=w, height=h)
        mm = io.mesh_mode_scene(cfg_path, width=w, height=h)
        ids = [[p["id"] for p in io.read_mesh_cache(str(Path(tmp) / "cache" / f"particle{k}.cache"))] for k in range(3)]
    c = mm["scenes"][0]["camera"]
    cam = (np.asarray(c["center"], np.float32), *hrt.configure_camera(c["center"], c["target"], c["up"], c.get("opengl", True)))
    per_file = mm["frame_counts"]
    link, by_prim = file_link(mm, ids, 1)
    print(f"link into file 1: {int(by_prim.sum())} of {len(link)} instances by primitive, {int((link == pref.NO_INSTANCE).sum())} new")

    states = oracle_py.rng_init(w, h, hrt.scenes.SEED_SALT)
    hist, prev = None, None
    for f, frame in [(0, k) for k in range(per_file[0])] + [(1, 0)]:
        sc = posed(mm, f, frame)
        osc = oracle_py.OracleScene(sc)
        color = osc.render(w, h, states, 1, want_linear=False)["color"]
        if f == 1:
            handed, _, L_h, _, _ = pref.temporal_frame(hist, link, by_prim, pref.scene_verts(prev), color, osc, sc, cam, w, h)
            reset, _, L_r, _, _ = tref.temporal_frame(None, color, osc, sc, cam, w, h)
            guides = ref.primary_guides(osc, sc, cam, w, h)
            t0 = time.time()
            conv = osc.render(w, h, oracle_py.rng_init(w, h, hrt.scenes.SEED_SALT), a.spp, want_linear=False)["color"]
            print(f"({a.spp} spp reference: {time.time() - t0:.0f} s)")
        else:
            _, _, _, _, hist = tref.temporal_frame(hist, color, osc, sc, cam, w, h)
        osc.close()
        prev = sc
    edge = _edge_pixels(guides)
    d = lambda x: ((x[..., :3].astype(np.float64) - conv[..., :3].astype(np.float64)) ** 2)      # noqa: E731
    mse = {k: d(v).mean() for k, v in (("raw", color), ("reset", reset), ("handover", handed))}
    emse = {k: d(v)[edge].mean() for k, v in (("raw", color), ("reset", reset), ("handover", handed))}
    hit = L_h > 0
    print(f"Mesh-mode sample {w}x{h}, 1 spp, first frame of file 1 (after {per_file[0]} frames of file 0) against {a.spp} spp:")
    print(f"  MSE raw {mse['raw']:.6g}  reset (= spatial filter) {mse['reset']:.6g}  hand-over {mse['handover']:.6g}"
          f"  ratio hand-over / reset {mse['handover'] / mse['reset']:.4f}")
    print(f"  next to guide edges ({edge.sum()} px): raw {emse['raw']:.6g}  reset {emse['reset']:.6g}  hand-over {emse['handover']:.6g}"
          f"  hand-over / raw {emse['handover'] / emse['raw']:.4f}")
    print(f"  hit pixels {hit.sum()}, with history (L > 1) {(L_h > 1).sum() / hit.sum():.4f}, mean L {L_h[hit].mean():.2f} (reset: {L_r[hit].mean():.2f})")
    ratio = mse["handover"] / mse["reset"]
    print(f"  bound of the test, halfway between the ratio and 1: {(ratio + 1) / 2:.4f}")


if __name__ == "__main__":
    main()
