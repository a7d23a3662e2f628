"""What the CPU and the GPU tests of the denoiser's history hand-over share (tests/test_denoise_handoff_cpu.py, _gpu.py): the animated
scene, its poses, and the sequence "frames 0-2 on TLAS A, rebind, frames 3-4 on TLAS B" run through the numpy specification."""
from __future__ import annotations

import numpy as np

import denoise_handoff_ref as href
import denoise_temporal_ref as tref
import denoise_variance_ref as vref

N_PARTICLES = 25
SIZES = [(96, 64), (61, 37)]          # 24 whole 256-thread blocks; 2257 pixels = 8 blocks and a partial one, odd sides
POSE_STEP = 0.25                      # animation frames of scenes.particle_poses per test frame: tumbling by at most 0.1 rad, falling 5 mm


def poses(hrt, k):
    """(26, 12) float32: the ground sphere's transform and the particles' at test frame k."""
    s = hrt.scenes
    ground = np.asarray(s.particle_scene(1)["instances"][0]["transform"], np.float32).reshape(12)
    return np.array([ground] + [np.asarray(m, np.float32).reshape(12) for m in s.particle_poses(N_PARTICLES, POSE_STEP * k)], np.float32)


def scene(hrt, w, h):
    sc = hrt.scenes.particle_scene(N_PARTICLES, w, h, 1)
    for it, m in zip(sc["instances"], poses(hrt, 0)):
        it["transform"] = m
    return sc


def camera(hrt, sc):
    c = sc["camera"]
    u, v, w = hrt.configure_camera(c["center"], c["target"], c["up"], c.get("opengl", True))
    return (np.asarray(c["center"], np.float32), u, v, w)


# test frame -> (TLAS, pose): A is load_scene's tree, B the one build_tlas makes; A is updated once (before frame 1), B before frame 4
SEQUENCE = [("A", 0), ("A", 1), ("A", 1), ("B", 2), ("B", 3)]


def spec_frame(oracle, variance, hist, link, color, sc, cam, w, h, instanced=False):
    """One call of the specification on `sc`: linked if link is not None.  Returns {"out", "A", "L", "motion", ("M", "var")} and the history."""
    osc = oracle.OracleScene(sc, instanced=instanced)
    try:
        if variance:
            r = (href.handoff_variance_frame(hist, link, color, osc, sc, cam, w, h) if link is not None
                 else vref.variance_frame(hist, color, osc, sc, cam, w, h))
            names = ("out", "A", "L", "motion", "M", "var")
        else:
            r = (href.handoff_temporal_frame(hist, link, color, osc, sc, cam, w, h) if link is not None
                 else tref.temporal_frame(hist, color, osc, sc, cam, w, h))
            names = ("out", "A", "L", "motion")
    finally:
        osc.close()
    return dict(zip(names, r[:-1])), r[-1]
