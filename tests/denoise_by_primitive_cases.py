"""What the CPU and the GPU tests of the denoiser's hand-over across rebuilt BLASes share (tests/test_denoise_by_primitive_cpu.py,
_gpu.py): tests/denoise_handoff_cases.py's scene and sequence, with TLAS B built over DEFORMED vertices for a fixed half of the
particles -- each of those gets a BLAS of its own, so it is linked by primitive -- while the others keep their shared BLAS and the
ground stays a sphere: every frame on B mixes the rigid and the by-primitive path in one wave."""
from __future__ import annotations

import numpy as np

import denoise_by_primitive_ref as pref
import denoise_handoff_cases as hcases
import denoise_handoff_ref as href
import denoise_temporal_ref as tref
import denoise_variance_ref as vref

N_PARTICLES = hcases.N_PARTICLES
SIZES = hcases.SIZES
SEQUENCE = hcases.SEQUENCE
poses, scene, camera = hcases.poses, hcases.scene, hcases.camera

# the particles whose BLAS is rebuilt for TLAS B: scene instances 1, 3, ..., 25 (instance 0 is the ground sphere) -- 13 of the 25
DEFORMED = list(range(1, N_PARTICLES + 1, 2))

# The deformation, a test input: object-space vertices (blobs of radius 0.05 .. 0.07) scaled by SCALE per axis, then displaced by
# AMPLITUDE sin(FREQUENCY q + phase) with q another component of the vertex -- a smooth, non-affine map of about 5 % of the radius.
SCALE = np.array([1.03, 0.97, 1.02], np.float32)
AMPLITUDE = np.float32(0.003)
FREQUENCY = np.float32(40.0)


def deform(vertices):
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3, 3)
    q = v[..., [1, 2, 0]]
    phase = np.array([0.0, 1.0, 2.0], np.float32)
    return (v * SCALE + AMPLITUDE * np.sin(FREQUENCY * q + phase).astype(np.float32)).astype(np.float32)


def deformed_vertices(hrt, sc, subset=DEFORMED):
    """({j: vertices}, {j: normals}) for Renderer.build_tlas and pref.with_vertices: the subset's deformed meshes and their face normals."""
    verts = {j: deform(sc["instances"][j]["vertices"]) for j in subset}
    return verts, {j: hrt.scenes.face_normals(v) for j, v in verts.items()}


def scene_b(hrt, sc, pose, subset=DEFORMED):
    """The scene TLAS B traces at test frame `pose`."""
    verts, normals = deformed_vertices(hrt, sc, subset)
    return pref.with_vertices(href.sub_scene(sc, None, poses(hrt, pose)), verts, normals, "B")


def spec_frame(oracle, variance, hist, link, color, sc, cam, w, h, instanced=False, diag=None):
    """One call of the specification on `sc`.  link: None (an ordinary call) or (link, by_prim, prev_verts).  Returns
    {"out", "A", "L", "motion", ("M", "var")} and the history."""
    osc = oracle.OracleScene(sc, instanced=instanced)
    try:
        if variance:
            r = (pref.variance_frame(hist, *link, color, osc, sc, cam, w, h) if link is not None
                 else vref.variance_frame(hist, color, osc, sc, cam, w, h))
            names = ("out", "A", "L", "motion", "M", "var")
        else:
            r = (pref.temporal_frame(hist, *link, color, osc, sc, cam, w, h, diag=diag) if link is not None
                 else tref.temporal_frame(hist, color, osc, sc, cam, w, h))
            names = ("out", "A", "L", "motion")
    finally:
        osc.close()
    return dict(zip(names, r[:-1])), r[-1]


def by_primitive_pixels(hist, by_prim):
    """(H, W) bool: the hit pixels of the frame `hist` was left by whose instance is linked by primitive."""
    hit = hist["inst"] != href.MISS
    out = np.zeros_like(hit)
    out[hit] = np.asarray(by_prim, bool)[hist["inst"][hit]]
    return out
