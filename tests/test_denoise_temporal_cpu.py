"""The denoiser's temporal mode without a GPU: its C ABI's defaults, argument checks and public layout through the built library, and
properties of the numpy specification (tests/denoise_temporal_ref.py) that the GPU tests pin the kernel to, over the oracle's primary
hits."""
import copy
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

import denoise_ref as ref
import denoise_temporal_ref as tref

ROOT = Path(__file__).resolve().parent.parent


def test_temporal_default_params_and_refusals(hrt):
    lib = hrt.load_library()
    p = hrt.DenoiseTemporalParams()
    assert lib.hrt_denoise_temporal_default_params(C.byref(p)) == 0
    assert p.max_history == tref.DEFAULTS["max_history"] and p.reserved == 0
    for k in ("alpha_min", "depth_tolerance"):
        assert getattr(p, k) == np.float32(tref.DEFAULTS[k])
    assert lib.hrt_denoise_temporal_default_params(None) == -1
    gp, rg = hrt.GlobalParams(), hrt.RayGenParams()
    assert lib.hrt_denoise_temporal_launch(None, C.byref(gp), C.byref(rg), None, None, C.c_void_p(16), None) == -1
    assert lib.hrt_denoise_temporal_reset(None) == -1
    assert lib.hrt_debug_denoise_temporal_state(None, None, None, None, None) == -1


def test_temporal_layout(hrt, tmp_path):
    """HrtDenoiseTemporalParams is 16 bytes: checked by the C++ compiler against include/hrt.h, and the ctypes mirror agrees."""
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include "hrt.h"\n'
                   'static_assert(sizeof(HrtDenoiseTemporalParams) == 16 && offsetof(HrtDenoiseTemporalParams, max_history) == 4 &&'
                   ' offsetof(HrtDenoiseTemporalParams, depth_tolerance) == 8, "temporal params");\n'
                   'int main() { return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", f"-I{ROOT / 'include'}", str(src)], check=True)
    assert C.sizeof(hrt.DenoiseTemporalParams) == 16


def _cam(hrt, scene):
    c = scene["camera"]
    u, v, w = hrt.configure_camera(c["center"], c["target"], c["up"], c.get("opengl", True))
    return (np.asarray(c["center"], np.float32), u, v, w)


def _noise(rng, h, w):
    return rng.uniform(0, 1, (h, w, 4)).astype(np.float32)


def test_spec_static_history_grows_to_its_cap(hrt, oracle):
    """Static scene and camera: every hit pixel's history length goes 1, 2, ... and stops at max_history; background stays 0."""
    w, h = 40, 32
    scene = hrt.scenes.cornell_box(w, h, 1)
    cam = _cam(hrt, scene)
    osc = oracle.OracleScene(scene)
    rng = np.random.default_rng(1)
    hist = None
    tp = {"max_history": 4}
    for k in range(1, 7):
        _, A, L, motion, hist = tref.temporal_frame(hist, _noise(rng, h, w), osc, scene, cam, w, h, tparams=tp)
        hit = hist["inst"] != tref.MISS
        assert hit.sum() > 0.5 * w * h
        assert np.all(L[~hit] == 0)
        np.testing.assert_allclose(L[hit], min(k, 4), rtol=1e-5)
        if k >= 4:
            assert np.all(L[hit] == 4)
        if k > 1:                                   # the camera did not move: every hit pixel projects onto itself
            iy, ix = np.nonzero(hit)
            assert np.abs(motion[iy, ix, 0] - ix).max() < 1e-3 and np.abs(motion[iy, ix, 1] - iy).max() < 1e-3
    osc.close()


def _move(scene, k, dx):
    s2 = copy.deepcopy(scene)
    m = np.asarray(s2["instances"][k]["transform"], np.float32).reshape(12).copy()
    m[3] += np.float32(dx)
    s2["instances"][k]["transform"] = m
    return s2


def test_spec_translated_instance_keeps_its_history_and_disocclusions_restart(hrt, oracle):
    """C2's sphere moves sideways between two frames: its pixels find their history where it was (L = 2, motion = the shift);
    the wall pixels it uncovers, whose every tap held the sphere, start afresh (L = 1)."""
    w, h = 64, 64
    scene = hrt.scenes.sphere_in_box(w, h, 1)
    sph = next(i for i, it in enumerate(scene["instances"]) if it["geometry"] == "spheres")
    cam = _cam(hrt, scene)
    rng = np.random.default_rng(2)
    osc0 = oracle.OracleScene(scene)
    _, _, _, _, h0 = tref.temporal_frame(None, _noise(rng, h, w), osc0, scene, cam, w, h)
    moved = _move(scene, sph, 0.08)
    osc1 = oracle.OracleScene(moved)
    _, A, L, motion, h1 = tref.temporal_frame(h0, _noise(rng, h, w), osc1, moved, cam, w, h)
    on_sphere = h1["inst"] == sph
    kept = (L[on_sphere] > 1).mean()
    iy, ix = np.nonzero(on_sphere)
    shift = np.median(motion[iy, ix, 0] - ix)
    print(f"sphere pixels {on_sphere.sum()}, with history {kept:.3f}, median x shift {shift:.2f} px")
    was = h0["inst"] == sph
    moved_px = np.nonzero(was)[1].mean() - ix.mean()         # how far the sphere's image moved between the frames, in x
    assert kept > 0.85
    assert abs(moved_px) > 2 and abs(shift - moved_px) < 1.0
    # uncovered: wall now, sphere in the whole 3x3 neighbourhood before
    core = was.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            core &= np.roll(np.roll(was, dy, 0), dx, 1)
    uncovered = core & (h1["inst"] != sph) & (h1["inst"] != tref.MISS)
    assert uncovered.sum() > 10
    assert np.all(L[uncovered] == 1)
    c_last = A[uncovered]
    assert np.isfinite(c_last).all()
    osc0.close()
    osc1.close()


def test_spec_changed_primitive_rejects_the_tap(hrt, oracle):
    """A history whose (instance, primitive) differs everywhere from this frame's: no tap is taken, A = C and L = 1 on every hit."""
    w, h = 40, 32
    scene = hrt.scenes.cornell_box(w, h, 1)
    cam = _cam(hrt, scene)
    osc = oracle.OracleScene(scene)
    rng = np.random.default_rng(3)
    _, _, _, _, hist = tref.temporal_frame(None, _noise(rng, h, w), osc, scene, cam, w, h)
    c = _noise(rng, h, w)
    for field in ("prim", "inst"):
        bad = dict(hist)
        bad[field] = np.where(hist["inst"] != tref.MISS, hist[field] + np.uint32(100000), hist[field]).astype(np.uint32)
        _, A, L, _, h2 = tref.temporal_frame(bad, c, osc, scene, cam, w, h)
        hit = h2["inst"] != tref.MISS
        assert np.all(L[hit] == 1)
        assert np.array_equal(A.view(np.uint32), c.view(np.uint32))
    _, A, L, _, _ = tref.temporal_frame(hist, c, osc, scene, cam, w, h)          # ... while the true history is taken
    assert np.all(L[hist["inst"] != tref.MISS] == 2)
    osc.close()


def test_spec_first_frame_is_the_spatial_filter(hrt, oracle):
    """Without history the accumulated colour is the colour buffer, so the output is hrt_denoise_launch's."""
    w, h = 32, 24
    scene = hrt.scenes.cornell_box(w, h, 1)
    cam = _cam(hrt, scene)
    osc = oracle.OracleScene(scene)
    c = _noise(np.random.default_rng(4), h, w)
    out, A, _, motion, _ = tref.temporal_frame(None, c, osc, scene, cam, w, h)
    assert np.array_equal(A.view(np.uint32), c.view(np.uint32)) and np.isnan(motion).all()
    want = ref.atrous(c, ref.primary_guides(osc, scene, cam, w, h))
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
    osc.close()

