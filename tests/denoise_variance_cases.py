"""The inputs of the variance-guided mode's tests, built deterministically from seeds in the style of tests/denoise_cases.py and shared
by tests/test_denoise_variance_cpu.py (which asserts on the numpy specification that they reach the branches they are for) and
tests/test_denoise_variance_gpu.py (which runs the kernels on exactly these inputs): frames of colour, guides and variance with
parameters for hrt_denoise_filter_variance, and whole sequences for hrt_denoise_variance_launch.

No test functions here."""
from __future__ import annotations

import copy

import numpy as np

import denoise_cases as dc
import denoise_variance_ref as vref

f32 = np.float32

# ---- filter cases: id -> (colour (H, W, 4), guides (H, W, 8) uint16, variance (H, W), params, vparams, in_place, var_out) ---------
SIZES = ((1, 1), (5, 3), (16, 16), (17, 16), (37, 29))          # (width, height)
PASSES = (1, 2, 5, 9)                                           # steps 1 .. 256: beyond every frame above
OTHER_PARAMS = {"sigma_albedo": 0.3, "sigma_depth": 0.1, "normal_power_log2": 1, "sigma_color": 123.0}      # (sigma_color: not used)
OTHER_VPARAMS = {"sigma_luminance": 1.5, "variance_floor": 1e-4, "history_min": 9}                           # (history_min: not the filter's)


def plain_variance(rng, h, w):
    """Variances of luminances in [0, 1]: up to about 0.05, a tenth of them exactly 0."""
    v = (rng.uniform(0, 0.22, (h, w)) ** 2).astype(np.float32)
    v[rng.uniform(size=(h, w)) < 0.1] = 0
    return v


def _plain(name, w, h, iterations, k):
    rng = np.random.default_rng(dc._seed(name))
    guides = dc.random_guides(rng, h, w, background=0.0 if w * h < 16 else 0.08)
    params = {"iterations": iterations}
    vparams = None
    if k % 2:
        params.update(OTHER_PARAMS)
        vparams = dict(OTHER_VPARAMS)
    # in place / out of place and d_var_out NULL / set / the variance itself, in turn
    return dc.plain_color(rng, h, w), guides, plain_variance(rng, h, w), params, vparams, bool((k // 2) % 2), ("set", "null", "same")[k % 3]


HOSTILE_VARIANCES = np.array([0.0, 1e-42, 1e-39, 1e30, dc.FLT_MAX, np.inf, np.nan, -1.0], np.float32)


def _hostile_variance(name):
    """A third of the pixels hold a hostile variance (0, subnormal, huge, inf, NaN, negative); strips where centre and taps all do."""
    w, h = 37, 29
    rng = np.random.default_rng(dc._seed(name))
    c, g, v = dc.plain_color(rng, h, w), dc.random_guides(rng, h, w), plain_variance(rng, h, w)
    kind = rng.integers(0, 3 * len(HOSTILE_VARIANCES), (h, w))
    for k, x in enumerate(HOSTILE_VARIANCES):
        v[kind == k] = x
    v[:3, :] = 0
    v[3:6, :] = f32(1e-42)
    v[6:9, :] = np.where(rng.uniform(size=(3, w)) < 0.5, f32(1e30), dc.FLT_MAX)
    v[9:11, :] = np.inf
    return c, g, v, {"iterations": 3}, None, False, "set"


def _hdr(name):
    """Colours up to 3e38 and negative ones (denoise_cases' hdr): dl * dl overflows, the tap's weight is 0."""
    c, g, _ = dc._hdr("hdr")
    h, w = c.shape[:2]
    rng = np.random.default_rng(dc._seed(name))
    return c, g, plain_variance(rng, h, w), {"iterations": 3}, {"sigma_luminance": 8.0}, True, "set"


def _holes(name):
    """Background holes: a third of the frame in blocks and single pixels, the top left corner's neighbours among them."""
    w, h = 37, 29
    rng = np.random.default_rng(dc._seed(name))
    n, a, z = dc.random_guides(rng, h, w, background=0.25, arrays=True)
    z[10:16, 8:20] = np.inf
    z[0, 0], z[0, 1], z[1, 0], z[1, 1] = 1.5, np.inf, 1.5, np.inf
    return dc.plain_color(rng, h, w), dc._pack(n, a, z), plain_variance(rng, h, w), {"iterations": 4}, None, False, "null"


def _all_hits(name):
    """No background, positive variance everywhere: all four of a corner pixel's 3x3 taps inside the frame count."""
    w, h = 17, 16
    rng = np.random.default_rng(dc._seed(name))
    v = (plain_variance(rng, h, w) + f32(1e-3)).astype(np.float32)
    return dc.plain_color(rng, h, w), dc.random_guides(rng, h, w, background=0.0), v, {"iterations": 1}, None, False, "set"


def _build():
    cases = {}
    k = 0
    for w, h in SIZES:
        for it in PASSES:
            name = f"plain-{w}x{h}-{it}"
            cases[name] = (_plain, (name, w, h, it, k))
            k += 1
    for name, fn in (("hostile-variance", _hostile_variance), ("hdr-negative", _hdr), ("holes", _holes), ("all-hits", _all_hits)):
        cases[name] = (fn, (name,))
    return cases


_FILTER = _build()
FILTER_CASES = list(_FILTER)
# one context through frames that grow and shrink
GROW_SHRINK = ("plain-5x3-2", "plain-37x29-5", "plain-1x1-1", "plain-17x16-9", "hostile-variance", "plain-16x16-2", "plain-37x29-1")


def filter_case(name):
    fn, args = _FILTER[name]
    return fn(*args)


# ---- sequences for hrt_denoise_variance_launch ----------------------------------------------
def _moved(transforms, angle, shift):
    """Every instance rotated by `angle` radians about the z axis through the origin, then shifted by `shift`."""
    c, s = np.cos(angle), np.sin(angle)
    lin = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float64)
    return {i: dc._about(m, lin, [0, 0, 0]) + np.array([0, 0, 0, shift[0], 0, 0, 0, shift[1], 0, 0, 0, shift[2]], np.float32)
            for i, m in enumerate(transforms)}


def sequences(hrt):
    """id -> {"scene", "size", "frames": [{"camera", "transforms"}], "params", "tparams", "vparams", "color", "in_place", "modes"}: six
    frames each, no larger than 64 x 48.  Frame 2 moves every instance (hrt_tlas_update), frame 4 pans the camera; a static pixel's
    history length goes 1, 2, ... so with history_min = 4 the variance changes branch at frame 3."""
    seq = {}
    modes = ("production", "two_level")
    for scene, (w, h) in (("c1", (64, 48)), ("mixed", (61, 47))):
        base = dc.scene_by_name(hrt, scene, w, h)
        cam = base["camera"]
        pan = np.array([0.03, 0.02, 0.0], np.float32)
        cam2 = dc.camera(np.asarray(cam["center"], np.float32) + pan, np.asarray(cam["target"], np.float32) + pan, cam["up"], cam.get("opengl", True))
        moved = _moved([it["transform"] for it in base["instances"]], 0.03, (0.02, -0.01, 0.015))
        frames = [{"camera": cam}, {}, {"transforms": moved}, {}, {"camera": cam2}, {}]
        for hm in (1, 4):
            seq[f"{scene}-hmin{hm}"] = {"scene": scene, "size": (w, h), "frames": frames, "params": {"iterations": 3},
                                        "tparams": {"alpha_min": 0.1}, "vparams": {"history_min": hm}, "modes": modes}
    # defaults everywhere, filtered in place
    seq["c1-defaults"] = {"scene": "c1", "size": (33, 19), "frames": seq["c1-hmin4"]["frames"], "params": None, "tparams": None,
                          "vparams": None, "in_place": True, "modes": ("production",)}
    # colour that is not benign (denoise_cases' hostile colour: HDR values, infinities and NaNs): m2 - m1 m1 = inf - inf
    seq["hostile-color"] = {"scene": "c1", "size": (47, 31), "frames": seq["c1-hmin4"]["frames"], "params": {"iterations": 2},
                            "tparams": {"alpha_min": 0.2}, "vparams": {"history_min": 3}, "color": "hostile", "modes": modes}
    for s in seq.values():
        s.setdefault("color", "plain")
        s.setdefault("in_place", False)
    return seq


def walk(hrt, oracle, name, seq, instanced=False, with_diag=False, hist=None):
    """The specification over the sequence (denoise_cases.walk_sequence's twin).  Yields per frame a dict: k, scene, camera, cam,
    changed, color, want, A, L, motion, M, var, diag (the variance's), hist."""
    w, h = seq["size"]
    cur = copy.deepcopy(dc.scene_by_name(hrt, seq["scene"], w, h))
    cam = cur["camera"]
    osc = None
    try:
        for k, fr in enumerate(seq["frames"]):
            changed = fr.get("transforms", {})
            for i, m in changed.items():
                cur["instances"][i]["transform"] = np.asarray(m, np.float32)
            if changed or osc is None:
                if osc is not None:
                    osc.close()
                osc = oracle.OracleScene(cur, instanced=instanced)
            cam = fr.get("camera", cam)
            color = dc.sequence_color(name, seq, k)
            diag = {} if with_diag else None
            want, A, L, motion, M, var, hist = vref.variance_frame(hist, color, osc, cur, dc.cam_of(hrt, cam), w, h, seq["params"],
                                                                   seq["tparams"], seq["vparams"], diag)
            yield {"k": k, "scene": cur, "camera": cam, "cam": dc.cam_of(hrt, cam), "changed": changed, "color": color, "want": want,
                   "A": A, "L": L, "motion": motion, "M": M, "var": var, "diag": diag, "hist": hist}
    finally:
        if osc is not None:
            osc.close()
