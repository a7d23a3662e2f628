"""The denoiser's edge cases, built deterministically from seeds and shared by tests/test_denoise_edges_cpu.py (which asserts on the
numpy specifications that every case reaches the expression it is for) and tests/test_denoise_edges_gpu.py (which runs the kernels on
exactly these inputs): frames of colour with guide arrays and parameters for the filter, scenes and frame sizes for the guide pass,
and whole sequences -- scene, per-frame instance transforms, camera and colour, parameters -- for the temporal mode.  The temporal
entry point filters Renderer.color, an ordinary device tensor, so a sequence brings its own colour and nothing is rendered.

No test functions here.  `hrt` is the product package (the conftest fixture), passed in where scenes are needed."""
from __future__ import annotations

import copy

import numpy as np

import denoise_ref as ref
import denoise_temporal_ref as tref

f32 = np.float32
FLT_MAX = np.finfo(np.float32).max
FLT_MIN = np.finfo(np.float32).tiny            # the smallest normal float32


# ---- comparison rule ------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(got, want):
    """Equal NaN masks, and the same bits everywhere else.  (The payload of a computed NaN is not compared.)"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    gn, wn = np.isnan(got), np.isnan(want)
    return got.shape == want.shape and np.array_equal(gn, wn) and np.array_equal(bits(np.where(gn, 0, got)), bits(np.where(wn, 0, want)))


def first_difference(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    gn, wn = np.isnan(got), np.isnan(want)
    d = np.argwhere((gn != wn) | (bits(np.where(gn, 0, got)) != bits(np.where(wn, 0, want))))
    if d.size == 0:
        return None
    i = tuple(d[0])
    return i, float(got[i]), float(want[i]), hex(int(bits(got)[i])), hex(int(bits(want)[i]))


def same_rgba(got, want):
    """A colour frame: red, green, blue under `same`, the alpha channel -- a copy of the input's -- on raw bits, NaN payloads included."""
    return same(got[..., :3], want[..., :3]) and np.array_equal(bits(got[..., 3]), bits(want[..., 3]))


def nan_payloads(got, want):
    """(NaNs both sides hold, those of them whose bits differ): what is seen of the two instruction sets' default NaNs."""
    both = np.isnan(got) & np.isnan(want)
    return int(both.sum()), int((bits(got)[both] != bits(want)[both]).sum())


# ---- colour ---------------------------------------------------------------------------------
def alpha_bits(rng, h, w):
    """Random bit patterns for the alpha channel: every third row has all exponent bits set (infinities, quiet and signalling NaNs
    with random payloads)."""
    a = rng.integers(0, 1 << 32, (h, w), dtype=np.uint64).astype(np.uint32)
    a[::3] |= np.uint32(0x7F800000)
    a[0, 0] = np.uint32(0x7FC12345)
    return a.view(np.float32)


def plain_color(rng, h, w):
    c = (rng.uniform(0, 1, (h, w, 4)) ** 2).astype(np.float32)
    c[..., 3] = alpha_bits(rng, h, w)
    return c


def random_guides(rng, h, w, background=0.08, arrays=False):
    """Guides with structure (tests/test_denoise_gpu.py's): blocks of a few normals and albedos, smooth depth with steps, some background."""
    by, bx = np.meshgrid(np.arange(h) // 7, np.arange(w) // 5, indexing="ij")
    dirs = np.array([[0, 0, 1], [0, 1, 0], [0.6, 0, 0.8], [-0.8, 0.6, 0], [0, -0.6, -0.8]], np.float32)
    n = dirs[(by * 3 + bx) % 5] + rng.normal(0, 0.05, (h, w, 3)).astype(np.float32)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    a = np.array([[0.73, 0.73, 0.73], [0.65, 0.05, 0.05], [0.12, 0.45, 0.15]], np.float32)[(by + bx) % 3]
    z = (1.0 + 0.01 * np.arange(w)[None, :] + 0.3 * ((by + 2 * bx) % 4)).astype(np.float32) + rng.uniform(0, 0.01, (h, w)).astype(np.float32)
    z[rng.uniform(size=(h, w)) < background] = np.inf
    return (n.astype(np.float32), a.copy(), z) if arrays else ref.pack_guides(n, a, z)


def _pack(n, a, z):
    with np.errstate(all="ignore"):
        return ref.pack_guides(n, a, z)


# ---- filter cases: id -> (colour (H, W, 4), guides (H, W, 8) uint16, params) -----------------
def _seed(name):
    return int.from_bytes(name.encode(), "little") % (1 << 63)


def _plain(name, w, h, params):
    rng = np.random.default_rng(_seed(name))
    return plain_color(rng, h, w), random_guides(rng, h, w), params


def _npow8(name):
    """normal_power_log2 = 8: normals in one plane at random angles, so that n . n' runs from cos(1.5) to 1 and (n . n')^256 through
    the normal range, the subnormals (n . n' about 0.67 to 0.71) and 0."""
    w, h = 67, 45
    rng = np.random.default_rng(_seed(name))
    _, a, z = random_guides(rng, h, w, arrays=True)
    th = rng.uniform(0, 1.5, (h, w))
    th[:, : w // 3] = rng.uniform(0, 0.08, (h, w // 3))                    # a third with nearly parallel normals: weights in the normal range
    n = np.stack([np.sin(th), np.zeros_like(th), np.cos(th)], axis=-1).astype(np.float32)
    return plain_color(rng, h, w), _pack(n, a, z), {"iterations": 3, "normal_power_log2": 8}


def _dark(name):
    w, h = 33, 17
    rng = np.random.default_rng(_seed(name))
    c = plain_color(rng, h, w)
    c[..., :3] = (rng.integers(1, 1 << 20, (h, w, 3)).astype(np.uint32)).view(np.float32)        # subnormals up to 1.5e-39
    return c, random_guides(rng, h, w), {"iterations": 3}


def _hdr(name):
    """Colours up to 3e38 next to ordinary ones: dr * dr overflows, dc2 = inf, the tap's weight is 0 (and 0 * 3e38 = 0, not NaN)."""
    w, h = 47, 31
    rng = np.random.default_rng(_seed(name))
    c = plain_color(rng, h, w)
    e = rng.choice([1.0, 1e10, 1e19, 1e25, 3e38], size=(h, w, 1), p=[0.5, 0.1, 0.1, 0.1, 0.2])
    c[..., :3] = (c[..., :3].astype(np.float64) * e).astype(np.float32)
    c[..., :3] *= rng.choice([1.0, -1.0], size=(h, w, 1), p=[0.8, 0.2]).astype(np.float32)         # negatives among them
    return c, random_guides(rng, h, w), {"iterations": 4, "sigma_color": 4.0}


FIREFLY_ITERATIONS = (1, 3, 5)


def _fireflies(name, iterations):
    """30 pixels of 257 x 61 (0.19 %) hold +inf, -inf or NaN in a colour channel, all of them left of x = 64: five passes carry a
    pixel 62 columns far at the most, so the right of the frame stays finite in every pass count."""
    w, h = 257, 61
    rng = np.random.default_rng(_seed("fireflies"))                         # one frame for every pass count
    c, g = plain_color(rng, h, w), random_guides(rng, h, w)
    ys, xs, ch = rng.integers(0, h, 30), rng.integers(0, 64, 30), rng.integers(0, 3, 30)
    c[ys, xs, ch] = np.array([np.inf, -np.inf, np.nan], np.float32)[np.arange(30) % 3]
    return c, g, {"iterations": iterations}


HOSTILE_DEPTHS = np.array([-0.0, -1.5, np.nan, -np.inf, 1e-40, 1e-30, 1e30, FLT_MAX], np.float32)


def _hostile_depth(name):
    w, h = 49, 33
    rng = np.random.default_rng(_seed(name))
    n, a, z = random_guides(rng, h, w, arrays=True)
    kind = rng.integers(0, 3 * len(HOSTILE_DEPTHS), (h, w))                # a third of the pixels, each value alike
    for k, v in enumerate(HOSTILE_DEPTHS):
        z[kind == k] = v
    z[:6, :] = np.where(rng.uniform(size=(6, w)) < 0.5, f32(1e-30), f32(1.5e-30))      # strips where centre and taps are both extreme
    z[6:10, :] = np.where(rng.uniform(size=(4, w)) < 0.5, f32(1e30), f32(1.01e30))
    z[10:13, :] = np.where(rng.uniform(size=(3, w)) < 0.5, f32(1e-40), f32(3e-40))
    z[13:15, :] = FLT_MAX
    return plain_color(rng, h, w), _pack(n, a, z), {"iterations": 3, "sigma_depth": 0.5}


def _hostile_normals(name):
    """Normals zero, of length 3, with a NaN or an infinite half, opposite to their neighbours'; albedos 65504 and 1e5 (half infinity)."""
    w, h = 49, 33
    rng = np.random.default_rng(_seed(name))
    n, a, z = random_guides(rng, h, w, arrays=True)
    kind = rng.integers(0, 12, (h, w))
    n[kind == 0] = 0
    n[kind == 1] *= f32(3)
    n[kind == 2, 0] = np.nan
    n[kind == 3, 1] = np.inf
    n[kind == 4, 2] = 1e6                                                   # rounds to a half infinity
    n[kind == 5] *= f32(-1)
    ak = rng.integers(0, 8, (h, w))
    a[ak == 0] = 65504
    a[ak == 1, 1] = 1e5
    return plain_color(rng, h, w), _pack(n, a, z), {"iterations": 3, "normal_power_log2": 1}


def _all_background(name):
    w, h = 17, 16
    rng = np.random.default_rng(_seed(name))
    n, a, z = random_guides(rng, h, w, arrays=True)
    z[:] = np.inf
    return plain_color(rng, h, w), _pack(n, a, z), {"iterations": 3}


def _single_hit(name):
    c, g, p = _all_background(name)
    n, a, z = ref.unpack_guides(g)
    z = z.copy()
    z[7, 9] = 2.0
    return c, _pack(n, a, z), p


def _ringed_hit(name):
    """Hit pixels whose eight neighbours are background, in a frame of hits."""
    w, h = 33, 17
    rng = np.random.default_rng(_seed(name))
    n, a, z = random_guides(rng, h, w, background=0.0, arrays=True)
    for y, x in ((4, 5), (8, 20), (12, 30)):
        z[y - 1: y + 2, x - 1: x + 2] = np.inf
        z[y, x] = 1.5
    return plain_color(rng, h, w), _pack(n, a, z), {"iterations": 3}


def _build_filter_cases():
    cases = {}

    def add(name, fn, *args):
        cases[name] = (fn, (name,) + args)

    add("npow8", _npow8)
    add("dark", _dark)
    add("hdr", _hdr)
    for it in FIREFLY_ITERATIONS:
        add(f"fireflies-{it}", _fireflies, it)
    add("hostile-depth", _hostile_depth)
    add("hostile-normals", _hostile_normals)
    add("all-background", _all_background)
    add("single-hit", _single_hit)
    add("ringed-hit", _ringed_hit)
    for w in (15, 16, 17, 31, 32, 33):                                       # the 16 x 16 workgroup's edges
        for h in (1, 16, 17):
            add(f"tile-{w}x{h}", _plain, w, h, {"iterations": 2, "normal_power_log2": 0 if h == 1 else 3})
    add("strip-1x300", _plain, 1, 300, {"iterations": 5})
    add("strip-300x1", _plain, 300, 1, {"iterations": 5})
    for s, it in ((4, 3), (16, 5), (64, 7)):                                 # the last pass's outer tap just outside / on the last pixel
        add(f"outer-tap-{2 * s}x3", _plain, 2 * s, 3, {"iterations": it})
        add(f"outer-tap-{2 * s + 1}x3", _plain, 2 * s + 1, 3, {"iterations": it})
    for it in (9, 12, 16):                                                   # steps far beyond the frame: only the centre tap is left
        add(f"deep-{it}-17x5", _plain, 17, 5, {"iterations": it, "sigma_color": 2.0})
    add("deep-9-523x3", _plain, 523, 3, {"iterations": 9})                   # step 256 still finds neighbours (x + 256, x + 512)
    return cases


_FILTER = _build_filter_cases()
FILTER_CASES = list(_FILTER)


def filter_case(name):
    fn, args = _FILTER[name]
    return fn(*args)


def filter_case_size(name):
    """(width, height) without building the case."""
    fn, args = _FILTER[name]
    if fn is _plain:
        return args[1], args[2]
    c = filter_case(name)[0]
    return c.shape[1], c.shape[0]


# constants that leave the finite range at a later pass only (hrt_denoise.cpp pass_constants): refused with 16 iterations, valid with 5.
#   sigma_color 1e-15: pass 15 has sc = 1e-15 * 2^-15 = 3.05e-20, sc^2 = 9.3e-40, 1 / sc^2 = 1.07e39 > FLT_MAX; pass 4 has 1 / 3.9e-33
#   sigma_depth 2e34:  pass 15 has 2e34 * 32768 = 6.6e38 > FLT_MAX; pass 4 has 3.2e35
LATE_REFUSALS = ({"sigma_color": 1e-15}, {"sigma_depth": 2e34})


# ---- scenes ---------------------------------------------------------------------------------
def camera(center, target, up=(0, 1, 0), opengl=True):
    return {"center": np.asarray(center, np.float32), "target": np.asarray(target, np.float32), "up": np.asarray(up, np.float32), "opengl": opengl}


def cam_of(hrt, cam):
    """(center, U, V, W) as Renderer.set_camera derives it."""
    u, v, w = hrt.configure_camera(cam["center"], cam["target"], cam["up"], cam.get("opengl", True))
    return (np.asarray(cam["center"], np.float32), u, v, w)


def degenerate_normals_scene(hrt):
    """Four quads in the plane z = 1 seen through a non-OpenGL camera, with vertex normals that are zero, 1e-7 long (both below the
    normalisation's 1e-6 threshold: the fallback normal), 1e-5 long (above it), mixed per vertex (the interpolated normal crosses the
    threshold inside a triangle) and of unit length; one albedo of 1e5 and 7e4, which round to half infinities."""
    s = hrt.scenes
    inst = []
    lengths = ((0.0, 0.0, 0.0), (1e-7, 1e-7, 1e-7), (1e-5, 1e-5, 1e-5), (0.0, 1e-7, 2e-6), (1.0, 1.0, 1.0))
    albedos = (s.WHITE, s.RED, np.array([1e5, 0.5, 7e4], np.float32), s.GREEN, s.SAND)
    for k, (ln, alb) in enumerate(zip(lengths, albedos)):
        x0, x1 = 0.2 * k, 0.2 * (k + 1)
        tris = s._quad([x0, 0, 1], [x1, 0, 1], [x1, 1, 1], [x0, 1, 1])
        it = s._tri_instance(tris, alb)
        nrm = np.zeros((2, 3, 3), np.float32)
        nrm[:, :, 2] = -np.asarray(ln, np.float32)[None, :]
        nrm[1, :, 0] = np.asarray(ln, np.float32) * f32(0.5)                # the second triangle's normals lean, so the guides differ
        it["normals"] = nrm
        inst.append(it)
    return {"name": "degenerate-normals", "instances": inst, "camera": camera([0.5, 0.5, -1.0], [0.5, 0.5, 0.9], opengl=False),
            "background": s.BACKGROUND.copy(), "width": 97, "height": 61, "spp": 1}


def scene_by_name(hrt, name, w, h):
    s = hrt.scenes
    if name == "c1":
        return s.cornell_box(w, h, 1)
    if name == "mixed":
        return s.mixed_test_scene(width=w, height=h, transforms=True)
    if name == "degenerate":
        return degenerate_normals_scene(hrt)
    if name == "wall":
        return wall_scene(hrt)
    raise KeyError(name)


# (scene, width, height): pixel counts that are no multiple of 256 or 64, aspect ratios far from 1
GUIDE_CASES = [("c1", 97, 61), ("mixed", 97, 61), ("degenerate", 97, 61), ("degenerate", 33, 17), ("c1", 1, 1), ("c1", 1, 37),
               ("mixed", 255, 1), ("c1", 257, 3)]


# ---- temporal sequences ----------------------------------------------------------------------
def _c1_cam(hrt, pan=(0, 0, 0), zoom=1.0, up=(0, 1, 0), opengl=True, dolly=0.0):
    c = hrt.scenes.cornell_box(8, 8, 1)["camera"]
    center = np.asarray(c["center"], np.float64) + np.asarray(pan, np.float64) + np.array([0, 0, dolly])
    w = (np.asarray(c["target"], np.float64) - np.asarray(c["center"], np.float64)) * zoom
    return camera(center, center + w, up, opengl)


def _about(m, lin, pivot):
    """The instance transform m (12 floats) followed by the linear map `lin` about the point `pivot`."""
    m = np.asarray(m, np.float64).reshape(3, 4)
    lin, pivot = np.asarray(lin, np.float64), np.asarray(pivot, np.float64)
    out = np.concatenate([lin @ m[:, :3], (lin @ (m[:, 3] - pivot) + pivot)[:, None]], axis=1)
    return out.astype(np.float32).reshape(12)


def wall_scene(hrt):
    """One wall in the plane x = 1, for the cameras of the `nonfinite` sequence."""
    s = hrt.scenes
    tris = s._quad([1, -4, -4], [1, 4, -4], [1, 4, 4], [1, -4, 4])
    return {"name": "wall", "instances": [s._tri_instance(tris, s.WHITE)], "camera": camera([0, 0, 0], [0, 0, 1e19]),
            "background": s.BACKGROUND.copy(), "width": 33, "height": 17, "spp": 1}


def temporal_sequences(hrt):
    """id -> {"scene": name, "size": (w, h), "frames": [{"camera": ..., "transforms": {instance: 12 floats}}, ...], "params", "tparams",
    "color": "plain" | "hostile", "in_place": bool, "modes": (...)}.  A frame without "camera" keeps the one before."""
    all_modes = ("production", "counting", "two_level")
    seq = {}
    pans = [(0.02 * k, 0.01 * k, 0.0) for k in range(8)]
    # alpha = max(1 / L, alpha_min) takes its 1 / L side
    seq["alpha-small"] = {"scene": "c1", "size": (97, 61), "frames": [{"camera": _c1_cam(hrt, pans[k])} for k in range(5)],
                          "params": {"iterations": 3, "sigma_color": 0.8, "normal_power_log2": 1}, "tparams": {"alpha_min": 0.05},
                          "in_place": True, "modes": all_modes}
    # the clamp of the history length, at 3 and at the default 32
    seq["cap-3"] = {"scene": "c1", "size": (97, 61), "frames": [{"camera": _c1_cam(hrt, pans[k % 3])} for k in range(7)],
                    "params": None, "tparams": {"max_history": 3, "alpha_min": 0.1}, "modes": all_modes}
    seq["cap-default-static"] = {"scene": "c1", "size": (33, 19), "frames": [{"camera": _c1_cam(hrt)}] + [{} for _ in range(39)],
                                 "params": {"iterations": 2}, "tparams": None, "modes": ("production",)}
    # the camera inside the room turns from the back wall to the right wall, then to the open front: s <= 0
    eye = [0.3, 0.7, 0.25]
    seq["turn"] = {"scene": "c1", "size": (97, 61),
                   "frames": [{"camera": camera(eye, [0.3, 0.7, 1.0])}, {"camera": camera(eye, [1.05, 0.7, 0.25])},
                              {"camera": camera(eye, [0.3, 0.65, -0.5])}, {"camera": camera(eye, [0.3, 0.7, 1.0])}],
                   "params": {"iterations": 4}, "tparams": {"alpha_min": 0.3}, "modes": all_modes}
    # pan, zoom, roll, a non-OpenGL camera: reprojections that leave the frame on every side and at its corners
    roll = (np.sin(0.5), np.cos(0.5), 0.0)
    seq["pan-zoom-roll"] = {"scene": "c1", "size": (97, 61),
                            "frames": [{"camera": _c1_cam(hrt)}, {"camera": _c1_cam(hrt, (0.55, 0.0, 0.0))},
                                       {"camera": _c1_cam(hrt, zoom=1.7)}, {"camera": _c1_cam(hrt, zoom=1.7, up=roll)},
                                       {"camera": _c1_cam(hrt, zoom=1.7, up=roll, opengl=False)},
                                       {"camera": _c1_cam(hrt, (0.013, 0.017, 0.0), zoom=1.7, opengl=False)},
                                       {"camera": _c1_cam(hrt, (-0.11, -0.09, 0.0), zoom=1.7)},
                                       {"camera": _c1_cam(hrt, (0.2, 0.15, 0.0), zoom=2.5)}],
                            "params": {"iterations": 2, "sigma_depth": 0.1}, "tparams": {"alpha_min": 0.2, "max_history": 4},
                            "modes": all_modes}
    # the depth test alone decides
    moving = [{"camera": _c1_cam(hrt, (0.03 * k, 0.02 * k, 0.0), dolly=0.05 * k)} for k in range(3)]
    seq["depth-tight"] = {"scene": "c1", "size": (97, 61), "frames": moving, "params": None,
                          "tparams": {"depth_tolerance": 1e-6, "alpha_min": 0.2}, "modes": all_modes}
    seq["depth-loose"] = {"scene": "c1", "size": (97, 61), "frames": moving, "params": None,
                          "tparams": {"depth_tolerance": 10.0, "alpha_min": 0.2}, "modes": all_modes}
    # instances: one moved in front of the others, one turned by 90 degrees, one scaled unevenly
    mixed = hrt.scenes.mixed_test_scene(width=97, height=61, transforms=True)
    xf = [np.asarray(it["transform"], np.float32) for it in mixed["instances"]]
    rot90 = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    seq["instances"] = {"scene": "mixed", "size": (97, 61),
                        "frames": [{}, {"transforms": {3: _about(xf[3], np.eye(3), [0, 0, 0]) + np.array([0, 0, 0, 0.3, 0, 0, 0, 0.1, 0, 0, 0, -0.4], np.float32)}},
                                   {"transforms": {0: _about(xf[0], rot90, [0, 0, 0])}},
                                   {"transforms": {2: _about(xf[2], np.diag([1.3, 0.8, 1.0]), [0, 0, 0])}},
                                   {"transforms": {1: _about(xf[1], np.diag([0.9, 1.0, 1.2]), [0.1, 0, 0])}}],
                        "params": {"iterations": 3}, "tparams": {"alpha_min": 0.2, "depth_tolerance": 0.05}, "modes": all_modes}
    # frame sizes that fill no block and no wavefront
    for w, h in ((1, 1), (1, 37), (255, 1), (257, 3)):
        seq[f"size-{w}x{h}"] = {"scene": "c1", "size": (w, h), "frames": [{"camera": _c1_cam(hrt, pans[k], zoom=1.5)} for k in range(3)],
                                "params": {"iterations": 2}, "tparams": {"alpha_min": 0.05, "max_history": 2}, "modes": all_modes}
    # colour that is not benign: HDR values, and from the second frame on a few infinities and NaNs
    seq["hostile-color"] = {"scene": "c1", "size": (61, 47), "frames": [{"camera": _c1_cam(hrt, pans[k])} for k in range(4)],
                            "params": {"iterations": 2}, "tparams": {"alpha_min": 0.3}, "color": "hostile", "modes": all_modes}
    # a reprojection that is not finite: both cameras at the origin with |W| = 1e19, the first along +z, the second along +x onto the
    # wall x = 1.  A hit has r.z = ndcy * 1e-19, s = r.z / 1e19 of the order 1e-39 and ndcx = 1 / (s aspect) beyond FLT_MAX.
    seq["nonfinite"] = {"scene": "wall", "size": (33, 17),
                        "frames": [{"camera": camera([0, 0, 0], [0, 0, 1e19])}, {"camera": camera([0, 0, 0], [1e19, 0, 0])},
                                   {"camera": camera([0, 0, 0], [0, 0, 1e19])}, {"camera": camera([0, 0, 0], [1e19, 0, 0])}],
                        "params": {"iterations": 1}, "tparams": {"alpha_min": 0.1}, "modes": all_modes}
    # index arithmetic at full size
    seq["full-size-pan"] = {"scene": "c1", "size": (1920, 1080), "frames": [{"camera": _c1_cam(hrt)}, {"camera": _c1_cam(hrt, (0.03, 0.02, 0.0))}],
                            "params": {"iterations": 2}, "tparams": {"alpha_min": 0.05}, "modes": ("production",), "gpu_only": True}
    for s in seq.values():
        s.setdefault("color", "plain")
        s.setdefault("in_place", False)
    return seq


def sequence_color(name, seq, k):
    """The colour buffer of frame k."""
    w, h = seq["size"]
    rng = np.random.default_rng(_seed(name) + k)
    c = plain_color(rng, h, w)
    if seq["color"] == "hostile":
        e = rng.choice([1.0, 1e19, 3e38], size=(h, w, 1), p=[0.7, 0.15, 0.15])
        c[..., :3] = (c[..., :3].astype(np.float64) * e).astype(np.float32)
        if k >= 1:
            m = max(1, w * h // 200)
            c[rng.integers(0, h, m), rng.integers(0, w, m), rng.integers(0, 3, m)] = np.array([np.inf, -np.inf, np.nan], np.float32)[np.arange(m) % 3]
    return c


def walk_sequence(hrt, oracle, name, seq, instanced=False, with_diag=False):
    """The specification over the sequence.  Yields per frame a dict: k, scene (with this frame's transforms), camera (the case's
    dict), cam (center, U, V, W), changed (instance -> transform set before this frame), color, want, A, L, motion, diag, hist.
    A generator: the GPU test steps its renderer frame by frame alongside."""
    w, h = seq["size"]
    cur = copy.deepcopy(scene_by_name(hrt, seq["scene"], w, h))
    cam = cur["camera"]
    hist = None
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
            color = sequence_color(name, seq, k)
            diag = {} if with_diag else None
            want, A, L, M, hist = tref.temporal_frame(hist, color, osc, cur, cam_of(hrt, cam), w, h, seq["params"], seq["tparams"], diag)
            yield {"k": k, "scene": cur, "camera": cam, "cam": cam_of(hrt, cam), "changed": changed, "color": color, "want": want,
                   "A": A, "L": L, "motion": M, "diag": diag, "hist": hist}
    finally:
        if osc is not None:
            osc.close()
