"""Hostile normals, materials, radiance values and cameras: one deterministic generator of small scenes (a plain module like ray_cases.py
and denoise_cases.py, shared by test_shading_cases_cpu.py, test_shading_cases_gpu.py and tools/stress_modes.py).

The traversal half of a path is pinned by ray_cases.py; this is the shading half (csrc/trav_common.h: normalize3, hit_normal, scatter_at,
scatter_programs, program_draws, fold_chain, primary_direction; oracle.c: closesthit_impl, raygen_program), which is mostly guards for
data no benign scene holds: normals that are zero, tiny, huge or non-finite (quirk Q2 hands vertex normals through as they are, quirk Q1
makes a transformed sphere's normal as long as its translation), metal fuzz that is negative, denormal, huge or NaN, albedos and
backgrounds that overflow, and camera bases normalize3 gives up on.

Every scene is a room of a few dozen triangles (the unit Cornell walls closed by a front wall, two boxes in it, a second shell around
it that catches what goes straight through a wall), rendered at 61 x 37 -- not a multiple of 64 pixels nor of 4 rows -- with 4 samples and
then 1 more on the same RNG streams.  Every scattered direction stays within the lengths DESIGN.md section 3 states for rays, 1e-30 .. 1e30:
the largest normal and the largest finite fuzz are 1e30.

CASES maps a name to (make(scenes) -> scene dict, {oracle branch counter: least count the case is there for}); the counters are
oracle_py.SHADE_COUNTERS.  Nothing here knows the product: the conditions are judged on the oracle alone (test_shading_cases_cpu.py)."""
import numpy as np

WIDTH, HEIGHT, SPP = 61, 37, (4, 1)
REACH = 32                                  # closest-hit invocations that take a branch, at least, in the case made for it

NORMAL_LENGTHS = (0.0, -0.0, 1e-30, 1e-7, float(np.nextafter(np.float32(1e-6), np.float32(0))), 1e-6, float(np.nextafter(np.float32(1e-6), np.float32(1))),
                  1e-3, 1.0, 37.0, 1e15, 1e19, 1e30)
# the order they are dealt in.  A direction of 1e15 and more finds nothing (a room's hits lie below tmin = 1e-6 of such a ray) and ends its
# path in the background, so the lengths that keep a path in the room come round twice: 3 triangles in 20 end it, not 3 in 13.
_LENGTH_DEAL = NORMAL_LENGTHS + (37.0, 1e-7, 1.0, NORMAL_LENGTHS[4], 1e-3, 0.0, NORMAL_LENGTHS[6])
FUZZ_VALUES = (-1.0, -0.0, 0.0, 1e-45, 1e-38, 1.1754944e-38, 1e-7, 1.0, 2.0, 1e30, float("inf"), float("nan"))
RADIANCE_VALUES = (0.0, -0.0, -0.5, 1.0, 4.0, 1e30, 1e-30, 1e-45, float("inf"), float("-inf"), float("nan"))
NON_FINITE_KINDS = ("nan-one", "nan-all", "plus-inf", "minus-inf", "inf-one")

_NAN, _INF = float("nan"), float("inf")


# ---------------------------------------------------------------------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------------------------------------------------------------------
def _shell(sc, front=True):
    """The unit Cornell walls (10 triangles) and the wall that closes them at z = 0 (2 more)."""
    white, red, green = sc._cornell_walls()
    tris = list(white) + list(red) + list(green)
    if front:
        tris += sc._quad([0, 0, 0], [0, 1, 0], [1, 1, 0], [1, 0, 0])
    return np.asarray(tris, np.float32)


def _outer(sc):
    return np.asarray(sc._box((-0.5, -0.5, -0.5), (1.5, 1.5, 1.5), skip_bottom=False), np.float32)


def _cube(sc, half):
    return np.asarray(sc._box((-half,) * 3, (half,) * 3, skip_bottom=False), np.float32)


def _box_poses(sc):
    """Two boxes afloat in the room, turned (and one of them scaled): quirk Q2 leaves their normals in object space, and a two-level tree
    keeps their triangles there."""
    return (sc.rigid_transform((0.30, 0.22, 0.34), (1, 2, 0.5), 0.4), sc.rigid_transform((0.68, 0.40, 0.62), (0.3, 1, 0), -0.7, 1.3))


def _camera(center=(0.5, 0.5, 0.03), target=(0.5, 0.45, 1.03)):
    return {"center": np.asarray(center, np.float32), "target": np.asarray(target, np.float32), "up": np.array([0, 1, 0], np.float32), "opengl": True}


def _scene(sc, name, instances, camera=None, background=None):
    return {"name": "shading-" + name, "instances": instances, "camera": camera or _camera(),
            "background": sc.BACKGROUND.copy() if background is None else np.asarray(background, np.float32), "width": WIDTH, "height": HEIGHT, "spp": SPP[0]}


def _scaled_normals(sc, tris, lengths):
    """Flat normals: the unit face normal times the triangle's length; a length of +-0 gives that zero in every component."""
    n = sc.face_normals(tris)
    lengths = np.asarray(lengths, np.float32)
    out = (n * lengths[:, None, None]).astype(np.float32)
    zero = lengths == 0
    out[zero] = lengths[zero][:, None, None]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------------------
def _material_parts(sc):
    """The room as ten groups of triangles with a transform and a material each: half of them rough, the others metal with fuzz 0 or
    0.3.  (triangles, transform, material, fuzz, albedo)"""
    shell, outer = _shell(sc), _outer(sc)
    pa, pb = _box_poses(sc)
    a, b = _cube(sc, 0.13), _cube(sc, 0.11)
    parts = [(shell[0::4], None, "rough", 0.0, sc.WHITE), (shell[1::4], None, "metal", 0.0, sc.STEEL),
             (shell[2::4], None, "rough", 0.0, sc.RED), (shell[3::4], None, "metal", 0.3, sc.STEEL),
             (outer[0::2], None, "rough", 0.0, sc.SAND), (outer[1::2], None, "metal", 0.0, sc.STEEL),
             (a[0::2], pa, "rough", 0.0, sc.GREEN), (a[1::2], pa, "metal", 0.3, sc.STEEL),
             (b[0::2], pb, "rough", 0.0, sc.WHITE), (b[1::2], pb, "metal", 0.0, sc.STEEL)]
    return parts


def _dealt(sc, deal):
    """The room of _material_parts with each triangle's normals made by deal(k, triangles (1, 3, 3)) -> (1, 3, 3), k counting the rough
    triangles and the metal ones apart (24 each), so that each material sees every value."""
    inst, k = [], {"rough": 0, "metal": 7}
    for tris, m, material, fuzz, albedo in _material_parts(sc):
        it = sc._tri_instance(tris, albedo, material, fuzz, m)
        it["normals"] = np.concatenate([deal(k[material] + j, tris[j:j + 1]) for j in range(len(tris))]).astype(np.float32)
        k[material] += len(tris)
        inst.append(it)
    return inst


def normal_lengths(sc, camera=None, name="normal-lengths"):
    """Flat normals of every length in NORMAL_LENGTHS.  From 1e19 on metal's 2 (v.n) n overflows, normalize3 of it is NaN and the
    direction falls back to the normal; at 1e15 len2 overflows instead, the normalised vector is 0 and, with fuzz 0, falls back too.
    Below 1e-6 the depth-1 normal AOV is normalize3's (0,0,1)."""
    return _scene(sc, name, _dealt(sc, lambda k, t: _scaled_normals(sc, t, [_LENGTH_DEAL[k % len(_LENGTH_DEAL)]])), camera)


def _non_finite(kind, n):
    n = n.copy()
    if kind == "nan-one":
        n[..., 1] = _NAN
    elif kind == "nan-all":
        n[...] = _NAN
    elif kind == "plus-inf":
        n[...] = _INF
    elif kind == "minus-inf":
        n[...] = -_INF
    elif kind == "inf-one":
        n[..., 0] = _INF
    return n


def non_finite_normals(sc):
    """NaN in one component or in all, +inf, -inf, one inf among finite components -- per triangle, under both materials.  Whatever
    such a normal meets, the scattered direction is non-finite and so is the normal it falls back to: every one of these bounces leaves
    along (0,0,1).  The triangles that face along z keep their unit normals (what a +z ray meets head on: with them hostile as well, no
    path would live to depth 5)."""
    def deal(k, t):
        n = sc.face_normals(t)
        return n if abs(n[0, 0, 2]) > 0.9 else _non_finite(NON_FINITE_KINDS[k % len(NON_FINITE_KINDS)], n)
    return _scene(sc, "non-finite-normals", _dealt(sc, deal))


def smooth_normals(sc):
    """Vertex normals that differ per vertex: leaning outward, leaning inward (the flip goes against the geometry), n1 = -n2 with n3
    half of n1 (the interpolated normal crosses zero along a line inside the triangle), and lengths 1e-3 / 1 / 1e3 on one triangle."""
    def deal(k, t):
        f = sc.face_normals(t)[0, 0]
        e = (t[0, [1, 2, 0]] - t[0]).astype(np.float32)
        e = (e / np.linalg.norm(e, axis=1, keepdims=True)).astype(np.float32)
        kind = k % 4
        if kind == 0:
            n = f[None] + np.float32(0.5) * e
        elif kind == 1:
            n = -f[None] + np.float32(0.5) * e
        elif kind == 2:
            n = np.stack([f, -f, np.float32(0.5) * f])
        else:
            n = f[None] * np.float32([1e-3, 1.0, 1e3])[:, None]
        if kind < 2:
            n = n / np.linalg.norm(n, axis=1, keepdims=True)
        return n.astype(np.float32)[None]
    return _scene(sc, "smooth-normals", _dealt(sc, deal))


SPHERE_CAMERA = (0.5, 0.5, 0.03)


def spheres(sc):
    """Spheres of radius 1e-3 .. 1 in the room, under instance transforms that translate by 10 and by 1000 and scale unevenly: quirk Q1
    takes the normal from the OBJECT-space centre, so it is 1e1 .. 1e6 long and points nowhere near the surface.  One sphere of radius 1
    holds the camera and the whole room (the room has no front wall here: that sphere closes it and is hit from inside), one touches the
    left wall, one of radius 1e-3 sits 0.012 in front of the camera."""
    def shift(x, y, z, sx=1.0, sy=1.0, sz=1.0):
        return np.array([sx, 0, 0, x, 0, sy, 0, y, 0, 0, sz, z], np.float32)
    shell = _shell(sc, front=False)
    inst = [sc._tri_instance(shell[0::2], sc.WHITE), sc._tri_instance(shell[1::2], sc.STEEL, "metal", 0.1)]
    world = lambda c, m: [(c[0] - m[3]) / m[0], (c[1] - m[7]) / m[5], (c[2] - m[11]) / m[10]]  # noqa: E731  (object-space centre of a world-space one)
    m = shift(0, 0, -10)
    inst.append(sc._sphere_instance([world((0.5, 0.5, 0.3), m)], [1.0], sc.SAND, "rough", 0.0, m))                      # holds camera and room
    m = shift(10, 0, 0)
    inst.append(sc._sphere_instance([world((0.3, 0.25, 0.5), m), world((0.75, 0.7, 0.6), m)], [0.2, 0.05], sc.GREEN, "rough", 0.0, m))
    m = shift(0, 1000, 0)
    inst.append(sc._sphere_instance([world((0.7, 0.3, 0.35), m), world((0.5, 0.5, 0.042), m)], [0.15, 1e-3], sc.STEEL, "metal", 0.0, m))
    m = shift(10, -10, 10, 1.0, 2.0, 0.5)
    inst.append(sc._sphere_instance([world((0.3, 0.7, 0.7), m), world((0.6, 0.55, 0.2), m)], [0.12, 0.02], sc.STEEL, "metal", 0.3, m))
    inst.append(sc._sphere_instance([[0.1, 0.5, 0.7], [0.85, 0.15, 0.85]], [0.1, 0.15], sc.RED, "rough"))                 # tangent to x = 0; in a corner
    return _scene(sc, "spheres", inst, _camera(SPHERE_CAMERA))


def fuzz(sc):
    """Every triangle metal, one instance per value of FUZZ_VALUES: `fuzz > 0` decides whether the RNG is drawn at all (false for -1, +-0
    and NaN, true from the smallest denormal on -- unless a comparison flushes it), fuzz 1e30 gives a direction of that length, fuzz inf a
    non-finite one that falls back to the normal."""
    tris = np.concatenate([_shell(sc), _outer(sc), _cube(sc, 0.13) + np.float32([0.30, 0.22, 0.34]), _cube(sc, 0.14) + np.float32([0.68, 0.40, 0.62])])
    n = len(FUZZ_VALUES)
    return _scene(sc, "fuzz", [sc._tri_instance(tris[k::n], sc.STEEL, "metal", float(np.float32(FUZZ_VALUES[k]))) for k in range(n)])


# albedos of the radiance cases' instances; A A B in a chain is 1e30 . 1e30 . 1e-30 in x and y
RADIANCE_ALBEDOS = {"A": (1e30, 1e30, 1.0), "B": (1e-30, 1e-30, 4.0), "C": (0.0, -0.0, -0.5), "D": (1e-45, 1.0, 1.0), "E": (_INF, 1.0, 0.0), "F": (1.0, -_INF, _NAN)}
RADIANCE_BACKGROUNDS = {"radiance": (1.0, 4.0, 1e-30), "radiance-zeros": (0.0, -0.0, -0.5), "radiance-huge": (1e30, 1e-45, _INF), "radiance-non-finite": (-_INF, _NAN, 1.0)}


def radiance(sc, name="radiance"):
    """Benign geometry and normals, hostile albedos and background (RADIANCE_VALUES).  The room's front wall has an opening so that paths
    end in the background (a fifth of that wall is open): one that met A, A, B on its way there multiplies bg . 1e-30 . 1e30 . 1e30, innermost bounce first -- outermost
    first that is 1e30 . 1e30 = inf; one that met C and then E multiplies 0 . inf.  Four backgrounds deal RADIANCE_VALUES over the three
    channels; the instances' albedos are the same in all four."""
    shell = np.concatenate([_shell(sc)[:-1], np.float32([[[0, 0, 0], [1, 1, 0], [0.6, 0, 0]]])])   # the wall at z = 0 is open between x = 0.6 and 1
    a, b = _cube(sc, 0.13) + np.float32([0.30, 0.22, 0.34]), _cube(sc, 0.14) + np.float32([0.68, 0.40, 0.62])
    alb = RADIANCE_ALBEDOS
    inst = [sc._tri_instance(shell[[0, 1, 2, 3, 6, 7]], alb["A"]),                             # floor, ceiling, left wall
            sc._tri_instance(shell[[4, 5]], alb["B"]),                                         # back wall
            sc._tri_instance(shell[[8, 9, 10, 11]], alb["C"]),                                     # right wall, the front wall's half
            sc._tri_instance(a[:8], alb["D"], "metal", 0.1), sc._tri_instance(a[8:], alb["E"]),
            sc._tri_instance(b[:8], alb["A"], "metal", 0.0), sc._tri_instance(b[8:], alb["F"])]
    return _scene(sc, name, inst, background=RADIANCE_BACKGROUNDS[name])


def _basis(center, u, v, w):
    """A camera given by its basis outright ("uvw": U, V, W as configure_camera would return them, which it never does for these)."""
    cam = _camera(center)
    cam["uvw"] = np.asarray([u, v, w], np.float32)
    return cam


CAMERAS = {
    "cameras-zero-basis": lambda: _basis((0.5, 0.5, 0.03), (0, 0, 0), (0, 0, 0), (0, 0, 0)),                  # every primary direction is normalize3's (0,0,1)
    "cameras-w-below-the-guard": lambda: _basis((0.5, 0.5, 0.03), (0, 0, 0), (0, 0, 0), (6e-8, 0, -8e-8)),    # len2 = 1e-14
    "cameras-w-on-the-guard": lambda: _basis((0.5, 0.5, 0.5), (0, 0, 0), (0, 0, 0), (0, 0, -1e-6)),           # len2 == 1e-12, the bits of 1e-6f * 1e-6f: <= holds, < does not
    "cameras-huge-basis": lambda: _basis((0.5, 0.5, 0.5), (1e15, 0, 0), (0, 1e15, 0), (0, 0, 1)),
    "cameras-on-a-wall": lambda: _camera((0.5, 0.5, 0.0), (0.5, 0.45, 1.0)),
    "cameras-on-a-vertex": lambda: _camera((0.0, 0.0, 0.0), (1.2, 1.1, 1.3)),
}


def camera_basis(scene):
    """(center, U, V, W) of a scene whose camera is given by its basis, else None: what a Renderer's .cam takes after load_scene."""
    cam = scene["camera"]
    if "uvw" not in cam:
        return None
    return (np.asarray(cam["center"], np.float32),) + tuple(np.asarray(cam["uvw"], np.float32))


_HITS = {"hit_triangle_rough": REACH, "hit_triangle_metal": REACH}
CASES = {
    "normal-lengths": (normal_lengths, dict(_HITS, flip=REACH, metal_draw=REACH, metal_no_draw=REACH, fallback_normal=REACH, fallback_nonfinite=REACH,
                                            depth_limit=REACH)),
    "non-finite-normals": (non_finite_normals, dict(_HITS, flip_nan=REACH, fallback_nonfinite=REACH, fallback_z=REACH)),
    "smooth-normals": (smooth_normals, dict(_HITS, flip=REACH, metal_draw=REACH)),
    "spheres": (spheres, dict(_HITS, hit_sphere_rough=REACH, hit_sphere_metal=REACH, flip=REACH, metal_draw=REACH, metal_no_draw=REACH)),
    "fuzz": (fuzz, dict(hit_triangle_metal=REACH, metal_draw=REACH, metal_no_draw=REACH, fallback_nonfinite=REACH)),
}
for _name in RADIANCE_BACKGROUNDS:
    CASES[_name] = ((lambda sc, _n=_name: radiance(sc, _n)), dict(_HITS, nonfinite_samples=REACH, depth_limit=REACH))
for _name, _cam in CAMERAS.items():
    CASES[_name] = ((lambda sc, _n=_name, _c=_cam: normal_lengths(sc, _c(), _n)), dict(_HITS, fallback_normal=REACH))
CASES["rough-degenerate"] = ((lambda sc: rough_degenerate(sc)), {"hit_triangle_rough": REACH, "rough_degenerate": 1})
CASES["cameras-zero-basis"][1]["primary_zero"] = WIDTH * HEIGHT * sum(SPP)
CASES["cameras-w-below-the-guard"][1]["primary_zero"] = WIDTH * HEIGHT * sum(SPP)
CASES["cameras-w-on-the-guard"][1]["primary_zero"] = WIDTH * HEIGHT * sum(SPP)


# The rough branch replaces normal + rsv by the normal when |len2 - 1e-12| < 1e-6, i.e. when the random unit vector lands within 1e-3 of
# -normal: 2.5e-7 per draw.  No case reaches that by chance; this one is the result of a search (test_shading_cases_cpu.py tells how): the
# rough room of 12 triangles on an 8 x 8 frame, where the sample after ROUGH_DEGENERATE_SAMPLES of the streams of this salt takes it.
ROUGH_DEGENERATE_SALT, ROUGH_DEGENERATE_SAMPLES = 269, 133


def rough_degenerate(sc):
    return _scene(sc, "rough-degenerate", [sc._tri_instance(_shell(sc), sc.WHITE)])


def search_rough_degenerate(sc, oracle, salts=range(1, 2000), spp=256, size=8):
    """The search that found the pin above (not run by any test): the rough room at size x size, spp samples per salt, salts in order until
    the oracle counts a degenerate replacement; then the same streams one sample at a time to find which.  Returns (salt, samples before
    it, rough draws made) or None.  Salts 1 .. 269 are 17.6 million draws and take a few seconds."""
    o, draws = oracle.OracleScene(rough_degenerate(sc)), 0
    for salt in salts:
        oracle.shade_counters()
        o.render(size, size, oracle.rng_init(size, size, salt), spp, want_linear=False)
        c = oracle.shade_counters()
        draws += c["hit_triangle_rough"] - c["depth_limit"]
        if c["rough_degenerate"]:
            states = oracle.rng_init(size, size, salt)
            for k in range(spp):
                o.render(size, size, states, 1, want_linear=False)
                if oracle.shade_counters()["rough_degenerate"]:
                    return salt, k, draws
    return None


def frame(name, salt):
    """(width, height, samples of the first and of the second launch, RNG salt) a case is rendered at; salt: scenes.SEED_SALT."""
    if name == "rough-degenerate":
        return 8, 8, (ROUGH_DEGENERATE_SAMPLES + 1, 1), ROUGH_DEGENERATE_SALT
    return WIDTH, HEIGHT, SPP, salt


_REFERENCES = {}


def reference(sc, oracle, name, instanced=False):
    """The oracle's frames of a case, made once per (case, canonical mode) for every test that asks, and never written to: a list with
    one dict per launch ("linear", "color", "states" after it, "rays" so far) and the branch counters of both launches together."""
    key = (name, bool(instanced))
    if key not in _REFERENCES:
        scene = CASES[name][0](sc)
        w, h, spps, salt = frame(name, sc.SEED_SALT)
        o = oracle.OracleScene(scene, instanced=instanced)
        states = oracle.rng_init(w, h, salt)
        oracle.shade_counters()
        launches, rays = [], 0
        for spp in spps:
            r = o.render(w, h, states, spp)
            rays += r["rays"]
            launches.append({"linear": r["linear"], "color": r["color"], "states": states.copy(), "rays": rays})
            for a in launches[-1].values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
        _REFERENCES[key] = (scene, launches, oracle.shade_counters())
        o.close()
    return _REFERENCES[key]


# ---------------------------------------------------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------------------------------------------------
def components_differ(got, want):
    """Elementwise: do two float32 arrays differ?  Where BOTH are NaN the component counts as equal whatever the payload and sign: x86 and
    gfx950 give different NaN bit patterns for the same invalid operation (0 x inf, inf - inf), and which operand's payload a NaN
    carries on is the hardware's business, so a NaN can only be compared by class.  Every other component has to be the same bits --
    that keeps +0 apart from -0 and +inf from -inf, and a NaN on one side only is a difference, so the set of NaN positions is equal.
    This is the only relaxation the shading cases take; nothing carries a tolerance and no pixel is left out."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    return (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
