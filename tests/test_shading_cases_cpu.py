"""Hostile normals, materials, radiance values and cameras (tests/shading_cases.py) on the CPU: the conditions test_shading_cases_gpu.py
relies on, judged on the oracle alone.  A case that is compared bit for bit proves nothing about a guard it never reaches, so the oracle
counts its branches (oracle.c: SC_*, oracle_py.shade_counters) and every case has to take the branches it was made for.

Per case, 61 x 37 at 4 + 1 samples, flattened mode:
  reach     each branch shading_cases.CASES names for the case is taken by at least 32 closest-hit invocations
  depth     at least a quarter of the paths trace a ray at depth 5
  envelope  every direction the oracle traces is 1e-30 .. 1e30 long; seen on the first sample of every pixel
  share     no pixel has a non-finite linear value, except in the radiance cases: there more than 5 % and less than 60 % have one
  same      a second render gives the same bytes, NaN payloads included (they are the host's own)

What the oracle counts (both launches together, flattened mode; "to normal / non-finite / z": the fallback to the normal, how many of
them for a non-finite direction, how many went on to (0,0,1); "nan": flips decided on a NaN dot product).  The four radiance cases
differ in the background only; the three cameras whose basis normalize3 gives up on see the same frame, all 11285 primary directions
its zero-length return:

    case                       tri rough/metal  sph rough/metal  flips / nan    metal draws/none  to normal/non-finite/z  rough deg.  depth limit  depth-5 share
    normal-lengths             20163 / 20920    -                25128 / 0      7147 / 11481      1227 / 1076 / 0         0           4035         0.536
    non-finite-normals         29802 / 26412    -                37559 / 12460  6087 / 15322      19611 / 19611 / 19611   0           11108        0.997
    smooth-normals             26935 / 27672    -                30371 / 0      7908 / 13928      0                       0           10252        0.948
    spheres                    12544 / 14071    19602 / 10190    35139 / 0      14536 / 7898      0                       0           11268        1.000
    fuzz                       0 / 44865        -                34702 / 0      27561 / 10154     2574 / 2574 / 0         0           7150         0.701
    radiance (all four)        47480 / 5174     -                42694 / 0      2609 / 2113       0                       0           9931         0.903
    cameras-zero-basis (x 3)   25230 / 28742    -                36700 / 0      2834 / 20809      1083 / 726 / 0          0           9079         0.978
    cameras-huge-basis         21729 / 18022    -                23231 / 0      6742 / 9320       1264 / 1104 / 0         0           3579         0.477
    cameras-on-a-wall          20128 / 20755    -                25053 / 0      7334 / 11183      1324 / 1178 / 0         0           3950         0.523
    cameras-on-a-vertex        19960 / 19576    -                24627 / 0      7943 / 9582       1938 / 1899 / 0         0           3728         0.488
    rough-degenerate           43160 / 0        -                34520 / 0      -                 0                       1           8624         0.999

Non-finite samples: radiance 1669, radiance-zeros 1555, radiance-huge and radiance-non-finite 2779 of 11285 (36 .. 58 % of the pixels of
the 4-sample frame); none anywhere else.  In radiance, of the 2257 first samples the order of the albedo products matters in 528, and
341 products are a zero times an infinity (test_radiance_chains_where_the_order_of_the_products_matters).

Two things the counts show that the issue's sketch did not expect.  A direction of 1e15 or more never hits anything in a unit room (the
hit distance is below tmin = 1e-6), so such a bounce ends the path in the background; "inf - inf in the flip's dot product" therefore
needs a non-finite normal and is reached in non-finite-normals only.  And the fallback to (0,0,1) is reached through non-finite normals
only: a normal short enough for it never comes with a degenerate scattered direction.  normalize3's zero-length return is reached by
the primary directions of three cameras; in normal-lengths the oracle also takes it 5720 times for the depth-1 normal AOV of short
normals, which the device's path kernels do not compute (quirk Q3 overwrites it).  cameras-w-on-the-guard is not in the issue's list:
W = (0, 0, -1e-6) has len2 == 1e-12 to the bit, the one input for which normalize3's `<=` and a `<` differ ((0,0,1) or (0,0,-1)).

The rough branch's degenerate replacement (normal + rsv within 1e-3 of zero: 2.5e-7 per draw for unit normals, no chance in a 61 x 37
frame) IS reached: shading_cases.search_rough_degenerate rendered the 12-triangle rough room at 8 x 8 and 256 samples under salts 1, 2, ...
and found it at salt 269 after 17.6 million draws (a few seconds of CPU time), in the sample after 133.  The case rough-degenerate pins
that: 134 + 1 samples at 8 x 8.  test_rough_degenerate_is_the_pinned_sample replays it; the search itself is not a test."""
import ctypes as C

import numpy as np
import pytest

import shading_cases as sh

NAMES = list(sh.CASES)
RADIANCE = tuple(sh.RADIANCE_BACKGROUNDS)


def _paths(hrt, oracle, name):
    """The first sample of every pixel of a case with its rays logged (OracleScene.pixel_path): [(rays (n, 10), radiance (3,))]."""
    scene = sh.CASES[name][0](hrt.scenes)
    w, h, _, salt = sh.frame(name, hrt.scenes.SEED_SALT)
    o = oracle.OracleScene(scene)
    states = oracle.rng_init(w, h, salt)
    out = [o.pixel_path(w, h, states, x, y) for y in range(h) for x in range(w)]
    o.close()
    return scene, out


@pytest.mark.parametrize("name", NAMES)
def test_a_case_reaches_what_it_is_there_for(hrt, oracle, name):
    scene, launches, counters = sh.reference(hrt.scenes, oracle, name)
    w, h, spps, _ = sh.frame(name, hrt.scenes.SEED_SALT)
    print(name, {k: v for k, v in counters.items() if v})
    assert counters["samples"] == w * h * sum(spps)
    for branch, least in sh.CASES[name][1].items():
        assert counters[branch] >= least, (name, branch, counters[branch])
    assert counters["depth5_rays"] >= 0.25 * counters["samples"], (name, counters["depth5_rays"] / counters["samples"])
    for launch in launches:
        share = (~np.isfinite(launch["linear"][..., :3])).any(-1).mean()
        if name in RADIANCE:
            assert 0.05 < share < 0.60, (name, share)
        else:
            assert share == 0 and counters["nonfinite_samples"] == 0, (name, share)
        assert np.isfinite(launch["color"]).all()                       # colorToFloat4 clamps: the sRGB buffer holds no NaN, whatever went in
    # the envelope: the lengths of the directions traced
    length = np.concatenate([np.linalg.norm(rays[:, 3:6].astype(np.float64), axis=1) for rays, _ in _paths(hrt, oracle, name)[1]])
    assert np.isfinite(length).all() and length.min() >= 1e-30 and length.max() <= 1.0001e30, (name, length.min(), length.max())


@pytest.mark.parametrize("name", ["normal-lengths", "spheres", "cameras-on-a-vertex"])
def test_the_instanced_mode_reaches_them_too(hrt, oracle, name):
    """What the two-level configuration is compared with: the transformed boxes and spheres stay in object space there."""
    counters = sh.reference(hrt.scenes, oracle, name, instanced=True)[2]
    for branch, least in sh.CASES[name][1].items():
        assert counters[branch] >= least, (name, branch, counters[branch])
    assert counters["depth5_rays"] >= 0.25 * counters["samples"]


@pytest.mark.parametrize("name", ["non-finite-normals", "radiance-non-finite", "fuzz"])
def test_two_renders_give_the_same_bytes(hrt, oracle, name):
    launches = sh.reference(hrt.scenes, oracle, name)[1]
    w, h, spps, salt = sh.frame(name, hrt.scenes.SEED_SALT)
    o = oracle.OracleScene(sh.CASES[name][0](hrt.scenes))
    states = oracle.rng_init(w, h, salt)
    for spp, want in zip(spps, launches):
        got = o.render(w, h, states, spp)
        assert got["linear"].tobytes() == want["linear"].tobytes() and got["color"].tobytes() == want["color"].tobytes()
        assert states.tobytes() == want["states"].tobytes()
    oracle.shade_counters()


def test_the_values_are_all_dealt(hrt, oracle):
    sc = hrt.scenes
    bits = lambda a: set(np.asarray(a, np.float32).reshape(-1).view(np.uint32).tolist())  # noqa: E731
    # normal lengths: every value on some triangle, under a rough and under a metal instance; the three around 1e-6 straddle the guard
    scene = sh.normal_lengths(sc)
    for material in ("rough", "metal"):
        n = np.concatenate([it["normals"][:, 0] for it in scene["instances"] if it["material"] == material])
        length = np.abs(n).max(axis=1)                                  # (the face normals of this room are axis-parallel in object space)
        assert bits(length) >= bits(np.abs(np.float32(sh.NORMAL_LENGTHS))), material
        assert (np.signbit(n).all(1) & (n == 0).all(1)).any() and (~np.signbit(n).any(1) & (n == 0).all(1)).any()
    guard = np.float32(1e-6) * np.float32(1e-6)
    below, on, above = (np.float32(v) * np.float32(v) for v in sh.NORMAL_LENGTHS[4:7])
    assert below < guard and on == guard and above > guard
    assert {it["fuzz"] for it in scene["instances"] if it["material"] == "metal"} == {0.0, 0.3}
    assert sum(it["material"] == "rough" for it in scene["instances"]) * 2 == len(scene["instances"])
    # non-finite normals: each kind under both materials
    scene = sh.non_finite_normals(sc)
    for material in ("rough", "metal"):
        n = np.concatenate([it["normals"][:, 0] for it in scene["instances"] if it["material"] == material])
        nan, inf = np.isnan(n), np.isinf(n)
        assert (nan.sum(1) == 1).any() and nan.all(1).any() and (n == np.inf).all(1).any() and (n == -np.inf).all(1).any() and ((inf.sum(1) == 1) & ~nan.any(1)).any()
    # smooth normals: a triangle with n1 = -n2, one with lengths 1e-3 / 1 / 1e3, vertex normals that differ
    n = np.concatenate([it["normals"] for it in sh.smooth_normals(sc)["instances"]])
    assert (n[:, 0] == -n[:, 1]).all(1).any() and (n[:, 0] != n[:, 1]).any(1).all()
    length = np.linalg.norm(n.astype(np.float64), axis=2)
    assert np.isclose(length, [1e-3, 1.0, 1e3], rtol=1e-6).all(1).any()
    # spheres: radii 1e-3 .. 1, translations of 10 and 1000, an uneven scale, the camera inside one, one tangent to the wall x = 0
    sph = [it for it in sh.spheres(sc)["instances"] if it["geometry"] == "spheres"]
    radii = np.concatenate([it["radii"] for it in sph])
    assert radii.min() == np.float32(1e-3) and radii.max() == 1.0 and {it["material"] for it in sph} == {"rough", "metal"}
    shifts = {float(np.abs(it["transform"][[3, 7, 11]]).max()) for it in sph}
    assert {0.0, 10.0, 1000.0} <= shifts and any(len({float(it["transform"][k]) for k in (0, 5, 10)}) == 3 for it in sph)
    big = sph[0]
    centre = big["centers"][0] * big["transform"][[0, 5, 10]] + big["transform"][[3, 7, 11]]
    assert np.linalg.norm(centre - np.float32(sh.SPHERE_CAMERA)) < big["radii"][0]
    assert any(it["transform"][3] == 0 and (it["centers"][:, 0] == it["radii"]).any() for it in sph)
    # fuzz: one metal instance per value, and the value arrives unrounded in the oracle's record and in the product's
    scene = sh.fuzz(sc)
    want = np.float32(sh.FUZZ_VALUES)
    assert len(bits(want)) == len(sh.FUZZ_VALUES) == len(scene["instances"])
    assert np.float32(1e-45) > 0 and np.float32(1e-45).view(np.uint32) == 1 and np.float32(1e-38) < np.float32(1.1754944e-38) == np.finfo(np.float32).tiny
    o = oracle.OracleScene(scene)
    for k, it in enumerate(scene["instances"]):
        theirs = hrt.HitGroupParams(fuzz=float(it["fuzz"]))             # what Renderer.load_scene does with it
        for arrived in (o._arr[k].fuzz, theirs.fuzz):
            a = np.float32(C.c_float(arrived).value)
            assert a.view(np.uint32) == want[k].view(np.uint32) or (np.isnan(a) and np.isnan(want[k])), (k, arrived)
    o.close()
    # radiance: albedos and backgrounds deal every value
    dealt = set()
    for name in RADIANCE:
        scene = sh.radiance(sc, name)
        dealt |= bits(scene["background"]) | bits([it["albedo"] for it in scene["instances"]])
    finite = [v for v in sh.RADIANCE_VALUES if v == v]
    assert dealt >= bits(finite) and any(np.isnan(np.uint32(b).view(np.float32)) for b in dealt)


def _fold(chain_albedos, end, inner_first):
    """The radiance of a path: `end` (background or black) times the albedos it met, innermost bounce first as the recursion unwinds
    (Shader.cu:236-238) -- or outermost first, which is what a throughput carried along the path would compute.  float32 throughout."""
    with np.errstate(all="ignore"):
        if inner_first:
            r = np.float32(end).copy()
            for a in chain_albedos[::-1]:
                r = (r * a).astype(np.float32)
            return r
        t = np.ones(3, np.float32)
        for a in chain_albedos:
            t = (t * a).astype(np.float32)
        return (np.float32(end) * t).astype(np.float32)


def test_radiance_chains_where_the_order_of_the_products_matters(hrt, oracle):
    """On the first sample of every pixel: the logged path folded innermost first is the oracle's radiance; at least 32 paths give
    something else folded outermost first (1e30 . 1e30 . 1e-30), and at least 32 multiply a zero by an infinity."""
    scene, paths = _paths(hrt, oracle, "radiance")
    albedo = [np.float32(it["albedo"]) for it in scene["instances"]]
    order_matters = zero_times_inf = 0
    for rays, result in paths:
        hit = rays[:, 7] >= 0
        missed = not hit[-1]
        assert hit[:-1].all() and (missed or len(rays) == 5)
        chain = [albedo[int(i)] for i in rays[:, 9].view(np.uint32)[: len(rays) - 1 if missed else 4]]
        end = scene["background"] if missed else np.zeros(3, np.float32)
        inner = _fold(chain, end, True)
        assert not sh.components_differ(inner, result).any()
        order_matters += bool(sh.components_differ(inner, _fold(chain, end, False)).any())
        r = np.float32(end).copy()
        for a in chain[::-1]:
            zero_times_inf += bool((((r == 0) & np.isinf(a)) | (np.isinf(r) & (a == 0))).any())
            with np.errstate(all="ignore"):
                r = (r * a).astype(np.float32)
    print("order matters in %d paths, 0 x inf in %d products, of %d paths" % (order_matters, zero_times_inf, len(paths)))
    assert order_matters >= sh.REACH and zero_times_inf >= sh.REACH


def test_rough_degenerate_is_the_pinned_sample(hrt, oracle):
    """The pin replayed: no sample before the pinned one takes the branch, the pinned one does, once; and there the scattered direction
    is the normal itself -- some ray of that sample runs exactly along an axis of the room."""
    sc = hrt.scenes
    w, h, spps, salt = sh.frame("rough-degenerate", sc.SEED_SALT)
    assert (w, h, spps, salt) == (8, 8, (sh.ROUGH_DEGENERATE_SAMPLES + 1, 1), sh.ROUGH_DEGENERATE_SALT)
    o = oracle.OracleScene(sh.rough_degenerate(sc))
    states = oracle.rng_init(w, h, salt)
    oracle.shade_counters()
    o.render(w, h, states, sh.ROUGH_DEGENERATE_SAMPLES, want_linear=False)
    assert oracle.shade_counters()["rough_degenerate"] == 0
    along_an_axis = 0
    for y in range(h):
        for x in range(w):
            d = o.pixel_path(w, h, states, x, y)[0][1:, 3:6]
            along_an_axis += int(((d == 0).sum(1) == 2).any())
    assert along_an_axis == 1
    assert sh.reference(sc, oracle, "rough-degenerate")[2]["rough_degenerate"] == 1
    o.close()


def test_the_colour_of_hostile_radiance(oracle):
    """colorToFloat4 clamps first: NaN, +inf and anything above 1 give what 1 gives, -inf and negative values +0 -- and so does -0.0, which CUDA's
    fmaxf orders below +0.0 (C leaves that open and glibc's fmaxf(0.0f, -0.0f) is -0.0: the oracle said -0.0 until the device, which was
    right, was compared with it under shading_cases.radiance); the smallest denormal is on the linear branch, 12.92 x."""
    src = np.zeros((9, 4), np.float32)
    src[:, 0] = [-0.0, -0.5, -np.inf, np.nan, np.inf, 4.0, 1e30, 0.0, 1e-45]
    dst = np.zeros_like(src)
    oracle.lib().oracle_color_to_float4_n(src.ctypes.data, dst.ctypes.data, len(src))
    one = np.float32(1.055) * np.float32(1.0) - np.float32(0.055)          # (0.99999994: what every channel of 1 and more becomes)
    want = np.float32([0, 0, 0, one, one, one, one, 0, np.float32(12.92) * np.float32(1e-45)])
    assert dst[:, 0].view(np.uint32).tolist() == want.view(np.uint32).tolist()


def test_nan_compares_by_class_and_nothing_else_does():
    f = lambda *b: np.array(b, np.uint32).view(np.float32)  # noqa: E731
    host_nan, device_nan, payload = 0xFFC00000, 0x7FC00000, 0x7FA00001
    assert not sh.components_differ(f(host_nan, host_nan, payload), f(device_nan, payload, host_nan)).any()
    zero, minus_zero, inf, minus_inf, one = 0, 0x80000000, 0x7F800000, 0xFF800000, 0x3F800000
    assert sh.components_differ(f(zero, inf, host_nan, one, one), f(minus_zero, minus_inf, one, device_nan, one + 1)).all()
    same = f(zero, minus_zero, inf, minus_inf, one, 1)
    assert not sh.components_differ(same, same.copy()).any()
