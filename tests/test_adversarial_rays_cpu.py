"""Adversarial rays (tests/ray_cases.py) on the CPU: the generator's conditions judged on the brute-force reference alone, and the host
BVH8 builder -- plain and with spatial splits -- walked by the oracle's bvh8_trace under them: six [tmin, tmax] windows, closest and any
hit, no tolerance; and at 2^-20 / 2^+20 of the scenes' size, where the walk still equals brute force and the record is the unscaled
walk's with t x 2^k, bit for bit.

What the reference gives for the counts used (open window; rays of the class / of these the reference's closest hit is the primitive
aimed at; the tangent class: hit / miss of its sphere; "at t*": rays whose hit distance is the most frequent bit pattern):

    case                  rays   vertex     edge       interior    tangent          centre    inside    hit share  t*          at t*
    soup-3000             20000  5200/339   5200/688   6934/1733   -                -         -         0.518      0.37500006  676
    soup-200              20000  5200/484   5200/1049  6934/2352   -                -         -         0.409      0.375       676
    cornell               20000  5200/206   5200/466   6934/1118   -                -         -         0.527      0.375       486
    mixed                 12000  3120/206   2080/333   1040/293    2496: 574/1922   832/351   832/512   0.499      0.37499997  391
    mixed instanced       12000  3120/204   2080/336   1040/292    2496: 574/1922   832/351   832/512   0.498      0.375       391
    cornell-12k           12000  3120/138   3120/290   4160/700    -                -         -         0.529      0.375       297
    soup-6000             12000  3120/151   3120/337   4160/848    -                -         -         0.629      0.44352087  429
    bodies instanced      12000  3120/83    2080/153   1040/156    2496: 689/1807   832/429   832/533   0.549      0.19297616  391
    mixed-moved           12000  3120/218   2080/329   1040/315    2496: 555/1941   832/341   832/518   0.495      0.36475152  391
    mixed-moved instanced 12000  3120/174   2080/307   1040/304    2496: 555/1941   832/341   832/518   0.494      0.36475158  391
    mixed-far             12000  3120/96    2080/263   1040/272    2496: 578/1918   832/351   832/512   0.491      0.3750072   391
    mixed-far instanced   12000  3120/152   2080/254   1040/256    2496: 578/1918   832/351   832/512   0.493      0.37499842  391

(from mixed on: what test_adversarial_rays_gpu.py sends through the device; every ray at t* changes its record under tmax = t* and under
tmin = t*.  Scenes with spheres give 30 / 20 / 10 % of the rays outside the plane block to vertex / edge / interior targets, 24 / 8 / 8 % to
tangent / centre / inside; triangle scenes 30 / 30 / 40 %.)
The host-builder tests see a scene's triangles as one instance in world space (what hrt_host_build_bvh8 takes); they reuse _host_bvh_lib /
_build of test_host_cpu.py, so `make asan-test` runs them against the sanitizer build of the builder."""
import ctypes as C

import numpy as np
import pytest

import ray_cases as rc
from test_host_cpu import _build

CASES = rc.CASES
TRIANGLE_CASES = ("soup-3000", "soup-200", "cornell")
_CACHE = {}


def _as_one_instance(hrt, scene):
    """The scene's world-space triangles as ONE identity instance: what the host builder takes (primitive = index into the whole)."""
    if len(scene["instances"]) == 1:
        return scene
    one = dict(scene)
    one["instances"] = [hrt.scenes._tri_instance(rc.world_triangles(scene)[0], hrt.scenes.WHITE)]
    return one


def _case(hrt, name):
    """(scene, o, d, class, details) of a case, made once."""
    if ("case", name) not in _CACHE:
        make, n, seed = CASES[name]
        scene = make(hrt.scenes)
        if name in TRIANGLE_CASES:
            scene = _as_one_instance(hrt, scene)
        _CACHE["case", name] = (scene,) + rc.adversarial_rays(scene, n, seed, rc.scene_extent(scene), details=True)
    return _CACHE["case", name]


def _reference(hrt, oracle, name, window, instanced=False):
    """Brute force, once per (case, mode, window); never written to."""
    key = ("ref", name, instanced, window)
    if key not in _CACHE:
        scene, o, d = _case(hrt, name)[:3]
        ref = oracle.OracleScene(scene, force_brute=True, instanced=instanced).trace(o, d, tmin=window[0], tmax=window[1])
        for a in ref:
            a.setflags(write=False)
        _CACHE[key] = ref
    return _CACHE[key]


def _windows(hrt, oracle, name, instanced=False):
    ref = _reference(hrt, oracle, name, rc.OPEN, instanced)
    return rc.six_windows(ref[0], ref[3])


@pytest.mark.parametrize("name,instanced", [(n, False) for n in CASES if n != "bodies"] + [("mixed", True), ("bodies", True), ("mixed-moved", True), ("mixed-far", True)])
def test_the_generator_meets_its_conditions_on_brute_force(hrt, oracle, name, instanced):
    """The classes do what they are named after -- on the reference alone, whatever the product does with them."""
    scene, o, d, cls, info = _case(hrt, name)
    assert o.dtype == np.float32 and d.dtype == np.float32 and len(o) == CASES[name][1] and np.isfinite(o).all()
    assert not (d == 0).all(1).any()
    ref = _reference(hrt, oracle, name, rc.OPEN, instanced)
    hit = ref[3] != rc.MISS
    on_target = hit & (ref[3] == info["target_prim"]) & (ref[4] == info["target_inst"])
    (w_max, w_min), star, at = rc.bound_windows(ref[0], ref[3])
    counts = {rc.CLASS_NAMES[k]: (int((cls == k).sum()), int((on_target & (cls == k)).sum())) for k in range(7)}
    print(name, "instanced" if instanced else "flattened", counts, "hit share %.3f" % hit.mean(), "t* = %r, %d rays" % (star, at.sum()))
    assert counts["vertex"][1] >= 50 and counts["edge"][1] >= 50
    assert 0.2 <= hit.mean() <= 0.8
    assert at.sum() >= 200
    if any(it["geometry"] == "spheres" for it in scene["instances"]):
        tangent = cls == rc.TANGENT
        assert (on_target & tangent).sum() >= 50 and (~on_target & tangent).sum() >= 50
        assert counts["centre"][1] >= 50 and counts["inside"][1] >= 50
        assert set(np.unique(info["factor"][tangent])) == set(rc.TANGENT_FACTORS)
    # every kind of direction and origin occurs, within the envelope
    assert set(np.unique(info["scale"])) == set(rc.DIRECTION_SCALES) and set(np.unique(info["dist"])) == set(rc.DISTANCES)
    for value in rc.COMPONENT_VALUES:
        v = np.float32(value)
        assert ((d.view(np.uint32) == v.view(np.uint32)).any(1) & info["replaced"]).any(), value
    assert np.abs(o).max() <= np.abs(rc.world_triangles(scene)[0]).max() + 5.0 * rc.scene_extent(scene) + 1e-3
    # the strict comparisons: a ray at t* loses that hit under tmax = t*, and under tmin = t*
    for window in (w_max, w_min):
        cut = _reference(hrt, oracle, name, window, instanced)
        assert rc.records_differ(cut, ref)[at].all()
        assert not (cut[0][cut[3] != rc.MISS].view(np.uint32) == np.float32(star).view(np.uint32)).any()


def test_vertex_targets_are_the_stored_vertices(hrt):
    """A vertex-class ray from distance 0 starts ON the float32 world-space vertex the flattened oracle and the product store: the
    transform is applied in xf_point's operation order (rotated, unevenly scaled instance 1 of the mixed scene included)."""
    scene, o, d, cls, info = _case(hrt, "mixed")
    tris, prim, inst = rc.world_triangles(scene)
    sel = np.flatnonzero((cls == rc.VERTEX) & (info["dist"] == 0.0))
    assert len(sel) > 100 and (info["target_inst"][sel] == 1).sum() > 20
    lookup = {(int(i), int(p)): k for k, (p, i) in enumerate(zip(prim, inst))}
    for j in sel:
        v = tris[lookup[int(info["target_inst"][j]), int(info["target_prim"][j])]]
        assert (v.view(np.uint32) == o[j].view(np.uint32)).all(1).any()
    m = scene["instances"][1]["transform"].astype(np.float64).reshape(3, 4)
    exact = scene["instances"][1]["vertices"].reshape(-1, 3).astype(np.float64) @ m[:, :3].T + m[:, 3]
    assert np.abs(tris[inst == 1].reshape(-1, 3) - exact).max() < 1e-6


@pytest.mark.parametrize("sbvh", ["plain", "spatial-splits"])
@pytest.mark.parametrize("name", TRIANGLE_CASES)
def test_host_builder_under_adversarial_rays(hrt, oracle, monkeypatch, name, sbvh):
    """hrt_host_build_bvh8's tree walked on the CPU: the brute-force record (t, u, v, primitive, instance) bit for bit in all six
    windows, and hit / no hit of an any-hit query."""
    scene, o, d, cls, info = _case(hrt, name)
    monkeypatch.setenv("HRT_SBVH", "1" if sbvh == "spatial-splits" else "0")
    lib, blob = _build(hrt, scene["instances"][0]["vertices"])
    try:
        n = len(scene["instances"][0]["vertices"])
        assert blob.n_triangles >= n if sbvh == "spatial-splits" else blob.n_triangles == n
        if sbvh == "spatial-splits" and n >= 3000:
            assert blob.n_triangles > 1.02 * n
        for window in _windows(hrt, oracle, name):
            want = _reference(hrt, oracle, name, window)
            got = oracle.bvh8_trace(blob.nodes, blob.triangles, o, d, tmin=window[0], tmax=window[1])
            diff = rc.records_differ(got, want)
            assert not diff.any(), (name, sbvh, window, int(diff.sum()), _first(diff, o, d, cls, got, want))
            any_got = oracle.bvh8_trace(blob.nodes, blob.triangles, o, d, tmin=window[0], tmax=window[1], any_hit=True)
            adiff = (any_got[3] != rc.MISS) != (want[3] != rc.MISS)
            assert not adiff.any(), (name, sbvh, window, int(adiff.sum()), _first(adiff, o, d, cls, any_got, want))
    finally:
        lib.hrt_host_free(C.byref(blob))


def _first(diff, o, d, cls, got, want):
    j = int(np.argmax(diff))
    return {"ray": j, "class": rc.CLASS_NAMES[cls[j]], "o": o[j].view(np.uint32).tolist(), "d": d[j].view(np.uint32).tolist(),
            "got": (got[0][j], got[3][j], got[4][j]), "want": (want[0][j], want[3][j], want[4][j])}


@pytest.mark.parametrize("sbvh", ["plain", "spatial-splits"])
@pytest.mark.parametrize("k", [-20, 20])
@pytest.mark.parametrize("name", TRIANGLE_CASES)
def test_host_builder_on_scaled_scenes(hrt, oracle, monkeypatch, name, k, sbvh):
    """The scene and the rays' origins times 2^k, directions as they are (node_exponent / quantise_axis far from unit size, the
    max(1, scale) floor of the padding): the walk equals brute force on the scaled scene for every ray; and for the rays whose
    arithmetic stays in the normal range (ray_cases.tame) its record is the UNSCALED walk's with t x 2^k -- u, v, primitive, instance the
    same bits -- so the check does not rest on the oracle's intersector alone."""
    scene, o, d, cls, info = _case(hrt, name)
    s = np.float32(2.0 ** k)
    big = rc.scaled(scene, k)
    o_k = o * s
    window = (rc.OPEN[0] * 2.0 ** k, rc.OPEN[1] * 2.0 ** k)
    monkeypatch.setenv("HRT_SBVH", "1" if sbvh == "spatial-splits" else "0")
    lib, blob = _build(hrt, scene["instances"][0]["vertices"])
    try:
        base = oracle.bvh8_trace(blob.nodes, blob.triangles, o, d)
    finally:
        lib.hrt_host_free(C.byref(blob))
    assert not rc.records_differ(base, _reference(hrt, oracle, name, rc.OPEN)).any()
    lib, blob = _build(hrt, big["instances"][0]["vertices"])
    try:
        got = oracle.bvh8_trace(blob.nodes, blob.triangles, o_k, d, tmin=window[0], tmax=window[1])
    finally:
        lib.hrt_host_free(C.byref(blob))
    want = oracle.OracleScene(big, force_brute=True).trace(o_k, d, tmin=window[0], tmax=window[1])
    diff = rc.records_differ(got, want)
    assert not diff.any(), (name, k, sbvh, int(diff.sum()), _first(diff, o_k, d, cls, got, want))
    tame = rc.tame(info)
    assert tame.mean() > 0.4 and (base[3][tame] != rc.MISS).mean() > 0.2
    expect = ((base[0] * s).astype(np.float32),) + tuple(base[1:5])
    diff = rc.records_differ(got, expect) & tame
    assert not diff.any(), (name, k, sbvh, int(diff.sum()), _first(diff, o_k, d, cls, got, expect))


def test_scaled_and_translated_scenes(hrt):
    scene = _case(hrt, "mixed")[0]
    big = rc.scaled(scene, 20)
    assert rc.scene_extent(big) == rc.scene_extent(scene) * 2.0 ** 20
    for a, b in zip(scene["instances"], big["instances"]):
        assert np.array_equal(np.asarray(b["transform"])[[0, 1, 2, 4, 5, 6, 8, 9, 10]], np.asarray(a["transform"])[[0, 1, 2, 4, 5, 6, 8, 9, 10]])
    back = rc.scaled(big, -20)
    assert np.array_equal(rc.world_triangles(back)[0], rc.world_triangles(scene)[0])
    moved = rc.translated(scene, (1000, -500, 250))
    shift = rc.world_triangles(moved)[0].astype(np.float64) - rc.world_triangles(scene)[0]
    assert np.abs(shift - np.array([1000.0, -500.0, 250.0])).max() < 2e-4          # (a float near 1000 resolves 6e-5)
    assert np.array_equal(moved["instances"][0]["vertices"], scene["instances"][0]["vertices"])
