"""Adversarial rays (tests/ray_cases.py) against brute force through every tree and traversal kernel of the device.

The hit record (t, u, v, primitive, instance) is canonical: it does not depend on the tree or on the kernel.  The rays here are the ones
for which a box is culled by one ULP, a clip box of a spatial split is a hair too small or a tie between two leaves is resolved
differently (exact vertices and edge points, tangents of spheres, origins on surfaces, directions scaled by 1e-30 .. 1e30, signed zeros
and denormals among their components), in six [tmin, tmax] windows -- two of them made from the reference so that a few hundred rays sit
exactly on the bound.  Every configuration sees the same cases; closest hits are compared bit for bit, any-hit queries by hit / no hit.
Nothing carries a tolerance.  The generator's conditions for the counts used here are checked on the reference alone in
test_adversarial_rays_cpu.py, case by case (ray_cases.CASES).

Origins lie within 10 x extent / 2 of their targets, the envelope DESIGN.md section 3 states; tools/stress_rays.py goes beyond."""
import numpy as np
import pytest

import ray_cases as rc
from test_two_level_fast_trace_gpu import _is_split_two_level, _load, _tree_stats, _unique_prims

pytestmark = pytest.mark.gpu

_CACHE = {}
SOUP = 6000                                      # above the 4096-primitive threshold: the device build's top-down phase runs


def _scene(hrt, name):
    """The cases of ray_cases.CASES, and the mixed scene at 2^-20 / 2^+20 of its size."""
    if ("scene", name) not in _CACHE:
        if name in ("mixed-small", "mixed-large"):
            _CACHE["scene", name] = rc.scaled(_scene(hrt, "mixed"), -20 if name == "mixed-small" else 20)
        else:
            _CACHE["scene", name] = rc.CASES[name][0](hrt.scenes)
    return _CACHE["scene", name]


def _rays(hrt, name):
    """(o, d, class, details) of a scene, made once from that scene's own geometry.  The scaled scenes take the unscaled scene's rays
    with their origins scaled alike, so that the records can be compared with the unscaled run's."""
    if ("rays", name) not in _CACHE:
        if name in ("mixed-small", "mixed-large"):
            o, d, cls, info = _rays(hrt, "mixed")
            _CACHE["rays", name] = (o * np.float32(2.0 ** (-20 if name == "mixed-small" else 20)), d, cls, info)
        else:
            scene = _scene(hrt, name)
            _CACHE["rays", name] = rc.adversarial_rays(scene, rc.CASES[name][1], rc.CASES[name][2], rc.scene_extent(scene), details=True)
    return _CACHE["rays", name]


def _reference(hrt, oracle, name, instanced, window):
    """Brute force, once per (scene, mode, window) for the whole matrix; never written to."""
    key = ("ref", name, instanced, window)
    if key not in _CACHE:
        o, d = _rays(hrt, name)[:2]
        ref = oracle.OracleScene(_scene(hrt, name), force_brute=True, instanced=instanced).trace(o, d, tmin=window[0], tmax=window[1])
        for a in ref:
            a.setflags(write=False)
        _CACHE[key] = ref
    return _CACHE[key]


def _windows(hrt, oracle, name, instanced):
    ref = _reference(hrt, oracle, name, instanced, rc.OPEN)
    return rc.six_windows(ref[0], ref[3])


def _describe(diff, o, d, cls, info, got, want):
    j = int(np.argmax(diff))
    return {"differing": int(diff.sum()), "by class": {rc.CLASS_NAMES[k]: int(diff[cls == k].sum()) for k in range(7) if diff[cls == k].any()},
            "by distance": {float(v): int(diff[info["dist"] == v].sum()) for v in np.unique(info["dist"][diff])},
            "by scale": {float(v): int(diff[info["scale"] == v].sum()) for v in np.unique(info["scale"][diff])},
            "first": j, "o bits": [hex(x) for x in o[j].view(np.uint32)], "d bits": [hex(x) for x in d[j].view(np.uint32)],
            "got": (float(got[0][j]), int(got[3][j]), int(got[4][j])), "want": (float(want[0][j]), int(want[3][j]), int(want[4][j]))}


def _records_are_the_references(hrt, oracle, r, name, instanced, windows=None):
    """The loaded scene `name` under its rays: the closest hit's record bit for bit and hit / no hit of an any-hit query, per window."""
    o, d, cls, info = _rays(hrt, name)
    for window in windows or _windows(hrt, oracle, name, instanced):
        want = _reference(hrt, oracle, name, instanced, window)
        got = r.trace_rays(o, d, tmin=window[0], tmax=window[1])
        diff = rc.records_differ(got, want)
        assert not diff.any(), (name, window, "closest", _describe(diff, o, d, cls, info, got, want))
        any_got = r.trace_rays(o, d, tmin=window[0], tmax=window[1], any_hit=True)
        adiff = (any_got[3] != rc.MISS) != (want[3] != rc.MISS)
        assert not adiff.any(), (name, window, "any hit", _describe(adiff, o, d, cls, info, any_got, want))


CONFIGURATIONS = {
    "production": (0, {}),                                                                # k_fused, v_rcp_f32 in the slab test
    "counting": ("CTX_COUNT", {}),                                                        # k_traverse, exact division, canonical walk order
    "wavefront": (0, {"HRT_FUSED": "0"}),                                                 # k_trace_queue
    "round-1-path-kernel": (0, {"HRT_FUSED_MAX_DEPTH": "1"}),
    "round-1-traverse-kernel": (0, {"HRT_FUSED": "0", "HRT_FUSED_MAX_DEPTH": "1"}),
    "host-build": (0, {"HRT_BUILD": "host"}),
    "aligned-records": (0, {"HRT_NODE_STRIDE": "128", "HRT_PRIM_STRIDE": "64"}),
    "fast-trace-device-split-build": ("CTX_FAST_TRACE", {"HRT_FAST_TRACE_BUILD": "device"}),
    "fast-trace-host-split-build": ("CTX_FAST_TRACE", {"HRT_FAST_TRACE_BUILD": "host"}),
    "two-level": ("CTX_TWO_LEVEL", {}),
}


def _renderer(hrt, gpu_available, monkeypatch, flags, env):
    if not gpu_available:
        pytest.skip("no GPU in this container")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    value = 0
    for f in (flags.split("|") if flags else ()):
        value |= getattr(hrt, f)
    return hrt.Renderer(0, value)


@pytest.mark.parametrize("configuration", sorted(CONFIGURATIONS))
def test_adversarial_rays_in_every_configuration(hrt, oracle, gpu_available, monkeypatch, configuration):
    """Three scenes x 12000 rays x six windows, closest and any hit, through the configuration's tree and kernel.  The flattened trees
    are pinned to the oracle's flattened mode, the two-level tree to its instanced mode."""
    flags, env = CONFIGURATIONS[configuration]
    r = _renderer(hrt, gpu_available, monkeypatch, flags, env)
    instanced = configuration == "two-level"
    try:
        for name in ("mixed", "cornell-12k", "soup-6000"):
            r.load_scene(_scene(hrt, name))
            _records_are_the_references(hrt, oracle, r, name, instanced)
            st = r.stats()
            if name == "soup-6000":
                records = (int(st.bvh_bytes) - 80 * int(st.bvh_nodes)) // 48
                print(configuration, "soup: %d nodes, %d records for %d triangles, depth %d" % (st.bvh_nodes, records, SOUP, st.bvh_depth))
                assert st.bvh_triangles == SOUP
                if configuration == "fast-trace-device-split-build":
                    assert records > SOUP                          # references were duplicated: clip boxes are under test
        if configuration == "round-1-path-kernel":
            assert r.stats().fused_fallback_launches > 0           # round 1's path kernel did run
    finally:
        r.close()


def test_adversarial_rays_through_a_two_level_tree_with_split_blases(hrt, oracle, gpu_available, monkeypatch):
    """HRT_CTX_TWO_LEVEL | HRT_CTX_FAST_TRACE: k_pack_blas's clip boxes in the object space of a shared BLAS, under instances that turn
    it and scale it unevenly.  The tree is two-level and split by the structure criterion of test_two_level_fast_trace_gpu.py
    (ray_cases.BODY_EDGE = 0.2 is the edge length taken)."""
    scene = _scene(hrt, "bodies")
    unique = _unique_prims(scene)
    assert unique == rc.BODY_TRIANGLES + 3
    flat_nodes = _tree_stats(hrt, gpu_available, scene, hrt.CTX_FAST_TRACE)[0]
    r = _renderer(hrt, gpu_available, monkeypatch, "CTX_TWO_LEVEL|CTX_FAST_TRACE", {})
    try:
        st = _load(r, scene)
        payload = int(st.bvh_bytes) - 80 * int(st.bvh_nodes)
        print("bodies: %d nodes (flattened split tree: %d), %d records for %d unique primitives (x %.3f)" % (st.bvh_nodes, flat_nodes, payload // 48, unique, payload / 48 / unique))
        assert _is_split_two_level(st, unique, flat_nodes)
        _records_are_the_references(hrt, oracle, r, "bodies", True)
        assert r.stats().fused_fallback_launches == 0
    finally:
        r.close()


@pytest.mark.parametrize("configuration", ["flattened", "flattened-asynchronous-update", "two-level"])
def test_after_an_update(hrt, oracle, gpu_available, monkeypatch, configuration):
    """Exact-vertex rays against the boxes refit.hip wrote: the mixed scene is loaded, every instance moves by a rigid step, and again;
    the second update is a refit.  The rays are made from the updated scene's geometry, the reference from its transforms."""
    flags = {"flattened": 0, "flattened-asynchronous-update": "CTX_ASYNC_UPDATE", "two-level": "CTX_TWO_LEVEL"}[configuration]
    r = _renderer(hrt, gpu_available, monkeypatch, flags, {})
    try:
        scene = _scene(hrt, "mixed")
        r.load_scene(scene)
        once = rc.moved(hrt.scenes, scene, 1)
        r.update_instances([it["transform"] for it in once["instances"]])
        before = r.stats()
        twice = rc.moved(hrt.scenes, once, 2)
        assert all(np.array_equal(a["transform"], b["transform"]) for a, b in zip(twice["instances"], _scene(hrt, "mixed-moved")["instances"]))
        r.update_instances([it["transform"] for it in twice["instances"]])
        after = r.stats()
        assert after.tlas_refits > before.tlas_refits and after.tlas_rebuilds == before.tlas_rebuilds, (int(after.tlas_refits), int(after.tlas_rebuilds))
        _records_are_the_references(hrt, oracle, r, "mixed-moved", configuration == "two-level")
    finally:
        r.close()


@pytest.mark.parametrize("configuration", ["production", "two-level"])
def test_records_do_not_depend_on_the_batch(hrt, gpu_available, monkeypatch, configuration):
    """No oracle involved.  The records of a permutation of the rays are the permutation of the records, and the first n rays traced
    alone give the first n records of the full call: a small batch ends in the drained phase almost at once, which puts tail splitting
    and the leaf-pass quorum under rays of very unequal cost."""
    r = _renderer(hrt, gpu_available, monkeypatch, "CTX_TWO_LEVEL" if configuration == "two-level" else 0, {})
    try:
        r.load_scene(_scene(hrt, "mixed"))
        o, d = _rays(hrt, "mixed")[:2]
        full = r.trace_rays(o, d)
        assert (full[3] != rc.MISS).mean() > 0.2
        p = np.random.default_rng(11).permutation(len(o))
        shuffled = r.trace_rays(o[p], d[p])
        assert not rc.records_differ(shuffled, tuple(a[p] for a in full)).any()
        for n in (1, 63, 64, 65, 4097):
            part = r.trace_rays(o[:n], d[:n])
            assert not rc.records_differ(part, tuple(a[:n] for a in full)).any(), n
    finally:
        r.close()


@pytest.mark.parametrize("configuration", ["production", "two-level"])
def test_scaled_and_translated_scenes(hrt, oracle, gpu_available, monkeypatch, configuration):
    """The mixed scene at 2^-20 and 2^+20 of its size (node_exponent / quantise_axis and the padding's max(1, scale) floor away from unit
    size) with the origins scaled alike and the directions as they are: the record is the oracle's for every ray, and for the rays whose
    arithmetic stays in the normal range (ray_cases.tame) it is the UNSCALED run's with t x 2^k, the other fields the same bits.  And
    the scene moved to (1000, -500, 250), where a float resolves 6e-5, against the oracle."""
    instanced = configuration == "two-level"
    r = _renderer(hrt, gpu_available, monkeypatch, "CTX_TWO_LEVEL" if instanced else 0, {})
    try:
        r.load_scene(_scene(hrt, "mixed"))
        o, d, cls, info = _rays(hrt, "mixed")
        base = r.trace_rays(o, d)
        tame = rc.tame(info)
        assert tame.mean() > 0.4 and (base[3][tame] != rc.MISS).mean() > 0.2
        for name, k in (("mixed-small", -20), ("mixed-large", 20)):
            window = (rc.OPEN[0] * 2.0 ** k, rc.OPEN[1] * 2.0 ** k)
            r.load_scene(_scene(hrt, name))
            _records_are_the_references(hrt, oracle, r, name, instanced, windows=[window])
            o_k = _rays(hrt, name)[0]
            got = r.trace_rays(o_k, d, tmin=window[0], tmax=window[1])
            expect = ((base[0] * np.float32(2.0 ** k)).astype(np.float32),) + tuple(base[1:])
            diff = rc.records_differ(got, expect) & tame
            assert not diff.any(), (name, _describe(diff, o_k, d, cls, info, got, expect))
        r.load_scene(_scene(hrt, "mixed-far"))
        _records_are_the_references(hrt, oracle, r, "mixed-far", instanced)
    finally:
        r.close()
