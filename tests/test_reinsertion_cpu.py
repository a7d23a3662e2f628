"""The reinsertion pass of the host builder (bvh8_build.cpp: Reinsert; HRT_REINSERT rounds over the finished BVH2, before the collapse):
the tree stays a valid cover of every primitive, its summed inner-node area never grows, the build is deterministic, and the image is the
one the oracle renders through its own BVH2 -- the closest hit is canonical, so a better tree may only be a faster one."""
import ctypes as C
import re

import numpy as np
import pytest

from test_host_cpu import _host_bvh_lib

ROUNDS = 3


def _soup(hrt, n, seed=7):
    return hrt.scenes.random_soup(n, max(0.02, min(0.5, 0.6 * n ** (-1.0 / 3.0))), seed, 96, 64, 2)


def _scene_of(hrt, tris):
    return {"name": "reinsertion", "instances": [hrt.scenes._tri_instance(np.ascontiguousarray(tris, np.float32), hrt.scenes.WHITE)],
            "camera": hrt.scenes._soup_camera(), "background": hrt.scenes.BACKGROUND.copy(), "width": 96, "height": 64, "spp": 2}


def _scenes(hrt):
    one = _soup(hrt, 200, 3)["instances"][0]["vertices"].reshape(-1, 3, 3)[:1]
    with_outlier = _soup(hrt, 300, 5)["instances"][0]["vertices"].reshape(-1, 3, 3).copy()
    with_outlier[-1] += np.float32(1000.0 * 2.0)        # the soup spans [-1, 1]: 1000 extents away
    out = {f"soup{n}": _soup(hrt, n) for n in (1, 2, 9, 64, 2000)}
    out["copies200"] = _scene_of(hrt, np.repeat(one, 200, 0))
    out["chain210"] = hrt.scenes.growing_chain(210)
    out["outlier"] = _scene_of(hrt, with_outlier)
    return out


SCENES = ["soup1", "soup2", "soup9", "soup64", "soup2000", "copies200", "chain210", "outlier"]


def _triangles(scene):
    return np.ascontiguousarray(np.concatenate([it["vertices"].reshape(-1, 3, 3) for it in scene["instances"]]), np.float32)


def _build_bytes(hrt, tris):
    lib = _host_bvh_lib(hrt)
    blob = hrt.BvhBlob()
    rc = lib.hrt_host_build_bvh8(tris.ctypes.data, tris.shape[0], C.byref(blob))       # (runs validate_bvh8: anything but "" fails the build)
    assert rc == 0, lib.hrt_last_error(None)
    nodes = np.ctypeslib.as_array(C.cast(blob.nodes, C.POINTER(C.c_uint8)), shape=(blob.n_nodes * 80,)).copy()
    prims = np.ctypeslib.as_array(C.cast(blob.triangles, C.POINTER(C.c_uint8)), shape=(blob.n_triangles * 48,)).copy()
    # every record is covered by exactly one leaf slot
    if not hasattr(lib, "hrt_host_leaf_parent") or lib.hrt_host_leaf_parent.argtypes is None:
        lib.hrt_host_leaf_parent.restype = C.c_int
        lib.hrt_host_leaf_parent.argtypes = [C.POINTER(hrt.BvhBlob), C.POINTER(C.c_uint32), C.c_uint64]
    table = np.zeros(max(int(blob.n_triangles), 1), np.uint32)
    rc = lib.hrt_host_leaf_parent(C.byref(blob), table.ctypes.data_as(C.POINTER(C.c_uint32)), int(blob.n_triangles))
    assert rc == 0, lib.hrt_last_error(None)
    assert (table[:blob.n_triangles] < blob.n_nodes).all()
    lib.hrt_host_free(C.byref(blob))
    return nodes, prims


@pytest.fixture(scope="module")
def scenes(hrt):
    return _scenes(hrt)


@pytest.fixture(scope="module")
def reference(hrt, oracle, scenes):
    """the image of each scene through the oracle's own BVH2, rendered once"""
    out = {}
    for name, scene in scenes.items():
        states = oracle.rng_init(96, 64, 3)
        out[name] = oracle.OracleScene(scene).render(96, 64, states, 2)
    return out


@pytest.mark.parametrize("splits", [0, 1])
@pytest.mark.parametrize("name", SCENES)
def test_reinserted_tree_is_valid_deterministic_and_renders_the_same_image(hrt, oracle, scenes, reference, monkeypatch, capfd, name, splits):
    scene = scenes[name]
    tris = _triangles(scene)
    monkeypatch.setenv("HRT_SBVH", str(splits))
    monkeypatch.setenv("HRT_REINSERT", str(ROUNDS))
    monkeypatch.setenv("HRT_BUILD_VERBOSE", "1")
    capfd.readouterr()
    nodes, prims = _build_bytes(hrt, tris)
    err = capfd.readouterr().err
    # the summed inner-node area after a round is not above the value before it, and a round starts where the last one ended
    areas = [(float(a), float(b)) for a, b in re.findall(r"reinsertion round \d+: .* inner area (\S+) -> (\S+) ", err)]
    assert len(tris) < 2 or 1 <= len(areas) <= ROUNDS, err        # (the rounds end early once one moves next to nothing)
    for k, (before, after) in enumerate(areas):
        assert after <= before
        assert k == 0 or before == areas[k - 1][1]
    # two builds give identical bytes
    nodes2, prims2 = _build_bytes(hrt, tris)
    assert np.array_equal(nodes, nodes2) and np.array_equal(prims, prims2)
    # the oracle walks the product's tree to the very image it renders through its own BVH2
    osc = oracle.OracleScene(scene)
    osc.attach_bvh8(nodes, prims)
    states = oracle.rng_init(96, 64, 3)
    got = osc.render(96, 64, states, 2)
    want = reference[name]
    assert np.array_equal(got["linear"].view(np.uint32), want["linear"].view(np.uint32)) and got["rays"] == want["rays"]


def test_the_pass_moves_nodes_and_lowers_the_area_of_a_soup(hrt, scenes, monkeypatch, capfd):
    """... and is not a no-op: on the 2000-triangle soup the first round moves nodes and the area falls; with HRT_REINSERT=0 no round runs."""
    tris = _triangles(scenes["soup2000"])
    monkeypatch.setenv("HRT_SBVH", "1")
    monkeypatch.setenv("HRT_BUILD_VERBOSE", "1")
    monkeypatch.setenv("HRT_REINSERT", "1")
    capfd.readouterr()
    _build_bytes(hrt, tris)
    m = re.search(r"reinsertion round 1: (\d+) of (\d+) nodes moved, .* inner area (\S+) -> (\S+) ", capfd.readouterr().err)
    assert m and int(m.group(1)) > 0 and float(m.group(4)) < float(m.group(3))
    monkeypatch.setenv("HRT_REINSERT", "0")
    _build_bytes(hrt, tris)
    assert "reinsertion round" not in capfd.readouterr().err
