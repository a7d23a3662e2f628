"""The reinsertion pass of the device builder (build_reinsert.hip: HRT_REINSERT rounds over the finished BVH2 of a fast-trace build,
before the collapse) changes the tree and nothing else: every scene of tests/test_reinsertion_cpu.py renders under HRT_CTX_FAST_TRACE with
HRT_REINSERT=0 and with the default on contexts of their own -- the same linear radiance bit for bit, the same ray counts, the same
kernel (HrtStats.direct_launches) -- and the tree downloaded from the device covers every record exactly once, is at most 12 levels deep
(growing_chain(210), which the device builds 20 levels deep without the pass: no deeper than without it) and gives the CPU walker the hits of a brute-force search.  One case fills the top-down phase's segment tables (HRT_SBVH_SEG_CAP)."""
import ctypes as C
import re

import numpy as np
import pytest

from test_reinsertion_cpu import SCENES, _scenes, _soup, _triangles

pytestmark = pytest.mark.gpu

W, H, SPP, SALT = 61, 37, 8, 5
ENV = (("HRT_SAMPLE_BLOCK", "auto"), ("HRT_SAMPLE_TAPER", "4:2!"), ("HRT_FUSED_LPT", "0"), ("HRT_BUILD_VERBOSE", "1"))


@pytest.fixture(scope="module")
def scenes(hrt):
    out = _scenes(hrt)
    out["soup6000"] = _soup(hrt, 6000)          # (above 4096 primitives: the top-down phase with spatial splits runs)
    return out


def _render(hrt, oracle, monkeypatch, capfd, scene, rounds, env=()):
    """the scene on a fast-trace context of its own, HRT_REINSERT=rounds (None: unset)"""
    for k, v in ENV + tuple(env):
        monkeypatch.setenv(k, v)
    if rounds is None:
        monkeypatch.delenv("HRT_REINSERT", raising=False)
    else:
        monkeypatch.setenv("HRT_REINSERT", str(rounds))
    capfd.readouterr()
    r = hrt.Renderer(0, hrt.CTX_FAST_TRACE)
    try:
        r.load_scene(scene)
        log = capfd.readouterr().err
        r.set_frame(W, H, SALT, linear=True)
        r.reset_stats()
        r.render(SPP)
        s = r.stats()
        blob = hrt.BvhBlob()
        assert r.lib.hrt_tlas_download(r.ctx, r.tlas, C.byref(blob)) == 0
        try:
            # every record is covered by exactly one leaf slot, and the walker finds what brute force finds
            table = np.zeros(max(int(blob.n_triangles), 1), np.uint32)
            assert r.lib.hrt_host_leaf_parent(C.byref(blob), table.ctypes.data_as(C.POINTER(C.c_uint32)), int(blob.n_triangles)) == 0, r.lib.hrt_last_error(None)
            o, d = oracle.random_rays(1500, 11)
            walked = oracle.bvh8_trace(blob.nodes, blob.triangles, o, d)
        finally:
            r.lib.hrt_host_free(C.byref(blob))
        return {"linear": r.linear.cpu().numpy().copy(), "rays": int(s.rays), "closest": int(s.rays_closest), "any": int(s.rays_any), "paths": int(s.paths),
                "direct": int(s.direct_launches), "depth": int(s.bvh_depth), "nodes": int(s.bvh_nodes), "walked": walked[:5], "rays_od": (o, d),
                "moved": [int(m) for m in re.findall(r"device build: reinsertion round \d+: (\d+) of", log)], "log": log}
    finally:
        r.close()


def _same(off, on):
    assert np.array_equal(off["linear"].view(np.uint32), on["linear"].view(np.uint32))
    assert (off["rays"], off["closest"], off["any"], off["paths"]) == (on["rays"], on["closest"], on["any"], on["paths"])
    assert off["direct"] == on["direct"]
    # at most 12 levels, what the path kernels take -- wherever the tree without the pass is (the device's tree of growing_chain(210) is 20
    # levels deep without it, and with it: there the pass must not have made it deeper)
    assert on["depth"] <= max(12, off["depth"])
    assert all(np.array_equal(a, b) for a, b in zip(off["walked"], on["walked"]))


@pytest.mark.parametrize("name", SCENES)
def test_default_rounds_against_none(hrt, oracle, scenes, monkeypatch, capfd, name):
    scene = scenes[name]
    off = _render(hrt, oracle, monkeypatch, capfd, scene, 0)
    on = _render(hrt, oracle, monkeypatch, capfd, scene, None)
    assert off["moved"] == []
    _same(off, on)
    brute = oracle.OracleScene(scene, force_brute=True).trace(*on["rays_od"])
    assert all(np.array_equal(a, b) for a, b in zip(on["walked"], brute))
    if name == "soup2000":
        assert on["moved"] and on["moved"][0] > 0, on["log"]          # the pass ran and moved nodes ...
        assert on["direct"] > 0                                          # ... under the kernel the flagship runs


def test_split_build_with_full_segment_tables(hrt, oracle, scenes, monkeypatch, capfd):
    """6000 triangles go through the top-down phase; with its segment tables full (HRT_SBVH_SEG_CAP) the cells are large and PLOC builds
    most of the tree: the pass runs over that tree all the same."""
    scene = scenes["soup6000"]
    env = (("HRT_SBVH_SEG_CAP", "40"),)
    off = _render(hrt, oracle, monkeypatch, capfd, scene, 0, env)
    on = _render(hrt, oracle, monkeypatch, capfd, scene, None, env)
    _same(off, on)
    assert on["moved"] and on["moved"][0] > 0, on["log"]
    monkeypatch.delenv("HRT_SBVH_SEG_CAP")
    plain = _render(hrt, oracle, monkeypatch, capfd, scene, None)
    _same(off, plain)
    assert plain["moved"] and plain["moved"][0] > 0, plain["log"]
