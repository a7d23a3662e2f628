"""HRT_PRIMARY_RESTART: a launch that would run k_path_one with the seed window (HRT_SEED_PRIMARY=2) runs k_path_restart (fused_restart.hip), whose
repeat primary rays start at the node whose leaf slot holds their known hit's record (DESIGN.md section 4.1 "The start under the known hit";
the argument on the CPU: tests/test_primary_restart_cpu.py).  It must compute what k_path_one computes.

Bar: every case renders tests/test_one_group_gpu.py's frame, 61 x 37 pixels (2257: above the floor of 8 waves sample blocks need), at 8 samples
under the forced tapered schedule 4 : 2 -- blocks of 4, 2, 2, so that restarted rays (samples 2, 3, 5, 7 of a pixel), windowed root walks
(1, 4, 6: a pixel's second sample and every later block's first) and plain ones (0) all occur, and so small a frame spends most of its time
in the drained phase, with tail splitting and the mailboxes at work -- with the knob on and off on contexts of their own.  Both are the
oracle's frame bit for bit: colour, linear radiance, final RNG states, with its ray count; the closest-hit / any-hit split and the path count
are equal between the two.  Which kernel ran is read from HrtStats.restart_launches, and the device's leaf_parent table is compared with the
host's over the downloaded tree."""
import ctypes as C

import numpy as np
import pytest

from test_one_group_gpu import H, SALT, W, _check, _oracle

pytestmark = pytest.mark.gpu

SPP = 8
TAPER = (("HRT_SAMPLE_BLOCK", "auto"), ("HRT_SAMPLE_TAPER", "4:2!"))


def _soup(hrt, n=2000, edge=0.12, seed=7):
    return hrt.scenes.random_soup(n, edge, seed, W, H, SPP)


def _tables(hrt, r):
    """(the device's leaf_parent of the renderer's TLAS, the host's over the tree downloaded from the device)"""
    n = C.c_uint64()
    assert r.lib.hrt_tlas_leaf_parent(r.ctx, r.tlas, None, 0, C.byref(n)) != 0 and n.value > 0          # too small: says how many
    dev = np.full(n.value, 0xFFFFFFFF, np.uint32)
    assert r.lib.hrt_tlas_leaf_parent(r.ctx, r.tlas, dev.ctypes.data_as(C.POINTER(C.c_uint32)), len(dev), C.byref(n)) == 0, r.lib.hrt_last_error(r.ctx)
    blob = hrt.BvhBlob()
    assert r.lib.hrt_tlas_download(r.ctx, r.tlas, C.byref(blob)) == 0
    try:
        assert blob.n_triangles == n.value
        host = np.zeros(n.value, np.uint32)
        assert r.lib.hrt_host_leaf_parent(C.byref(blob), host.ctypes.data_as(C.POINTER(C.c_uint32)), len(host)) == 0, r.lib.hrt_last_error(None)
        assert host.max() < blob.n_nodes
    finally:
        r.lib.hrt_host_free(C.byref(blob))
    return dev, host


def _render(hrt, monkeypatch, scene, knob, launches=(SPP,), env=(), flags=0, moves=None):
    """The scene on a context of its own with HRT_PRIMARY_RESTART=knob; one render per entry of `launches` on the same RNG streams, after
    update_instances(moves[k]) where that is given -> (what every launch left, the counters, the device and host tables after each launch)"""
    monkeypatch.setenv("HRT_PRIMARY_RESTART", str(knob))
    monkeypatch.setenv("HRT_FUSED_LPT", "0")
    env = TAPER + tuple(env)
    for k, v in env:
        monkeypatch.setenv(k, v)
    r = hrt.Renderer(0, flags)
    try:
        r.load_scene(scene)
        r.set_frame(W, H, SALT, linear=True)
        r.reset_stats()
        out, tables = [], []
        for k, spp in enumerate(launches):
            if moves is not None and moves[k] is not None:
                r.update_instances([moves[k]])
            r.render(spp)
            s = r.stats()
            out.append({"linear": r.linear.cpu().numpy().copy(), "color": r.color.cpu().numpy().copy(), "states": r.rng_states_numpy(),
                        "counts": (int(s.rays), int(s.rays_closest), int(s.rays_any), int(s.paths))})
            tables.append(_tables(hrt, r))
        s = r.stats()
        return out, {"restart": int(s.restart_launches), "one": int(s.one_group_launches), "blocks": int(s.sample_block_launches),
                     "fallback": int(s.fused_fallback_launches), "refits": int(s.tlas_refits), "rebuilds": int(s.tlas_rebuilds), "stats": s}, tables
    finally:
        r.close()
        for k, _ in env:
            monkeypatch.delenv(k)


def _both(hrt, oracle, monkeypatch, scene, env=(), flags=0):
    on, c_on, t_on = _render(hrt, monkeypatch, scene, 1, env=env, flags=flags)
    off, c_off, _ = _render(hrt, monkeypatch, scene, 0, env=env, flags=flags)
    assert (c_on["restart"], c_on["one"], c_on["blocks"], c_on["fallback"]) == (1, 1, 1, 0), c_on
    assert (c_off["restart"], c_off["one"], c_off["blocks"], c_off["fallback"]) == (0, 1, 1, 0), c_off
    assert tuple(int(x) for x in c_on["stats"].sample_block_schedule) == (4, 2, 8, 3), list(c_on["stats"].sample_block_schedule)
    _check(on, off, _oracle(oracle, scene, (SPP,)))
    dev, host = t_on[0]
    assert np.array_equal(dev, host)
    return on, c_on


@pytest.mark.parametrize("tree", ["default", "fast_trace"])
@pytest.mark.parametrize("builder", ["device", "host"])
def test_soup_on_every_tree(hrt, oracle, gpu_available, monkeypatch, builder, tree):
    """2000 triangles through the device's and the host's builder, and through each one's tree with spatial splits (HRT_CTX_FAST_TRACE: a
    triangle has several records, and the record a walk accepts its hit from need not be the one whose box holds the hit point)"""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    env = (("HRT_BUILD", builder), ("HRT_FAST_TRACE_BUILD", builder))
    # (the device's split build starts with its top-down phase above 4096 primitives: 6000 long thin triangles for the split trees)
    n, edge = (6000, 0.2) if tree == "fast_trace" else (2000, 0.12)
    _, c = _both(hrt, oracle, monkeypatch, _soup(hrt, n, edge), env=env, flags=hrt.CTX_FAST_TRACE if tree == "fast_trace" else 0)
    if tree == "fast_trace":
        assert c["stats"].bvh_bytes > c["stats"].bvh_nodes * 80 + n * 48, (c["stats"].bvh_bytes, c["stats"].bvh_nodes)      # duplicated references


def test_every_triangle_twice(hrt, oracle, gpu_available, monkeypatch):
    """tests/test_primary_restart_cpu.py's soup with every triangle stored twice, the copy with other normals: every hit is a tie in t, and the
    lower id wins it from the restart as from the root -- the frame is that of the scene without the copies"""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    scene = _soup(hrt, 3000, 0.12, 17)
    it = scene["instances"][0]
    v = it["vertices"]
    tilt = (it["normals"] + np.float32(0.5) * np.roll(it["normals"], 1, axis=2)).astype(np.float32)
    it["vertices"], it["normals"] = np.ascontiguousarray(np.concatenate([v, v])), np.ascontiguousarray(np.concatenate([it["normals"], tilt]))
    on, _ = _both(hrt, oracle, monkeypatch, scene)
    want = _oracle(oracle, _soup(hrt, 3000, 0.12, 17), (SPP,))
    assert np.array_equal(on[0]["linear"].view(np.uint32), want[0]["linear"].view(np.uint32)) and np.array_equal(on[0]["states"], want[0]["states"])


@pytest.mark.parametrize("how", ["refit", "rebuild"])
def test_after_an_update(hrt, oracle, gpu_available, monkeypatch, how):
    """Render, move the instance (hrt_tlas_update), render again on the same RNG streams.  A refit keeps topology and record order, so the
    table stays and still equals the host's over the refitted tree; a rebuild (HRT_REFIT=0) is a new tree, whose table is made again."""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    scene = _soup(hrt)
    moved = hrt.scenes.rigid_transform((0.05, -0.04, 0.03), (0.2, 1.0, 0.1), 0.3, 1.05)
    env = (("HRT_REFIT", "1"), ("HRT_REFIT_REBUILD_RATIO", "1e30"), ("HRT_REFIT_MOVED_FAR", "0")) if how == "refit" else (("HRT_REFIT", "0"),)
    launches, moves = (SPP, SPP), (None, moved)
    on, c_on, t_on = _render(hrt, monkeypatch, scene, 1, launches, env, moves=moves)
    off, c_off, _ = _render(hrt, monkeypatch, scene, 0, launches, env, moves=moves)
    assert (c_on["restart"], c_on["one"], c_on["blocks"]) == (2, 2, 2) and (c_off["restart"], c_off["one"], c_off["blocks"]) == (0, 2, 2), (c_on, c_off)
    assert (c_on["refits"], c_on["rebuilds"]) == ((1, 1) if how == "refit" else (0, 2)), c_on
    ref = _oracle(oracle, scene, (SPP,))
    scene["instances"][0]["transform"] = moved
    o = oracle.OracleScene(scene)
    states = ref[0]["states"].copy()
    second = o.render(W, H, states, SPP)
    o.close()
    ref.append({"linear": second["linear"], "color": second["color"], "states": states.copy(), "rays": ref[0]["rays"] + int(second["rays"])})
    _check(on, off, ref)
    for dev, host in t_on:
        assert np.array_equal(dev, host)
    if how == "refit":
        assert np.array_equal(t_on[0][0], t_on[1][0])          # kept


def test_the_gate(hrt, gpu_available, monkeypatch):
    """Two instances, HRT_SEED_PRIMARY=1 and HRT_ONE_GROUP=0 each run the kernel they ran before, and restart_launches stays 0"""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    two = _soup(hrt)
    v = two["instances"][0]["vertices"]
    two["instances"] = [hrt.scenes._tri_instance(v[0::2], hrt.scenes.WHITE), hrt.scenes._tri_instance(v[1::2], hrt.scenes.RED, "metal", 0.1)]
    monkeypatch.setenv("HRT_PRIMARY_RESTART", "1")
    monkeypatch.setenv("HRT_FUSED_LPT", "0")
    for k, val in TAPER:
        monkeypatch.setenv(k, val)
    seen = {}
    for name, scene, env in (("two instances", two, ()), ("seed level 1", _soup(hrt), (("HRT_SEED_PRIMARY", "1"),)), ("seed off", _soup(hrt), (("HRT_SEED_PRIMARY", "0"),)),
                             ("k_path_blocks", _soup(hrt), (("HRT_ONE_GROUP", "0"),)), ("default", _soup(hrt), ())):
        for k, val in env:
            monkeypatch.setenv(k, val)
        r = hrt.Renderer(0, 0)
        try:
            r.load_scene(scene)
            r.set_frame(W, H, SALT, linear=True)
            r.reset_stats()
            r.render(SPP)
            s = r.stats()
            seen[name] = (int(s.restart_launches), int(s.one_group_launches), int(s.sample_block_launches))
        finally:
            r.close()
            for k, _ in env:
                monkeypatch.delenv(k)
    assert seen == {"two instances": (0, 0, 1), "seed level 1": (0, 1, 1), "seed off": (0, 1, 1), "k_path_blocks": (0, 0, 1), "default": (1, 1, 1)}, seen
    # a two-level tree and a tree with spheres have no table, and say so
    r = hrt.Renderer(0, 0)
    try:
        r.load_scene(hrt.scenes.sphere_in_box(W, H, 1))
        n = C.c_uint64()
        assert r.lib.hrt_tlas_leaf_parent(r.ctx, r.tlas, None, 0, C.byref(n)) != 0
    finally:
        r.close()
