"""The node step's interval form (csrc/trav_common.h) on the device: the path kernels map a ray's interval
[tmin, bt] onto [0, 1] in every node step, so what is checked here is what depends on tmin, tmax and bt -- callers' windows of every size
through the production path kernel against brute force, a tie at bt between leaves, and renders against the CPU oracle bit for bit through
every kernel that runs the shared loop.  Scenes of a few thousand triangles, frames of at most 64 x 64, at most 8 spp."""
import numpy as np
import pytest

import ray_cases as rc

pytestmark = pytest.mark.gpu

SALT = 17
_CACHE = {}


def _need_gpu(gpu_available):
    if not gpu_available:
        pytest.skip("no GPU in this container")


def _mixed(hrt):
    """2500 triangles, 50 spheres, transforms, all four programs; 6000 adversarial rays made from its own geometry"""
    if "mixed" not in _CACHE:
        scene = hrt.scenes.mixed_test_scene(2500, 50, 13)
        o, d, cls, info = rc.adversarial_rays(scene, 6000, 5, rc.scene_extent(scene), details=True)
        _CACHE["mixed"] = (scene, o, d, info)
    return _CACHE["mixed"]


def _brute(oracle, scene, o, d, tmin, tmax):
    return oracle.OracleScene(scene, force_brute=True).trace(o, d, tmin=tmin, tmax=tmax)


def _same_records(r, oracle, scene, o, d, tmin, tmax, what):
    want = _brute(oracle, scene, o, d, tmin, tmax)
    got = r.trace_rays(o, d, tmin=tmin, tmax=tmax)
    diff = rc.records_differ(got, want)
    j = int(np.argmax(diff))
    assert not diff.any(), (what, tmin, tmax, int(diff.sum()), o[j], d[j], [float(a[j]) for a in got[:3]], int(got[3][j]), [float(a[j]) for a in want[:3]], int(want[3][j]))
    any_got = r.trace_rays(o, d, tmin=tmin, tmax=tmax, any_hit=True)
    adiff = (any_got[3] != rc.MISS) != (want[3] != rc.MISS)
    assert not adiff.any(), (what, tmin, tmax, "any hit", int(adiff.sum()))
    return want


# ---------------------------------------------------------------- callers' rays ----------------------------------------------------------------
def test_callers_windows_through_the_production_path_kernel(hrt, oracle, gpu_available):
    """hrt_trace_rays on k_fused, closest and any hit, against brute force: tmin = 0 with directions of length 1e-30, 1 and 1e30 (the
    generator's own scales, and every ray rescaled to each of them: |d| (tmax - tmin) is 1e46 for the longest, which the ray's start
    bounds), tmin = 1e-30, and the two windows that end and begin at a distance a few hundred rays share bit for bit."""
    _need_gpu(gpu_available)
    scene, o, d, info = _mixed(hrt)
    r = hrt.Renderer(0, 0)
    try:
        r.load_scene(scene)
        open_ref = _same_records(r, oracle, scene, o, d, 0.0, 1e16, "tmin = 0")
        assert (open_ref[3] != rc.MISS).mean() > 0.2
        for s in (1e-30, 1e30):
            unit = np.isin(info["scale"], (1.0,)) & ~info["replaced"]
            with np.errstate(over="ignore", under="ignore"):
                ds = (d[unit].astype(np.float64) * s).astype(np.float32)
            want = _same_records(r, oracle, scene, o[unit], ds, 0.0, 1e16, "tmin = 0, |d| = %g" % s)
            if s == 1e30:
                assert (want[3] != rc.MISS).mean() > 0.2 and float(want[0][want[3] != rc.MISS].max()) < 1e-28
            else:
                assert (want[3] == rc.MISS).all()                 # every hit lies beyond 1e16
        _same_records(r, oracle, scene, o, d, 1e-30, 1e16, "tmin = 1e-30")
        ref = _brute(oracle, scene, o, d, *rc.OPEN)
        (below, above), star, at = rc.bound_windows(ref[0], ref[3])
        assert at.sum() >= 100
        w_below = _same_records(r, oracle, scene, o, d, below[0], below[1], "(1e-6, t*)")
        w_above = _same_records(r, oracle, scene, o, d, above[0], above[1], "(t*, 1e16)")
        # both bounds are strict: a ray at t* loses that hit in either window (it misses, or hits another primitive elsewhere)
        assert (w_below[3][at] != ref[3][at]).all() and (w_above[3][at] != ref[3][at]).all()
        assert r.stats().fused_fallback_launches == 0
    finally:
        r.close()


@pytest.mark.parametrize("tmin, tmax", [(0.5, 0.5), (0.0, 0.0), (2.0, 0.5), (1e16, 1e-6), (1e-6, float("nan"))])
def test_an_empty_interval_is_all_misses_and_the_launch_returns(hrt, gpu_available, monkeypatch, tmin, tmax):
    """tmax = tmin, tmax < tmin and a NaN: t = tmax, no primitive, no instance -- from the host's answer where the path kernel would run
    (HRT_FUSED=1), and from k_traverse, which is launched on every interval (HRT_FUSED=0)."""
    _need_gpu(gpu_available)
    scene, o, d, info = _mixed(hrt)
    for fused in ("1", "0"):
        monkeypatch.setenv("HRT_FUSED", fused)
        r = hrt.Renderer(0, 0)
        try:
            r.load_scene(scene)
            for any_hit in (False, True):
                t, u, v, prim, inst = r.trace_rays(o[:1000], d[:1000], tmin=tmin, tmax=tmax, any_hit=any_hit)
                assert (prim == rc.MISS).all() and (inst == rc.MISS).all()
                assert np.array_equal(t.view(np.uint32), np.full(1000, tmax, np.float32).view(np.uint32)) and not u.any() and not v.any()
        finally:
            r.close()


# ---------------------------------------------------------------- a tie at bt ----------------------------------------------------------------
COPIES = 24


def _tie_scene(hrt):
    """COPIES coincident quads at z = 0.5 (primitives 2 .. 2 + 2 COPIES - 1 of instance 0: more than any leaf holds, so the copies lie in
    several leaves with one and the same box), a large slanted surface behind them whose box contains them (primitives 0 and 1: a leaf
    that a ray can meet first), and a soup around them that gives the tree its levels."""
    q = hrt.scenes._quad([0.2, 0.2, 0.5], [0.8, 0.2, 0.5], [0.8, 0.8, 0.5], [0.2, 0.8, 0.5])
    back = hrt.scenes._quad([-0.5, -0.5, 0.4], [1.5, -0.5, 0.4], [1.5, 1.5, 1.6], [-0.5, 1.5, 1.6])
    soup = hrt.scenes.random_soup(1500, 0.15, 3, 64, 64, 1)["instances"][0]["vertices"].reshape(-1, 3, 3).copy()
    soup[:, :, 2] = soup[:, :, 2] * np.float32(0.3) + np.float32(2.0)                  # behind everything: never the closest hit of a ray at the quads
    v = np.concatenate([np.asarray(back, np.float32), np.tile(np.asarray(q, np.float32), (COPIES, 1, 1)), soup.astype(np.float32)])
    return {"name": "tie", "instances": [hrt.scenes._tri_instance(v, hrt.scenes.WHITE)], "camera": hrt.scenes._cornell_camera(),
            "background": hrt.scenes.BACKGROUND.copy(), "width": 64, "height": 64, "spp": 1}


@pytest.mark.parametrize("env", [{}, {"HRT_FUSED": "0"}, {"HRT_BUILD": "host"}], ids=["path-kernel", "queue-form", "host-build"])
def test_a_tie_at_bt_reports_the_lowest_primitive(hrt, oracle, gpu_available, monkeypatch, env):
    """64 x 64 rays at the coincident quads, from in front of them and straight or slanted.  Whichever copy a ray finds first, bt is then
    the distance of all the others, whose leaves must still be visited: every hit on the quads reports primitive 2 or 3, the lowest of
    its triangle's copies (brute force says which).  The surface behind shrinks bt before that for the rays that meet its leaf first."""
    _need_gpu(gpu_available)
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    scene = _tie_scene(hrt)
    g = (np.arange(64, dtype=np.float64) + 0.5) / 64
    x, y = np.meshgrid(0.1 + 0.8 * g, 0.1 + 0.8 * g)
    o = np.stack([x.ravel(), y.ravel(), np.full(4096, -0.25)], 1).astype(np.float32)
    d = np.tile(np.float32([0, 0, 1]), (4096, 1))
    d[1::2] = np.float32([0.3, -0.2, 1.0])                                             # (not normalised: t is whatever it is)
    d[2::4, 2] = np.float32(2.0)                                                       # t = 0.375 exactly for the straight ones
    r = hrt.Renderer(0, 0)
    try:
        r.load_scene(scene)
        want = _same_records(r, oracle, scene, o, d, 1e-6, 1e16, "tie")
        assert r.stats().bvh_nodes > 8                                                 # (the tree last traced)
        got = r.trace_rays(o, d)
        on_quads = (want[3] >= 2) & (want[3] < 2 + 2 * COPIES)
        assert on_quads.sum() > 1500 and (got[3][on_quads] <= 3).all() and set(np.unique(got[3][on_quads])) == {2, 3}
    finally:
        r.close()


# ---------------------------------------------------------------- renders against the oracle ----------------------------------------------------------------
def _render_is_the_oracles(hrt, oracle, monkeypatch, scene, w, h, spp, flags=0, env=(), instanced=False):
    for k, v in env:
        monkeypatch.setenv(k, v)
    r = hrt.Renderer(0, flags)
    try:
        r.load_scene(scene)
        r.set_frame(w, h, SALT, linear=True)
        r.reset_stats()
        r.render(spp)
        st = r.stats()
        linear = r.linear.cpu().numpy().copy()
        key = (scene["name"], w, h, spp, instanced)
        if key not in _CACHE:
            _CACHE[key] = oracle.OracleScene(scene, instanced=instanced).render(w, h, oracle.rng_init(w, h, SALT), spp)
        ref = _CACHE[key]
        assert np.array_equal(linear.view(np.uint32), ref["linear"].view(np.uint32)), int((linear.view(np.uint32) != ref["linear"].view(np.uint32)).any(-1).sum())
        assert int(st.rays) == int(ref["rays"]) and int(st.fused_fallback_launches) == 0
        return st
    finally:
        r.close()


def _soup(hrt, w, h, spp):
    return hrt.scenes.random_soup(3000, 0.15, 5, w, h, spp, name="soup-3000")


def test_one_level_triangles_through_k_fused(hrt, oracle, gpu_available, monkeypatch):
    _need_gpu(gpu_available)
    st = _render_is_the_oracles(hrt, oracle, monkeypatch, _soup(hrt, 64, 64, 8), 64, 64, 8, env=(("HRT_SAMPLE_BLOCK", "0"),))
    assert int(st.sample_block_launches) == 0


def test_the_same_scene_through_k_path_blocks(hrt, oracle, gpu_available, monkeypatch):
    """64 x 64 = 64 waves: every slice counter is some wave's home, the grid rule of test_sample_blocks_gpu.py"""
    _need_gpu(gpu_available)
    st = _render_is_the_oracles(hrt, oracle, monkeypatch, _soup(hrt, 64, 64, 8), 64, 64, 8, env=(("HRT_SAMPLE_BLOCK", "2"),))
    assert int(st.sample_block_launches) == 1


def test_a_sphere_scene(hrt, oracle, gpu_available, monkeypatch):
    _need_gpu(gpu_available)
    _render_is_the_oracles(hrt, oracle, monkeypatch, hrt.scenes.sphere_in_box(48, 48, 8), 48, 48, 8)


def test_a_two_level_scene(hrt, oracle, gpu_available, monkeypatch):
    _need_gpu(gpu_available)
    _render_is_the_oracles(hrt, oracle, monkeypatch, hrt.scenes.particle_cloud(200, 48, 48, 4), 48, 48, 4, flags=hrt.CTX_TWO_LEVEL, instanced=True)


def test_a_tile_that_is_drained_at_once(hrt, oracle, gpu_available, monkeypatch):
    """16 x 12 = 192 pixels in three waves at 8 spp: the tile is used up by the first regeneration, the render is the drained phase with
    tail splitting from there on."""
    _need_gpu(gpu_available)
    monkeypatch.setenv("HRT_TAIL_SPLIT", "1")
    _render_is_the_oracles(hrt, oracle, monkeypatch, _soup(hrt, 16, 12, 8), 16, 12, 8)


def test_one_frame_through_the_queue_form(hrt, oracle, gpu_available, monkeypatch):
    _need_gpu(gpu_available)
    _render_is_the_oracles(hrt, oracle, monkeypatch, _soup(hrt, 48, 32, 2), 48, 32, 2, env=(("HRT_FUSED", "0"),))
