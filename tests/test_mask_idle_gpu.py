"""HRT_MASK_IDLE: a launch that would run k_path_restart runs k_path_idle (fused_idle.hip), whose loop switches the lanes without a record / a
node off for the primitive test / the node step instead of letting them compute on stale registers (DESIGN.md sections 2.1 and 4.1; the
static side: tests/test_mask_idle_cpu.py).  Nothing that was used is left out, so it must compute what k_path_restart computes, bit for bit.

Bar: every case renders tests/test_primary_restart_gpu.py's frame -- 61 x 37 pixels at 8 samples, the smallest that takes sample blocks and the
restart -- with HRT_MASK_IDLE=1 and =0 on contexts of their own (HRT_PRIMARY_RESTART=1 in both), and both are the oracle's frame bit for bit:
colour, linear radiance, final RNG states, HrtStats.rays; the closest-hit / any-hit split and the path count are equal between the two.
Which kernel ran is read from HrtStats.mask_idle_launches (of restart_launches, of one_group_launches)."""
import numpy as np
import pytest

from test_one_group_gpu import H, SALT, W, _check, _oracle

pytestmark = pytest.mark.gpu

SPP = 8
UNIFORM = (("HRT_SAMPLE_BLOCK", "2"),)
TAPER = (("HRT_SAMPLE_BLOCK", "auto"), ("HRT_SAMPLE_TAPER", "4:2!"))


def _soup(hrt, n=2000, edge=0.12, seed=7):
    return hrt.scenes.random_soup(n, edge, seed, W, H, SPP)


def _render(hrt, monkeypatch, scene, knob, env=TAPER, flags=0, h=H):
    """The scene on a context of its own with HRT_MASK_IDLE=knob -> (what the launch left, the launch counters)"""
    env = (("HRT_MASK_IDLE", str(knob)), ("HRT_PRIMARY_RESTART", "1"), ("HRT_FUSED_LPT", "0")) + tuple(env)
    for k, v in env:
        monkeypatch.setenv(k, v)
    r = hrt.Renderer(0, flags)
    try:
        r.load_scene(scene)
        r.set_frame(W, h, SALT, linear=True)
        r.reset_stats()
        r.render(SPP)
        s = r.stats()
        out = [{"linear": r.linear.cpu().numpy().copy(), "color": r.color.cpu().numpy().copy(), "states": r.rng_states_numpy(),
                "counts": (int(s.rays), int(s.rays_closest), int(s.rays_any), int(s.paths))}]
        return out, {"idle": int(s.mask_idle_launches), "restart": int(s.restart_launches), "one": int(s.one_group_launches),
                     "blocks": int(s.sample_block_launches), "fallback": int(s.fused_fallback_launches), "stats": s}
    finally:
        r.close()
        for k, _ in env:
            monkeypatch.delenv(k)


def _both(hrt, oracle, monkeypatch, scene, env=TAPER, flags=0, h=H):
    on, c_on = _render(hrt, monkeypatch, scene, 1, env, flags, h)
    off, c_off = _render(hrt, monkeypatch, scene, 0, env, flags, h)
    assert (c_on["idle"], c_on["restart"], c_on["one"], c_on["blocks"], c_on["fallback"]) == (1, 1, 1, 1, 0), c_on
    assert (c_off["idle"], c_off["restart"], c_off["one"], c_off["blocks"], c_off["fallback"]) == (0, 1, 1, 1, 0), c_off
    ref = _oracle(oracle, scene, (SPP,), h=h)
    _check(on, off, ref)
    return on, c_on, ref


@pytest.mark.parametrize("schedule", ["uniform", "tapered"])
@pytest.mark.parametrize("tree", ["default", "fast_trace"])
def test_soup(hrt, oracle, gpu_available, monkeypatch, tree, schedule):
    """2000 triangles on the default tree; 6000 long thin ones on the tree with spatial splits (a triangle has several records) -- in uniform
    forced blocks of 2 and under the tapered schedule 4 : 2"""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    n, edge = (6000, 0.2) if tree == "fast_trace" else (2000, 0.12)
    _, c, _ = _both(hrt, oracle, monkeypatch, _soup(hrt, n, edge), env=UNIFORM if schedule == "uniform" else TAPER,
                    flags=hrt.CTX_FAST_TRACE if tree == "fast_trace" else 0)
    assert (int(c["stats"].sample_block_schedule[2]) != 0) == (schedule == "tapered")
    if tree == "fast_trace":
        assert c["stats"].bvh_bytes > c["stats"].bvh_nodes * 80 + n * 48      # duplicated references


def test_all_background(hrt, oracle, gpu_available, monkeypatch):
    """The camera looks away from the soup: every ray misses at the root, no lane ever has a primitive -- every primitive pass is empty and the
    node step's mask is the only one that is ever set"""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    scene = _soup(hrt)
    scene["camera"]["target"] = np.array([0, 0, 7], dtype=np.float32)
    on, _, _ = _both(hrt, oracle, monkeypatch, scene)
    assert on[0]["counts"][0] == W * H * SPP        # one ray per sample: the primary ray, which misses


def test_inside_a_closed_box(hrt, oracle, gpu_available, monkeypatch):
    """The soup and the camera inside a closed box, all one instance: no ray misses, every path runs to the depth limit"""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    scene = _soup(hrt)
    box = np.asarray(hrt.scenes._box((-2.0, -2.0, -2.0), (2.0, 2.0, 4.0), skip_bottom=False), np.float32)
    scene["instances"] = [hrt.scenes._tri_instance(np.concatenate([scene["instances"][0]["vertices"], box]), hrt.scenes.WHITE)]
    on, _, _ = _both(hrt, oracle, monkeypatch, scene)
    assert on[0]["counts"][0] > 4 * W * H * SPP          # (nothing escapes: the paths run on towards the depth limit of 5)


def test_every_triangle_twice(hrt, oracle, gpu_available, monkeypatch):
    """tests/test_primary_restart_gpu.py's soup with every triangle stored twice, the copy with other normals: every hit is a tie in t, decided
    by the masked test as by the wave-wide one -- the frame is that of the scene without the copies"""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    scene = _soup(hrt, 3000, 0.12, 17)
    it = scene["instances"][0]
    v = it["vertices"]
    tilt = (it["normals"] + np.float32(0.5) * np.roll(it["normals"], 1, axis=2)).astype(np.float32)
    it["vertices"], it["normals"] = np.ascontiguousarray(np.concatenate([v, v])), np.ascontiguousarray(np.concatenate([it["normals"], tilt]))
    on, _, _ = _both(hrt, oracle, monkeypatch, scene)
    want = _oracle(oracle, _soup(hrt, 3000, 0.12, 17), (SPP,))
    assert np.array_equal(on[0]["linear"].view(np.uint32), want[0]["linear"].view(np.uint32)) and np.array_equal(on[0]["states"], want[0]["states"])


def test_a_last_wave_with_fewer_pixels_than_lanes(hrt, oracle, gpu_available, monkeypatch):
    """61 x 10 = 610 pixels: nine waves' worth and 34 more (and a last slice of 2 pixels), still above the 448 that sample blocks need -- lanes
    that have neither a node nor a primitive for whole calls of the loop"""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    assert (W * 10) % 64 != 0 and W * 10 > 448
    _both(hrt, oracle, monkeypatch, _soup(hrt), h=10)


def test_the_gate(hrt, gpu_available, monkeypatch):
    """Two instances, HRT_ONE_GROUP=0, HRT_PRIMARY_RESTART=0 and HRT_SEED_PRIMARY=1 each run the kernel they ran before and say so"""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    two = _soup(hrt)
    v = two["instances"][0]["vertices"]
    two["instances"] = [hrt.scenes._tri_instance(v[0::2], hrt.scenes.WHITE), hrt.scenes._tri_instance(v[1::2], hrt.scenes.RED, "metal", 0.1)]
    seen = {}
    for name, scene, env in (("two instances", two, ()), ("k_path_blocks", _soup(hrt), (("HRT_ONE_GROUP", "0"),)),
                             ("seed level 1", _soup(hrt), (("HRT_SEED_PRIMARY", "1"),)), ("default", _soup(hrt), ())):
        _, c = _render(hrt, monkeypatch, scene, 1, TAPER + env)
        seen[name] = (c["idle"], c["restart"], c["one"], c["blocks"])
    monkeypatch.setenv("HRT_PRIMARY_RESTART", "0")      # (set after _render's own, which it removes again)
    env = (("HRT_MASK_IDLE", "1"), ("HRT_FUSED_LPT", "0")) + TAPER
    for k, val in env:
        monkeypatch.setenv(k, val)
    r = hrt.Renderer(0, 0)
    try:
        r.load_scene(_soup(hrt))
        r.set_frame(W, H, SALT, linear=True)
        r.reset_stats()
        r.render(SPP)
        s = r.stats()
        seen["no restart"] = (int(s.mask_idle_launches), int(s.restart_launches), int(s.one_group_launches), int(s.sample_block_launches))
    finally:
        r.close()
    assert seen == {"two instances": (0, 0, 0, 1), "k_path_blocks": (0, 0, 0, 1), "seed level 1": (0, 0, 1, 1), "default": (1, 1, 1, 1),
                    "no restart": (0, 0, 1, 1)}, seen
