"""HRT_PRIMARY_DIRECT: a launch that would run k_path_idle runs k_path_direct (fused_direct.hip), whose repeat primary rays are decided in the
regeneration that makes them -- the lane fetches the record its pixel's last primary ray accepted its hit from and runs the canonical primitive
test on it with the culling bound at that hit -- and never enter the traversal loop (DESIGN.md sections 2.1 and 4.1; the argument on the CPU and
the static side: tests/test_primary_direct_cpu.py).  The identical ray recomputes the identical hit, so it must compute what k_path_idle computes.

Bar: every case renders the neighbouring tests' frame -- 61 x 37 pixels at 8 samples, the smallest that takes sample blocks on 8 waves -- of the
3000-triangle soup with HRT_PRIMARY_DIRECT=1 and =0 on contexts of their own (HRT_FUSED_LPT=0), and both are the oracle's frame bit for bit after
every launch: colour, linear radiance, final RNG states, HrtStats.rays; the closest-hit / any-hit split and the path count are equal between the
two.  Which kernel ran is read from HrtStats.direct_launches (of mask_idle_launches, of restart_launches, of one_group_launches)."""
import copy

import numpy as np
import pytest

from test_one_group_gpu import H, SALT, W, _check, _oracle

pytestmark = pytest.mark.gpu

SPP = 8
UNIFORM = (("HRT_SAMPLE_BLOCK", "2"),)
TAPER = (("HRT_SAMPLE_BLOCK", "auto"), ("HRT_SAMPLE_TAPER", "4:2!"))


def _soup(hrt, n=3000, edge=0.12, seed=17):
    return hrt.scenes.random_soup(n, edge, seed, W, H, SPP)


def _render(hrt, monkeypatch, scene, knob, launches=(SPP,), env=TAPER, flags=0, h=H, moves=None, cameras=None):
    """The scene on a context of its own with HRT_PRIMARY_DIRECT=knob; one render per entry of `launches` on the same RNG streams, after
    update_instances(moves[k]) / set_camera(cameras[k]) where one is given -> (what every launch left, the launch counters)"""
    env = (("HRT_PRIMARY_DIRECT", str(knob)), ("HRT_FUSED_LPT", "0")) + tuple(env)
    for k, v in env:
        monkeypatch.setenv(k, v)
    r = hrt.Renderer(0, flags)
    try:
        r.load_scene(scene)
        r.set_frame(W, h, SALT, linear=True)
        r.reset_stats()
        out = []
        for k, spp in enumerate(launches):
            if moves is not None and moves[k] is not None:
                r.update_instances([moves[k]])
            if cameras is not None and cameras[k] is not None:
                cam = cameras[k]
                r.set_camera(cam["center"], cam["target"], cam["up"], cam.get("opengl", True))
            r.render(spp)
            s = r.stats()
            out.append({"linear": r.linear.cpu().numpy().copy(), "color": r.color.cpu().numpy().copy(), "states": r.rng_states_numpy(),
                        "counts": (int(s.rays), int(s.rays_closest), int(s.rays_any), int(s.paths))})
        s = r.stats()
        return out, {"direct": int(s.direct_launches), "idle": int(s.mask_idle_launches), "restart": int(s.restart_launches), "one": int(s.one_group_launches),
                     "blocks": int(s.sample_block_launches), "fallback": int(s.fused_fallback_launches), "refits": int(s.tlas_refits),
                     "rebuilds": int(s.tlas_rebuilds), "stats": s}
    finally:
        r.close()
        for k, _ in env:
            monkeypatch.delenv(k)


def _kernels(c):
    return c["direct"], c["idle"], c["restart"], c["one"], c["blocks"], c["fallback"]


def _both(hrt, oracle, monkeypatch, scene, env=TAPER, flags=0, h=H, n=1, ref=None, **how):
    launches = how.get("launches", (SPP,))
    on, c_on = _render(hrt, monkeypatch, scene, 1, env=env, flags=flags, h=h, **how)
    off, c_off = _render(hrt, monkeypatch, scene, 0, env=env, flags=flags, h=h, **how)
    assert _kernels(c_on) == (n, n, n, n, n, 0), c_on
    assert _kernels(c_off) == (0, n, n, n, n, 0), c_off
    ref = _oracle(oracle, scene, launches, h=h) if ref is None else ref
    _check(on, off, ref)
    for k, frame in enumerate(on):
        assert frame["counts"][3] == W * h * sum(launches[:k + 1])
    return on, c_on, ref


@pytest.mark.parametrize("schedule", ["uniform", "tapered"])
@pytest.mark.parametrize("tree", ["default", "fast_trace"])
def test_soup(hrt, oracle, gpu_available, monkeypatch, tree, schedule):
    """on the default tree, and on the fast-trace tree with spatial splits (a triangle has several records, and the record a pixel's first,
    unwindowed walk accepts its hit from need not be the one whose box holds the hit point) -- in uniform forced blocks of 2 (a block's first
    primary ray walks, its second is tested) and under the tapered schedule 4 : 2"""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    env = (UNIFORM if schedule == "uniform" else TAPER) + ((("HRT_FAST_TRACE_BUILD", "host"),) if tree == "fast_trace" else ())
    _, c, _ = _both(hrt, oracle, monkeypatch, _soup(hrt), env=env, flags=hrt.CTX_FAST_TRACE if tree == "fast_trace" else 0)
    assert (int(c["stats"].sample_block_schedule[2]) != 0) == (schedule == "tapered")
    if tree == "fast_trace":
        assert c["stats"].bvh_bytes > c["stats"].bvh_nodes * 80 + 3000 * 48      # duplicated references


def test_every_triangle_twice(hrt, oracle, gpu_available, monkeypatch):
    """every triangle stored twice, the copy with other normals: every hit is a tie in t, which the walk gave to the lower id -- and the record
    that is tested is that one's: the frame is that of the scene without the copies"""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    scene = _soup(hrt)
    it = scene["instances"][0]
    v = it["vertices"]
    tilt = (it["normals"] + np.float32(0.5) * np.roll(it["normals"], 1, axis=2)).astype(np.float32)
    it["vertices"], it["normals"] = np.ascontiguousarray(np.concatenate([v, v])), np.ascontiguousarray(np.concatenate([it["normals"], tilt]))
    on, _, _ = _both(hrt, oracle, monkeypatch, scene)
    want = _oracle(oracle, _soup(hrt), (SPP,))
    assert np.array_equal(on[0]["linear"].view(np.uint32), want[0]["linear"].view(np.uint32)) and np.array_equal(on[0]["states"], want[0]["states"])


def test_inside_a_closed_box(hrt, oracle, gpu_available, monkeypatch):
    """The soup and the camera inside a closed box, all one instance: every primary ray hits, so every lane that keeps its pixel holds a record"""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    scene = _soup(hrt)
    box = np.asarray(hrt.scenes._box((-2.0, -2.0, -2.0), (2.0, 2.0, 4.0), skip_bottom=False), np.float32)
    scene["instances"] = [hrt.scenes._tri_instance(np.concatenate([scene["instances"][0]["vertices"], box]), hrt.scenes.WHITE)]
    on, _, _ = _both(hrt, oracle, monkeypatch, scene)
    assert on[0]["counts"][0] > 4 * W * H * SPP          # (nothing escapes: the paths run on towards the depth limit of 5)


def test_all_background(hrt, oracle, gpu_available, monkeypatch):
    """The camera looks away from the soup: every primary ray misses, no lane ever holds a record, and nothing is ever tested in the regeneration"""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    scene = _soup(hrt)
    scene["camera"]["target"] = np.array([0, 0, 7], dtype=np.float32)
    on, _, _ = _both(hrt, oracle, monkeypatch, scene)
    assert on[0]["counts"][0] == W * H * SPP        # one ray per sample: the primary ray, which misses


def test_a_last_wave_with_fewer_pixels_than_lanes(hrt, oracle, gpu_available, monkeypatch):
    """61 x 10 = 610 pixels: nine waves' worth and 34 more (and a last slice of 2 pixels), still above the 448 that sample blocks need"""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    assert (W * 10) % 64 != 0 and W * 10 > 448
    _both(hrt, oracle, monkeypatch, _soup(hrt), h=10)


def test_a_render_cut_into_launches(hrt, oracle, gpu_available, monkeypatch):
    """HRT_FUSED_MAX_SPP=4 at 8 samples: two launches of 4 samples in blocks of 2, the second continuing the first's sums -- and starting without
    records, like every launch"""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    _both(hrt, oracle, monkeypatch, _soup(hrt), env=UNIFORM + (("HRT_FUSED_MAX_SPP", "4"),), n=2)


def test_the_camera_turns_between_two_launches(hrt, oracle, gpu_available, monkeypatch):
    """Render, turn the camera, render again on the same RNG streams and the same context: no record (and no seed) survives a launch"""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    scene = _soup(hrt)
    turned = {"center": np.array(scene["camera"]["center"], np.float32) + np.array([0.3, 0.2, 0.0], np.float32),
              "target": np.array(scene["camera"]["target"], np.float32) + np.array([-0.4, 0.1, 0.0], np.float32),
              "up": np.array(scene["camera"]["up"], np.float32), "opengl": scene["camera"].get("opengl", True)}
    ref = _oracle(oracle, scene, (SPP,))
    second_scene = copy.deepcopy(scene)
    second_scene["camera"].update(turned)
    o = oracle.OracleScene(second_scene)
    states = ref[0]["states"].copy()
    second = o.render(W, H, states, SPP)
    o.close()
    ref.append({"linear": second["linear"], "color": second["color"], "states": states.copy(), "rays": ref[0]["rays"] + int(second["rays"])})
    assert not np.array_equal(ref[0]["linear"], ref[1]["linear"])
    _both(hrt, oracle, monkeypatch, scene, n=2, ref=ref, launches=(SPP, SPP), cameras=(None, turned))


@pytest.mark.parametrize("how", ["refit", "rebuild"])
def test_after_an_update(hrt, oracle, gpu_available, monkeypatch, how):
    """Render, move the instance (hrt_tlas_update), render again on the same RNG streams: after a refit the records hold other coordinates,
    after a rebuild (HRT_REFIT=0) they are other records in another order"""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    scene = _soup(hrt)
    moved = hrt.scenes.rigid_transform((0.05, -0.04, 0.03), (0.2, 1.0, 0.1), 0.3, 1.05)
    env = TAPER + ((("HRT_REFIT", "1"), ("HRT_REFIT_REBUILD_RATIO", "1e30"), ("HRT_REFIT_MOVED_FAR", "0")) if how == "refit" else (("HRT_REFIT", "0"),))
    ref = _oracle(oracle, scene, (SPP,))
    second_scene = copy.deepcopy(scene)
    second_scene["instances"][0]["transform"] = moved
    o = oracle.OracleScene(second_scene)
    states = ref[0]["states"].copy()
    second = o.render(W, H, states, SPP)
    o.close()
    ref.append({"linear": second["linear"], "color": second["color"], "states": states.copy(), "rays": ref[0]["rays"] + int(second["rays"])})
    _, c, _ = _both(hrt, oracle, monkeypatch, scene, env=env, n=2, ref=ref, launches=(SPP, SPP), moves=(None, moved))
    assert (c["refits"], c["rebuilds"]) == ((1, 1) if how == "refit" else (0, 2)), c


@pytest.mark.parametrize("material,fuzz", [("rough", 0.0), ("rough", 0.3), ("metal", 0.0), ("metal", 0.3)])
def test_materials(hrt, oracle, gpu_available, monkeypatch, material, fuzz):
    """rough and metal, with and without fuzz: the scatter that now runs once for both kinds of lanes draws or does not draw, for the whole wave"""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    scene = _soup(hrt)
    it = scene["instances"][0]
    it["material"], it["fuzz"] = material, fuzz
    if material == "metal":
        it["albedo"] = hrt.scenes.STEEL.copy()
    _both(hrt, oracle, monkeypatch, scene)


def test_the_gate(hrt, gpu_available, monkeypatch):
    """Two instances, HRT_ONE_GROUP=0, HRT_SEED_PRIMARY=1, HRT_PRIMARY_RESTART=0 and HRT_MASK_IDLE=0 each run the kernel they ran before, and
    direct_launches stays 0; with defaults every k_path_idle launch is a k_path_direct launch"""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    two = _soup(hrt)
    v = two["instances"][0]["vertices"]
    two["instances"] = [hrt.scenes._tri_instance(v[0::2], hrt.scenes.WHITE), hrt.scenes._tri_instance(v[1::2], hrt.scenes.RED, "metal", 0.1)]
    seen = {}
    for name, scene, env in (("two instances", two, ()), ("k_path_blocks", _soup(hrt), (("HRT_ONE_GROUP", "0"),)),
                             ("seed level 1", _soup(hrt), (("HRT_SEED_PRIMARY", "1"),)), ("no restart", _soup(hrt), (("HRT_PRIMARY_RESTART", "0"),)),
                             ("no idle lanes off", _soup(hrt), (("HRT_MASK_IDLE", "0"),))):
        _, c = _render(hrt, monkeypatch, scene, 1, env=TAPER + env)
        seen[name] = _kernels(c)[:5]
    assert seen == {"two instances": (0, 0, 0, 0, 1), "k_path_blocks": (0, 0, 0, 0, 1), "seed level 1": (0, 0, 0, 1, 1), "no restart": (0, 0, 0, 1, 1),
                    "no idle lanes off": (0, 0, 1, 1, 1)}, seen
    # defaults: no knob of this chain in the environment
    for k, val in (("HRT_FUSED_LPT", "0"),) + TAPER:
        monkeypatch.setenv(k, val)
    r = hrt.Renderer(0, 0)
    try:
        r.load_scene(_soup(hrt))
        r.set_frame(W, H, SALT, linear=True)
        r.reset_stats()
        r.render(SPP)
        r.render(SPP)
        s = r.stats()
        assert int(s.direct_launches) == int(s.mask_idle_launches) > 0, (int(s.direct_launches), int(s.mask_idle_launches))
    finally:
        r.close()
