"""HRT_ONE_GROUP: a launch in sample blocks of a scene with one hit group -- a one-level tree of triangles over exactly one instance -- runs
k_path_one (fused_one.hip), whose regeneration reads the one material with scalar loads and keeps no albedo chain, and whose primitive
test decides ties by the primitive id alone (DESIGN.md sections 2.1 and 4.1).  It must compute what k_path_blocks<false> computes.

Bar: every case renders 61 x 37 pixels (2257: above the floor of 8 waves sample blocks need) with HRT_ONE_GROUP=1 and with HRT_ONE_GROUP=0 on
contexts of their own, and both are the oracle's frame bit for bit -- colour, linear radiance, final RNG states -- with its ray count; the
closest-hit / any-hit split of the count, which the oracle does not report, is equal between the two.  The hostile albedo cases compare NaNs
by class (shading_cases.components_differ says why), everything else by bits.  Which kernel ran is read from HrtStats.one_group_launches.

(The gate's last case switches a context between a one-instance and a two-instance TLAS of the same scene: hrt_tlas_update itself keeps the
instance count, so "an update from one instance to two" is a second TLAS in this library.)"""
import numpy as np
import pytest

import shading_cases as sh

pytestmark = pytest.mark.gpu

W, H = 61, 37
SALT = 57
BLOCKS = (("HRT_SAMPLE_BLOCK", "2"),)
TAPER = (("HRT_SAMPLE_BLOCK", "auto"), ("HRT_SAMPLE_TAPER", "4:2!"))


def _soup(hrt, material="rough", fuzz=0.0, n=2000, spp=5):
    scene = hrt.scenes.random_soup(n, 0.12, 7, W, H, spp)
    it = scene["instances"][0]
    it["material"], it["fuzz"] = material, fuzz
    if material == "metal":
        it["albedo"] = hrt.scenes.STEEL.copy()
    return scene


def _render(hrt, monkeypatch, scene, knob, launches=(5,), env=BLOCKS, flags=0, tile=None, salt=SALT, h=H):
    """The scene on a context of its own with HRT_ONE_GROUP=knob, one render per entry of `launches` on the same RNG streams -> what every
    launch left (buffers, states, counts) and the context's launch counters"""
    monkeypatch.setenv("HRT_ONE_GROUP", str(knob))
    monkeypatch.setenv("HRT_FUSED_LPT", "0")
    for k, v in env:
        monkeypatch.setenv(k, v)
    r = hrt.Renderer(0, flags)
    try:
        r.load_scene(scene)
        r.set_frame(W, h, salt, linear=True)
        r.reset_stats()
        out = []
        for spp in launches:
            r.render(spp, tile=tile)
            s = r.stats()
            out.append({"linear": r.linear.cpu().numpy().copy(), "color": r.color.cpu().numpy().copy(), "states": r.rng_states_numpy(),
                        "counts": (int(s.rays), int(s.rays_closest), int(s.rays_any), int(s.paths))})
        s = r.stats()
        return out, {"one": int(s.one_group_launches), "blocks": int(s.sample_block_launches), "fallback": int(s.fused_fallback_launches), "stats": s}
    finally:
        r.close()
        for k, _ in env:
            monkeypatch.delenv(k)


def _oracle(oracle, scene, launches=(5,), salt=SALT, h=H):
    o = oracle.OracleScene(scene)
    states, out, rays = oracle.rng_init(W, h, salt), [], 0
    for spp in launches:
        ref = o.render(W, h, states, spp)
        rays += int(ref["rays"])
        out.append({"linear": ref["linear"], "color": ref["color"], "states": states.copy(), "rays": rays})
    o.close()
    return out


def _differ(a, b, nan_by_class):
    if nan_by_class:
        return bool(sh.components_differ(a, b).any())
    return not np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _check(on, off, ref, nan_by_class=False):
    """knob 1 against knob 0 and against the oracle, after every launch"""
    assert len(on) == len(off) == len(ref)
    for k, (a, b, want) in enumerate(zip(on, off, ref)):
        for what in ("color", "linear"):
            assert not _differ(a[what], b[what], nan_by_class), (k, what, "knob 1 against knob 0")
            assert not _differ(a[what], want[what], nan_by_class), (k, what, "knob 1 against the oracle")
            assert not _differ(b[what], want[what], nan_by_class), (k, what, "knob 0 against the oracle")
        assert np.array_equal(a["states"], b["states"]) and np.array_equal(a["states"], want["states"]), k
        assert a["counts"] == b["counts"] and a["counts"][0] == want["rays"], (k, a["counts"], b["counts"], want["rays"])
        assert a["counts"][1] + a["counts"][2] == a["counts"][0]


def _both(hrt, oracle, monkeypatch, scene, launches=(5,), env=BLOCKS, flags=0, nan_by_class=False, salt=SALT, block_launches=None):
    on, c_on = _render(hrt, monkeypatch, scene, 1, launches, env, flags, salt=salt)
    off, c_off = _render(hrt, monkeypatch, scene, 0, launches, env, flags, salt=salt)
    n = len(launches) if block_launches is None else block_launches
    assert (c_on["one"], c_on["blocks"], c_on["fallback"]) == (n, n, 0), c_on
    assert (c_off["one"], c_off["blocks"], c_off["fallback"]) == (0, n, 0), c_off
    _check(on, off, _oracle(oracle, scene, launches, salt), nan_by_class)
    return on, c_on


@pytest.mark.parametrize("schedule", ["uniform", "tapered"])
def test_soup_of_one_instance(hrt, oracle, gpu_available, monkeypatch, schedule):
    """2000 rough triangles, 5 samples: in blocks of 2, 2, 1 and under the tapered schedule 4 : 2"""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    _, c = _both(hrt, oracle, monkeypatch, _soup(hrt), env=BLOCKS if schedule == "uniform" else TAPER)
    assert (int(c["stats"].sample_block_schedule[2]) != 0) == (schedule == "tapered")


@pytest.mark.parametrize("fuzz", [0.0, 0.3])
def test_metal_soup(hrt, oracle, gpu_available, monkeypatch, fuzz):
    """the wave-uniform choice between rough and metal, and between drawing and not drawing (fuzz > 0)"""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    _both(hrt, oracle, monkeypatch, _soup(hrt, "metal", fuzz))


def _radiance_room(hrt, background, albedo, material="rough", fuzz=0.0):
    """shading_cases.radiance's room -- an opening in the front wall, two boxes -- as ONE instance with one hostile albedo"""
    scene = sh.radiance(hrt.scenes, background)
    tris = np.concatenate([it["vertices"] for it in scene["instances"]])
    scene["instances"] = [hrt.scenes._tri_instance(tris, albedo, material, fuzz)]
    return scene


@pytest.mark.parametrize("background", sorted(sh.RADIANCE_BACKGROUNDS))
def test_hostile_albedos_and_backgrounds(hrt, oracle, gpu_available, monkeypatch, background):
    """Every albedo of shading_cases.RADIANCE_ALBEDOS (1e30, 1e-30, 0, -0, -0.5, denormal, inf, -inf, NaN) as the one instance's, under each of
    the four backgrounds: the fold multiplies the same products in the same order -- bg . a . a . a . a, 0 x inf and the signs included.  One
    context pair per albedo, 4 samples and then 1 more on the same streams (a launch of one sample is one block: the plain kernel continues
    the sums k_path_one left)."""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    for key in sorted(sh.RADIANCE_ALBEDOS):
        metal = key in ("D", "A")                 # (the rooms of shading_cases deal metal to these two)
        scene = _radiance_room(hrt, background, sh.RADIANCE_ALBEDOS[key], "metal" if metal else "rough", 0.1 if key == "D" else 0.0)
        _both(hrt, oracle, monkeypatch, scene, launches=sh.SPP, nan_by_class=True, salt=hrt.scenes.SEED_SALT, block_launches=1)


def test_every_triangle_twice_on_a_split_tree(hrt, oracle, gpu_available, monkeypatch):
    """1500 long thin triangles, each present twice in the instance -- the copy with other normals, so that who wins a tie shows in the next
    bounce -- on the fast-trace tree of the host builder, whose leaves reference a triangle several times: every hit is a tie at the same
    distance, between the two copies and between the references of each, and the lower primitive id wins it."""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    n = 1500
    scene = hrt.scenes.random_soup(n, 0.2, 13, W, H, 5)
    it = scene["instances"][0]
    v = it["vertices"]
    tilt = (it["normals"] + np.float32(0.5) * np.roll(it["normals"], 1, axis=2)).astype(np.float32)
    it["vertices"], it["normals"] = np.ascontiguousarray(np.concatenate([v, v])), np.ascontiguousarray(np.concatenate([it["normals"], tilt]))
    env = BLOCKS + (("HRT_FAST_TRACE_BUILD", "host"),)
    _, c = _both(hrt, oracle, monkeypatch, scene, env=env, flags=hrt.CTX_FAST_TRACE)
    st = c["stats"]
    assert st.bvh_triangles == 2 * n and st.bvh_bytes > st.bvh_nodes * 80 + 2 * n * 48 * 1.05, (st.bvh_triangles, st.bvh_bytes, st.bvh_nodes)      # duplicated references
    # the copy never wins: the frame is that of the scene with the tilted normals nowhere
    plain = hrt.scenes.random_soup(n, 0.2, 13, W, H, 5)
    want = _oracle(oracle, plain)
    on, _ = _render(hrt, monkeypatch, scene, 1, env=env, flags=hrt.CTX_FAST_TRACE)
    assert np.array_equal(on[0]["linear"].view(np.uint32), want[0]["linear"].view(np.uint32)) and np.array_equal(on[0]["states"], want[0]["states"])


def test_all_miss_frame(hrt, oracle, gpu_available, monkeypatch):
    """the camera looks away from the soup: every path is one ray and the background, every block ends at once"""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    scene = _soup(hrt)
    scene["camera"] = dict(scene["camera"], target=np.array([0, 0, 7.0], np.float32))
    on, _ = _both(hrt, oracle, monkeypatch, scene)
    assert on[0]["counts"][0] == W * H * 5 and on[0]["counts"][2] == 0


def test_sum_continued_over_two_launches(hrt, oracle, gpu_available, monkeypatch):
    """HRT_FUSED_MAX_SPP=3 at 5 samples: launches of 3 and 2 samples, the second continuing the first's sums -- one render call, two launches in
    blocks of 1 -- and then a second render call of 5 samples on the same RNG streams"""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    _both(hrt, oracle, monkeypatch, _soup(hrt), launches=(5, 5), env=(("HRT_SAMPLE_BLOCK", "1"), ("HRT_FUSED_MAX_SPP", "3")), block_launches=4)


def test_tile_with_a_row_stride(hrt, oracle, gpu_available, monkeypatch):
    """A frame of 61 x 77 of which the tile is every other row of 2 .. 75 (a rank's share): 61 x 37 = 2257 pixels through a row list"""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    h_frame = 77
    tile = hrt.Tile(2, 76, 1, 2, 1)
    rows = [y for y in range(2, 76) if y % 2 == 1]
    assert len(rows) == 37
    scene = _soup(hrt)
    on, c_on = _render(hrt, monkeypatch, scene, 1, tile=tile, h=h_frame)
    off, c_off = _render(hrt, monkeypatch, scene, 0, tile=tile, h=h_frame)
    ref = _oracle(oracle, scene, h=h_frame)
    assert (c_on["one"], c_on["blocks"], c_off["one"], c_off["blocks"]) == (1, 1, 0, 1)
    assert on[0]["counts"][3] == W * 37 * 5 and on[0]["counts"] == off[0]["counts"]
    for what in ("color", "linear"):
        assert np.array_equal(on[0][what].view(np.uint32), off[0][what].view(np.uint32))
        assert np.array_equal(on[0][what][rows].view(np.uint32), ref[0][what][rows].view(np.uint32))
    assert np.array_equal(on[0]["states"], off[0]["states"])
    assert np.array_equal(on[0]["states"].reshape(h_frame, W, 12)[rows], ref[0]["states"].reshape(h_frame, W, 12)[rows])


def test_the_gate(hrt, gpu_available, monkeypatch):
    """Two instances, and spheres, go to k_path_blocks; so does everything under HRT_ONE_GROUP=0; one instance of triangles raises the counter
    by one per launch; and the gate looks at the tree that is launched, launch by launch."""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    two = _soup(hrt)
    v = two["instances"][0]["vertices"]
    two["instances"] = [hrt.scenes._tri_instance(v[0::2], hrt.scenes.WHITE), hrt.scenes._tri_instance(v[1::2], hrt.scenes.RED, "metal", 0.1)]
    _, c = _render(hrt, monkeypatch, two, 1, launches=(5, 3))
    assert (c["one"], c["blocks"]) == (0, 2), c
    spheres = hrt.scenes.sphere_in_box(W, H, 5)
    spheres["instances"] = spheres["instances"][-1:]            # the sphere alone: one instance, but not of triangles
    _, c = _render(hrt, monkeypatch, spheres, 1)
    assert (c["one"], c["blocks"]) == (0, 1), c
    _, c = _render(hrt, monkeypatch, _soup(hrt), 0, launches=(5, 3))
    assert (c["one"], c["blocks"]) == (0, 2), c
    _, c = _render(hrt, monkeypatch, _soup(hrt), 1, launches=(5, 3, 4))
    assert (c["one"], c["blocks"]) == (3, 3), c
    # one context, the two-instance scene and a TLAS over its first instance alone: the kernel follows the tree
    monkeypatch.setenv("HRT_ONE_GROUP", "1")
    monkeypatch.setenv("HRT_FUSED_LPT", "0")
    monkeypatch.setenv("HRT_SAMPLE_BLOCK", "2")
    r = hrt.Renderer(0, 0)
    try:
        r.load_scene(two)
        both = r.tlas
        single = r.build_tlas(order=[0])
        r.set_frame(W, H, SALT, linear=True)
        seen = []
        for tlas in (single, both, single, single, both):
            r.use_tlas(tlas)
            r.render(5)
            s = r.stats()
            seen.append((int(s.one_group_launches), int(s.sample_block_launches)))
        assert seen == [(1, 1), (1, 2), (2, 3), (3, 4), (3, 5)], seen
    finally:
        r.close()
