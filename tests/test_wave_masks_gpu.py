"""The path kernels keep `alive`, `waiting` and `any` of their lanes as wave masks (trav_loop.h: LaneFlags), decide who runs the
bookkeeping, who has finished and when the loop ends with scalar mask arithmetic, and carry the masks of the lanes that want a
primitive / a node round the loop from the bookkeeping sequence.  A wrong bit shows as a ray that is never shaded, shaded twice, or
traversed with another lane's work -- so every case here is compared with the CPU oracle (renders: linear radiance bit for bit, ray
counts equal) or with brute force (hrt_trace_rays: the record bit for bit, hit / no hit for any-hit queries), on the smallest shapes at
which a flag can go wrong.  Nothing carries a tolerance."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SALT = 173
_REF = {}


def _gpu(hrt, gpu_available, monkeypatch, scene, w, h, spp, flags=0, env=()):
    """One render on a context of its own, the knobs of `env` set while it is made -> linear buffer and counters"""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    for k, v in env:
        monkeypatch.setenv(k, v)
    r = hrt.Renderer(0, flags)
    try:
        r.load_scene(scene)
        r.set_frame(w, h, SALT, linear=True)
        r.reset_stats()
        r.render(spp)
        s = r.stats()
        return {"linear": r.linear.cpu().numpy().copy(), "rays": int(s.rays), "rays_closest": int(s.rays_closest), "paths": int(s.paths),
                "block_launches": int(s.sample_block_launches), "fallback": int(s.fused_fallback_launches)}
    finally:
        r.close()
        for k, _ in env:
            monkeypatch.delenv(k)


def _oracle(oracle, key, scene, w, h, spp, instanced=False):
    """The oracle's render of a case, made once and never written to"""
    if key not in _REF:
        ref = oracle.OracleScene(scene, instanced=instanced).render(w, h, oracle.rng_init(w, h, SALT), spp)
        ref["linear"].setflags(write=False)
        _REF[key] = (scene, ref)
    return _REF[key]


def _is_the_oracles(got, ref):
    assert np.array_equal(got["linear"].view(np.uint32), ref["linear"].view(np.uint32)), "linear radiance must be bit-exact"
    assert got["rays"] == ref["rays"] and got["fallback"] == 0


@pytest.mark.parametrize("w,h", [(7, 5), (67, 3)])
def test_frames_that_do_not_fill_their_waves(hrt, oracle, gpu_available, monkeypatch, w, h):
    """35 pixels: 29 lanes of the only wave never own a pixel.  201 pixels: the last wave has 9."""
    spp = 5
    scene, ref = _oracle(oracle, ("cornell", w, h), hrt.scenes.cornell_box(w, h, spp), w, h, spp)
    got = _gpu(hrt, gpu_available, monkeypatch, scene, w, h, spp)
    _is_the_oracles(got, ref)
    assert got["paths"] == w * h * spp


def test_a_scene_every_ray_misses(hrt, oracle, gpu_available, monkeypatch):
    """The camera looks away from the box: every lane's ray finishes in the iteration it started in, all 64 at once."""
    w, h, spp = 40, 20, 3
    scene = hrt.scenes.cornell_box(w, h, spp)
    cam = dict(scene["camera"])
    cam["target"] = (2.0 * cam["center"] - cam["target"]).astype(np.float32)
    scene["camera"] = cam
    scene, ref = _oracle(oracle, "away", scene, w, h, spp)
    assert ref["rays"] == w * h * spp                      # one ray per path: nothing was hit
    _is_the_oracles(_gpu(hrt, gpu_available, monkeypatch, scene, w, h, spp), ref)


def _closed_box(hrt, w, h, spp):
    """The unit box closed on all six sides, rough, the camera inside: no path leaves, every path ends at the depth limit"""
    sc = hrt.scenes
    walls = sc._tri_instance(sc._box((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), skip_bottom=False), sc.WHITE)
    block = sc._tri_instance(sc._box((0.3, 0.0, 0.5), (0.6, 0.4, 0.8)), sc.RED)
    cam = {"center": np.array([0.5, 0.5, 0.1], dtype=np.float32), "target": np.array([0.5, 0.45, 0.9], dtype=np.float32),
           "up": np.array([0, 1, 0], dtype=np.float32), "opengl": True}
    return {"name": "closed-box", "instances": [walls, block], "camera": cam, "background": sc.BACKGROUND.copy(), "width": w, "height": h, "spp": spp}


def test_closed_box_where_paths_reach_the_depth_limit(hrt, oracle, gpu_available, monkeypatch):
    """Every path's last ray is an any-hit query (a hit at the depth limit is black whatever it is), and it always hits: lanes that finish
    by an any-hit and lanes that finish with nothing left to do leave the loop in the same iterations."""
    w, h, spp = 64, 48, 2
    scene, ref = _oracle(oracle, "closed", _closed_box(hrt, w, h, spp), w, h, spp)
    got = _gpu(hrt, gpu_available, monkeypatch, scene, w, h, spp)
    _is_the_oracles(got, ref)
    assert got["paths"] == w * h * spp and got["rays"] - got["rays_closest"] > 0.99 * got["paths"]        # an any-hit ray ends (nearly) every path


@pytest.mark.parametrize("threshold", [1, 64])
def test_the_two_ends_of_the_exit_compare(hrt, oracle, gpu_available, monkeypatch, threshold):
    """HRT_REFILL_THRESHOLD = 1: the loop ends as soon as one lane is idle (at most 63 alive).  64: only when none is alive."""
    w, h, spp = 48, 32, 4
    scene, ref = _oracle(oracle, ("cornell", w, h), hrt.scenes.cornell_box(w, h, spp), w, h, spp)
    _is_the_oracles(_gpu(hrt, gpu_available, monkeypatch, scene, w, h, spp, env=(("HRT_REFILL_THRESHOLD", str(threshold)),)), ref)


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("regen", [1, 16])
def test_the_drained_copy_of_the_loop(hrt, oracle, gpu_available, monkeypatch, split, regen):
    """300 pixels are five waves whose pixels are handed out at once: from then on every wave is in the copy of the loop with the drained
    phase's exit rule, with and without tail splitting, regenerating for every finished ray and for sixteen."""
    w, h, spp = 20, 15, 8
    scene, ref = _oracle(oracle, ("cornell", w, h), hrt.scenes.cornell_box(w, h, spp), w, h, spp)
    env = (("HRT_TAIL_SPLIT", str(split)), ("HRT_TAIL_REGEN", str(regen)))
    _is_the_oracles(_gpu(hrt, gpu_available, monkeypatch, scene, w, h, spp, env=env), ref)


def test_a_wave_that_holds_an_item_with_no_lane_alive(hrt, oracle, gpu_available, monkeypatch):
    """Sample blocks forced on 512 pixels (eight waves, one per slice counter) at 7 spp in blocks of 2, 2, 2, 1: a wave whose item waits
    for its predecessor passes through the loop with no lane alive."""
    w, h, spp = 32, 16, 7
    scene, ref = _oracle(oracle, ("cornell", w, h), hrt.scenes.cornell_box(w, h, spp), w, h, spp)
    got = _gpu(hrt, gpu_available, monkeypatch, scene, w, h, spp, env=(("HRT_SAMPLE_BLOCK", "2"),))
    _is_the_oracles(got, ref)
    assert got["block_launches"] == 1


@pytest.mark.parametrize("kernel", ["path-kernel", "k_trace_queue"])
@pytest.mark.parametrize("name", ["cornell", "mixed"])
def test_callers_rays_in_batches_round_a_wave(hrt, oracle, gpu_available, monkeypatch, kernel, name):
    """hrt_trace_rays, closest and any hit, on 1, 63, 64, 65 and 130 rays (triangles only, and the sphere instantiation) against brute force"""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    if ("rays", name) not in _REF:
        scene = hrt.scenes.cornell_box(8, 8, 1) if name == "cornell" else hrt.scenes.mixed_test_scene(600, 20, 7, 8, 8, 1)
        o, d = oracle.random_rays(130, 29)
        if name == "cornell":                             # (the box is the unit cube: start in front of its open side)
            o = (o * np.float32(0.2) + np.array([0.5, 0.5, -0.6], dtype=np.float32)).astype(np.float32)
            d = (d * np.float32(0.5) + np.array([0.0, 0.0, 1.0], dtype=np.float32)).astype(np.float32)
        want = oracle.OracleScene(scene, force_brute=True).trace(o, d)
        assert 0.2 < (want[3] != 0xFFFFFFFF).mean() < 1.0
        _REF["rays", name] = (scene, o, d, want)
    scene, o, d, want = _REF["rays", name]
    if kernel == "k_trace_queue":
        monkeypatch.setenv("HRT_FUSED", "0")
    r = hrt.Renderer(0, 0)
    try:
        r.load_scene(scene)
        for n in (1, 63, 64, 65, 130):
            got = r.trace_rays(o[:n], d[:n])
            for g, x in zip(got[:3], want[:3]):
                assert np.array_equal(g.view(np.uint32), x[:n].view(np.uint32)), n
            assert np.array_equal(got[3], want[3][:n]) and np.array_equal(got[4], want[4][:n]), n
            hit = r.trace_rays(o[:n], d[:n], any_hit=True)
            assert np.array_equal(hit[3] != 0xFFFFFFFF, want[3][:n] != 0xFFFFFFFF), n
    finally:
        r.close()


def test_a_two_level_cloud(hrt, oracle, gpu_available, monkeypatch):
    """40 instances of shared shapes under HRT_CTX_TWO_LEVEL: the work masks are made again after the lanes entered and left instances"""
    w, h, spp = 48, 32, 2
    scene, ref = _oracle(oracle, "cloud", hrt.scenes.particle_cloud(40, w, h, spp), w, h, spp, instanced=True)
    _is_the_oracles(_gpu(hrt, gpu_available, monkeypatch, scene, w, h, spp, flags=hrt.CTX_TWO_LEVEL), ref)
