"""HRT_SAMPLE_BLOCK: k_fused hands pixels out in blocks of K samples, pass by pass -- item (b, q) is samples [b K, (b + 1) K) of slice
q's pixels --, and a pixel's running sum and RNG state travel through memory from the lane that ended block b - 1 to the lane that takes
block b (path_lane.h).  Every pixel still adds its samples in sample order from one RNG stream.

Bar: the same render with HRT_SAMPLE_BLOCK=0 on a second context -- colour and linear buffers and the final RNG states bit for bit, and
the ray and path counts equal.  The frames are tiny against the machine (a few hundred slices against thousands in flight), so nearly
every item of a later pass meets a predecessor that is still under way: the hand-over, the deferral and the waiting wave's exit rule are
all on the path of every test here."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SALT = 91


def _render(hrt, monkeypatch, scene, w, h, spp, block, flags=0, tile=None, env=()):
    """One render on a context of its own with HRT_SAMPLE_BLOCK=block (None: the default, auto) -> buffers, states, counts"""
    if block is None:
        monkeypatch.delenv("HRT_SAMPLE_BLOCK", raising=False)
    else:
        monkeypatch.setenv("HRT_SAMPLE_BLOCK", str(block))
    for k, v in env:
        monkeypatch.setenv(k, v)
    r = hrt.Renderer(0, flags)
    try:
        r.load_scene(scene)
        r.set_frame(w, h, SALT, linear=True)
        r.reset_stats()
        r.render(spp, tile=tile)
        s = r.stats()
        return {"linear": r.linear.cpu().numpy().copy(), "color": r.color.cpu().numpy().copy(), "states": r.rng_states_numpy(),
                "rays": int(s.rays), "rays_closest": int(s.rays_closest), "paths": int(s.paths),
                "block_launches": int(s.sample_block_launches), "fallback": int(s.fused_fallback_launches)}
    finally:
        r.close()
        for k, _ in env:
            monkeypatch.delenv(k)


def _same(a, b):
    assert np.array_equal(a["color"].view(np.uint32), b["color"].view(np.uint32))
    assert np.array_equal(a["linear"].view(np.uint32), b["linear"].view(np.uint32))
    assert np.array_equal(a["states"], b["states"])
    assert (a["rays"], a["rays_closest"], a["paths"]) == (b["rays"], b["rays_closest"], b["paths"])


CORNELL = (96, 64, 24)
_cornell_ref = {}


def _cornell(hrt, monkeypatch):
    """C1 at 96x64, 24 spp without blocks: rendered once for all the cases below"""
    w, h, spp = CORNELL
    if not _cornell_ref:
        _cornell_ref["scene"] = hrt.scenes.cornell_box(w, h, spp)
        _cornell_ref["off"] = _render(hrt, monkeypatch, _cornell_ref["scene"], w, h, spp, 0)
    return _cornell_ref["scene"], _cornell_ref["off"]


@pytest.mark.parametrize("k", [1, 4, 7, 24, 32])
def test_cornell_in_blocks_is_the_same_bits(hrt, oracle, gpu_available, monkeypatch, k):
    """K = 1: every sample changes hands; 7: a short last block; 24 and 32: one block, which is the launch without blocks."""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    w, h, spp = CORNELL
    scene, off = _cornell(hrt, monkeypatch)
    assert off["block_launches"] == 0 and off["fallback"] == 0 and off["paths"] == w * h * spp
    on = _render(hrt, monkeypatch, scene, w, h, spp, k)
    _same(on, off)
    assert on["block_launches"] == (1 if k < spp else 0) and on["fallback"] == 0
    if k == 1:
        ref = oracle.OracleScene(scene).render(w, h, oracle.rng_init(w, h, SALT), spp)
        assert np.array_equal(on["linear"].view(np.uint32), ref["linear"].view(np.uint32)) and on["rays"] == ref["rays"]


@pytest.mark.parametrize("name", ["sky", "spheres", "mixed"])
def test_background_spheres_and_all_programs_in_blocks(hrt, gpu_available, monkeypatch, name):
    """A frame that is mostly background (paths of one ray: blocks end fast and far apart), the sphere instantiation of the kernel in
    a closed box, and all four programs in one scene."""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    w, h, spp = 112, 72, 12
    scene = {"sky": lambda: hrt.scenes.mixed_test_scene(60, 3, 8, w, h, spp),
             "spheres": lambda: hrt.scenes.sphere_in_box(w, h, spp),
             "mixed": lambda: hrt.scenes.mixed_test_scene(3000, 40, 5, w, h, spp)}[name]()
    off = _render(hrt, monkeypatch, scene, w, h, spp, 0)
    on = _render(hrt, monkeypatch, scene, w, h, spp, 5)             # blocks of 5, 5, 2
    _same(on, off)
    assert on["block_launches"] == 1 and off["block_launches"] == 0


def test_striped_tile_whose_pixel_count_is_no_multiple_of_a_slice(hrt, gpu_available, monkeypatch):
    """A rank's stripes of a frame (a row list) of 101 x 21 = 2121 pixels: the last slice has 9."""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    w, h, spp = 101, 45, 9
    scene = hrt.scenes.mixed_test_scene(3000, 40, 11, w, h, spp)
    tile = hrt.Tile(2, 44, 3, 2, 1)
    off = _render(hrt, monkeypatch, scene, w, h, spp, 0, tile=tile)
    on = _render(hrt, monkeypatch, scene, w, h, spp, 2, tile=tile)
    assert off["paths"] == 2121 * spp and off["paths"] % 16 != 0
    _same(on, off)
    assert on["block_launches"] == 1


def test_blocks_inside_the_launches_of_a_long_render(hrt, gpu_available, monkeypatch):
    """HRT_FUSED_MAX_SPP=10 at 24 spp with K = 4: launches of 10, 10 and 4 samples that continue the sums, in blocks of 4, 4, 2 / 4, 4, 2 / 4
    (the last launch is one block: no blocks)."""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    w, h, spp = CORNELL
    scene, off = _cornell(hrt, monkeypatch)
    on = _render(hrt, monkeypatch, scene, w, h, spp, 4, env=(("HRT_FUSED_MAX_SPP", "10"),))
    _same(on, off)
    assert on["block_launches"] == 2


def test_primary_reuse_keeps_its_pixels_in_one_lane(hrt, gpu_available, monkeypatch):
    """With the primary-hit cache blocks are off whatever the knob says: one traversed primary ray per pixel and launch."""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    w, h, spp = CORNELL
    scene, off = _cornell(hrt, monkeypatch)
    reuse = _render(hrt, monkeypatch, scene, w, h, spp, 0, flags=hrt.CTX_REUSE_PRIMARY)
    forced = _render(hrt, monkeypatch, scene, w, h, spp, 4, flags=hrt.CTX_REUSE_PRIMARY)
    _same(forced, reuse)
    assert forced["block_launches"] == 0 and off["rays"] - forced["rays"] == w * h * (spp - 1)
    assert np.array_equal(forced["linear"].view(np.uint32), off["linear"].view(np.uint32))


def test_two_level_tree_with_the_knob_forced(hrt, gpu_available, monkeypatch):
    """The instanced kernel keeps a pixel in its lane: the forced knob changes nothing."""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    w, h, spp = 96, 64, 8
    cloud = hrt.scenes.particle_cloud(300, w, h, spp)
    off = _render(hrt, monkeypatch, cloud, w, h, spp, 0, flags=hrt.CTX_TWO_LEVEL)
    on = _render(hrt, monkeypatch, cloud, w, h, spp, 3, flags=hrt.CTX_TWO_LEVEL)
    _same(on, off)
    assert on["fallback"] == 0 and on["block_launches"] == 0 and off["block_launches"] == 0


def test_auto_keeps_blocks_off_on_a_small_frame(hrt, gpu_available, monkeypatch):
    """256 x 256 has fewer than four slices per slice in flight: an item's predecessor could still be running, so `auto` does not
    hand out blocks -- and does on nothing but the knob's say-so.  At 64 spp = 2 K and with the slice cost order, which would apply to a
    tile of this size and keep blocks off by its precedence, switched off: it is the slice gate that says no."""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    w, h, spp = 256, 256, 64
    scene = hrt.scenes.cornell_box(w, h, spp)
    no_lpt = (("HRT_FUSED_LPT", "0"),)
    auto = _render(hrt, monkeypatch, scene, w, h, spp, None, env=no_lpt)
    forced = _render(hrt, monkeypatch, scene, w, h, spp, 32, env=no_lpt)
    assert auto["block_launches"] == 0 and forced["block_launches"] == 1
    _same(forced, auto)
    ordered = _render(hrt, monkeypatch, scene, w, h, spp, 32)         # the cost order applies: it keeps precedence over the forced knob
    assert ordered["block_launches"] == 0
    _same(ordered, auto)


def test_auto_hands_out_blocks_on_a_large_frame(hrt, gpu_available, monkeypatch):
    """1024 x 1024 = 65536 slices, four per slice in flight on a machine of 256 CUs x 16 waves (more on a smaller one), at 64 spp = 2 K:
    both gates open and `auto` runs the launch in blocks -- the path production takes."""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    w, h, spp = 1024, 1024, 64
    scene = hrt.scenes.cornell_box(w, h, spp)
    off = _render(hrt, monkeypatch, scene, w, h, spp, 0)
    auto = _render(hrt, monkeypatch, scene, w, h, spp, None)
    assert auto["block_launches"] == 1 and off["block_launches"] == 0
    _same(auto, off)
    below = _render(hrt, monkeypatch, scene, w, h, 63, None)       # one sample short of two whole blocks
    assert below["block_launches"] == 0


@pytest.mark.parametrize("w,h,spp,k,waves", [(8, 6, 8, 2, 1), (20, 20, 24, 1, 7), (32, 16, 8, 2, 8)])
def test_no_blocks_on_a_grid_of_fewer_waves_than_slice_counters(hrt, gpu_available, monkeypatch, w, h, spp, k, waves):
    """A wave keeps an item that is not ready and leaves its home counter only once that is drained, so the hand-out is free of
    deadlock only where each of the 8 counters is some wave's home (fused_body.h).  Tiles of up to 448 pixels have fewer waves: there the
    forced knob hands out no blocks either.  512 pixels are 8 waves, one per counter: blocks."""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    assert (w * h + 63) // 64 == waves
    scene = hrt.scenes.cornell_box(w, h, spp)
    off = _render(hrt, monkeypatch, scene, w, h, spp, 0)
    on = _render(hrt, monkeypatch, scene, w, h, spp, k)
    assert on["block_launches"] == (1 if waves >= 8 else 0) and on["fallback"] == 0
    _same(on, off)
