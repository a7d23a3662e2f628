"""HRT_SAMPLE_TAPER: k_path_blocks hands a pixel out in blocks that start large and end small -- pass b is samples [first(b), first(b + 1))
of a slice's pixels (device_types.h: block_first, block_ends; path_plan.h: sample_schedule).  A pixel still adds its samples in sample
order from one RNG stream, whichever lanes take its blocks.

Bars, for every render: the same render with HRT_SAMPLE_BLOCK=0 (k_fused, a lane keeps its pixel) on a context of its own AND the oracle
-- colour and linear buffers and the final RNG states bit for bit, the ray counts equal.  The frames are 64 x 48 = 48 waves' worth of
slices, tiny against the machine: nearly every item of a later pass meets a predecessor that is still under way.  `8:2!` forces the
schedule on such a frame, as HRT_SAMPLE_BLOCK=N forces uniform blocks."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SALT = 23
W, H = 64, 48
_refs = {}


def _scene(hrt, name, w, h, spp):
    return {"cornell": lambda: hrt.scenes.cornell_box(w, h, spp),
            "spheres": lambda: hrt.scenes.sphere_in_box(w, h, spp),
            "mixed": lambda: hrt.scenes.mixed_test_scene(1500, 20, 5, w, h, spp)}[name]()


def _render(hrt, monkeypatch, scene, w, h, spp, taper, tiles=(None,), max_spp=None):
    """One frame (one render per tile) on a context of its own; taper None: HRT_SAMPLE_BLOCK=0"""
    monkeypatch.setenv("HRT_SAMPLE_BLOCK", "0" if taper is None else "auto")
    monkeypatch.setenv("HRT_SAMPLE_TAPER", "0" if taper is None else taper)
    monkeypatch.setenv("HRT_FUSED_LPT", "0")
    if max_spp is None:
        monkeypatch.delenv("HRT_FUSED_MAX_SPP", raising=False)
    else:
        monkeypatch.setenv("HRT_FUSED_MAX_SPP", str(max_spp))
    r = hrt.Renderer(0, 0)
    try:
        r.load_scene(scene)
        r.set_frame(w, h, SALT, linear=True)
        r.reset_stats()
        for tile in tiles:
            r.render(spp, tile=tile)
        s = r.stats()
        return {"linear": r.linear.cpu().numpy().copy(), "color": r.color.cpu().numpy().copy(), "states": r.rng_states_numpy(),
                "rays": int(s.rays), "rays_closest": int(s.rays_closest), "paths": int(s.paths), "launches": int(s.kernel_launches[hrt.K_PATHS]),
                "block_launches": int(s.sample_block_launches), "fallback": int(s.fused_fallback_launches),
                "schedule": [int(x) for x in s.sample_block_schedule]}
    finally:
        r.close()


def _references(hrt, oracle, monkeypatch, name, w, h, spp):
    """(scene, the render without blocks, the oracle's frame and final states): made once per scene and sample count"""
    key = (name, w, h, spp)
    if key not in _refs:
        scene = _scene(hrt, name, w, h, spp)
        off = _render(hrt, monkeypatch, scene, w, h, spp, None)
        assert off["block_launches"] == 0 and off["fallback"] == 0 and off["launches"] == 1 and off["paths"] == w * h * spp
        states = oracle.rng_init(w, h, SALT)
        ref = oracle.OracleScene(scene).render(w, h, states, spp)
        _refs[key] = (scene, off, {"linear": ref["linear"], "color": ref["color"], "states": states, "rays": int(ref["rays"])})
    return _refs[key]


def _same_bits(got, off, ref):
    for want in (off, ref):
        assert np.array_equal(got["color"].view(np.uint32), want["color"].view(np.uint32))
        assert np.array_equal(got["linear"].view(np.uint32), want["linear"].view(np.uint32))
        assert np.array_equal(got["states"], want["states"])
        assert got["rays"] == want["rays"]
    assert (got["rays_closest"], got["paths"], got["fallback"]) == (off["rays_closest"], off["paths"], 0)


def _sizes(hrt, spp, big, small):
    first = (C.c_uint32 * (spp + 1))()
    n = C.c_uint32(0)
    assert hrt.load_library().hrt_sample_schedule(spp, big, small, first, spp + 1, C.byref(n)) == 0
    return [first[i + 1] - first[i] for i in range(n.value)]


@pytest.mark.parametrize("spp,taper,sizes,schedule", [
    (16, "8:2!", [8, 4, 2, 2], [8, 2, 16, 4]),
    (13, "8:2!", [4, 2, 2, 2, 2, 1], [8, 2, 8, 6]),           # no multiple of any block: blocks of 2 behind the halvings and a last short one
    (7, "8:2!", [2, 2, 2, 1], [4, 2, 4, 4]),                  # fewer samples than the largest block, which comes down to 4
    (13, "64:4!", [4, 4, 4, 1], [8, 4, 8, 4]),                # K_big far above the samples: 8, whose window is 4, 4
    (16, "4:4!", [4, 4, 4, 4], [4, 4, 16, 4]),                # no halvings at all
    (7, "2:1!", [2, 2, 1, 1, 1], [2, 1, 6, 5]),               # ends on single samples
])
def test_cornell_in_tapered_blocks_is_the_same_bits(hrt, oracle, gpu_available, monkeypatch, spp, taper, sizes, schedule):
    if not gpu_available:
        pytest.skip("no GPU in this container")
    big, small = (int(x) for x in taper.rstrip("!").split(":"))
    assert _sizes(hrt, spp, big, small) == sizes
    scene, off, ref = _references(hrt, oracle, monkeypatch, "cornell", W, H, spp)
    got = _render(hrt, monkeypatch, scene, W, H, spp, taper)
    assert got["block_launches"] == 1 and got["launches"] == 1 and got["schedule"] == schedule
    _same_bits(got, off, ref)


def test_a_render_cut_into_two_launches_inside_a_block(hrt, oracle, gpu_available, monkeypatch):
    """HRT_FUSED_MAX_SPP=10 at 16 spp: the cut lies inside the block [8, 12) of the uncut schedule.  Each launch has its own: 10 samples as 4, 2, 2, 2
    and 6 that continue the sums as 2, 2, 2."""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    assert _sizes(hrt, 10, 8, 2) == [4, 2, 2, 2] and _sizes(hrt, 6, 8, 2) == [2, 2, 2]
    scene, off, ref = _references(hrt, oracle, monkeypatch, "cornell", W, H, 16)
    got = _render(hrt, monkeypatch, scene, W, H, 16, "8:2!", max_spp=10)
    assert got["launches"] == 2 and got["block_launches"] == 2 and got["schedule"] == [4, 2, 4, 3]
    _same_bits(got, off, ref)


def test_the_striped_tiles_of_two_ranks(hrt, oracle, gpu_available, monkeypatch):
    """Tiles with row lists: the stripes (4 rows) of rank 0 and of rank 1, 24 rows x 64 pixels = 24 waves each, one after the other"""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    scene, off, ref = _references(hrt, oracle, monkeypatch, "cornell", W, H, 13)
    got = _render(hrt, monkeypatch, scene, W, H, 13, "8:2!", tiles=[hrt.tile_for_rank(H, rank, 2, stripe_rows=4) for rank in range(2)])
    assert got["launches"] == 2 and got["block_launches"] == 2
    _same_bits(got, off, ref)


def test_a_frame_below_the_eight_wave_floor_runs_without_blocks(hrt, oracle, gpu_available, monkeypatch):
    """20 x 20 = 7 waves: a counter would be nobody's home (fused_body.h), so the forced taper hands out no blocks either -- and the stats say so"""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    scene, off, ref = _references(hrt, oracle, monkeypatch, "cornell", 20, 20, 7)
    got = _render(hrt, monkeypatch, scene, 20, 20, 7, "8:2!")
    assert got["block_launches"] == 0 and got["launches"] == 1 and got["schedule"] == [0, 0, 0, 0]
    _same_bits(got, off, ref)


def test_an_unforced_taper_leaves_a_small_frame_alone(hrt, oracle, gpu_available, monkeypatch):
    """without the `!` the gates of `auto` hold: fewer than 4 slices per slice in flight, fewer than 64 samples"""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    scene, off, ref = _references(hrt, oracle, monkeypatch, "cornell", W, H, 16)
    got = _render(hrt, monkeypatch, scene, W, H, 16, "8:2")
    assert got["block_launches"] == 0
    _same_bits(got, off, ref)


@pytest.mark.parametrize("name", ["spheres", "mixed"])
def test_sphere_scenes_in_tapered_blocks(hrt, oracle, gpu_available, monkeypatch, name):
    """k_path_blocks<1>: a sphere in a closed box, and all four programs in one scene"""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    scene, off, ref = _references(hrt, oracle, monkeypatch, name, W, H, 13)
    got = _render(hrt, monkeypatch, scene, W, H, 13, "8:2!")
    assert got["block_launches"] == 1 and got["schedule"] == [8, 2, 8, 6]
    _same_bits(got, off, ref)
