"""HRT_SEED_PRIMARY=2 (DESIGN.md sections 2.1 and 4.1; trav_common.h: kSeedWindow, TravState::tlo): a pixel's repeat primary ray is bounded
from below as well -- the node step's interval begins a window of 2^-10 of the distance under the hit its previous sample found.  Nothing a
caller can see may change: every case renders at level 2 and at level 0 from the same RNG states and requires identical bits in `color`,
`linear` and the RNG end states and equal ray and path counts, and the oracle's bits.  A windowed ray that turned its hit into a miss, lost
a tie at equal t, or kept a window for another ray, pixel, frame or launch would show as a difference.

Every path kernel without the primary-hit cache got the window: the one-level kernels (k_fused, k_path_blocks, k_path_capture), their
sphere instantiations and the two-level (INSTANCED) ones; the last two cases run those."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SALT = 43


def _camera(center, target):
    return {"center": np.array(center, dtype=np.float32), "target": np.array(target, dtype=np.float32), "up": np.array([0, 1, 0], dtype=np.float32), "opengl": True}


def _take(r):
    import torch
    torch.cuda.synchronize()
    s = r.stats()
    return {"color": r.color.cpu().numpy().copy(), "linear": r.linear.cpu().numpy().copy(), "states": r.rng_states_numpy(),
            "counts": (int(s.rays), int(s.rays_closest), int(s.rays_any), int(s.paths))}


def _frames(hrt, monkeypatch, level, scene, w, h, spp, flags=0, cameras=(None,), tile=None):
    """One context at HRT_SEED_PRIMARY = level: a frame per camera (None: the scene's), each from fresh RNG states, one after the other."""
    monkeypatch.setenv("HRT_SEED_PRIMARY", level)
    r = hrt.Renderer(0, flags)
    out = []
    try:
        r.load_scene(scene)
        for cam in cameras:
            if cam is not None:
                r.set_camera(cam["center"], cam["target"], cam["up"], cam["opengl"])
            r.set_frame(w, h, SALT, linear=True)
            r.reset_stats()
            r.render(spp, tile=tile)
            out.append(_take(r))
    finally:
        r.close()
    return out


def _same(a, b):
    assert np.array_equal(a["color"].view(np.uint32), b["color"].view(np.uint32))
    assert np.array_equal(a["linear"].view(np.uint32), b["linear"].view(np.uint32))
    assert np.array_equal(a["states"], b["states"])
    assert a["counts"] == b["counts"]


def _oracle(oracle, scene, w, h, spp, got, instanced=False):
    states = oracle.rng_init(w, h, SALT)
    ref = oracle.OracleScene(scene, instanced=instanced).render(w, h, states, spp)
    assert np.array_equal(got["linear"].view(np.uint32), ref["linear"].view(np.uint32))
    assert np.array_equal(got["color"].view(np.uint32), ref["color"].view(np.uint32))
    assert np.array_equal(got["states"], states) and got["counts"][0] == ref["rays"] and got["counts"][3] == w * h * spp
    return ref


def _both_levels(hrt, oracle, monkeypatch, scene, w, h, spp, flags=0, instanced=False):
    window, off = (_frames(hrt, monkeypatch, level, scene, w, h, spp, flags)[0] for level in ("2", "0"))
    _same(window, off)
    _oracle(oracle, scene, w, h, spp, window, instanced)
    return window


def _soup(hrt, w=61, h=37, spp=8):
    return hrt.scenes.random_soup(3000, 0.12, 11, w, h, spp)


def _scaled(scene, s):
    """the scene and its camera times s (a power of two: every coordinate scales exactly)"""
    out = copy.deepcopy(scene)
    for inst in out["instances"]:
        inst["vertices"] = (inst["vertices"] * np.float32(s)).astype(np.float32)
    cam = out["camera"]
    cam["center"] = (cam["center"] * np.float32(s)).astype(np.float32); cam["target"] = (cam["target"] * np.float32(s)).astype(np.float32)
    return out


def test_cornell_ties_on_the_walls_diagonals(hrt, oracle, gpu_available, monkeypatch):
    """C1, 64 x 48 at 5 spp: primary rays on a wall's diagonal hit both of its triangles at equal t, and the lower id must still win when the
    interval is [t (1 - 2^-10), t]."""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    _both_levels(hrt, oracle, monkeypatch, hrt.scenes.cornell_box(64, 48, 5), 64, 48, 5)


@pytest.mark.parametrize("tree", ["default", "fast-trace"])
def test_a_soup_of_odd_size(hrt, oracle, gpu_available, monkeypatch, tree):
    """3000 triangles, 61 x 37 at 8 spp, on the default tree and with spatial splits (a primitive referenced from several leaves: the windowed
    walk may meet the known hit through any of those whose box holds it)."""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    got = _both_levels(hrt, oracle, monkeypatch, _soup(hrt), 61, 37, 8, flags=hrt.CTX_FAST_TRACE if tree == "fast-trace" else 0)
    assert 61 * 37 * 8 < got["counts"][0] < 61 * 37 * 8 * 50          # (some primaries hit: there was something to seed)


@pytest.mark.parametrize("env", [{"HRT_SAMPLE_BLOCK": "2"}, {"HRT_SAMPLE_TAPER": "4:1!"}], ids=["blocks-of-2", "taper-4:1"])
def test_sample_blocks_end_a_lanes_hold_and_its_window(hrt, oracle, gpu_available, monkeypatch, env):
    """k_path_blocks: 2257 pixels are above the 8-wave floor, so the forced schedules run; a block's first primary ray has no seed, the
    others have a window."""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _both_levels(hrt, oracle, monkeypatch, _soup(hrt), 61, 37, 8)


def test_a_frame_of_background(hrt, oracle, gpu_available, monkeypatch):
    """The camera looks away: every seed says "none", no ray ever has a window."""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    scene = _soup(hrt, 32, 16, 4)
    scene["camera"] = _camera([0, 0, 3.5], [0, 0, 9.0])
    got = _both_levels(hrt, oracle, monkeypatch, scene, 32, 16, 4)
    assert got["counts"] == (32 * 16 * 4, 32 * 16 * 4, 0, 32 * 16 * 4)


def test_a_miss_then_hits_when_the_camera_turns_between_launches(hrt, oracle, gpu_available, monkeypatch):
    """One context: frame A looks away from a distant soup (all background), frame B at it (mostly background, hits in the middle).  B is what
    a fresh context and level 0 make of it: no seed and no window outlive a launch."""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    w, h, spp = 48, 32, 6
    scene = _soup(hrt, w, h, spp)
    away, at = _camera([0, 0, 12.0], [0, 0, 30.0]), _camera([0, 0, 12.0], [0, 0, 0])
    a_then_b = _frames(hrt, monkeypatch, "2", scene, w, h, spp, cameras=(away, at))
    fresh_b = _frames(hrt, monkeypatch, "2", scene, w, h, spp, cameras=(at,))[0]
    off_b = _frames(hrt, monkeypatch, "0", scene, w, h, spp, cameras=(at,))[0]
    assert a_then_b[0]["counts"][0] == w * h * spp and w * h * spp < a_then_b[1]["counts"][0] < 3 * w * h * spp      # all / mostly background
    _same(a_then_b[1], fresh_b)
    _same(a_then_b[1], off_b)
    scene["camera"] = at
    _oracle(oracle, scene, w, h, spp, fresh_b)


@pytest.mark.parametrize("case", ["continued-sum", "tile"])
def test_launches_that_continue_a_sum_and_tiles(hrt, oracle, gpu_available, monkeypatch, case):
    """HRT_FUSED_MAX_SPP=2 at 6 spp (three launches: each starts without seeds); a tile of every third row."""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    w, h, spp = 48, 32, 6
    scene = hrt.scenes.cornell_box(w, h, spp)
    if case == "continued-sum":
        monkeypatch.setenv("HRT_FUSED_MAX_SPP", "2")
        _both_levels(hrt, oracle, monkeypatch, scene, w, h, spp)
    else:
        tile = hrt.Tile(0, h, 1, 3, 1)
        window, off = (_frames(hrt, monkeypatch, level, scene, w, h, spp, tile=tile)[0] for level in ("2", "0"))
        _same(window, off)
        assert window["counts"][3] < w * h * spp


@pytest.mark.parametrize("extents", [1, 12])
def test_a_camera_one_and_twelve_extents_away(hrt, oracle, gpu_available, monkeypatch, extents):
    """The soup's extent is 2: the camera 2 and 24 units in front of its nearest face.  Far away the offsets (p - o) k are large against the
    window: the rounding the error budget of section 4.1 is about."""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    scene = _soup(hrt, 48, 32, 6)
    scene["camera"] = _camera([0.1, 0.05, 1.0 + 2.0 * extents], [0, 0, 0])
    _both_levels(hrt, oracle, monkeypatch, scene, 48, 32, 6)


@pytest.mark.parametrize("log2_scale", [-20, 20])
def test_scenes_scaled_by_powers_of_two(hrt, oracle, gpu_available, monkeypatch, log2_scale):
    if not gpu_available:
        pytest.skip("no GPU in this container")
    scene = _scaled(_soup(hrt, 48, 32, 6), 2.0 ** log2_scale)
    _both_levels(hrt, oracle, monkeypatch, scene, 48, 32, 6)


def test_a_primary_hit_at_a_tiny_t(hrt, oracle, gpu_available, monkeypatch):
    """The camera 2^-16 in front of the Cornell box's back wall: t is about 1.5e-5 against tmin = 1e-6, the window's width about 1.5e-8 and
    k = 1 / (t 2^-10) about 2^26, inside the floor's 2^36."""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    scene = hrt.scenes.cornell_box(48, 32, 6)
    scene["camera"] = _camera([0.5, 0.5, 1.0 - 2.0 ** -16], [0.5, 0.5, 2.0])
    got = _both_levels(hrt, oracle, monkeypatch, scene, 48, 32, 6)
    assert got["counts"][0] > 48 * 32 * 6          # the primaries hit the wall and bounce


def test_all_four_programs_on_the_sphere_kernel(hrt, oracle, gpu_available, monkeypatch):
    """scenes.mixed_test_scene, 64 x 48 at 6 spp: rough and metal triangles and spheres, non-identity transforms.  The sphere instantiations have
    the window too."""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    scene = hrt.scenes.mixed_test_scene(2000, 40, 7, 64, 48, 6)
    window = _both_levels(hrt, oracle, monkeypatch, scene, 64, 48, 6)
    _same(window, _frames(hrt, monkeypatch, "1", scene, 64, 48, 6)[0])


def test_two_level_tree(hrt, oracle, gpu_available, monkeypatch):
    """12 particles through transform nodes over shared BLASes (the INSTANCED instantiation: bt and tlo are the world ray's while the lane is
    inside an instance -- the parameter is shared), 64 x 48 at 4 spp.  It has the window too."""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    scene = hrt.scenes.particle_scene(12, 64, 48, 4, frame=2)
    window = _both_levels(hrt, oracle, monkeypatch, scene, 64, 48, 4, flags=hrt.CTX_TWO_LEVEL, instanced=True)
    _same(window, _frames(hrt, monkeypatch, "1", scene, 64, 48, 4, flags=hrt.CTX_TWO_LEVEL)[0])
