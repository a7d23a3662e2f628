"""HRT_SEED_PRIMARY (DESIGN.md sections 2.1 and 4.1; path_lane.h: PathLane::px_seed): the reference's raygen has no pixel jitter, so every
sample's primary ray of a pixel is the same ray, and the path kernels start a pixel's repeat primary rays with the culling bound at the hit
distance the previous sample found.  Nothing a caller can see may change: every case here renders with the knob on and off from the same
RNG states and requires identical bits in `color`, `linear` and the RNG end states and equal ray and path counts -- and the oracle's bits
where the oracle is cheap.  A seeded ray that reported a miss, lost a tie at equal t, or carried a seed into another pixel, frame or launch
would show as a difference."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SALT = 41


def _camera(center, target):
    return {"center": np.array(center, dtype=np.float32), "target": np.array(target, dtype=np.float32), "up": np.array([0, 1, 0], dtype=np.float32), "opengl": True}


def _take(r):
    import torch
    torch.cuda.synchronize()
    s = r.stats()
    return {"color": r.color.cpu().numpy().copy(), "linear": r.linear.cpu().numpy().copy(), "states": r.rng_states_numpy(),
            "counts": (int(s.rays), int(s.rays_closest), int(s.rays_any), int(s.paths))}


def _frames(hrt, monkeypatch, seed, scene, w, h, spp, flags=0, cameras=(None,), tile=None):
    """One context with HRT_SEED_PRIMARY = seed: a frame per camera (None: the scene's), each from fresh RNG states and cleared buffers,
    one after the other; what each frame left."""
    monkeypatch.setenv("HRT_SEED_PRIMARY", seed)
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


def _on_off(hrt, oracle, monkeypatch, scene, w, h, spp, flags=0, instanced=False):
    on, off = (_frames(hrt, monkeypatch, seed, scene, w, h, spp, flags)[0] for seed in ("1", "0"))
    _same(on, off)
    _oracle(oracle, scene, w, h, spp, on, instanced)


@pytest.mark.parametrize("block", ["auto", "1", "2", "3"])
def test_cornell_ties_on_the_walls_diagonals(hrt, oracle, gpu_available, monkeypatch, block):
    """C1, 48 x 32 at 8 spp: every wall is two coplanar triangles that share a diagonal, so primary rays on the diagonal hit both at equal t
    and the lower primitive id must win under a seed of exactly that t.  Blocks of 1 (no sample is ever seeded), 2, and 3 (which does
    not divide 8) are passes of k_path_blocks whose boundaries end a lane's hold on its pixel; `auto` is one k_fused launch."""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    monkeypatch.setenv("HRT_SAMPLE_BLOCK", block)
    _on_off(hrt, oracle, monkeypatch, hrt.scenes.cornell_box(48, 32, 8), 48, 32, 8)


def test_all_four_programs_and_the_sphere_kernels(hrt, oracle, gpu_available, monkeypatch):
    """scenes.mixed_test_scene, 64 x 48 at 6 spp: rough and metal triangles and spheres, non-identity transforms, metal fuzz."""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    _on_off(hrt, oracle, monkeypatch, hrt.scenes.mixed_test_scene(2000, 40, 7, 64, 48, 6), 64, 48, 6)


def test_a_soup_with_spatial_splits(hrt, oracle, gpu_available, monkeypatch):
    """2000 triangles under HRT_CTX_FAST_TRACE, 64 x 48 at 5 spp: a primitive is referenced from several leaves, the seeded walk may meet
    the known hit through any of them."""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    _on_off(hrt, oracle, monkeypatch, hrt.scenes.random_soup(2000, 0.12, 3, 64, 48, 5), 64, 48, 5, flags=hrt.CTX_FAST_TRACE)


@pytest.mark.parametrize("case", ["empty", "all-miss"])
def test_nothing_to_seed(hrt, oracle, gpu_available, monkeypatch, case):
    """16 x 8 at 4 spp, no instances / a camera that looks away from the box: the seed is "none" throughout."""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    if case == "empty":
        scene = {"instances": [], "camera": hrt.scenes._soup_camera(), "background": hrt.scenes.BACKGROUND}
    else:
        scene = hrt.scenes.cornell_box(16, 8, 4)
        scene["camera"] = _camera([0.5, 0.5, -1.5], [0.5, 0.5, -4.0])
    _on_off(hrt, oracle, monkeypatch, scene, 16, 8, 4)
    assert _frames(hrt, monkeypatch, "1", scene, 16, 8, 4)[0]["counts"] == (16 * 8 * 4, 16 * 8 * 4, 0, 16 * 8 * 4)


@pytest.mark.parametrize("case", ["plain", "continued-sum", "tile"])
def test_no_seed_leaks_into_the_next_frame(hrt, gpu_available, monkeypatch, case):
    """One context renders frame A, then frame B from a camera that is nearer to the left of the box and farther from the right, so B's
    primary hits are nearer than A's in some pixels and farther in others: B equals what a fresh context makes of it, and what the knob
    off makes.  Also with launches that continue a sum (HRT_FUSED_MAX_SPP=2 at 6 spp: three launches per frame) and with a tile of
    every third row."""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    w, h, spp = 48, 32, 6
    if case == "continued-sum":
        monkeypatch.setenv("HRT_FUSED_MAX_SPP", "2")
    tile = hrt.Tile(0, h, 1, 3, 1) if case == "tile" else None
    scene = hrt.scenes.cornell_box(w, h, spp)
    cam_a = scene["camera"]
    cam_b = _camera([0.1, 0.6, -0.9], [0.75, 0.4, 1.0])
    a_then_b = _frames(hrt, monkeypatch, "1", scene, w, h, spp, cameras=(cam_a, cam_b), tile=tile)
    fresh_b = _frames(hrt, monkeypatch, "1", scene, w, h, spp, cameras=(cam_b,), tile=tile)[0]
    off_b = _frames(hrt, monkeypatch, "0", scene, w, h, spp, cameras=(cam_b,), tile=tile)[0]
    assert not np.array_equal(a_then_b[0]["linear"], a_then_b[1]["linear"])
    _same(a_then_b[1], fresh_b)
    _same(a_then_b[1], off_b)


def test_two_level_tree(hrt, oracle, gpu_available, monkeypatch):
    """12 particles through transform nodes over shared BLASes (k_fused's INSTANCED instantiation, where the bound is the world ray's
    while the lane is inside an instance), 64 x 48 at 4 spp."""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    _on_off(hrt, oracle, monkeypatch, hrt.scenes.particle_scene(12, 64, 48, 4, frame=2), 64, 48, 4, flags=hrt.CTX_TWO_LEVEL, instanced=True)
