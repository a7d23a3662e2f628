"""The seed travels with the pixel (path_lane.h: handover_store, handover_load, path_take): in a render by sample
blocks the lane that ends a block leaves the hit distance its pixel's last primary ray found in the free word next to the sum, and the
lane that takes the pixel's next block starts its first primary ray bounded there instead of walking the whole tree.  Nothing a caller
can see may change: every case renders under forced blocks at HRT_SEED_PRIMARY 2, 1 and 0 from the same RNG states and requires
identical bits in `color`, `linear` and the RNG end states, equal ray and path counts, and the oracle's bits.  A carried seed that
turned a hit into a miss, lost a tie, or was believed by pass 0 of a later launch (another camera's, another frame's) shows as a
difference.

Every render runs under a time limit of its own: a wave that waited for ever for a hand-over ends the process with a traceback."""
import faulthandler

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SALT = 43
RENDER_LIMIT_S = 60
SCHEDULES = {"blocks-of-2": {"HRT_SAMPLE_BLOCK": "2"}, "taper-4:1": {"HRT_SAMPLE_TAPER": "4:1!"}}


def _camera(center, target):
    return {"center": np.array(center, dtype=np.float32), "target": np.array(target, dtype=np.float32), "up": np.array([0, 1, 0], dtype=np.float32), "opengl": True}


def _take(r):
    import torch
    torch.cuda.synchronize()
    s = r.stats()
    return {"color": r.color.cpu().numpy().copy(), "linear": r.linear.cpu().numpy().copy(), "states": r.rng_states_numpy(),
            "counts": (int(s.rays), int(s.rays_closest), int(s.rays_any), int(s.paths)),
            "block_launches": int(s.sample_block_launches)}


def _frames(hrt, monkeypatch, level, scene, w, h, spp, flags=0, cameras=(None,)):
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
            faulthandler.dump_traceback_later(RENDER_LIMIT_S, exit=True)      # the render's time limit: a hang ends the run here
            try:
                r.render(spp)
                out.append(_take(r))
            finally:
                faulthandler.cancel_dump_traceback_later()
    finally:
        r.close()
    return out


def _same(a, b):
    assert np.array_equal(a["color"].view(np.uint32), b["color"].view(np.uint32))
    assert np.array_equal(a["linear"].view(np.uint32), b["linear"].view(np.uint32))
    assert np.array_equal(a["states"], b["states"])
    assert a["counts"] == b["counts"]


_ORACLE = {}


def _oracle(oracle, key, scene, w, h, spp, got):
    """the oracle's frame of `scene`, computed once per key and left unchanged"""
    if key not in _ORACLE:
        states = oracle.rng_init(w, h, SALT)
        ref = oracle.OracleScene(scene).render(w, h, states, spp)
        _ORACLE[key] = (ref["linear"].copy(), ref["color"].copy(), states.copy(), int(ref["rays"]))
    linear, color, states, rays = _ORACLE[key]
    assert np.array_equal(got["linear"].view(np.uint32), linear.view(np.uint32))
    assert np.array_equal(got["color"].view(np.uint32), color.view(np.uint32))
    assert np.array_equal(got["states"], states) and got["counts"][0] == rays and got["counts"][3] == w * h * spp


def _all_levels(hrt, oracle, monkeypatch, key, scene, w, h, spp, flags=0, block_launches=1):
    window, above, off = (_frames(hrt, monkeypatch, level, scene, w, h, spp, flags)[0] for level in ("2", "1", "0"))
    for got in (window, above, off):
        assert got["block_launches"] == block_launches      # (the forced schedule ran: k_path_blocks rendered this)
    _same(window, off)
    _same(above, off)
    _oracle(oracle, key, scene, w, h, spp, window)
    return window


def _soup(hrt, w=61, h=37, spp=8):
    return hrt.scenes.random_soup(3000, 0.12, 11, w, h, spp)


@pytest.mark.parametrize("tree", ["default", "fast-trace"])
@pytest.mark.parametrize("schedule", sorted(SCHEDULES))
def test_a_soup_of_odd_size_under_forced_blocks(hrt, oracle, gpu_available, monkeypatch, schedule, tree):
    """3000 triangles, 61 x 37 (2257 pixels: above the 8-wave floor) at 8 spp: blocks of 2 hand every pixel over three times, the taper 4:1
    on blocks of 4, 2, 1, 1; on the default tree and with spatial splits (the seeded walk may meet the known hit through any leaf that
    references it)."""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    for k, v in SCHEDULES[schedule].items():
        monkeypatch.setenv(k, v)
    got = _all_levels(hrt, oracle, monkeypatch, "soup", _soup(hrt), 61, 37, 8, flags=hrt.CTX_FAST_TRACE if tree == "fast-trace" else 0)
    assert 61 * 37 * 8 < got["counts"][0] < 61 * 37 * 8 * 50          # (some primaries hit: there was a seed to carry)


def test_a_frame_of_background_under_forced_blocks(hrt, oracle, gpu_available, monkeypatch):
    """The camera looks away (tests/test_primary_window_gpu.py: test_a_frame_of_background, the same frame and the same counts): every seed
    that travels says "none"."""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    monkeypatch.setenv("HRT_SAMPLE_BLOCK", "2")
    scene = _soup(hrt, 32, 16, 4)
    scene["camera"] = _camera([0, 0, 3.5], [0, 0, 9.0])
    got = _all_levels(hrt, oracle, monkeypatch, "background", scene, 32, 16, 4)
    assert got["counts"] == (32 * 16 * 4, 32 * 16 * 4, 0, 32 * 16 * 4)


@pytest.mark.parametrize("max_spp", [None, "4"], ids=["one-launch", "cut-at-4"])
def test_the_camera_turns_between_two_launches(hrt, oracle, gpu_available, monkeypatch, max_spp):
    """One context under forced blocks of 2: frame A looks at the soup from the front, frame B from the side, so the words A's hand-overs left
    next to the sums are hit distances of another camera.  B is what a fresh context and level 0 make of it -- pass 0 of a launch believes
    nothing it finds there.  With HRT_FUSED_MAX_SPP=4 each 8-spp frame is two launches, the second continuing the sum: its pass 0 reads the
    sum and still takes no seed."""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    monkeypatch.setenv("HRT_SAMPLE_BLOCK", "2")
    if max_spp:
        monkeypatch.setenv("HRT_FUSED_MAX_SPP", max_spp)
    launches = 2 if max_spp else 1
    w, h, spp = 61, 37, 8
    scene = _soup(hrt, w, h, spp)
    front, side = _camera([0, 0, 3.5], [0, 0, 0]), _camera([3.5, 0.4, 0.3], [0, 0, 0])
    a_then_b = _frames(hrt, monkeypatch, "2", scene, w, h, spp, cameras=(front, side))
    fresh_b = _frames(hrt, monkeypatch, "2", scene, w, h, spp, cameras=(side,))[0]
    off_b = _frames(hrt, monkeypatch, "0", scene, w, h, spp, cameras=(side,))[0]
    assert a_then_b[1]["block_launches"] == 2 * launches and fresh_b["block_launches"] == launches
    assert a_then_b[0]["counts"][0] > w * h * spp and a_then_b[1]["counts"][0] > w * h * spp          # both frames have hits: seeds were left, and wanted
    assert not np.array_equal(a_then_b[0]["linear"], a_then_b[1]["linear"])
    _same(a_then_b[1], fresh_b)
    _same(a_then_b[1], off_b)
    scene["camera"] = side
    _oracle(oracle, "soup-side", scene, w, h, spp, fresh_b)


def test_cornell_ties_on_the_walls_diagonals_under_forced_blocks(hrt, oracle, gpu_available, monkeypatch):
    """C1, 32 x 32 at 4 spp in blocks of 2: primary rays on a wall's diagonal hit both of its triangles at equal t, and the lower id must
    still win when the bound came from another lane."""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    monkeypatch.setenv("HRT_SAMPLE_BLOCK", "2")
    _all_levels(hrt, oracle, monkeypatch, "cornell", hrt.scenes.cornell_box(32, 32, 4), 32, 32, 4)
