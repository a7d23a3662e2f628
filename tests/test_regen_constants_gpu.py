"""The regeneration phase of the path kernels (k_fused, k_path_blocks) reads its constants -- camera, background, frame size, sample counts,
buffer addresses -- from the kernel-argument segment WHEN IT USES THEM, all through the kernel's run, not once at its start
(fused_body.h: kernarg_traverse_args).  That is right only while every launch keeps its own arguments for as long as it runs.  What
could go wrong: a kernel that picks up the arguments of a launch enqueued after it -- another context's, or the next launch of its own
context with other frame constants.  Both are provoked here, with sample blocks (k_path_blocks) and without (k_fused).

Bars: the same render done alone -- colour and linear buffers and the final RNG states bit for bit, ray counts equal -- and, at a few
samples per pixel, the oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SALT = 57
ROUNDS = 2


def _scene_a(hrt, spp):
    """64 x 48, the Cornell box: triangles only, its own camera, the usual background"""
    return hrt.scenes.cornell_box(64, 48, spp), 64, 48


def _scene_b(hrt, spp):
    """96 x 40, all four programs (the sphere instantiations of the kernels), the soup camera, a background of its own"""
    scene = hrt.scenes.mixed_test_scene(1500, 20, 5, 96, 40, spp)
    scene["background"] = np.array([0.25, 0.5, 0.95], dtype=np.float32)
    return scene, 96, 40


def _open(hrt, scene, w, h):
    r = hrt.Renderer(0, 0)
    r.load_scene(scene)
    r.set_frame(w, h, SALT, linear=True)
    r.reset_stats()
    return r


def _take(hrt, r):
    import torch
    torch.cuda.synchronize()
    s = r.stats()
    return {"color": r.color.cpu().numpy().copy(), "linear": r.linear.cpu().numpy().copy(), "states": r.rng_states_numpy(),
            "rays": int(s.rays), "paths": int(s.paths), "launches": int(s.kernel_launches[hrt.K_PATHS]),
            "block_launches": int(s.sample_block_launches), "fallback": int(s.fused_fallback_launches)}


def _same(a, b):
    assert np.array_equal(a["color"].view(np.uint32), b["color"].view(np.uint32))
    assert np.array_equal(a["linear"].view(np.uint32), b["linear"].view(np.uint32))
    assert np.array_equal(a["states"], b["states"])
    assert (a["rays"], a["paths"]) == (b["rays"], b["paths"])


@pytest.mark.parametrize("block,spp_a,spp_b,with_oracle", [(8, 24, 64, False), (0, 24, 64, False), (2, 3, 4, True)])
def test_two_contexts_with_their_launches_interleaved(hrt, oracle, gpu_available, monkeypatch, block, spp_a, spp_b, with_oracle):
    """Two contexts in one process with different scenes, frame sizes, cameras, backgrounds and sample counts; each renders ROUNDS frames
    (the second continues the RNG streams of the first), the launches enqueued alternately without waiting, each context on a stream
    of its own so that the kernels may run side by side.  Blocks of 8 at 24 / 64 spp and of 2 at 3 / 4 spp are passes of k_path_blocks
    (both frames have more than 448 pixels); 0: k_fused."""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    import torch
    monkeypatch.setenv("HRT_SAMPLE_BLOCK", str(block))
    frames = [_scene_a(hrt, spp_a) + (spp_a,), _scene_b(hrt, spp_b) + (spp_b,)]
    alone = []
    for scene, w, h, spp in frames:
        r = _open(hrt, scene, w, h)
        try:
            for _ in range(ROUNDS):
                r.render(spp)
            alone.append(_take(hrt, r))
        finally:
            r.close()
    both = [_open(hrt, scene, w, h) for scene, w, h, _ in frames]
    try:
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        torch.cuda.synchronize()                    # (the frames' buffers were cleared on the default stream)
        for _ in range(ROUNDS):
            for r, stream, (_, _, _, spp) in zip(both, streams, frames):
                with torch.cuda.stream(stream):
                    r.render(spp, sync=False)
        together = [_take(hrt, r) for r in both]
    finally:
        for r in both:
            r.close()
    for got, want, (scene, w, h, spp) in zip(together, alone, frames):
        assert got["paths"] == ROUNDS * w * h * spp and got["fallback"] == 0
        assert got["block_launches"] == want["block_launches"] == (ROUNDS if block else 0)
        _same(got, want)
        if with_oracle:
            states = oracle.rng_init(w, h, SALT)
            osc = oracle.OracleScene(scene)
            rays = 0
            for _ in range(ROUNDS):
                ref = osc.render(w, h, states, spp)
                rays += ref["rays"]
            assert np.array_equal(got["linear"].view(np.uint32), ref["linear"].view(np.uint32))
            assert np.array_equal(got["color"].view(np.uint32), ref["color"].view(np.uint32))
            assert np.array_equal(got["states"], states) and got["rays"] == rays


_single = {}


def _single_launch(hrt, monkeypatch, name):
    """The frame as ONE launch of k_fused (no blocks, no probe), rendered once for the cases below.  Every caller leaves here with
    HRT_SAMPLE_BLOCK=0 and HRT_FUSED_LPT=0 set, whether the render was made in this call or an earlier one, and sets what its case needs."""
    monkeypatch.setenv("HRT_SAMPLE_BLOCK", "0")
    monkeypatch.setenv("HRT_FUSED_LPT", "0")
    monkeypatch.delenv("HRT_FUSED_MAX_SPP", raising=False)
    if name not in _single:
        scene, w, h, spp = {"small": lambda: _scene_b(hrt, 24) + (24,), "probe": lambda: (hrt.scenes.cornell_box(256, 256, 16), 256, 256, 16)}[name]()
        r = _open(hrt, scene, w, h)
        try:
            r.render(spp)
            _single[name] = (scene, w, h, spp, _take(hrt, r))
        finally:
            r.close()
        assert _single[name][4]["launches"] == 1 and _single[name][4]["block_launches"] == 0
    return _single[name]


@pytest.mark.parametrize("block", [0, 4])
def test_a_render_cut_into_three_launches(hrt, gpu_available, monkeypatch, block):
    """HRT_FUSED_MAX_SPP=10 at 24 spp: launches of 10, 10 and 4 samples enqueued back to back, whose sample counts and continue_sum differ
    (with blocks of 4: 4, 4, 2 / 4, 4, 2 / one block)."""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    scene, w, h, spp, want = _single_launch(hrt, monkeypatch, "small")
    monkeypatch.setenv("HRT_SAMPLE_BLOCK", str(block))
    monkeypatch.setenv("HRT_FUSED_MAX_SPP", "10")
    r = _open(hrt, scene, w, h)
    try:
        r.render(spp, sync=False)
        got = _take(hrt, r)
    finally:
        r.close()
    assert got["launches"] == 3 and got["block_launches"] == (2 if block else 0)
    _same(got, want)


@pytest.mark.parametrize("block", [0, 8])
def test_the_tiles_of_a_frame_one_after_the_other(hrt, gpu_available, monkeypatch, block):
    """The frame as the striped tiles of two ranks, each with its rows table and pixel count, enqueued back to back on one context: 20 rows of
    96 pixels each (more than 448: blocks where forced)."""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    scene, w, h, spp, want = _single_launch(hrt, monkeypatch, "small")
    monkeypatch.setenv("HRT_SAMPLE_BLOCK", str(block))
    r = _open(hrt, scene, w, h)
    try:
        for rank in range(2):
            r.render(spp, tile=hrt.tile_for_rank(h, rank, 2, stripe_rows=4), sync=False)
        got = _take(hrt, r)
    finally:
        r.close()
    assert got["launches"] == 2 and got["block_launches"] == (2 if block else 0)
    _same(got, want)


def test_the_cost_probe_launch_and_the_ordered_launch_after_it(hrt, gpu_available, monkeypatch):
    """256 x 256 at 16 spp has 4096 slices and few pixels per lane: a probe launch of 2 samples (slice costs recorded) and then the other
    14 with the slices handed out in cost order and the sums continued."""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    scene, w, h, spp, want = _single_launch(hrt, monkeypatch, "probe")
    monkeypatch.setenv("HRT_FUSED_LPT", "2")
    r = _open(hrt, scene, w, h)
    try:
        r.render(spp, sync=False)
        got = _take(hrt, r)
    finally:
        r.close()
    assert got["launches"] == 2 and got["block_launches"] == 0
    _same(got, want)
