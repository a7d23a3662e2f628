"""HRT_MISS_BLOCK: in k_path_direct's regeneration a pixel's primary ray that walked the launch's whole interval from the root and left the
scene decides the pixel's further samples up to the end of the lane's sample block, or of the launch (path_lane.h: path_finish, kDirect;
DESIGN.md section 2.1).  The same ray misses again in every sample, draws no random number and adds the same background colour in the same
order, and each of those samples is counted as the closest-hit ray it stands for -- so nothing anyone can read may change.

Bar: every case renders a 61 x 37 frame (the neighbouring tests' size, the smallest that takes sample blocks on 8 waves) with HRT_MISS_BLOCK=1
and =0 on contexts of their own, and both are the CPU oracle's frame bit for bit: colour, linear radiance, the RNG states after the render,
and rays / rays_closest / rays_any (the oracle counts rays; the split and the paths are equal between the knobs and rays_any is checked
against closest + any == rays).  Every launch that has at least two blocks must have run k_path_direct (HrtStats.direct_launches); one
that has a single block -- 1 sample, or a block above the samples -- is no block render and runs k_fused, on which the knob must change
nothing either.  (A render's rays end at the shader's FLOAT_INFINITY_VALUE, 1e16, which no call sets and no float32 scene reaches without
overflowing the primitive test's own products: a hit cut off by tmax cannot be staged through a render, and has no case here.)  The oracle's frames depend on the scene and the samples only: one per (scene, spp), shared by the schedules."""
import copy
import ctypes as C

import numpy as np
import pytest

from test_one_group_gpu import H, SALT, W, _check, _oracle

pytestmark = pytest.mark.gpu

SPPS = (1, 2, 9, 64, 130)
# uniform blocks of 1, 4, 7 (divides none of the sample counts), 64 and 100 (above every count but 130: a launch of fewer samples than the block
# is no block render); a small forced taper whose last block the launch's end cuts short (9 = 8 + 1, 130 = 128 + 2); the default schedule,
# forced onto the small tile
SCHEDULES = {"block-1": (("HRT_SAMPLE_BLOCK", "1"),), "block-4": (("HRT_SAMPLE_BLOCK", "4"),), "block-7": (("HRT_SAMPLE_BLOCK", "7"),),
             "block-64": (("HRT_SAMPLE_BLOCK", "64"),), "block-100": (("HRT_SAMPLE_BLOCK", "100"),),
             "taper-8:2": (("HRT_SAMPLE_BLOCK", "auto"), ("HRT_SAMPLE_TAPER", "8:2!")), "taper-default": (("HRT_SAMPLE_BLOCK", "auto"), ("HRT_SAMPLE_TAPER", "64:8!"))}
SCENES = ("half-sky", "sparse", "all-sky", "no-sky")


def _scene(hrt, which):
    s = hrt.scenes
    if which == "sparse":       # (ii) 200 triangles, four fifths of the frame sky: most primary rays cross the root box, walk several nodes and still miss
        return s.random_soup(200, 0.2, 23, W, H, 1)
    scene = s.random_soup(2000, 0.12, 7, W, H, 1)
    if which == "half-sky":     # (i) the cube over about the middle half of the frame: sky and soup pixels share waves and 16-pixel slices
        scene["camera"]["center"] = np.array([0, 0, 4.6], dtype=np.float32)
    elif which == "all-sky":    # (iii) the camera turned away: every primary ray misses at the root
        scene["camera"]["target"] = np.array([0, 0, 7], dtype=np.float32)
    elif which == "no-sky":     # (iv) the soup and the camera inside a closed box, all one instance: no sky pixel at all
        box = np.asarray(s._box((-2.0, -2.0, -2.0), (2.0, 2.0, 4.0), skip_bottom=False), np.float32)
        scene["instances"] = [s._tri_instance(np.concatenate([scene["instances"][0]["vertices"], box]), s.WHITE)]
    return scene


_REF = {}


def _ref(hrt, oracle, which, launches):
    key = (which, tuple(launches))
    if key not in _REF:
        _REF[key] = _oracle(oracle, _scene(hrt, which), launches)
    return _REF[key]


def _passes(hrt, spp, env):
    """how many blocks the launch's schedule has (hrt_sample_schedule: the host's own)"""
    env = dict(env)
    if env["HRT_SAMPLE_BLOCK"] == "auto":
        big, small = (int(x) for x in env["HRT_SAMPLE_TAPER"].rstrip("!").split(":"))
    else:
        big, small = int(env["HRT_SAMPLE_BLOCK"]), 0
    first = (C.c_uint32 * (spp + 1))()
    n = C.c_uint32(0)
    assert hrt.load_library().hrt_sample_schedule(spp, big, small, first, spp + 1, C.byref(n)) == 0
    return n.value


def _render(hrt, monkeypatch, scene, knob, launches, env):
    env = (("HRT_MISS_BLOCK", str(knob)), ("HRT_FUSED_LPT", "0")) + tuple(env)
    for k, v in env:
        monkeypatch.setenv(k, v)
    r = hrt.Renderer(0, 0)
    try:
        r.load_scene(scene)
        r.set_frame(W, H, SALT, linear=True)
        r.reset_stats()
        out = []
        for spp in launches:
            r.render(spp)
            s = r.stats()
            out.append({"linear": r.linear.cpu().numpy().copy(), "color": r.color.cpu().numpy().copy(), "states": r.rng_states_numpy(),
                        "counts": (int(s.rays), int(s.rays_closest), int(s.rays_any), int(s.paths))})
        s = r.stats()
        return out, {"direct": int(s.direct_launches), "blocks": int(s.sample_block_launches), "fallback": int(s.fused_fallback_launches)}
    finally:
        r.close()
        for k, _ in env:
            monkeypatch.delenv(k)


def _both(hrt, oracle, monkeypatch, which, launches, env, direct):
    scene = _scene(hrt, which)
    on, c_on = _render(hrt, monkeypatch, copy.deepcopy(scene), 1, launches, env)
    off, c_off = _render(hrt, monkeypatch, copy.deepcopy(scene), 0, launches, env)
    assert c_on == c_off == {"direct": direct, "blocks": direct, "fallback": 0}, (which, launches, env, c_on, c_off)
    ref = _ref(hrt, oracle, which, launches)
    _check(on, off, ref)
    done = 0
    for frame, spp in zip(on, launches):
        done += spp
        assert frame["counts"][3] == W * H * done
    return on, ref


@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("which", SCENES)
def test_scenes_samples_and_schedules(hrt, oracle, gpu_available, monkeypatch, which, schedule):
    """the four scenes at 1, 2, 9, 64 and 130 samples under every schedule"""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    env = SCHEDULES[schedule]
    ran_direct = 0
    for spp in SPPS:
        direct = 1 if _passes(hrt, spp, env) >= 2 else 0
        on, ref = _both(hrt, oracle, monkeypatch, which, (spp,), env, direct)
        ran_direct += direct
        if which == "all-sky":
            assert on[0]["counts"][:3] == (W * H * spp, W * H * spp, 0)     # one ray per sample, walked or not: the primary ray, which misses
    assert ran_direct >= 1, (schedule, ran_direct)


def test_the_scenes_are_what_they_claim(hrt, oracle, gpu_available):
    """half-sky: between a third and two thirds of the pixels are sky, and sky and soup meet inside 16-pixel slices; sparse: most are sky although
    the root box fills much of the frame; all-sky and no-sky: all and none (the oracle's one-sample frames: a sky pixel is the background)"""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    share, mixed = {}, {}
    for which in SCENES:
        scene = _scene(hrt, which)
        lin = _ref(hrt, oracle, which, (1,))[0]["linear"].reshape(-1, 4)[:, :3]
        sky = (lin == np.asarray(scene["background"], np.float32)[:3]).all(axis=1)
        share[which] = float(sky.mean())
        sl = sky[:sky.size // 16 * 16].reshape(-1, 16)
        mixed[which] = int((sl.any(axis=1) & ~sl.all(axis=1)).sum())
    assert 1 / 3 < share["half-sky"] < 2 / 3 and mixed["half-sky"] >= 30, (share, mixed)
    assert share["sparse"] > 0.5 and mixed["sparse"] >= 30, (share, mixed)
    assert share["all-sky"] == 1.0 and share["no-sky"] == 0.0, share


def test_a_render_cut_into_launches_continues_its_sums(hrt, oracle, gpu_available, monkeypatch):
    """HRT_FUSED_MAX_SPP=9 at 18 samples: two launches of 9 samples in blocks of 4, 4 and 1 into the same sums -- the second starts with px_first
    false, so a sky pixel's first addend of that launch is an addition, not an assignment -- and then a second render on the same context and
    RNG streams.  (hrt_render_accumulate, the other way to continue a sum, runs k_path_counts: no launch of k_path_direct to look at.)"""
    if not gpu_available:
        pytest.skip("no GPU in this container")
    for which in ("half-sky", "all-sky"):
        _both(hrt, oracle, monkeypatch, which, (18, 9), (("HRT_SAMPLE_BLOCK", "4"), ("HRT_FUSED_MAX_SPP", "9")), direct=3)
