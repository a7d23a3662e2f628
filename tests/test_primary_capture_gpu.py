"""HRT_CTX_CAPTURE_PRIMARY on the MI355X (include/hrt.h; csrc/fused_capture.hip k_path_capture, csrc/hrt_denoise.cpp run_guides): the render
launch keeps every pixel's primary hit and the denoiser's guide pass takes it instead of tracing the frame's primary rays again.
Everything is compared bit for bit: the capture with hrt_trace_rays of the same rays, the guides with the specification over the
oracle, image / RNG states / ray counts and all three denoisers with a context without the flag; a stale capture is never used, and
the launches that do not capture say so."""
import numpy as np
import pytest

import denoise_ref as ref

pytestmark = pytest.mark.gpu
MISS = 0xFFFFFFFF
TMIN, TMAX = np.float32(1e-6), np.float32(1e16)      # FLOAT_ZERO_VALUE / FLOAT_INFINITY_VALUE: the interval of every ray the path kernel starts


@pytest.fixture(scope="module")
def hrt_gpu(hrt):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return hrt


def _scene(hrt, name, w, h):
    s = hrt.scenes
    return {"c1": lambda: s.cornell_box(w, h, 1), "sphere_in_box": lambda: s.sphere_in_box(w, h, 1),
            "mixed": lambda: s.mixed_test_scene(width=w, height=h, transforms=True),
            "particles": lambda: s.particle_scene(12, w, h, 1, frame=2)}[name]()


def _renderer(hrt, scene, flags, w, h, linear=False):
    r = hrt.Renderer(0, flags)
    r.load_scene(scene)
    r.set_frame(w, h, hrt.scenes.SEED_SALT, linear=linear)
    return r


def _pair(hrt, scene, flags, w, h, linear=False):
    """(a context with the flag, one without), same scene, frame and tree flags"""
    return _renderer(hrt, scene, flags | hrt.CTX_CAPTURE_PRIMARY, w, h, linear), _renderer(hrt, scene, flags, w, h, linear)


def _bits(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint32)


def _traced(r, w, h):
    """hrt_trace_rays of the frame's primary rays as the path kernel starts them: the reference's "zero" and "infinity", (1e-6, 1e16)"""
    center, U, V, Wv = r.cam
    dirs = ref.primary_directions(w, h, U, V, Wv)
    origins = np.broadcast_to(np.asarray(center, np.float32), dirs.shape).copy()
    return r.trace_rays(origins, dirs, tmin=float(TMIN), tmax=float(TMAX))


def _same_hits(got, want):
    """t, prim, inst of every record; u, v of the hits (a miss's are not defined)"""
    t, u, v, prim, inst = got
    wt, wu, wv, wprim, winst = want
    hit = wprim != MISS
    assert np.array_equal(t.view(np.uint32), wt.view(np.uint32)), np.argwhere(t.view(np.uint32) != wt.view(np.uint32))[:8]
    assert np.array_equal(prim, wprim) and np.array_equal(inst, winst)
    assert np.array_equal(u[hit].view(np.uint32), wu[hit].view(np.uint32)) and np.array_equal(v[hit].view(np.uint32), wv[hit].view(np.uint32))
    assert np.all(t[~hit] == TMAX) and np.all(inst[~hit] == MISS)


def _moved(transforms, angle, shift):
    """every instance rotated by `angle` radians about the z axis through the origin, then shifted by `shift`"""
    c, s = np.cos(angle), np.sin(angle)
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float64)
    out = []
    for m in transforms:
        m = np.asarray(m, np.float64).reshape(3, 4)
        out.append(np.concatenate([R @ m[:, :3], (R @ m[:, 3] + np.asarray(shift, np.float64))[:, None]], axis=1).astype(np.float32).reshape(12))
    return np.array(out, np.float32)


def _no_capture(hrt, r):
    with pytest.raises(hrt.HrtError, match="status -5"):
        r.primary_hits()


@pytest.mark.parametrize("mode", ["flattened", "two_level", "fast_trace"])
@pytest.mark.parametrize("name", ["c1", "sphere_in_box", "mixed"])
def test_the_capture_is_the_hit(hrt_gpu, oracle, name, mode):
    """render(1) with the flag: primary_hits() is hrt_trace_rays of the frame's primary rays in a context without it, denoise_guides()
    is the specification over the oracle's hits (its instanced mode for two-level trees), and that guide pass did not trace."""
    hrt = hrt_gpu
    w, h = 96, 64
    flags = {"flattened": 0, "two_level": hrt.CTX_TWO_LEVEL, "fast_trace": hrt.CTX_FAST_TRACE}[mode]
    scene = _scene(hrt, name, w, h)
    rc, rp = _pair(hrt, scene, flags, w, h)
    try:
        _no_capture(hrt, rc)                                       # nothing rendered yet
        rc.render(1)
        _same_hits(rc.primary_hits(), _traced(rp, w, h))
        rays = rc.stats().rays
        got = rc.denoise_guides().cpu().numpy().view(np.uint16)
        osc = oracle.OracleScene(scene, instanced=(mode == "two_level"))
        want = ref.primary_guides(osc, scene, rc.cam, w, h)
        osc.close()
        assert np.array_equal(got, want), np.argwhere((got != want).any(axis=-1))[:8]
        s = rc.stats()
        assert (s.primary_capture_launches, s.guide_passes_captured, s.guide_passes_traced) == (1, 1, 0)
        assert s.rays == rays                                      # a captured guide pass counts no rays
        _no_capture(hrt, rp)
        rp.render(1)
        _no_capture(hrt, rp)                                       # ... and a context without the flag never has a capture
        assert rp.stats().primary_capture_launches == 0
    finally:
        rc.close(); rp.close()


@pytest.mark.parametrize("name,flags_of", [("mixed", lambda hrt: 0), ("particles", lambda hrt: hrt.CTX_TWO_LEVEL)])
@pytest.mark.parametrize("size", [(61, 37), (8, 6), (1, 1)])
def test_the_render_is_untouched(hrt_gpu, name, flags_of, size):
    """Colour, linear radiance, RNG states and ray count of render(spp), spp 1, 3 and 5, are the same with and without the flag (all four
    capture kernels between the two scenes: triangles and spheres, one and two levels); the capture does not depend on spp."""
    hrt = hrt_gpu
    w, h = size
    scene = _scene(hrt, name, w, h)
    rc, rp = _pair(hrt, scene, flags_of(hrt), w, h, linear=True)
    try:
        first = None
        for spp in (1, 3, 5):
            for r in (rc, rp):
                r.set_frame(w, h, hrt.scenes.SEED_SALT, linear=True)
                r.reset_stats()
                r.render(spp)
            assert np.array_equal(_bits(rc.color), _bits(rp.color)), spp
            assert np.array_equal(_bits(rc.linear), _bits(rp.linear)), spp
            assert np.array_equal(rc.rng_states_numpy(), rp.rng_states_numpy()), spp
            sc, sp = rc.stats(), rp.stats()
            assert (sc.rays, sc.rays_closest, sc.rays_any, sc.paths) == (sp.rays, sp.rays_closest, sp.rays_any, sp.paths) and sc.rays > 0
            hits = rc.primary_hits()
            if first is None:
                first = hits
                _same_hits(hits, _traced(rp, w, h))
            else:
                _same_hits(hits, first)
        assert rc.stats().primary_capture_launches == 3 and rp.stats().primary_capture_launches == 0
    finally:
        rc.close(); rp.close()


@pytest.mark.parametrize("name,flags_of", [("mixed", lambda hrt: 0), ("particles", lambda hrt: hrt.CTX_TWO_LEVEL)])
def test_the_denoisers_are_untouched(hrt_gpu, name, flags_of):
    """denoise(), three frames of denoise_temporal() and three of denoise_variance(), the instances moved between frames: the same output
    with and without the flag, w * h rays fewer per call, every guide pass served from the capture."""
    hrt = hrt_gpu
    w, h = 96, 64
    scene = _scene(hrt, name, w, h)
    rc, rp = _pair(hrt, scene, flags_of(hrt), w, h)
    try:
        calls = 0
        xf = np.array([it["transform"] for it in scene["instances"]], np.float32)

        def frame(denoiser, move):
            nonlocal calls, xf
            if move:
                xf = _moved(xf, 0.03, (0.02, -0.01, 0.015))
            outs = []
            for r in (rc, rp):
                if move:
                    r.update_instances(xf)
                r.render(1)
                outs.append(_bits(getattr(r, denoiser)()))
            calls += 1
            assert np.array_equal(outs[0], outs[1]), (denoiser, calls, np.argwhere(outs[0] != outs[1])[:8])
            sc, sp = rc.stats(), rp.stats()
            assert sp.rays - sc.rays == calls * w * h and sc.paths == sp.paths
            assert (sc.guide_passes_captured, sc.guide_passes_traced) == (calls, 0) and (sp.guide_passes_captured, sp.guide_passes_traced) == (0, calls)

        frame("denoise", False)
        for k in range(3):
            frame("denoise_temporal", k > 0)
        assert (rc.denoise_temporal_state()[1].cpu().numpy() > 1).any()          # the sequence did reuse history
        for r in (rc, rp):
            r.denoise_temporal_reset()
        for k in range(3):
            frame("denoise_variance", True)
        for a, b in zip(rc.denoise_variance_state(), rp.denoise_variance_state()):
            assert np.array_equal(_bits(a), _bits(b))
    finally:
        rc.close(); rp.close()


@pytest.mark.parametrize("mode", ["flattened", "two_level"])
@pytest.mark.parametrize("what", ["tile", "camera", "update", "frame_size", "set_flags"])
def test_a_stale_capture_is_never_used(hrt_gpu, what, mode):
    """A complete capture, then something that makes it another frame's: the guides are those of a context without the flag, the pass
    traced, and primary_hits() has nothing to give.  After an update (a refit: the tree keeps its handle and generation) the guides
    show the new poses."""
    hrt = hrt_gpu
    w, h = 64, 48
    flags = hrt.CTX_TWO_LEVEL if mode == "two_level" else 0
    scene = _scene(hrt, "particles", w, h)
    rc, rp = _pair(hrt, scene, flags, w, h)
    try:
        rc.render(1)
        rc.primary_hits()
        before = rc.denoise_guides().cpu().numpy()
        assert rc.stats().guide_passes_captured == 1
        for r in (rc, rp):
            if what == "tile":
                r.render(1, tile=hrt.Tile(0, h // 2, 1, 1, 0))
            elif what == "camera":
                c = scene["camera"]
                pan = np.array([0.05, 0.03, 0.0], np.float32)
                r.set_camera(np.asarray(c["center"], np.float32) + pan, np.asarray(c["target"], np.float32) + pan, c["up"], c.get("opengl", True))
            elif what == "update":
                r.update_instances(_moved([it["transform"] for it in scene["instances"]], 0.2, (0.05, -0.02, 0.03)))
            elif what == "frame_size":
                r.set_frame(w // 2, h // 2, hrt.scenes.SEED_SALT)
            else:
                r.set_flags(flags | (hrt.CTX_CAPTURE_PRIMARY if r is rc else 0))
        if what != "camera":               # (the camera is the caller's: the library sees the new one with the guide pass below)
            _no_capture(hrt, rc)
        got, want = rc.denoise_guides().cpu().numpy(), rp.denoise_guides().cpu().numpy()
        assert np.array_equal(got, want)
        s = rc.stats()
        assert (s.guide_passes_captured, s.guide_passes_traced) == (1, 1)
        if what in ("camera", "update"):
            assert not np.array_equal(got, before)
        _no_capture(hrt, rc)
        # ... and the next full-frame render captures again
        rc.render(1); rp.render(1)
        assert np.array_equal(rc.denoise_guides().cpu().numpy(), rp.denoise_guides().cpu().numpy())
        assert rc.stats().guide_passes_captured == 2
        rw, rh = (w // 2, h // 2) if what == "frame_size" else (w, h)
        _same_hits(rc.primary_hits(), _traced(rp, rw, rh))
    finally:
        rc.close(); rp.close()


@pytest.mark.parametrize("case", ["wavefront", "round1_kernel", "counting", "reuse_primary", "sample_blocks"])
def test_launches_that_do_not_capture(hrt_gpu, monkeypatch, case):
    """With the flag set, a launch outside the plain path kernel renders the same bits as without it, captures nothing, and the denoise
    that follows traces its guides and gives the same frame."""
    hrt = hrt_gpu
    w, h = 96, 64
    env = {"wavefront": ("HRT_FUSED", "0"), "round1_kernel": ("HRT_FUSED_MAX_DEPTH", "0"), "sample_blocks": ("HRT_SAMPLE_BLOCK", "2")}.get(case)
    if env:
        monkeypatch.setenv(*env)
    flags = {"counting": hrt.CTX_COUNT, "reuse_primary": hrt.CTX_REUSE_PRIMARY}.get(case, 0)
    spp = {"reuse_primary": 4, "sample_blocks": 4}.get(case, 2)
    scene = _scene(hrt, "mixed", w, h)
    rc, rp = _pair(hrt, scene, flags, w, h, linear=True)
    try:
        rc.render(spp); rp.render(spp)
        assert np.array_equal(_bits(rc.color), _bits(rp.color)) and np.array_equal(_bits(rc.linear), _bits(rp.linear))
        assert np.array_equal(rc.rng_states_numpy(), rp.rng_states_numpy())
        _no_capture(hrt, rc)
        assert np.array_equal(_bits(rc.denoise()), _bits(rp.denoise()))
        sc, sp = rc.stats(), rp.stats()
        assert (sc.primary_capture_launches, sc.guide_passes_captured, sc.guide_passes_traced) == (0, 0, 1)
        assert sc.rays == sp.rays
        # the case is the one it says
        if case == "sample_blocks":
            assert sc.sample_block_launches == 1
        if case == "round1_kernel":
            assert sc.fused_fallback_launches > 0
        if case in ("wavefront", "counting"):
            assert sc.kernel_launches[hrt.K_PATHS] == 0
    finally:
        rc.close(); rp.close()


def test_of_a_cut_render_the_first_launch_captures(hrt_gpu, monkeypatch):
    """HRT_FUSED_MAX_SPP=2 at 5 spp: three launches, one capture -- the single launch's --, the image of a context without the flag."""
    hrt = hrt_gpu
    w, h = 61, 37
    scene = _scene(hrt, "mixed", w, h)
    whole = _renderer(hrt, scene, hrt.CTX_CAPTURE_PRIMARY, w, h, linear=True)
    monkeypatch.setenv("HRT_FUSED_MAX_SPP", "2")
    rc, rp = _pair(hrt, scene, 0, w, h, linear=True)
    try:
        for r in (whole, rc, rp):
            r.render(5)
        s = rc.stats()
        assert s.primary_capture_launches == 1 and s.kernel_launches[hrt.K_PATHS] == 3 and whole.stats().kernel_launches[hrt.K_PATHS] == 1
        _same_hits(rc.primary_hits(), whole.primary_hits())
        for r in (whole, rc):
            assert np.array_equal(_bits(r.color), _bits(rp.color)) and np.array_equal(_bits(r.linear), _bits(rp.linear))
        assert np.array_equal(rc.rng_states_numpy(), rp.rng_states_numpy())
    finally:
        whole.close(); rc.close(); rp.close()


@pytest.mark.parametrize("view", ["all_background", "all_hit"])
def test_frames_of_background_only_and_of_hits_only(hrt_gpu, view):
    """A camera that looks away from the Cornell box: every record is (tmax, ., ., miss) and every guide's depth +inf.  A camera
    with a narrow view of its inside: every pixel a hit.  Both equal hrt_trace_rays and the traced guides."""
    hrt = hrt_gpu
    w, h = 48, 32
    scene = _scene(hrt, "c1", w, h)
    rc, rp = _pair(hrt, scene, 0, w, h)
    try:
        c = scene["camera"]
        center, target = np.asarray(c["center"], np.float32), np.asarray(c["target"], np.float32)
        new_target = center - (target - center) if view == "all_background" else center + 8.0 * (target - center)
        for r in (rc, rp):
            r.set_camera(center, new_target, c["up"], c.get("opengl", True))
        rc.render(1)
        t, u, v, prim, inst = rc.primary_hits()
        _same_hits((t, u, v, prim, inst), _traced(rp, w, h))
        got = rc.denoise_guides().cpu().numpy()
        assert np.array_equal(got, rp.denoise_guides().cpu().numpy()) and rc.stats().guide_passes_captured == 1
        z = ref.unpack_guides(got.view(np.uint16))[2]
        if view == "all_background":
            assert np.all(t == TMAX) and np.all(prim == MISS) and np.all(inst == MISS) and np.all(np.isposinf(z))
        else:
            assert np.all(t < TMAX) and np.all(t > 0) and np.all(prim != MISS) and np.all(inst < len(scene["instances"])) and np.all(np.isfinite(z))
    finally:
        rc.close(); rp.close()
