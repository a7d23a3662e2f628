"""The denoiser's accumulated mode on the MI355X (include/hrt.h "Accumulated mode"; csrc/denoise_accum.hip k_denoise_accumulated, then
csrc/denoise.hip k_denoise_pass<.., true> and csrc/kernels.hip k_color_to_float4): everything bit for bit against the numpy specification
(tests/denoise_accumulated_ref.py), no tolerance -- the filter form on the named synthetic cases (tests/denoise_accumulated_cases.py;
tests/test_denoise_accumulated_cpu.py asserts that they reach the branches they are for), the existing entry points composed by hand, the
launch form over frames hrt_render_accumulate has sampled, and what the call must leave alone."""
import ctypes as C

import numpy as np
import pytest

import denoise_accumulated_cases as ac
import denoise_accumulated_ref as aref
import denoise_cases as dc
import denoise_ref as ref
import denoise_variance_cases as vc
import denoise_variance_ref as vref

pytestmark = pytest.mark.gpu
BLACK = np.array([0, 0, 0, 1], np.float32)


@pytest.fixture(scope="module")
def hrt_gpu(hrt):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    lib = hrt.load_library()
    for name in ("hrt_denoise_accumulated_filter", "hrt_denoise_accumulated_launch"):
        getattr(lib, name)                                       # (AttributeError, not a skip, where the library lacks the mode)
    return hrt


@pytest.fixture(scope="module")
def filter_renderer(hrt_gpu):
    """One context for every filter case: its frames grow and shrink with the cases' sizes."""
    r = hrt_gpu.Renderer(0, 0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def wanted():
    """name -> the specification's (out, linear, var_out), computed once for the tests that share a case"""
    cache = {}

    def get(name):
        if name not in cache:
            c = ac.case(name)
            cache[name] = (c, aref.denoise_accumulated(*c[:5]))
        return cache[name]
    return get


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    return t.cpu().numpy()


def _check(got, want, what):
    assert dc.same(got, want), (what, dc.first_difference(got, want))


def _check_rgba(got, want, what):
    assert dc.same_rgba(got, want), (what, dc.first_difference(got[..., :3], want[..., :3]))


def _run_case(r, name, wanted):
    (s, t, g, p, vp, linear_mode, var_mode), (want, want_linear, want_var) = wanted(name)
    ds, dt, dg = _dev(s), _dev(t.view(np.int32)), _dev(g.view(np.int16))
    out, linear, var = r.denoise_accumulated_filter(ds, dt, dg, p, vp, linear_out=None if linear_mode == "set" else False,
                                                    var_out=None if var_mode == "set" else False)
    _check_rgba(_host(out), want, name + " colour")
    if linear_mode == "set":
        _check_rgba(_host(linear), want_linear, name + " linear")
    else:
        assert linear is None
    if var_mode == "set":
        _check(_host(var), want_var, name + " variance")
    else:
        assert var is None
    # the inputs are the caller's: not a bit of them has changed
    assert np.array_equal(dc.bits(_host(ds)), dc.bits(s)) and np.array_equal(_host(dt).view(np.uint32), t)
    assert np.array_equal(_host(dg).view(np.uint16), g)


@pytest.mark.parametrize("name", ac.CASES)
def test_filter_form_bit_exact(filter_renderer, wanted, name):
    """hrt_denoise_accumulated_filter: encoded colour, filtered linear frame and filtered variance of every case -- 1x1 to 37x29, 1 to 5
    passes, every map of totals, history_min 1 to 65536, plain, HDR, subnormal and hostile sums, d_linear_out and d_var_out set and NULL."""
    _run_case(filter_renderer, name, wanted)


def test_one_context_grows_shrinks_and_changes_modes(hrt_gpu, wanted):
    """The sizes in grow-and-shrink order on one context, hrt_denoise_filter and hrt_denoise_filter_variance in between at sizes of their own:
    the frames, variance frames and guide buffer the three share are allocated by whichever call needs them first and again after every growth."""
    r = hrt_gpu.Renderer(0, 0)
    try:
        p = {"iterations": 3}
        others = ((False, (5, 3)), (True, (41, 31)), (False, (64, 48)), (True, (17, 5)), (False, (3, 2)), (True, (70, 50)), (False, (9, 9)))
        for name, (variance, (w, h)) in zip(ac.GROW_SHRINK, others):
            _run_case(r, name, wanted)
            what = f"{'variance' if variance else 'plain'} {w}x{h} after {name}"
            rng = np.random.default_rng(dc._seed(what))
            c, g = dc.plain_color(rng, h, w), dc.random_guides(rng, h, w)
            if variance:
                v = vc.plain_variance(rng, h, w)
                want, want_v = vref.filter_variance(c, g, v, p)
                out, vo = r.denoise_filter_variance(_dev(c), _dev(g.view(np.int16)), _dev(v), p)
                _check(_host(vo), want_v, what + " variance")
            else:
                want = ref.atrous(c, g, p)
                out = r.denoise_filter(_dev(c), _dev(g.view(np.int16)), p)
            _check_rgba(_host(out), want, what + " colour")
        _run_case(r, ac.GROW_SHRINK[0], wanted)
    finally:
        r.close()


def test_equals_the_existing_entry_points(hrt_gpu):
    """An all-hit frame whose every total has reached history_min: the call is hrt_denoise_filter_variance of (mean, guides, var) followed
    by hrt_color_to_float4, bit for bit -- mean and var worked out with torch from the downloaded inputs."""
    import torch
    hrt = hrt_gpu
    w, h = 37, 29
    s, t, g = ac.full_frame(w, h, 4242)
    p, vp = {"iterations": 4}, {"history_min": 4, "sigma_luminance": 3.0}
    r = hrt.Renderer(0, 0)
    try:
        ds, dt, dg = _dev(s), _dev(t.view(np.int32)), _dev(g.view(np.int16))
        out, linear, var = r.denoise_accumulated_filter(ds, dt, dg, p, vp)
        hs, n = ds.cpu(), dt.cpu().to(torch.float32)
        mean = torch.ones((h, w, 4), dtype=torch.float32)
        mean[..., :3] = hs[..., :3] / n[..., None]
        lum = (hs[..., 0] * 0.2126 + hs[..., 1] * 0.7152) + hs[..., 2] * 0.0722
        m1, m2 = lum / n, hs[..., 3] / n
        v = torch.fmax(torch.zeros(()), m2 - m1 * m1) / n
        assert (v > 0).any()
        want_linear, want_var = r.denoise_filter_variance(mean.cuda(), dg, v.cuda(), p, vp)
        want = torch.empty_like(want_linear)
        r._check(r.lib.hrt_color_to_float4(r.ctx, want_linear.data_ptr(), want.data_ptr(), w * h, r._stream()), "hrt_color_to_float4")
        torch.cuda.synchronize()
        for got, exp in ((out, want), (linear, want_linear), (var, want_var)):
            assert np.array_equal(dc.bits(_host(got)), dc.bits(_host(exp)))
    finally:
        r.close()


# ---- the launch form over hrt_render_accumulate's frames ------------------------------------
def _start(hrt, mode, w, h):
    scene = hrt.scenes.mixed_test_scene(width=w, height=h, transforms=True)        # (tests/test_render_accumulate_gpu.py's "mixed")
    r = hrt.Renderer(0, {"production": 0, "two_level": hrt.CTX_TWO_LEVEL, "capture": hrt.CTX_CAPTURE_PRIMARY}[mode])
    r.load_scene(scene)
    r.set_frame(w, h, hrt.scenes.SEED_SALT)
    return r, scene


def _adaptive(r):
    """pilot 3, counts up to 16 in total, one refinement"""
    r.accumulation_reset()
    r.accumulate(3, sync=False)
    counts = r.sample_counts({"max_total": 16})
    r.accumulate(16, counts=counts)


def _state(r):
    return (dc.bits(_host(r.sum)), _host(r.taken).view(np.uint32), r.rng_states_numpy(), dc.bits(_host(r.color)))


def _want(oracle, r, scene, instanced, p=None, vp=None):
    """The specification over the GPU's own sums and totals (pinned to the oracle by tests/test_render_accumulate_gpu.py) and the
    oracle's primary guides."""
    osc = oracle.OracleScene(scene, instanced=instanced)
    try:
        guides = ref.primary_guides(osc, scene, r.cam, r.width, r.height)
    finally:
        osc.close()
    return aref.denoise_accumulated(_host(r.sum), _host(r.taken).view(np.uint32), guides, p, vp)[0]


@pytest.mark.parametrize("size", [(61, 37), (1, 1)])
@pytest.mark.parametrize("mode", ["production", "two_level"])
def test_adaptive_frame_end_to_end(hrt_gpu, oracle, mode, size):
    """accumulation_reset, pilot, sample_counts, refinement, denoise_accumulated(): the specification over the downloaded sums and the
    oracle's guides; sums, totals, RNG states and the colour buffer as they were."""
    hrt = hrt_gpu
    w, h = size
    r, scene = _start(hrt, mode, w, h)
    try:
        _adaptive(r)
        taken = _host(r.taken)
        assert taken.min() >= 3 and taken.max() <= 16 and (w * h == 1 or taken.max() > taken.min())
        before = _state(r)
        for p, vp in ((None, None), ({"iterations": 3}, {"history_min": 8})):
            got = _host(r.denoise_accumulated(p, vp))
            _check_rgba(got, _want(oracle, r, scene, mode == "two_level", p, vp), f"{mode} {w}x{h} {vp}")
            for a, b, what in zip(_state(r), before, ("sums", "totals", "states", "colour")):
                assert np.array_equal(a, b), what
        # into the colour buffer: the same bits
        assert r.denoise_accumulated(p, vp, out=r.color) is r.color
        assert np.array_equal(dc.bits(_host(r.color)), dc.bits(got))
    finally:
        r.close()


def test_striped_tile(hrt_gpu, oracle):
    """Accumulated through a tile only, denoised as a full frame: the rows outside come out (0, 0, 0, 1), the rows inside are the
    specification's, whose taps stop at the stripe's edge."""
    hrt = hrt_gpu
    w, h = 37, 16
    rows = [3, 4, 10]
    r, scene = _start(hrt, "production", w, h)
    try:
        r.accumulation_reset()
        r.accumulate(5, tile=hrt.Tile(3, 11, 5, 2, 0))            # rows y of [3, 11) with (y / 5) % 2 == 0
        taken = _host(r.taken)
        outside = np.ones(h, bool)
        outside[rows] = False
        assert (taken[rows] == 5).all() and not taken[outside].any()
        p, vp = {"iterations": 4}, {"history_min": 4}
        got = _host(r.denoise_accumulated(p, vp))
        assert np.array_equal(got[outside], np.broadcast_to(BLACK, got[outside].shape))
        want = _want(oracle, r, scene, False, p, vp)
        _check_rgba(got, want, "striped tile")
        assert (want[rows, :, :3] > 0).any()
    finally:
        r.close()


def test_capture_context_traces_its_guides(hrt_gpu):
    """HRT_CTX_CAPTURE_PRIMARY: hrt_render_accumulate captures nothing and invalidates what there was, so the guide pass is traced --
    guide_passes_traced grows by one -- and the result is the bits of a context without the flag."""
    hrt = hrt_gpu
    w, h = 61, 37
    rc, _ = _start(hrt, "capture", w, h)
    rp, _ = _start(hrt, "production", w, h)
    try:
        for r in (rc, rp):
            r.render(1)                                           # (rc holds a capture of this frame now)
            _adaptive(r)
        s0 = rc.stats()
        got = _host(rc.denoise_accumulated())
        s1 = rc.stats()
        assert (s1.guide_passes_traced - s0.guide_passes_traced, s1.guide_passes_captured - s0.guide_passes_captured) == (1, 0)
        assert np.array_equal(dc.bits(got), dc.bits(_host(rp.denoise_accumulated())))
    finally:
        rc.close(); rp.close()


def test_temporal_history_is_left_alone(hrt_gpu):
    """denoise_variance frame 1, a denoise_accumulated still, denoise_variance frame 2: frame 2 and its state are what they are without
    the still in between."""
    hrt = hrt_gpu
    w, h = 61, 37
    ra, _ = _start(hrt, "production", w, h)
    rb, _ = _start(hrt, "production", w, h)
    try:
        frames = {}
        for r in (ra, rb):
            _adaptive(r)
            first = _host(r.denoise_variance())
            if r is ra:
                r.denoise_accumulated()
                r.denoise_accumulated({"iterations": 2}, {"history_min": 1})
            r.render(2)
            second = _host(r.denoise_variance())
            frames[r] = (first, second) + tuple(_host(x) for x in r.denoise_temporal_state()) + tuple(_host(x) for x in r.denoise_variance_state())
        for a, b in zip(frames[ra], frames[rb]):
            assert np.array_equal(dc.bits(a), dc.bits(b))
        assert (frames[ra][3] > 1).any()                          # (frame 2 did blend with frame 1's history)
    finally:
        ra.close(); rb.close()


def test_refusals_touch_nothing(hrt_gpu):
    """Every refusal of both forms by status, with the buffers -- inputs and outputs -- as they were after each."""
    import torch
    hrt = hrt_gpu
    w, h = 16, 12
    r, _ = _start(hrt, "production", w, h)
    try:
        _adaptive(r)
        lib = r.lib
        g = r.denoise_guides()
        out, lin = torch.full_like(r.color, 0.3125), torch.full_like(r.color, 0.3125)
        var = torch.full((h, w), 0.3125, dtype=torch.float32, device=r.device)
        before = _state(r) + (dc.bits(_host(out)), dc.bits(_host(lin)), dc.bits(_host(var)), _host(g).copy())

        def untouched(what):
            torch.cuda.synchronize()
            now = _state(r) + (dc.bits(_host(out)), dc.bits(_host(lin)), dc.bits(_host(var)), _host(g))
            for a, b in zip(now, before):
                assert np.array_equal(a, b), what

        S, T, G, O, L, V = (x.data_ptr() for x in (r.sum, r.taken, g, out, lin, var))
        f = lambda *a: lib.hrt_denoise_accumulated_filter(r.ctx, *a, None)      # noqa: E731
        for what, args in (("NULL sum", (None, T, G, O, L, V, w, h, None, None)), ("NULL taken", (S, None, G, O, L, V, w, h, None, None)),
                           ("NULL guides", (S, T, None, O, L, V, w, h, None, None)), ("NULL out", (S, T, G, None, L, V, w, h, None, None)),
                           ("out is sum", (S, T, G, S, L, V, w, h, None, None)), ("linear is sum", (S, T, G, O, S, V, w, h, None, None)),
                           ("linear is out", (S, T, G, O, O, V, w, h, None, None)),
                           ("no width", (S, T, G, O, L, V, 0, h, None, None)), ("too high", (S, T, G, O, L, V, w, 65537, None, None))):
            assert f(*args) == -1, what
            untouched(what)
        assert lib.hrt_denoise_accumulated_filter(None, S, T, G, O, L, V, w, h, None, None, None) == -1
        params_blk, rg = r._launch_blocks()
        launch = lambda ctx, pb, rgb, s, t, o: lib.hrt_denoise_accumulated_launch(ctx, pb, rgb, s, t, None, None, o, None)      # noqa: E731
        for what, args in (("NULL ctx", (None, C.byref(params_blk), C.byref(rg), S, T, O)), ("NULL params", (r.ctx, None, C.byref(rg), S, T, O)),
                           ("NULL raygen", (r.ctx, C.byref(params_blk), None, S, T, O)), ("NULL sum", (r.ctx, C.byref(params_blk), C.byref(rg), None, T, O)),
                           ("NULL taken", (r.ctx, C.byref(params_blk), C.byref(rg), S, None, O)), ("NULL out", (r.ctx, C.byref(params_blk), C.byref(rg), S, T, None)),
                           ("out is sum", (r.ctx, C.byref(params_blk), C.byref(rg), S, T, S))):
            assert launch(*args) == -1, what
            untouched(what)
        # the parameters: hrt_denoise_filter_variance's refusals, in both forms
        for bad in ({"sigma_luminance": 0.0}, {"sigma_luminance": float("nan")}, {"sigma_luminance": 1e30}, {"sigma_luminance": 1e-30},
                    {"history_min": 0}, {"history_min": 65537}, {"variance_floor": 0.0}, {"variance_floor": float("inf")}, {"reserved": 1}):
            with pytest.raises(hrt.HrtError, match="status -1"):
                r.denoise_accumulated(vparams=bad, out=out)
            with pytest.raises(hrt.HrtError, match="status -1"):
                r.denoise_accumulated_filter(r.sum, r.taken, g, vparams=bad, out=out, linear_out=lin, var_out=var)
            untouched(bad)
        for bad in ({"iterations": 0}, {"iterations": 17}, {"sigma_albedo": 0.0}, {"sigma_color": -1.0}, {"reserved": 1}, {"sigma_depth": 2e34, "iterations": 16}):
            with pytest.raises(hrt.HrtError, match="status -1"):
                r.denoise_accumulated(params=bad, out=out)
            with pytest.raises(hrt.HrtError, match="status -1"):
                r.denoise_accumulated_filter(r.sum, r.taken, g, params=bad, out=out, linear_out=lin, var_out=var)
            untouched(bad)
        # the edges are taken
        r.denoise_accumulated(vparams={"sigma_luminance": 1e-15, "history_min": 65536, "variance_floor": 1e-38}, out=out)
        r.denoise_accumulated(vparams={"history_min": 1, "sigma_luminance": 1e15}, out=out)
    finally:
        r.close()


def test_state_refusals(hrt_gpu):
    """HRT_ERR_STATE as the guide pass gives it: before hrt_materials_set, and a two-level tree under HRT_CTX_COUNT."""
    import torch
    hrt = hrt_gpu
    w, h = 32, 24
    r = hrt.Renderer(0, 0)
    try:
        s = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        t = torch.ones((h, w), dtype=torch.int32, device="cuda")
        out = torch.full((h, w, 4), 0.3125, dtype=torch.float32, device="cuda")
        rg = hrt.RayGenParams()
        rg.width, rg.height = w, h
        params_blk = hrt.GlobalParams(0, None)
        assert r.lib.hrt_denoise_accumulated_launch(r.ctx, C.byref(params_blk), C.byref(rg), s.data_ptr(), t.data_ptr(), None, None, out.data_ptr(), None) == -5
        torch.cuda.synchronize()
        assert (out == 0.3125).all().item()
    finally:
        r.close()
    r = hrt.Renderer(0, hrt.CTX_TWO_LEVEL)
    try:
        r.load_scene(hrt.scenes.particle_scene(12, w, h, 1, frame=2))
        r.set_frame(w, h, hrt.scenes.SEED_SALT)
        r.accumulate(2)
        r.set_flags(hrt.CTX_TWO_LEVEL | hrt.CTX_COUNT)
        out = torch.full_like(r.color, 0.3125)
        before = _state(r)
        with pytest.raises(hrt.HrtError, match="status -5"):
            r.denoise_accumulated(out=out)
        torch.cuda.synchronize()
        assert (out == 0.3125).all().item()
        for a, b in zip(_state(r), before):
            assert np.array_equal(a, b)
    finally:
        r.close()
