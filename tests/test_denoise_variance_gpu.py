"""The denoiser's variance-guided mode on the MI355X (include/hrt.h "Variance-guided mode"; csrc/denoise.hip k_denoise_temporal<true>,
k_denoise_variance, k_denoise_pass<.., true>): everything bit for bit against the numpy specification (tests/denoise_variance_ref.py), no
tolerance -- the filter alone on synthetic frames, whole sequences over the oracle's primary hits, the rules of the shared history,
and the other two modes left as they were.  The inputs are tests/denoise_variance_cases.py's; tests/test_denoise_variance_cpu.py
asserts on the specification that they reach the branches they are for."""
import numpy as np
import pytest

import denoise_cases as dc
import denoise_ref as ref
import denoise_temporal_ref as tref
import denoise_variance_cases as vc
import denoise_variance_ref as vref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hrt_gpu(hrt):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    lib = hrt.load_library()
    for name in ("hrt_denoise_variance_default_params", "hrt_denoise_filter_variance", "hrt_denoise_variance_launch",
                 "hrt_debug_denoise_variance_state"):
        getattr(lib, name)                                       # (AttributeError, not a skip, where the library lacks the mode)
    return hrt


@pytest.fixture(scope="module")
def filter_renderer(hrt_gpu):
    """One context for every filter case: its frames grow and shrink with the cases' sizes."""
    r = hrt_gpu.Renderer(0, 0)
    yield r
    r.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    return t.cpu().numpy()


def _check(got, want, what):
    assert dc.same(got, want), (what, dc.first_difference(got, want))


def _check_rgba(got, want, what):
    assert dc.same_rgba(got, want), (what, dc.first_difference(got[..., :3], want[..., :3]))


def _filter_and_check(r, name):
    c, g, v, p, vp, in_place, var_mode = vc.filter_case(name)
    want, want_v = vref.filter_variance(c, g, v, p, vp)
    dcol, dg, dv = _dev(c), _dev(g.view(np.int16)), _dev(v)
    var_out = {"set": None, "null": False, "same": dv}[var_mode]
    out, vo = r.denoise_filter_variance(dcol, dg, dv, p, vp, out=dcol if in_place else None, var_out=var_out)
    _check_rgba(_host(out), want, name + " colour")
    if var_mode != "null":
        _check(_host(vo), want_v, name + " variance")
    if not in_place:
        assert np.array_equal(dc.bits(_host(dcol)), dc.bits(c))
    if var_mode != "same":
        assert np.array_equal(dc.bits(_host(dv)), dc.bits(v))
    assert np.array_equal(_host(dg).view(np.uint16), g)


@pytest.mark.parametrize("name", vc.FILTER_CASES)
def test_filter_variance_bit_exact(filter_renderer, name):
    """hrt_denoise_filter_variance: colour and filtered variance of every case -- 1x1 to 37x29, 1 to 9 passes, in place and not,
    d_var_out NULL, set and the variance itself, default and other parameters, hostile variances and colours, background holes."""
    _filter_and_check(filter_renderer, name)


def test_filter_variance_one_context_grows_and_shrinks(hrt_gpu):
    r = hrt_gpu.Renderer(0, 0)
    try:
        for name in vc.GROW_SHRINK:
            _filter_and_check(r, name)
    finally:
        r.close()


def test_plain_and_variance_filters_share_one_context(hrt_gpu):
    """hrt_denoise_filter and hrt_denoise_filter_variance in alternation on one context, at sizes that make the frames they share grow
    between the calls: the variance frames are allocated by the first variance call, after the plain filter has set the capacity, and
    again after the plain filter has raised it."""
    r = hrt_gpu.Renderer(0, 0)
    try:
        p = {"iterations": 3}
        for variance, (w, h) in ((False, (5, 3)), (True, (37, 29)), (False, (64, 48)), (True, (17, 5))):
            what = f"{'variance' if variance else 'plain'} {w}x{h}"
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
    finally:
        r.close()


def _flags(hrt, mode):
    return {"production": 0, "two_level": hrt.CTX_TWO_LEVEL}[mode]


def _check_frame(r, f, got, what):
    A, L, motion = (_host(x) for x in r.denoise_temporal_state())
    M, var = (_host(x) for x in r.denoise_variance_state())
    _check_rgba(A, f["A"], what + " A")
    _check(L, f["L"], what + " L")
    _check(motion, f["motion"], what + " motion")
    _check(M, f["M"], what + " M")
    _check(var, f["var"], what + " variance")
    _check_rgba(got, f["want"], what + " output")


def _step(r, seq, f, xf):
    """Bring the renderer to frame f's scene, camera and colour."""
    if f["changed"]:
        for i, m in f["changed"].items():
            xf[i] = np.asarray(m, np.float32).reshape(12)
        r.update_instances(np.array(xf, np.float32))
    cam = f["camera"]
    r.set_camera(cam["center"], cam["target"], cam["up"], cam.get("opengl", True))
    r.color.copy_(_dev(f["color"]))


def _start(hrt, seq, mode):
    w, h = seq["size"]
    scene = dc.scene_by_name(hrt, seq["scene"], w, h)
    r = hrt.Renderer(0, _flags(hrt, mode))
    r.load_scene(scene)
    r.set_frame(w, h, hrt.scenes.SEED_SALT)
    return r, [np.asarray(it["transform"], np.float32).reshape(12) for it in scene["instances"]]


@pytest.fixture(scope="module")
def sequences(hrt_gpu):
    return vc.sequences(hrt_gpu)


def _sequence_ids():
    # (the names and modes of denoise_variance_cases.sequences, which needs the package to build its scenes)
    ids = [(f"{s}-hmin{h}", m) for s in ("c1", "mixed") for h in (1, 4) for m in ("production", "two_level")]
    return ids + [("c1-defaults", "production"), ("hostile-color", "production"), ("hostile-color", "two_level")]


@pytest.mark.parametrize("name,mode", _sequence_ids())
def test_variance_sequence_bit_exact(hrt_gpu, oracle, sequences, name, mode):
    """Six frames of hrt_denoise_variance_launch: A, L, motion, M, the variance and the output of every frame.  Frame 2 moves every
    instance through hrt_tlas_update, frame 4 pans the camera; history_min 1 and 4; flattened and two-level trees."""
    hrt = hrt_gpu
    assert sorted(_sequence_ids()) == sorted((n, m) for n, s in sequences.items() for m in s["modes"])
    seq = sequences[name]
    r, xf = _start(hrt, seq, mode)
    try:
        frames = 0
        for f in vc.walk(hrt, oracle, name, seq, instanced=(mode == "two_level")):
            _step(r, seq, f, xf)
            got = _host(r.denoise_variance(seq["params"], seq["tparams"], seq["vparams"], out=r.color if seq["in_place"] else None))
            _check_frame(r, f, got, f"{name} {mode} frame {f['k']}")
            if f["k"] > 0:
                assert (f["L"] > 1).sum() > 0.3 * (f["L"] > 0).sum()          # the sequence does reuse history
            frames += 1
        assert frames == 6
    finally:
        r.close()


def test_state_rules(hrt_gpu, oracle, sequences):
    """The debug call before the first launch is HRT_ERR_STATE.  A mode switch starts afresh in both directions, and so do
    hrt_denoise_temporal_reset, a new frame size, a new TLAS handle with the same instance count, and one with another count: the
    call after each equals the specification without history.  (Handles are never reused and hrt_tlas_update keeps the count, so the
    count cannot change under one handle.)  After variance calls hrt_denoise_launch and hrt_denoise_temporal_launch give their own
    specifications' bits, and hrt_debug_denoise_temporal_state keeps working."""
    hrt = hrt_gpu
    name = "c1-hmin4"
    seq = sequences[name]
    w, h = seq["size"]
    p, tp, vp = seq["params"], seq["tparams"], seq["vparams"]
    r, xf = _start(hrt, seq, "production")
    try:
        with pytest.raises(hrt.HrtError, match="status -5"):
            r.denoise_variance_state()
        frames = list(vc.walk(hrt, oracle, name, seq))
        scene0 = dc.scene_by_name(hrt, seq["scene"], w, h)
        osc = oracle.OracleScene(scene0)
        cam0 = frames[0]["cam"]

        def fresh(color):
            return vref.variance_frame(None, color, osc, scene0, cam0, w, h, p, tp, vp)

        def run(k):
            _step(r, seq, frames[k], xf)
            return _host(r.denoise_variance(p, tp, vp))

        _check_frame(r, frames[0], run(0), "frame 0")
        _check_frame(r, frames[1], run(1), "frame 1")
        # variance -> temporal: the temporal call has no history and is hrt_denoise_launch's result; temporal's own bits after that
        color = frames[1]["color"]
        t_out = _host(r.denoise_temporal(p, tp))
        want_t, wA, wL, wM, thist = tref.temporal_frame(None, color, osc, scene0, cam0, w, h, p, tp)
        _check_rgba(t_out, want_t, "temporal after variance")
        assert np.array_equal(dc.bits(t_out), dc.bits(_host(r.denoise(p))))
        A, L, motion = (_host(x) for x in r.denoise_temporal_state())
        _check(L, wL, "temporal L after variance")
        assert np.isnan(motion).all()
        with pytest.raises(hrt.HrtError, match="status -1"):
            r.denoise_variance(vparams={"history_min": 0})                     # (a refused call leaves the history alone)
        t_out = _host(r.denoise_temporal(p, tp))
        want_t, _, wL, _, _ = tref.temporal_frame(thist, color, osc, scene0, cam0, w, h, p, tp)
        _check_rgba(t_out, want_t, "temporal, second call")
        assert (wL > 1).any()
        _check_rgba(_host(r.denoise(p)), ref.atrous(color, ref.primary_guides(osc, scene0, cam0, w, h), p), "denoise after variance")
        # temporal -> variance: afresh
        got = _host(r.denoise_variance(p, tp, vp))
        want = fresh(color)
        _check_rgba(got, want[0], "variance after temporal")
        _check(_host(r.denoise_temporal_state()[1]), want[2], "variance after temporal: L")
        M, var = (_host(x) for x in r.denoise_variance_state())
        _check(M, want[4], "variance after temporal: M")
        _check(var, want[5], "variance after temporal: variance")
        # ... and the call after it has history
        got = _host(r.denoise_variance(p, tp, vp))
        second = vref.variance_frame(want[6], color, osc, scene0, cam0, w, h, p, tp, vp)
        _check_rgba(got, second[0], "variance, second call")
        assert (second[2] > 1).any()
        # reset
        r.denoise_temporal_reset()
        _check_rgba(_host(r.denoise_variance(p, tp, vp)), want[0], "variance after reset")
        assert np.isnan(_host(r.denoise_temporal_state()[2])).all()
        osc.close()
        # a new frame size
        w2, h2 = 23, 17
        r.set_frame(w2, h2, hrt.scenes.SEED_SALT)
        scene2 = dc.scene_by_name(hrt, "c1", w2, h2)
        osc = oracle.OracleScene(scene2)
        c2 = dc.plain_color(np.random.default_rng(2317), h2, w2)
        r.color.copy_(_dev(c2))
        got = _host(r.denoise_variance(p, tp, vp))
        want2 = vref.variance_frame(None, c2, osc, scene2, cam0, w2, h2, p, tp, vp)
        _check_rgba(got, want2[0], "variance after a new frame size")
        got = _host(r.denoise_variance(p, tp, vp))
        _check_rgba(got, vref.variance_frame(want2[6], c2, osc, scene2, cam0, w2, h2, p, tp, vp)[0], "variance, new size, second call")
        # a new TLAS handle, the same scene and instance count
        old = r.tlas
        r.load_scene(scene2)
        assert r.tlas != old
        got = _host(r.denoise_variance(p, tp, vp))
        want2b = vref.variance_frame(None, c2, osc, scene2, r.cam, w2, h2, p, tp, vp)
        _check_rgba(got, want2b[0], "variance after a new TLAS handle of the same scene")
        _check(_host(r.denoise_temporal_state()[1]), want2b[2], "variance after a new TLAS handle of the same scene: L")
        osc.close()
        # a new TLAS handle and instance count
        scene3 = hrt.scenes.sphere_in_box(w2, h2, 1)
        r.load_scene(scene3)
        osc = oracle.OracleScene(scene3)
        got = _host(r.denoise_variance(p, tp, vp))
        want3 = vref.variance_frame(None, c2, osc, scene3, r.cam, w2, h2, p, tp, vp)
        _check_rgba(got, want3[0], "variance after a new TLAS")
        _check(_host(r.denoise_variance_state()[1]), want3[5], "variance after a new TLAS: variance")
        osc.close()
    finally:
        r.close()


def test_variance_rejects_bad_parameters(hrt_gpu):
    hrt = hrt_gpu
    w, h = 16, 12
    r = hrt.Renderer(0, 0)
    try:
        r.load_scene(hrt.scenes.cornell_box(w, h, 1))
        r.set_frame(w, h, hrt.scenes.SEED_SALT)
        import torch
        g = torch.zeros((h, w, 8), dtype=torch.int16, device=r.device)
        v = torch.zeros((h, w), dtype=torch.float32, device=r.device)
        for bad in ({"sigma_luminance": 0.0}, {"sigma_luminance": -1.0}, {"sigma_luminance": float("nan")}, {"sigma_luminance": float("inf")},
                    {"sigma_luminance": 1e30}, {"sigma_luminance": 1e-30}, {"history_min": 0}, {"history_min": 65537},
                    {"variance_floor": 0.0}, {"variance_floor": float("inf")}, {"variance_floor": float("nan")}, {"reserved": 1}):
            with pytest.raises(hrt.HrtError, match="status -1"):
                r.denoise_variance(vparams=bad)
            with pytest.raises(hrt.HrtError, match="status -1"):
                r.denoise_filter_variance(r.color, g, v, vparams=bad)
        for bad in ({"iterations": 0}, {"sigma_albedo": 0.0}, {"reserved": 1}):
            with pytest.raises(hrt.HrtError, match="status -1"):
                r.denoise_variance(params=bad)
        with pytest.raises(hrt.HrtError, match="status -1"):
            r.denoise_variance(tparams={"alpha_min": 0.0})
        with pytest.raises(hrt.HrtError, match="status -5"):
            r.denoise_variance_state()                                        # every call above was refused
        assert r.lib.hrt_denoise_filter_variance(r.ctx, r.color.data_ptr(), g.data_ptr(), None, r.color.data_ptr(), None, w, h, None, None, None) == -1
        r.denoise_variance(vparams={"sigma_luminance": 1e-15, "history_min": 65536, "variance_floor": 1e-38})     # the edges are taken
        r.denoise_variance(vparams={"history_min": 1, "sigma_luminance": 1e15})
    finally:
        r.close()
