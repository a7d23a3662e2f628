"""The denoiser's kernels on the MI355X against the numpy specifications, bit for bit, on the edge cases of tests/denoise_cases.py --
the cases tests/test_denoise_edges_cpu.py shows to reach the branches, sizes and values the other denoiser tests leave out:
non-default temporal parameters (the 1 / L side of alpha, the history cap, the depth test), cameras that turn, zoom, roll and flip,
reprojections behind the camera and beyond the finite range, frames that fill no block, hostile colours, depths, normals and
albedos, deep iteration counts, and one context that changes size between calls.

One comparison rule (denoise_cases.same): equal NaN masks, every other element the same bits; the payload of a computed NaN is not
compared.  The alpha channel is a copy and is compared on raw bits, payloads included.  No tolerance anywhere.
Figures and the mutations these tests were shown to catch: profiles/r08_denoise_edges.txt."""
import importlib

import numpy as np
import pytest

import denoise_cases as dc
import denoise_ref as ref

pytestmark = pytest.mark.gpu
_HRT = importlib.import_module("nvidia-optix-ray-tracer_amd")
SEQUENCES = dc.temporal_sequences(_HRT)
MODES = ("production", "counting", "two_level")


@pytest.fixture(scope="module")
def hrt_gpu(hrt):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return hrt


def _flags(hrt, mode):
    return {"production": 0, "counting": hrt.CTX_COUNT, "two_level": hrt.CTX_TWO_LEVEL}[mode]


@pytest.fixture(scope="module")
def shared(hrt_gpu):
    """One production context for the filter-only cases, so that consecutive cases change the frame size under it."""
    r = hrt_gpu.Renderer(0, 0)
    yield r
    r.close()


def _dev(a):
    """A float32 array on the device with its bits as they are."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda().view(torch.float32)


def _dev_guides(g):
    import torch
    return torch.from_numpy(np.ascontiguousarray(g).view(np.int16)).cuda()


def _host(t):
    import torch
    return t.view(torch.int32).cpu().numpy().view(np.float32)


def _check(got, want, what):
    n, differ = dc.nan_payloads(got, want)
    if n:
        print(f"{what}: {n} NaNs on both sides, {differ} with different bits")
    assert dc.same(got, want), (what, dc.first_difference(got, want))


def _check_rgba(got, want, what):
    _check(got[..., :3], want[..., :3], what)
    assert np.array_equal(dc.bits(got[..., 3]), dc.bits(want[..., 3])), (what, "alpha", dc.first_difference(got[..., 3], want[..., 3]))


def _filter_and_check(r, c, g, p, what):
    with np.errstate(all="ignore"):
        want = ref.atrous(c, g, p)
    dcol, dg = _dev(c), _dev_guides(g)
    _check_rgba(_host(r.denoise_filter(dcol, dg, p)), want, what)
    assert np.array_equal(dc.bits(_host(dcol)), dc.bits(c))                  # the input is left alone
    r.denoise_filter(dcol, dg, p, out=dcol)
    _check_rgba(_host(dcol), want, what + " in place")


# ---- the filter -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", dc.FILTER_CASES)
def test_filter_edge_case(shared, name):
    c, g, p = dc.filter_case(name)
    _filter_and_check(shared, c, g, p, name)


def test_late_refusals_leave_the_context_usable(hrt_gpu):
    """Parameters whose constants leave the finite range at a later pass only: status -1 from every entry point, and the same
    parameters with fewer passes, where every constant is finite, filter bit-exactly on the same context right after."""
    hrt = hrt_gpu
    w, h = 33, 17
    r = hrt.Renderer(0, 0)
    try:
        r.load_scene(hrt.scenes.cornell_box(w, h, 1))
        r.set_frame(w, h, hrt.scenes.SEED_SALT)
        c, g, _ = dc.filter_case("tile-33x17")
        for bad in dc.LATE_REFUSALS:
            deep, shallow = dict(bad, iterations=16), dict(bad, iterations=5)
            with pytest.raises(hrt.HrtError, match="status -1"):
                r.denoise_filter(_dev(c), _dev_guides(g), deep)
            with pytest.raises(hrt.HrtError, match="status -1"):
                r.denoise(deep)
            with pytest.raises(hrt.HrtError, match="status -1"):
                r.denoise_temporal(deep)
            _filter_and_check(r, c, g, shallow, f"after refusing {deep}")
            _filter_and_check(r, c, g, dict(iterations=16), "16 passes of the defaults")
    finally:
        r.close()


# ---- the guide pass and the convenience call -------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", dc.GUIDE_CASES, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}")
def test_guides_and_launch_edge_case(hrt_gpu, oracle, case, mode):
    hrt = hrt_gpu
    name, w, h = case
    scene = dc.scene_by_name(hrt, name, w, h)
    osc = oracle.OracleScene(scene, instanced=(mode == "two_level"))
    r = hrt.Renderer(0, _flags(hrt, mode))
    try:
        r.load_scene(scene)
        r.set_frame(w, h, hrt.scenes.SEED_SALT)
        with np.errstate(all="ignore"):
            want = ref.primary_guides(osc, scene, r.cam, w, h)
        got = r.denoise_guides().cpu().numpy().view(np.uint16)
        assert np.array_equal(got, want), np.argwhere((got != want).any(axis=-1))[:8]
        color = dc.plain_color(np.random.default_rng(w * 1000 + h), h, w)
        r.color.copy_(_dev(color))
        params = {"iterations": 3, "normal_power_log2": 2}
        with np.errstate(all="ignore"):
            want_out = ref.atrous(color, want, params)
        _check_rgba(_host(r.denoise(params)), want_out, f"denoise {case}")
    finally:
        r.close()
        osc.close()


# ---- the temporal mode -------------------------------------------------------------------------
def _run_sequence(hrt, oracle, name, seq, mode, before_frame=None):
    w, h = seq["size"]
    scene = dc.scene_by_name(hrt, seq["scene"], w, h)
    r = hrt.Renderer(0, _flags(hrt, mode))
    try:
        r.load_scene(scene)
        r.set_frame(w, h, hrt.scenes.SEED_SALT)
        xf = [np.asarray(it["transform"], np.float32).reshape(12) for it in scene["instances"]]
        frames = 0
        for f in dc.walk_sequence(hrt, oracle, name, seq, instanced=(mode == "two_level")):
            k = f["k"]
            if f["changed"]:
                for i, m in f["changed"].items():
                    xf[i] = np.asarray(m, np.float32).reshape(12)
                r.update_instances(np.array(xf, np.float32))
            cam = f["camera"]
            r.set_camera(cam["center"], cam["target"], cam["up"], cam.get("opengl", True))
            assert all(np.array_equal(dc.bits(a), dc.bits(b)) for a, b in zip(r.cam, f["cam"]))
            if before_frame is not None:
                before_frame(r, k)
            r.color.copy_(_dev(f["color"]))
            out = r.denoise_temporal(seq["params"], seq["tparams"], out=r.color if seq["in_place"] else None)
            got = _host(out)
            A, L, M = (_host(x) for x in r.denoise_temporal_state())
            what = f"{name} {mode} frame {k}"
            _check_rgba(A, f["A"], what + " A")
            _check(L, f["L"], what + " L")
            _check(M, f["motion"], what + " motion")
            _check_rgba(got, f["want"], what + " output")
            if not seq["in_place"]:
                assert np.array_equal(dc.bits(_host(r.color)), dc.bits(f["color"]))
            frames += 1
        assert frames == len(seq["frames"])
    finally:
        r.close()


@pytest.mark.parametrize("name,mode", [(n, m) for n, s in SEQUENCES.items() for m in s["modes"]])
def test_temporal_sequence(hrt_gpu, oracle, name, mode):
    """Output, accumulated colour, history length and motion of every frame of the sequence."""
    _run_sequence(hrt_gpu, oracle, name, SEQUENCES[name], mode)


def test_history_survives_a_larger_filter_call(hrt_gpu, oracle):
    """A 640 x 360 hrt_denoise_filter between frames 2 and 3 of a 97 x 61 sequence grows the context's work arrays (and frees the
    guide pass's): frame 3 and the frames after it still equal the specification continuing from frame 2's history."""
    rng = np.random.default_rng(640360)
    c, g, p = dc.plain_color(rng, 360, 640), dc.random_guides(rng, 360, 640), {"iterations": 3}
    calls = []

    def between(r, k):
        if k == 3:
            _filter_and_check(r, c, g, p, "640x360 between frames")
            calls.append(k)

    _run_sequence(hrt_gpu, oracle, "cap-3", SEQUENCES["cap-3"], "production", before_frame=between)
    assert calls == [3]


def test_one_context_through_growing_and_shrinking_frames(hrt_gpu, oracle):
    """filter 5 x 17, guides 97 x 61, filter 640 x 360, denoise() 97 x 61, filter 1 x 1 on one context, in this order: the work arrays
    grow, the guide pass's are freed by the larger filter call and come back."""
    hrt = hrt_gpu
    w, h = 97, 61
    scene = hrt.scenes.cornell_box(w, h, 1)
    osc = oracle.OracleScene(scene)
    r = hrt.Renderer(0, 0)
    try:
        r.load_scene(scene)
        r.set_frame(w, h, hrt.scenes.SEED_SALT)
        rng = np.random.default_rng(51797)
        _filter_and_check(r, dc.plain_color(rng, 17, 5), dc.random_guides(rng, 17, 5), {"iterations": 4}, "5x17")
        want_g = ref.primary_guides(osc, scene, r.cam, w, h)
        got_g = r.denoise_guides().cpu().numpy().view(np.uint16)
        assert np.array_equal(got_g, want_g)
        _filter_and_check(r, dc.plain_color(rng, 360, 640), dc.random_guides(rng, 360, 640), {"iterations": 3}, "640x360")
        color = dc.plain_color(rng, h, w)
        r.color.copy_(_dev(color))
        _check_rgba(_host(r.denoise()), ref.atrous(color, want_g), "denoise 97x61")
        _filter_and_check(r, dc.plain_color(rng, 1, 1), dc.random_guides(rng, 1, 1, background=0.0), {"iterations": 2}, "1x1")
        assert np.array_equal(r.denoise_guides().cpu().numpy().view(np.uint16), want_g)
    finally:
        r.close()
        osc.close()
