"""The denoiser's variance-guided mode without a GPU: its C ABI's defaults, argument checks and public layout through the built
library, properties of the numpy specification (tests/denoise_variance_ref.py) that the GPU tests pin the kernels to, and the reach
check: over the inputs tests/test_denoise_variance_gpu.py runs (tests/denoise_variance_cases.py), every branch listed in
test_cases_reach_every_listed_branch decides at least one output bit.  The cap: no listed branch may be unreached."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

import denoise_cases as dc
import denoise_ref as ref
import denoise_temporal_ref as tref
import denoise_variance_cases as vc
import denoise_variance_ref as vref

ROOT = Path(__file__).resolve().parent.parent
f32 = np.float32


def test_variance_default_params_and_refusals(hrt):
    lib = hrt.load_library()
    p = hrt.DenoiseVarianceParams()
    assert lib.hrt_denoise_variance_default_params(C.byref(p)) == 0
    assert p.history_min == vref.DEFAULTS["history_min"] and p.reserved == 0
    for k in ("sigma_luminance", "variance_floor"):
        assert getattr(p, k) == np.float32(vref.DEFAULTS[k])
    assert lib.hrt_denoise_variance_default_params(None) == -1                  # HRT_ERR_INVALID
    gp, rg = hrt.GlobalParams(), hrt.RayGenParams()
    assert lib.hrt_denoise_variance_launch(None, C.byref(gp), C.byref(rg), None, None, None, C.c_void_p(16), None) == -1
    assert lib.hrt_denoise_filter_variance(None, C.c_void_p(16), C.c_void_p(16), C.c_void_p(16), C.c_void_p(16), None, 4, 4, None, None, None) == -1
    assert lib.hrt_debug_denoise_variance_state(None, None, None, None) == -1


def test_variance_layout(hrt, tmp_path):
    """HrtDenoiseVarianceParams is 16 bytes: checked by the C++ compiler against include/hrt.h, and the ctypes mirror agrees."""
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include "hrt.h"\n'
                   'static_assert(sizeof(HrtDenoiseVarianceParams) == 16 && offsetof(HrtDenoiseVarianceParams, history_min) == 4 &&'
                   ' offsetof(HrtDenoiseVarianceParams, variance_floor) == 8 && offsetof(HrtDenoiseVarianceParams, reserved) == 12,'
                   ' "variance params");\n'
                   'int main() { return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", f"-I{ROOT / 'include'}", str(src)], check=True)
    assert C.sizeof(hrt.DenoiseVarianceParams) == 16
    assert [getattr(hrt.DenoiseVarianceParams, f).offset for f in ("sigma_luminance", "history_min", "variance_floor", "reserved")] == [0, 4, 8, 12]


def _cam(hrt, scene):
    c = scene["camera"]
    u, v, w = hrt.configure_camera(c["center"], c["target"], c["up"], c.get("opengl", True))
    return (np.asarray(c["center"], np.float32), u, v, w)


def test_spec_constant_colour_has_zero_variance_and_is_kept(hrt, oracle):
    """A constant-colour sequence: the variance is 0 from the first frame (the spatial branch) on (the temporal one from frame 4),
    and the output equals the input, bit for bit.  The colour is the grey 0.5: l(c) = 0.5 and l * l = 0.25 are powers of two, so
    every weighted sum of them is the weight sum scaled and every mean is exact.  (For another colour the sums round, and "zero" and
    "equal" hold to a few ulps only: the specification's arithmetic is float32's, not the reals'.)"""
    w, h = 40, 32
    scene = hrt.scenes.cornell_box(w, h, 1)
    cam = _cam(hrt, scene)
    osc = oracle.OracleScene(scene)
    c = np.empty((h, w, 4), np.float32)
    c[...] = np.array([0.5, 0.5, 0.5, 1.0], np.float32)
    hist = None
    for k in range(6):
        diag = {}
        out, A, L, _, M, var, hist = vref.variance_frame(hist, c, osc, scene, cam, w, h, {"iterations": 3}, {"alpha_min": 0.1}, None, diag)
        hit = hist["inst"] != tref.MISS
        assert hit.sum() > 0.5 * w * h
        assert (diag["spatial"][hit].all() if k < 3 else diag["temporal"][hit].all()), k
        assert np.all(var == 0), (k, var.max())
        assert np.array_equal(dc.bits(out), dc.bits(c)), k
    osc.close()


def test_spec_variance_branches_follow_the_history_length(hrt, oracle):
    """A first call takes the spatial branch on every hit pixel; once the sequence is longer than history_min the pixels that keep
    their history take the temporal one, and the ones that lost it (L = 1 again) the spatial one."""
    w, h = 40, 32
    scene = hrt.scenes.cornell_box(w, h, 1)
    cam = _cam(hrt, scene)
    osc = oracle.OracleScene(scene)
    rng = np.random.default_rng(5)
    hist = None
    for k in range(5):
        diag = {}
        c = rng.uniform(0, 1, (h, w, 4)).astype(np.float32)
        _, _, L, _, M, var, hist = vref.variance_frame(hist, c, osc, scene, cam, w, h, {"iterations": 1}, None, {"history_min": 3}, diag)
        hit = hist["inst"] != tref.MISS
        assert not diag["temporal"][~hit].any() and not diag["spatial"][~hit].any() and np.all(var[~hit] == 0)
        if k == 0:
            assert diag["spatial"][hit].all() and np.all(L[hit] == 1)
            assert (diag["n"][hit] >= 1).all() and (diag["n"][hit] <= 25).all()
        if k >= 2:
            assert np.array_equal(diag["temporal"], hit & (L >= 3))
            assert diag["temporal"][hit].mean() > 0.9
            t = diag["temporal"]
            assert np.array_equal(var[t], np.fmax(f32(0), M[t][:, 1] - M[t][:, 0] * M[t][:, 0]))
    # a lost history: the same frame against a history of another instance everywhere
    bad = dict(hist)
    bad["inst"] = np.where(hist["inst"] != tref.MISS, hist["inst"] + np.uint32(1000), hist["inst"]).astype(np.uint32)
    diag = {}
    _, _, L, _, _, _, _ = vref.variance_frame(bad, c, osc, scene, cam, w, h, {"iterations": 1}, None, {"history_min": 3}, diag)
    assert np.all(L[hit] == 1) and diag["spatial"][hit].all()
    osc.close()


def test_spec_variance_of_a_uniform_region_shrinks_by_the_kernel():
    """One pass over a region where every tap has the centre's weight stops (equal colour and guides) and the variance v: each tap's
    weight is h[dx] h[dy], so var_out = v sum h^2 / (sum h)^2 = v (sum_i h_i^2)^2 = v * (35 / 128)^2 in the interior."""
    h, w = 9, 11
    c = np.full((h, w, 4), 0.5, np.float32)
    n = np.zeros((h, w, 3), np.float32)
    n[..., 2] = 1
    g = ref.pack_guides(n, np.full((h, w, 3), 0.5, np.float32), np.full((h, w), 2.0, np.float32))
    v = np.full((h, w), 0.01, np.float32)
    out, vo = vref.filter_variance(c, g, v, {"iterations": 1})
    assert np.array_equal(dc.bits(out), dc.bits(c))
    k2 = float((ref.H_B3.astype(np.float64) ** 2).sum()) ** 2
    assert k2 == (35 / 128) ** 2
    np.testing.assert_allclose(vo[2:-2, 2:-2], 0.01 * k2, rtol=1e-6)
    # at the frame's edge fewer taps count: the variance shrinks less
    assert vo[0, 0] > vo[4, 5]
    sw_corner = float(ref.H_B3[2:].astype(np.float64).sum()) ** 2
    np.testing.assert_allclose(vo[0, 0], 0.01 * float((ref.H_B3[2:].astype(np.float64) ** 2).sum()) ** 2 / sw_corner ** 2, rtol=1e-6)


def test_spec_luminance_stop_follows_the_variance():
    """Two halves of different luminance, one albedo, normal and depth: with a small variance the step survives, with a large one it is
    smoothed away -- the stop is measured in standard deviations."""
    h, w = 8, 16
    c = np.full((h, w, 4), 0.2, np.float32)
    c[:, w // 2:, :3] = 0.6
    n = np.zeros((h, w, 3), np.float32)
    n[..., 2] = 1
    g = ref.pack_guides(n, np.full((h, w, 3), 0.5, np.float32), np.full((h, w), 2.0, np.float32))
    sharp, _ = vref.filter_variance(c, g, np.full((h, w), 1e-6, np.float32), {"iterations": 3})
    soft, _ = vref.filter_variance(c, g, np.full((h, w), 1.0, np.float32), {"iterations": 3})
    step = lambda x: float(x[4, w // 2, 0] - x[4, w // 2 - 1, 0])
    assert step(sharp) > 0.39 and step(soft) < 0.1


# ---- the reach check ------------------------------------------------------------------------
def test_filter_cases_cover_the_listed_shapes_and_switches():
    got = [vc.filter_case(n) for n in vc.FILTER_CASES]
    sizes = {(c.shape[1], c.shape[0]) for c, *_ in got}
    assert set(vc.SIZES) <= sizes
    assert {p["iterations"] for _, _, _, p, *_ in got} >= set(vc.PASSES)
    assert {x[5] for x in got} == {True, False} and {x[6] for x in got} == {"set", "null", "same"}
    assert any(x[4] is None for x in got) and any(x[4] is not None for x in got)
    for w, h in vc.SIZES:                                       # every size with every pass count
        assert {vc.filter_case(f"plain-{w}x{h}-{it}")[3]["iterations"] for it in vc.PASSES} == set(vc.PASSES)
    v = vc.filter_case("hostile-variance")[2]
    assert (v == 0).any() and ((v > 0) & (v < dc.FLT_MIN)).any() and (v >= 1e30).any() and np.isinf(v).any() and np.isnan(v).any()
    c = vc.filter_case("hdr-negative")[0][..., :3]
    assert (np.abs(c) > 1e30).any() and (c < 0).any()
    z = ref.unpack_guides(vc.filter_case("holes")[1])[2]
    assert 0.2 < np.isinf(z).mean() < 0.6


def test_cases_reach_every_listed_branch(hrt, oracle, monkeypatch):
    """Over the GPU test's inputs each of these decides at least one output bit -- the output differs when the branch is taken away:
    both variance branches, a tap dropped from the spatial estimate for a foreign instance, the NaN -> 0 of fmax (over the launch
    sequences), and the 3x3 renormalisation at a frame corner (over the filter cases).  No listed branch may be unreached."""
    reached = {"temporal": 0, "spatial": 0, "foreign_instance": 0, "nan_to_zero": 0, "corner_renormalisation": 0}
    for name, seq in vc.sequences(hrt).items():
        hmin = vref._params(seq["vparams"])["history_min"]
        for f in vc.walk(hrt, oracle, name, seq, with_diag=True):
            d, M, L, inst = f["diag"], f["M"], f["L"], f["hist"]["inst"]
            # each branch against the other's value on its pixels
            other_t = vref.variance(M, np.zeros_like(L), inst, hmin)               # all spatial
            other_s = vref.variance(M, np.full_like(L, 1e9), inst, hmin)            # all temporal
            reached["temporal"] += int((dc.bits(f["var"]) != dc.bits(other_t))[d["temporal"]].sum())
            reached["spatial"] += int((dc.bits(f["var"]) != dc.bits(other_s))[d["spatial"]].sum())
            one_instance = np.where(inst != tref.MISS, np.uint32(0), inst).astype(np.uint32)
            reached["foreign_instance"] += int((dc.bits(f["var"]) != dc.bits(vref.variance(M, L, one_instance, hmin)))[d["spatial"]].sum())
            with_maximum = vref.variance(M, L, inst, hmin, fmax=np.maximum)         # (leaves a NaN there: another bit pattern)
            nan_to_zero = dc.bits(f["var"]) != dc.bits(with_maximum)
            reached["nan_to_zero"] += int(nan_to_zero.sum())
            assert np.array_equal(nan_to_zero, d["nan_to_zero"]) and np.all(f["var"][nan_to_zero] == 0)
    plain = vref.smoothed_variance

    def unnormalised(var, hit, diag=None):
        tmp = {}
        gv = plain(var, hit, tmp)
        with np.errstate(all="ignore"):
            return (gv * tmp["sgw"]).astype(np.float32)                           # (sum g var_q, but for a rounding)

    for name in vc.FILTER_CASES:
        c, g, v, p, vp, _, _ = vc.filter_case(name)
        h, w = v.shape
        if h < 2 or w < 2:
            continue
        diag = {}
        out, _ = vref.filter_variance(c, g, v, p, vp, diag)
        monkeypatch.setattr(vref, "smoothed_variance", unnormalised)
        alt, _ = vref.filter_variance(c, g, v, p, vp)
        monkeypatch.setattr(vref, "smoothed_variance", plain)
        for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
            if 0 < diag["sgw"][y, x] < 1 and not np.array_equal(dc.bits(out[y, x, :3]), dc.bits(alt[y, x, :3])):
                reached["corner_renormalisation"] += 1
    print(reached)
    assert all(v > 0 for v in reached.values()), reached


def test_spec_quality_at_4spp_beats_the_temporal_mode(hrt, oracle):
    """C1 at 64 x 48 rendered by the oracle, fixed seed, 8 static frames of 4 spp against 2048 spp: with every parameter at its default
    the variance-guided output's MSE is below the temporal mode's on the same frames.  Recorded ratio 0.755
    (profiles/r12_denoise_variance.txt), which is below the 0.9 that asks for this assertion."""
    w, h = 64, 48
    scene = hrt.scenes.cornell_box(w, h, 1)
    cam = _cam(hrt, scene)
    osc = oracle.OracleScene(scene)
    conv = osc.render(w, h, oracle.rng_init(w, h, hrt.scenes.SEED_SALT + 1), 2048)["color"][..., :3].astype(np.float64)
    states = oracle.rng_init(w, h, hrt.scenes.SEED_SALT)
    th = vh = None
    for _ in range(8):
        raw = osc.render(w, h, states, 4)["color"].copy()
        t_out, _, _, _, th = tref.temporal_frame(th, raw, osc, scene, cam, w, h)
        res = vref.variance_frame(vh, raw, osc, scene, cam, w, h)
        v_out, vh = res[0], res[6]
    osc.close()
    mse_t = ((t_out[..., :3].astype(np.float64) - conv) ** 2).mean()
    mse_v = ((v_out[..., :3].astype(np.float64) - conv) ** 2).mean()
    print(f"c1 64x48 4 spp x 8: mse temporal {mse_t:.6g} variance {mse_v:.6g} ratio {mse_v / mse_t:.4f}")
    assert mse_v < mse_t
