"""The denoiser's accumulated mode without a GPU (include/hrt.h "Accumulated mode"): the numpy specification
(tests/denoise_accumulated_ref.py) reaches every branch of the definition on the named cases (tests/denoise_accumulated_cases.py) that
tests/test_denoise_accumulated_gpu.py runs the kernels on, and has the properties the mode is for; the library exports the two calls and
Renderer has the two methods; and csrc/denoise_accum.hip compiles to one kernel that uses no scratch."""
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import denoise_accumulated_cases as ac
import denoise_accumulated_ref as aref
import denoise_cases as dc
import denoise_ref as ref
import sample_counts_ref as sref

ROOT = Path(__file__).resolve().parent.parent
SOURCE = "nvidia-optix-ray-tracer_amd/csrc/denoise_accum.hip"
f32 = np.float32


@pytest.fixture(scope="module")
def prepared():
    """name -> (case, (mean, var, guides'), diag) of every named case, computed once"""
    out = {}
    for name in ac.CASES:
        c = ac.case(name)
        diag = {}
        out[name] = (c, aref.prepare(c[0], c[1], c[2], c[4], diag), diag)
    return out


def _hmin(c):
    return (c[4] or {}).get("history_min", 4)


def test_case_table_covers_what_it_names(prepared):
    names = set(ac.CASES)
    assert {f"{k}-{w}x{h}" for k in ac.TAKEN_MAPS for w, h in ac.SIZES} <= names
    grid = [c for n, (c, _, _) in prepared.items() if n.split("-")[0] in [t.split("-")[0] for t in ac.TAKEN_MAPS] and "x" in n]
    assert {c[3]["iterations"] for c in grid} == set(ac.PASSES)
    assert {_hmin(c) for c, _, _ in prepared.values()} == set(ac.HISTORY_MIN)
    assert {c[5] for c in grid} == {"set", "null"} and {c[6] for c in grid} == {"set", "null"}
    assert {(c[5], c[6]) for c in grid} == {("set", "set"), ("set", "null"), ("null", "set"), ("null", "null")}
    for name in ac.GROW_SHRINK:
        assert name in names
    for w, h in ac.SIZES:                                    # every value of the mixed map, where the frame has room for them
        t = prepared[f"mixed-{w}x{h}"][0][1]
        assert set(ac.MIXED[: t.size].tolist()) <= set(t.reshape(-1).tolist())


def test_every_branch_is_reached(prepared):
    """The union of the cases' branch counters, then the cases that are there for one branch each."""
    total = {}
    for _, _, d in prepared.values():
        for k in ("unsampled", "one", "many", "background", "turned", "own", "spatial", "clipped", "nan_to_zero", "negative_to_zero"):
            total[k] = total.get(k, 0) + int(d[k].sum())
    assert all(v > 0 for v in total.values()), total
    nan_own = sum(int((d["nan_to_zero"] & d["own"]).sum()) for _, _, d in prepared.values())
    nan_spatial = sum(int((d["nan_to_zero"] & d["spatial"]).sum()) for _, _, d in prepared.values())
    neg_own = sum(int((d["negative_to_zero"] & d["own"]).sum()) for _, _, d in prepared.values())
    assert nan_own > 0 and nan_spatial > 0 and neg_own > 0, (nan_own, nan_spatial, neg_own)
    # a background pixel that holds samples (a true miss) keeps its mean and has no variance
    assert any((d["background"] & ~d["unsampled"]).any() for _, _, d in prepared.values())
    # inf and NaN in xyz and in w, subnormal sums, w smaller than m1^2 n: as a pixel's own moments and as taps of a block
    for name in ("synthetic-hmin4", "synthetic-hmin65536"):
        (s, t, *_), _, d = prepared[name]
        sampled = t > 0
        assert (np.isinf(s[..., :3]).any(-1) & sampled).any() and (np.isnan(s[..., :3]).any(-1) & sampled).any()
        assert (np.isinf(s[..., 3]) & sampled).any() and (np.isnan(s[..., 3]) & sampled).any()
        assert ((np.abs(s[..., 0]) < dc.FLT_MIN) & (s[..., 0] != 0) & sampled).any()
    far = prepared["synthetic-hmin65536"]
    assert prepared["synthetic-hmin4"][2]["own"].sum() > 100 and far[2]["spatial"].sum() > 300
    assert not (far[2]["own"] & (far[0][1] < 65536)).any()
    assert prepared["negative"][2]["negative_to_zero"].sum() >= 12


def test_history_min_one_still_needs_two_samples(prepared):
    """history_min 1 reads as 2: a pixel with one sample has no variance of its own."""
    hits = 0
    for name, (c, _, d) in prepared.items():
        if _hmin(c) == 1:
            assert not (d["own"] & d["one"]).any(), name
            hits += int((d["spatial"] & d["one"]).sum())
    assert hits > 0
    c, _, d = prepared["hmin-5x3"]
    assert _hmin(c) == 1 and (c[1] == 1).all() and d["spatial"].any() and not d["own"].any()
    # ... and with history_min 2 and 4 a pixel that holds exactly that many is believed
    for name, (c, _, d) in prepared.items():
        if name.startswith("hmin-") and _hmin(c) in (2, 4):
            assert not d["spatial"].any() and (d["own"] | d["background"]).all(), name


def test_zero_frames_are_black_background(prepared, oracle):
    for w, h in ac.SIZES:
        c, (mean, var, g2), d = prepared[f"zero-{w}x{h}"]
        assert d["background"].all() and not var.any() and not mean[..., :3].any() and (mean[..., 3] == 1).all()
        out, linear, var_out = aref.denoise_accumulated(c[0], c[1], c[2], c[3], c[4])
        assert np.array_equal(out, np.broadcast_to(np.array([0, 0, 0, 1], np.float32), out.shape)) and not var_out.any()
        assert np.array_equal(dc.bits(linear), dc.bits(mean))


def test_island_has_one_tap_and_no_variance(prepared):
    for w, h in ac.SIZES:
        c, (mean, var, g2), d = prepared[f"island-{w}x{h}"]
        y, x = h // 2, w // 2
        assert d["spatial"][y, x] and d["spatial"].sum() == 1 and d["k"][y, x] == 1 and var[y, x] == 0
        assert np.array_equal(dc.bits(mean[y, x, :3]), dc.bits(c[0][y, x, :3]))


def test_young_pixels_sit_in_every_corner_and_on_every_edge(prepared):
    w, h = 37, 29
    c, (mean, var, g2), d = prepared[f"young-edges-{w}x{h}"]
    assert _hmin(c) != 65536
    pos = ac.young_positions(h, w)
    assert len(pos) == 8
    for y, x in pos:
        assert d["spatial"][y, x] and d["clipped"][y, x], (y, x)
        rows, cols = min(y, 2) + min(h - 1 - y, 2) + 1, min(x, 2) + min(w - 1 - x, 2) + 1
        assert 1 < d["k"][y, x] <= rows * cols < 25, (y, x, d["k"][y, x])
    assert (d["k"][0, 0] == 9) == bool(np.isfinite(ref.unpack_guides(g2)[2][:3, :3]).all())
    assert d["own"].sum() > 0.7 * w * h
    # (the smaller frames clip the block on both sides at once)
    for ww, hh in ((2, 1), (5, 3), (17, 5)):
        d2 = prepared[f"young-edges-{ww}x{hh}"][2]
        assert d2["clipped"].any() and d2["k"].max() <= min(ww, 5) * min(hh, 5)


def test_stripe_rows_outside_are_background(prepared, oracle):
    w, h = 37, 29
    c, (mean, var, g2), d = prepared[f"stripe-{w}x{h}"]
    rows = list(ac.stripe_rows(h))
    outside = np.ones(h, bool)
    outside[rows] = False
    assert d["background"][outside].all() and d["turned"][outside].any() and not d["unsampled"][rows].any()
    out, linear, _ = aref.denoise_accumulated(*c[:5])
    assert np.array_equal(out[outside], np.broadcast_to(np.array([0, 0, 0, 1], np.float32), out[outside].shape))
    # the taps stop at the stripe's edge: the stripe alone, cut out of the frame, filters to the same bits
    cut = aref.denoise_accumulated(c[0][rows], c[1][rows], c[2][rows], c[3], c[4])
    assert dc.same_rgba(out[rows], cut[0]) and dc.same_rgba(linear[rows], cut[1])


def test_believed_pixels_take_the_allocators_variance():
    """Every total >= max(history_min, 2) on an all-hit frame: var is hrt_sample_counts' variance over n, bit for bit, and the guides pass
    through untouched."""
    for hmin, (w, h) in ((1, (17, 5)), (4, (37, 29))):
        s, t, g = ac.full_frame(w, h, 1000 + hmin, max(hmin, 2))
        diag = {}
        mean, var, g2 = aref.prepare(s, t, g, {"history_min": hmin}, diag)
        assert diag["own"].all()
        with np.errstate(all="ignore"):
            want = (sref.variance(s, t) / t.astype(np.float32)).astype(np.float32)
        assert dc.same(var, want) and (var > 0).any()
        assert np.array_equal(g2, g)
        assert np.array_equal(dc.bits(mean[..., :3]), dc.bits(sref.mean(s, t))) and (mean[..., 3] == 1).all()


@pytest.mark.parametrize("name", ["mixed-37x29", "stripe-37x29", "synthetic-hmin65536", "mixed-5x3"])
def test_an_unsampled_pixel_changes_no_other(prepared, oracle, name):
    """Whatever the sum of a pixel without a sample holds -- NaN, infinities, large values -- the frame's result is the same."""
    c = prepared[name][0]
    s, t = c[0], c[1]
    assert (t == 0).any() and (t != 0).any()
    want = aref.denoise_accumulated(s, t, *c[2:5])
    for fill in (np.nan, np.inf, 3e38, 0.0):
        s2 = s.copy()
        s2[t == 0] = f32(fill)
        got = aref.denoise_accumulated(s2, t, *c[2:5])
        assert dc.same_rgba(got[0], want[0]) and dc.same_rgba(got[1], want[1]) and dc.same(got[2], want[2]), fill
    assert np.array_equal(want[0][t == 0], np.broadcast_to(np.array([0, 0, 0, 1], np.float32), want[0][t == 0].shape))


def test_filter_runs_on_linear_radiance_and_encodes_last(prepared, oracle):
    """The output is colorToFloat4 of the filtered linear frame -- not the filter of the encoded mean."""
    import denoise_variance_ref as vref
    c, (mean, var, g2), _ = prepared["mixed-37x29"]
    out, linear, var_out = aref.denoise_accumulated(*c[:5])
    want_linear, want_var = vref.filter_variance(mean, g2, var, c[3], c[4])
    assert dc.same_rgba(linear, want_linear) and dc.same(var_out, want_var) and dc.same_rgba(out, aref.encode(linear))
    other, _ = vref.filter_variance(aref.encode(mean), g2, var, c[3], c[4])
    assert not dc.same_rgba(out, other)


# ---- the library ------------------------------------------------------------------------------
def test_library_exports_the_mode(hrt):
    lib = hrt.load_library()
    for name in ("hrt_denoise_accumulated_filter", "hrt_denoise_accumulated_launch"):
        assert name in hrt.EXPORTS and hasattr(lib, name), name
    for name in ("denoise_accumulated_filter", "denoise_accumulated"):
        assert callable(getattr(hrt.Renderer, name, None)), name
    assert lib.hrt_denoise_accumulated_filter(None, None, None, None, None, None, None, 1, 1, None, None, None) == -1
    assert lib.hrt_denoise_accumulated_launch(None, None, None, None, None, None, None, None, None) == -1
    header = (ROOT / "include" / "hrt.h").read_text()
    assert "samples a pixel needs before its own moments are believed" in header


# ---- the kernel -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{mangled kernel name: {metadata key: int}} of csrc/denoise_accum.hip, compiled with the Makefile's flags (in the manner of
    tests/test_denoise_kernels_cpu.py)"""
    sys.path.insert(0, str(ROOT / "tools"))
    from audit_asm_loads import makefile_hipflags
    asm = tmp_path_factory.mktemp("denoise_accum") / "denoise_accum.s"
    flags = [f for f in makefile_hipflags() if f != "-fPIC"]
    subprocess.check_call(["/opt/rocm/bin/hipcc", *flags, "-S", "--cuda-device-only", "-o", str(asm), SOURCE], cwd=ROOT, stderr=subprocess.DEVNULL)
    out = {}
    for entry in asm.read_text().split("amdhsa.kernels:")[1].split("\n  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", entry).group(1)
        out[name] = {k: int(v) for k, v in re.findall(r"^    \.(\w+):\s+(\d+)\s*$", entry, re.M)}
    return out


def test_one_kernel_without_scratch(kernels):
    assert len(kernels) == 1 and "k_denoise_accumulated" in next(iter(kernels)), sorted(kernels)
    (meta,) = kernels.values()
    assert meta["private_segment_fixed_size"] == 0, meta
    assert meta["vgpr_count"] <= 64, meta                    # eight waves per SIMD: the kernel streams 72 B per pixel and hides it with waves


def test_makefile_builds_the_unit_into_the_library():
    mk = (ROOT / "Makefile").read_text()
    other = re.search(r"^OTHER_OBJS := .*$", mk, re.M).group(0)
    assert "denoise_accum.o" in other and "$(LIBDIR)/denoise_accum.o: $(CSRC)/denoise_accum.hip" in mk
