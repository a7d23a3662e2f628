"""The denoiser without a GPU: its C ABI refuses to run (no CPU path) and checks its arguments, its public layouts, and properties of
the numpy specification (tests/denoise_ref.py) that the GPU tests pin the kernels to."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import denoise_ref as ref

ROOT = Path(__file__).resolve().parent.parent


def test_denoise_entry_points_refuse_without_a_device_and_check_arguments(hrt):
    lib = hrt.load_library()
    ctx = C.c_void_p()
    assert lib.hrt_ctx_create(0, 0, C.byref(ctx)) == -2            # HRT_ERR_NO_DEVICE: no context, hence no denoiser
    p = hrt.DenoiseParams()
    assert lib.hrt_denoise_default_params(C.byref(p)) == 0
    assert (p.iterations, p.normal_power_log2, p.reserved) == (ref.DEFAULTS["iterations"], ref.DEFAULTS["normal_power_log2"], 0)
    for k in ("sigma_color", "sigma_albedo", "sigma_depth"):
        assert getattr(p, k) == np.float32(ref.DEFAULTS[k])
    assert lib.hrt_denoise_default_params(None) == -1
    gp, rg = hrt.GlobalParams(), hrt.RayGenParams()
    assert lib.hrt_denoise_guides(None, C.byref(gp), C.byref(rg), C.c_void_p(16), None) == -1
    assert lib.hrt_denoise_filter(None, C.c_void_p(16), C.c_void_p(16), C.c_void_p(16), 4, 4, None, None) == -1
    assert lib.hrt_denoise_launch(None, C.byref(gp), C.byref(rg), None, C.c_void_p(16), None) == -1


def test_denoise_layouts(hrt, tmp_path):
    """HrtDenoiseGuide is 16 bytes (normal, albedo as halves, depth at byte 12), HrtDenoiseParams 24: checked by the C++ compiler
    against include/hrt.h, and the ctypes mirror agrees."""
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include "hrt.h"\n'
                   'static_assert(sizeof(HrtDenoiseGuide) == 16 && offsetof(HrtDenoiseGuide, albedo) == 6 && offsetof(HrtDenoiseGuide, depth) == 12, "guide");\n'
                   'static_assert(sizeof(HrtDenoiseParams) == 24 && offsetof(HrtDenoiseParams, normal_power_log2) == 16, "params");\n'
                   'int main() { return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", f"-I{ROOT / 'include'}", str(src)], check=True)
    assert C.sizeof(hrt.DenoiseParams) == 24 and hrt.DENOISE_GUIDE_BYTES == 16


def _guides(h, w, normal, albedo=(0.5, 0.5, 0.5), depth=1.0):
    n = np.broadcast_to(np.asarray(normal, np.float32), (h, w, 3))
    a = np.broadcast_to(np.asarray(albedo, np.float32), (h, w, 3))
    return ref.pack_guides(n, a, np.full((h, w), depth, np.float32))


def test_guide_records_round_trip():
    rng = np.random.default_rng(3)
    n = rng.uniform(-1, 1, (5, 7, 3)).astype(np.float32)
    a = rng.uniform(0, 1, (5, 7, 3)).astype(np.float32)
    z = rng.uniform(0.1, 9, (5, 7)).astype(np.float32)
    z[0, 0] = np.inf
    g = ref.pack_guides(n, a, z)
    assert g.shape == (5, 7, 8) and g.dtype == np.uint16 and g.nbytes == 16 * 35
    n2, a2, z2 = ref.unpack_guides(g)
    assert np.array_equal(n2, n.astype(np.float16).astype(np.float32)) and np.array_equal(a2, a.astype(np.float16).astype(np.float32))
    assert np.array_equal(z2.view(np.uint32), z.view(np.uint32))


@pytest.mark.parametrize("iterations", [1, 3, 5])
def test_spec_regions_across_a_normal_discontinuity_do_not_mix(iterations):
    """Two regions whose normals face apart (n . n' <= 0 gives wn = 0): changing the colours of one leaves the other's output bit-identical."""
    h, w = 24, 40
    g = _guides(h, w, (0, 0, 1))
    nrm = ref.unpack_guides(g)[0].copy()
    right = np.zeros((h, w), bool)
    right[:, 17:] = True
    g2 = ref.pack_guides(np.where(right[..., None], np.array([1, 0, 0], np.float32), nrm), ref.unpack_guides(g)[1], ref.unpack_guides(g)[2])
    rng = np.random.default_rng(iterations)
    c1 = rng.uniform(0, 1, (h, w, 4)).astype(np.float32)
    c2 = c1.copy()
    c2[right] = rng.uniform(0, 4, (int(right.sum()), 4)).astype(np.float32)
    o1 = ref.atrous(c1, g2, {"iterations": iterations})
    o2 = ref.atrous(c2, g2, {"iterations": iterations})
    assert np.array_equal(o1[~right].view(np.uint32), o2[~right].view(np.uint32))
    assert not np.array_equal(o1[right], o2[right])
    assert not np.array_equal(o1[~right], c1[~right])              # ... and the region itself was filtered


def test_spec_misses_pass_through():
    h, w = 19, 23
    rng = np.random.default_rng(5)
    n = rng.normal(size=(h, w, 3)).astype(np.float32)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    z = rng.uniform(0.5, 2, (h, w)).astype(np.float32)
    miss = rng.uniform(size=(h, w)) < 0.3
    z[miss] = np.inf
    z[0, :3] = (0.0, -1.0, np.nan)                                  # depth outside (0, inf): background too
    miss[0, :3] = True
    g = ref.pack_guides(n, rng.uniform(size=(h, w, 3)), z)
    c = rng.uniform(0, 1, (h, w, 4)).astype(np.float32)
    out = ref.atrous(c, g, {"iterations": 4})
    assert np.array_equal(out[miss].view(np.uint32), c[miss].view(np.uint32))
    assert np.array_equal(out[..., 3].view(np.uint32), c[..., 3].view(np.uint32))      # alpha is the centre's everywhere
    assert not np.array_equal(out[~miss], c[~miss])


@pytest.mark.parametrize("value", [0.0, 0.25, 0.7071, 1.0, 3.3])
def test_spec_constant_region_keeps_its_value(value):
    """Uniform guides and a constant colour: the weighted mean is the value itself; only the rounding of the float32 sums remains."""
    h, w = 21, 33
    g = _guides(h, w, (0.6, 0.0, 0.8), depth=2.5)
    c = np.full((h, w, 4), value, np.float32)
    c[..., 3] = 1.0
    out = ref.atrous(c, g, {"iterations": 5})
    ulp = np.abs(out[..., :3].view(np.int32).astype(np.int64) - c[..., :3].view(np.int32).astype(np.int64))
    assert ulp.max() <= 32, ulp.max()


def test_spec_smooths_noise_on_a_plane():
    """On a plane with uniform guides the filter is a blur: the noise of a noisy constant image shrinks."""
    h, w = 64, 64
    g = _guides(h, w, (0, 0, 1))
    rng = np.random.default_rng(11)
    c = np.full((h, w, 4), 0.5, np.float32) + rng.normal(0, 0.1, (h, w, 4)).astype(np.float32)
    out = ref.atrous(c, g)
    assert np.std(out[..., :3] - 0.5) < 0.25 * np.std(c[..., :3] - 0.5)
