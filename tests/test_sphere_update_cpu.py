"""hrt_blas_update_spheres (include/hrt.h: OPTIX_BUILD_OPERATION_UPDATE for a sphere GAS) without a GPU: the symbol and its signature,
the refusal that needs no device, the host mirrors, and that the scenes of tests/test_sphere_update_gpu.py ask a real question."""
import ctypes as C
import re
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
MISS = 0xFFFFFFFF


def test_symbol_is_exported_with_the_documented_signature(hrt):
    lib = hrt.load_library()
    assert "hrt_blas_update_spheres" in hrt.EXPORTS
    fn = lib.hrt_blas_update_spheres                 # (without the feature: AttributeError at this lookup)
    assert fn.restype is C.c_int
    assert fn.argtypes == [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    header = (ROOT / "include" / "hrt.h").read_text()
    decl = re.search(r"int\s+hrt_blas_update_spheres\s*\(([^)]*)\)\s*;", header)
    assert decl, "include/hrt.h declares it"
    args = [re.sub(r"\s+", " ", a).strip() for a in decl.group(1).split(",")]
    assert args == ["HrtContext *ctx", "HrtTraversable blas", "const HrtFloat3 *d_centers", "const float *d_radii", "uint32_t n_spheres", "void *stream"]
    assert "Sphere BLASes have no update" not in header


def test_null_context_is_refused(hrt):
    lib = hrt.load_library()
    assert lib.hrt_blas_update_spheres(None, 0x1000, None, None, 0, None) == -1          # HRT_ERR_INVALID
    assert lib.hrt_blas_update_spheres(None, 0x1000, None, None, 3, None) == -1


def test_host_mirrors_exist(hrt):
    assert callable(getattr(hrt.Renderer, "update_blas_spheres"))
    hpp = (ROOT / "nvidia-optix-ray-tracer_amd" / "csrc" / "host" / "renderer_host.hpp").read_text()
    assert re.search(r"inline\s+void\s+updateGASForSpheres\s*\(\s*HrtContext\s*\*ctx,\s*const GAS &gas,\s*const RendererSphere &\w+,\s*hipStream_t stream", hpp)
    assert "hrt_blas_update_spheres" in hpp
    assert "hrt_blas_update_spheres" in (ROOT / "INTEGRATION.md").read_text()


def test_the_motion_moves_what_the_rays_see(oracle):
    """With the oracle alone: the scene is the one the issue describes, at least 30 % of the rays hit both before and after the 2 % motion,
    and the hit records differ -- so a renderer that missed the update could not pass the GPU tests by accident."""
    import sphere_update_cases as sc
    spheres, xf = sc.state("base")
    assert [c.shape for c, _ in spheres] == [(40, 3), (700, 3), (5000, 3)] and [r.shape for _, r in spheres] == [(40,), (700,), (5000,)]
    assert sc.BLAS_OF_INSTANCE.count(1) == 2 and [it["shape"] for it in sc.scene_of("base")["instances"]] == list(sc.BLAS_OF_INSTANCE)
    assert len({tuple(m) for m in xf}) == len(xf) and not any(np.array_equal(m, sc.scenes.IDENTITY) for m in xf)
    for which in (1, 2):
        for c, r in spheres:
            c2, r2 = sc.move(c, r, which)
            d = np.abs(c2.astype(np.float64) - c)
            extent = (c.max(axis=0) - c.min(axis=0)).max()
            assert 0.0 < d.max() <= 0.0201 * extent and d.mean() > 0.002 * extent
            assert (r2 > 0).all() and (np.abs(r2 / r - 1.0) <= 0.1001).all() and (r2 != r).mean() > 0.9
    for instanced in (False, True):
        before, after = sc.reference("base", instanced)["hits"], sc.reference("moved", instanced)["hits"]
        both = (before[3] != MISS) & (after[3] != MISS)
        assert both.mean() >= 0.30, both.mean()
        moved = before[0].view(np.uint32)[both] != after[0].view(np.uint32)[both]
        assert moved.mean() > 0.9, moved.mean()
        for b in range(3):                                   # ... in every BLAS, through every instance
            for i in [k for k, s in enumerate(sc.BLAS_OF_INSTANCE) if s == b]:
                assert (both & (before[4] == i)).sum() > 50
    # the ray bundle of the non-finite case finds its sphere while it is finite, and never while it is NaN or has an infinite radius
    o, d = sc.rays_at_nan_prim()
    fin = oracle.OracleScene(sc.scene_of("base"), force_brute=True).trace(o, d)
    assert ((fin[3] == sc.NAN_PRIM) & (fin[4] == 0)).sum() >= 1
    for name in ("nan_built", "inf_after"):
        gone = sc.reference(name, False, True)["hits"]
        assert not ((gone[3] == sc.NAN_PRIM) & (gone[4] == 0)).any(), name
    c, r = sc.state("inf_after")[0][0]
    assert np.isfinite(c).all() and np.isinf(r[sc.NAN_PRIM]) and np.isnan(sc.state("nan_after")[0][0][0][sc.NAN_PRIM]).all()
