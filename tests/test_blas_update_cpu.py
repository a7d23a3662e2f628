"""hrt_blas_update_triangles (include/hrt.h: OPTIX_BUILD_OPERATION_UPDATE for a triangle GAS) without a GPU: the symbol and its
signature, the refusal that needs no device, the host mirrors, and that the scenes of tests/test_blas_update_gpu.py ask a real question."""
import ctypes as C
import re
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent


def test_symbol_is_exported_with_the_documented_signature(hrt):
    lib = hrt.load_library()
    assert "hrt_blas_update_triangles" in hrt.EXPORTS
    fn = lib.hrt_blas_update_triangles               # (without the feature: AttributeError at this lookup)
    assert fn.restype is C.c_int
    assert fn.argtypes == [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p]
    header = (ROOT / "include" / "hrt.h").read_text()
    decl = re.search(r"int\s+hrt_blas_update_triangles\s*\(([^)]*)\)\s*;", header)
    assert decl, "include/hrt.h declares it"
    args = [re.sub(r"\s+", " ", a).strip() for a in decl.group(1).split(",")]
    assert args == ["HrtContext *ctx", "HrtTraversable blas", "const HrtFloat3 *d_vertices", "uint32_t n_vertices", "void *stream"]


def test_null_context_is_refused(hrt):
    lib = hrt.load_library()
    assert lib.hrt_blas_update_triangles(None, 0x1000, None, 0, None) == -1          # HRT_ERR_INVALID
    assert lib.hrt_blas_update_triangles(None, 0x1000, None, 3, None) == -1


def test_host_mirrors_exist(hrt):
    assert callable(getattr(hrt.Renderer, "update_blas_vertices"))
    hpp = (ROOT / "nvidia-optix-ray-tracer_amd" / "csrc" / "host" / "renderer_host.hpp").read_text()
    assert re.search(r"inline\s+void\s+updateGASForTriangles\s*\(\s*HrtContext\s*\*ctx,\s*const GAS &gas,\s*const RendererTriangle &\w+,\s*hipStream_t stream", hpp)
    assert "hrt_blas_update_triangles" in hpp
    assert "hrt_blas_update_triangles" in (ROOT / "INTEGRATION.md").read_text()


def test_the_deformation_moves_what_the_rays_see(oracle):
    """With the oracle alone: the scene is the one the issue describes, at least 30 % of the rays hit both before and after the 2 %
    deformation, and the hit records differ -- so a renderer that missed the update could not pass the GPU tests by accident."""
    import blas_update_cases as bc
    verts, xf = bc.state("base")
    assert [v.shape[0] for v in verts] == [96, 700, 5000] and bc.BLAS_OF_INSTANCE.count(1) == 2
    assert len({tuple(m) for m in xf}) == len(xf) and not any(np.array_equal(m, bc.scenes.IDENTITY) for m in xf)
    for which in (1, 2):
        for v in verts:
            d = np.abs(bc.deform(v, which).astype(np.float64) - v).reshape(-1, 3)
            extent = (v.reshape(-1, 3).max(axis=0) - v.reshape(-1, 3).min(axis=0)).max()
            assert 0.0 < d.max() <= 0.0201 * extent and d.mean() > 0.002 * extent
    for instanced in (False, True):
        before, after = bc.reference("base", instanced)["hits"], bc.reference("deformed", instanced)["hits"]
        both = (before[3] != 0xFFFFFFFF) & (after[3] != 0xFFFFFFFF)
        assert both.mean() >= 0.30, both.mean()
        moved = before[0].view(np.uint32)[both] != after[0].view(np.uint32)[both]
        assert moved.mean() > 0.9, moved.mean()
        for b in range(3):                                   # ... in every BLAS, through every instance
            for i in [k for k, s in enumerate(bc.BLAS_OF_INSTANCE) if s == b]:
                assert (both & (before[4] == i)).sum() > 50
    # the ray bundle of the non-finite case finds its triangle while it is finite, and never while it is NaN
    o, d = bc.rays_at_nan_prim()
    fin = oracle.OracleScene(bc.scene_of("base"), force_brute=True).trace(o, d)
    nan = bc.reference("nan_built", False, True)["hits"]
    assert ((fin[3] == bc.NAN_PRIM) & (fin[4] == 0)).sum() >= 1 and not ((nan[3] == bc.NAN_PRIM) & (nan[4] == 0)).any()
