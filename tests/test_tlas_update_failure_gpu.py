"""A refused hrt_tlas_update leaves the TLAS as it was.  build_tlas_into builds the new tree on the side and lets it take the old one's
place only when everything has succeeded; on the way it moves the tree's pinned host words and its event into the new tree, and back when
the build fails.  Here the build fails on the host, before any kernel runs: one instance names a traversable that is not a BLAS.  The call
returns an error that says so, the statistics do not move, the tree still renders the frame it rendered before, bit for bit, and the next
valid update works -- in every structure hrt_tlas_build makes for such a scene: flattened, over instances, two levels."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_PARTICLES, W, H, SPP, SALT = 25, 32, 32, 1, 4242


def _frame(r):
    r.set_frame(W, H, SALT, linear=True)      # (re-seeds the RNG states)
    r.render(SPP)
    return r.linear.cpu().numpy().copy()


@pytest.mark.parametrize("structure", ["flattened", "over-instances", "two-level"])
def test_refused_update_leaves_the_tlas_valid_and_traceable(hrt, oracle, gpu_available, monkeypatch, structure):
    if not gpu_available:
        pytest.skip("no GPU")
    if structure == "over-instances":
        monkeypatch.setenv("HRT_TLAS_INSTANCED", "1")
    r = hrt.Renderer(0, hrt.CTX_TWO_LEVEL if structure == "two-level" else 0)
    try:
        scene = hrt.scenes.particle_scene(N_PARTICLES, W, H, SPP)
        r.load_scene(scene)
        n = len(scene["instances"])
        first = _frame(r)
        before = r.stats()
        # the instance array with one traversable that is no BLAS (the TLAS's own handle), in device memory of its own
        bad = (hrt.Instance * n).from_buffer_copy(bytes(r._h_inst))
        bad[n // 2].traversableHandle = r.tlas
        d_bad = r._dev(np.frombuffer(bytes(bad), dtype=np.uint8).copy())
        rc = r.lib.hrt_tlas_update(r.ctx, r.tlas, d_bad.data_ptr(), n, r._stream())
        assert rc < 0, rc
        assert "BLAS" in r.lib.hrt_last_error(r.ctx).decode()
        after = r.stats()
        assert (after.tlas_refits, after.tlas_rebuilds) == (before.tlas_refits, before.tlas_rebuilds)
        assert (after.bvh_nodes, after.bvh_triangles, after.bvh_spheres, after.bvh_depth) == (before.bvh_nodes, before.bvh_triangles, before.bvh_spheres, before.bvh_depth)
        assert np.array_equal(_frame(r).view(np.uint32), first.view(np.uint32))
        # a valid update afterwards: the particles two frames on
        moved = hrt.scenes.particle_scene(N_PARTICLES, W, H, SPP, frame=2)
        r.update_instances([it["transform"] for it in moved["instances"]])
        done = r.stats()
        assert done.tlas_refits + done.tlas_rebuilds == before.tlas_refits + before.tlas_rebuilds + 1
        ref = oracle.OracleScene(moved, instanced=structure == "two-level").render(W, H, oracle.rng_init(W, H, SALT), SPP)
        assert np.array_equal(_frame(r).view(np.uint32), ref["linear"].view(np.uint32))
    finally:
        r.close()
