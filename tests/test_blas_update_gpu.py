"""hrt_blas_update_triangles on the GPU: a deformed mesh keeps its BLAS handle, and the next hrt_tlas_update of every TLAS over it picks the
new vertices up -- by a refit where the tree holds every primitive as a record of its own, by a rebuild elsewhere.

"Equal" (_equal) is three things: the hit records (t, u, v, primitive, instance) of 20000 rays are bit-identical to the oracle's brute
force over the deformed scene, in the oracle mode the tree structure is pinned to (two-level: INSTANCED, else FLATTENED, as
tests/test_two_level_gpu.py chooses); linear radiance, colour and RNG states of a 48 x 32 frame at 2 spp are bit-identical to the oracle's
render of it; and all of these are identical to a fresh Renderer of the same flags that loaded the deformed scene.  The scene, the
deformations and the oracle's results (computed once per state and mode) are tests/blas_update_cases.py's; four instances stand over
the three BLASes because the 700-triangle one is shared by two."""
import ctypes as C

import numpy as np
import pytest

import blas_update_cases as bc

pytestmark = pytest.mark.gpu


def _renderer(hrt, gpu_available, flags=0, state="base"):
    if not gpu_available:
        pytest.skip("no GPU in this container")
    r = hrt.Renderer(0, flags)
    r.load_scene(bc.scene_of(state))
    return r


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _observe(r, rays=None):
    """hit records of the ray set, then a frame from fresh RNG states"""
    o, d = rays if rays is not None else bc.rays()
    hits = r.trace_rays(o, d)
    r.set_frame(bc.W, bc.H, bc.SALT, linear=True)
    r.render(bc.SPP)
    return {"hits": hits, "linear": r.linear.cpu().numpy(), "color": r.color.cpu().numpy(), "states": r.rng_states_numpy()}


def _same(got, ref, what):
    for k, name in enumerate(("t", "u", "v", "prim", "inst")):
        assert np.array_equal(_bits(got["hits"][k]), _bits(ref["hits"][k])), f"{what}: {name} of the hit records"
    for key in ("linear", "color", "states"):
        assert np.array_equal(_bits(got[key]), _bits(ref[key])), f"{what}: {key}"


def _equal(hrt, r, flags, state, nan_rays=False):
    got = _observe(r, bc.rays_at_nan_prim() if nan_rays else None)
    _same(got, bc.reference(state, bool(flags & hrt.CTX_TWO_LEVEL), nan_rays), "against the oracle")
    fresh = hrt.Renderer(0, flags)
    try:
        fresh.load_scene(bc.scene_of(state))
        _same(got, _observe(fresh, bc.rays_at_nan_prim() if nan_rays else None), "against a fresh renderer")
    finally:
        fresh.close()
    return got


def _deform_all(r, state):
    """every BLAS of the renderer's scene to `state`'s vertices, each named through one of its instances"""
    verts, _ = bc.state(state)
    for b, i in enumerate(bc.INSTANCE_OF_BLAS):
        r.update_blas_vertices(i, verts[b])


def _counts(r):
    s = r.stats()
    return int(s.tlas_refits), int(s.tlas_rebuilds)


def _refit_cases(hrt, gpu_available, flags):
    """Cases 1, 3 and 4: an update of unchanged transforms (the first refit after the build; under HRT_CTX_ASYNC_UPDATE the synchronous one
    that the asynchronous path follows), then deformation + update: equal, and a REFIT; then another deformation with moved instances
    in the same update."""
    r = _renderer(hrt, gpu_available, flags)
    try:
        r.update_instances(bc.state("base")[1])
        before = _counts(r)
        _deform_all(r, "deformed")
        r.update_instances(bc.state("deformed")[1])
        assert _counts(r) == (before[0] + 1, before[1]), "the update that picks the deformation up is a refit"
        _equal(hrt, r, flags, "deformed")
        before = _counts(r)
        _deform_all(r, "deformed_again")
        r.update_instances(bc.state("deformed_again")[1])
        assert _counts(r) == (before[0] + 1, before[1])
        _equal(hrt, r, flags, "deformed_again")
    finally:
        r.close()


def test_flattened_default_context_refits(hrt, gpu_available):
    _refit_cases(hrt, gpu_available, 0)


def test_asynchronous_update_refits(hrt, gpu_available):
    _refit_cases(hrt, gpu_available, hrt.CTX_ASYNC_UPDATE)


def test_two_level_refits_the_blas_subtrees_and_the_top_level(hrt, gpu_available):
    """... the 700-triangle BLAS, shared by two instances, moves in both (every instance's hits are compared)."""
    _refit_cases(hrt, gpu_available, hrt.CTX_TWO_LEVEL)
    ref = bc.reference("deformed", True)["hits"]
    for i in (1, 2):
        assert (ref[4] == i).sum() > 100


def test_two_level_asynchronous_update_refits(hrt, gpu_available):
    _refit_cases(hrt, gpu_available, hrt.CTX_TWO_LEVEL | hrt.CTX_ASYNC_UPDATE)


@pytest.mark.parametrize("two_level", [False, True])
def test_a_stale_tlas_shows_the_old_geometry_bit_for_bit(hrt, gpu_available, two_level):
    flags = hrt.CTX_TWO_LEVEL if two_level else 0
    r = _renderer(hrt, gpu_available, flags)
    try:
        o, d = bc.rays()
        old = r.trace_rays(o, d)
        _deform_all(r, "deformed")
        stale = r.trace_rays(o, d)
        for a, b, c in zip(stale, old, bc.reference("base", two_level)["hits"]):
            assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(c))
        r.update_instances(bc.state("deformed")[1])
        new = r.trace_rays(o, d)
        for a, c in zip(new, bc.reference("deformed", two_level)["hits"]):
            assert np.array_equal(_bits(a), _bits(c))
    finally:
        r.close()


@pytest.mark.parametrize("case", ["fast_trace", "fast_trace_two_level", "refit_off"])
def test_rebuild_branches(hrt, gpu_available, monkeypatch, case):
    """What a refit cannot follow rebuilds, and is counted so: a flattened tree with split references (which rebuilds at its first
    update anyway), a two-level tree whose 5000-triangle BLAS carries a split tree (after a plain update that refits), HRT_REFIT=0."""
    flags = {"fast_trace": hrt.CTX_FAST_TRACE, "fast_trace_two_level": hrt.CTX_FAST_TRACE | hrt.CTX_TWO_LEVEL, "refit_off": 0}[case]
    if case == "refit_off":
        monkeypatch.setenv("HRT_REFIT", "0")
    r = _renderer(hrt, gpu_available, flags)
    try:
        if case == "fast_trace_two_level":
            before = _counts(r)
            r.update_instances(bc.state("base")[1])
            assert _counts(r) == (before[0] + 1, before[1]), "moved instances alone: the two-level tree with split BLASes is refitted"
        before = _counts(r)
        _deform_all(r, "deformed")
        r.update_instances(bc.state("deformed")[1])
        assert _counts(r) == (before[0], before[1] + 1), "this update is a rebuild"
        _equal(hrt, r, flags, "deformed")
    finally:
        r.close()


def test_quality_guard_rebuilds_after_a_deformation_that_degrades_the_tree(hrt, gpu_available, monkeypatch):
    """test_refit_quality_guard_rebuilds' protocol with the geometry moving instead of the instances: the vertices of the 700-triangle
    BLAS scattered over 30 x its extent are REFITTED; the following update sees the verdict and rebuilds."""
    monkeypatch.setenv("HRT_REFIT_REBUILD_RATIO", "1.2")
    r = _renderer(hrt, gpu_available, 0)
    try:
        xf = bc.state("base")[1]
        r.update_instances(xf)                       # first refit after the build: checked on the spot, fine
        assert _counts(r) == (1, 1)
        r.update_blas_vertices(bc.INSTANCE_OF_BLAS[1], bc.state("scattered")[0][1])
        r.update_instances(xf)                       # refit, boxes grow a lot (checked at the next update)
        assert _counts(r) == (2, 1), r.stats().tlas_refit_ratio
        r.update_instances(xf)                       # sees the degraded tree -> rebuild
        s = r.stats()
        assert _counts(r) == (2, 2) and s.tlas_refit_ratio > 1.2, s.tlas_refit_ratio
        _equal(hrt, r, 0, "scattered")
    finally:
        r.close()


def test_non_finite_vertices_in_both_directions(hrt, gpu_available):
    """A triangle that was NaN at the build is left out of the tree: the update that makes it finite rebuilds, and it is hit.  A finite
    triangle that becomes NaN is refitted away and never hit again.  Everything else is equal."""
    r = _renderer(hrt, gpu_available, 0, "nan_built")
    try:
        r.update_instances(bc.state("nan_built")[1])
        before = _counts(r)
        r.update_blas_vertices(bc.INSTANCE_OF_BLAS[0], bc.state("base")[0][0])
        r.update_instances(bc.state("base")[1])
        assert _counts(r) == (before[0], before[1] + 1), "the tree had no record for the NaN triangle: a rebuild"
        got = _equal(hrt, r, 0, "base", nan_rays=True)
        assert ((got["hits"][3] == bc.NAN_PRIM) & (got["hits"][4] == 0)).sum() >= 1
        # the reverse
        before = _counts(r)
        r.update_blas_vertices(bc.INSTANCE_OF_BLAS[0], bc.state("nan_after")[0][0])
        r.update_instances(bc.state("nan_after")[1])
        assert _counts(r) == (before[0] + 1, before[1])
        got = _equal(hrt, r, 0, "nan_after", nan_rays=True)
        assert not ((got["hits"][3] == bc.NAN_PRIM) & (got["hits"][4] == 0)).any()
    finally:
        r.close()


def test_one_blas_under_two_tlases(hrt, gpu_available):
    """Each TLAS picks the change up at its own update; the one not yet updated stays on the old geometry."""
    r = _renderer(hrt, gpu_available, 0)
    try:
        o, d = bc.rays()
        first = r.tlas
        second = r.build_tlas(transforms=bc.state("base_moved")[1])
        _deform_all(r, "deformed")
        r.update_instances(bc.state("deformed")[1])

        def hits_are(state):
            for a, c in zip(r.trace_rays(o, d), bc.reference(state, False)["hits"]):
                assert np.array_equal(_bits(a), _bits(c)), state

        hits_are("deformed")
        r.use_tlas(second)
        hits_are("base_moved")
        r.update_instances(bc.state("deformed_moved_old")[1])
        hits_are("deformed_moved_old")
        r.use_tlas(first)
        hits_are("deformed")
    finally:
        r.close()


def test_refusals_change_nothing(hrt, gpu_available):
    r = _renderer(hrt, gpu_available, 0)
    try:
        import torch
        lib, st = r.lib, r._stream()
        o, d = bc.rays()
        verts = bc.state("deformed")[0]
        d_v = r._dev(verts[0].reshape(-1, 3))
        tri = int(r._h_inst[0].traversableHandle)
        centers, radii = r._dev(np.zeros((2, 3), np.float32)), r._dev(np.ones(2, np.float32))
        sph = C.c_uint64()
        assert lib.hrt_blas_build_spheres(r.ctx, centers.data_ptr(), radii.data_ptr(), 2, st, C.byref(sph)) == 0
        assert lib.hrt_blas_update_triangles(r.ctx, 0xDEAD, d_v.data_ptr(), 3 * 96, st) == -1            # an unknown handle
        assert lib.hrt_blas_update_triangles(r.ctx, r.tlas, d_v.data_ptr(), 3 * 96, st) == -1            # (a TLAS is not a BLAS)
        assert lib.hrt_blas_update_triangles(r.ctx, sph.value, d_v.data_ptr(), 6, st) == -1              # a sphere BLAS
        assert lib.hrt_blas_update_triangles(r.ctx, tri, d_v.data_ptr(), 3 * 96 - 3, st) == -1           # n_vertices off by 3
        assert lib.hrt_blas_update_triangles(r.ctx, tri, d_v.data_ptr(), 3 * 96 + 3, st) == -1
        assert lib.hrt_blas_update_triangles(r.ctx, tri, None, 3 * 96, st) == -1                         # a NULL pointer
        assert b"NULL" in lib.hrt_last_error(r.ctx)
        torch.cuda.synchronize()
        before = _counts(r)
        r.update_instances(bc.state("base")[1])
        assert _counts(r) == (before[0] + 1, before[1]), "nothing changed: the plain first refit"
        for a, c in zip(r.trace_rays(o, d), bc.reference("base", False)["hits"]):
            assert np.array_equal(_bits(a), _bits(c))
        # a BLAS of zero primitives with n_vertices == 0 is fine
        empty = C.c_uint64()
        assert lib.hrt_blas_build_triangles(r.ctx, None, 0, st, C.byref(empty)) == 0
        assert lib.hrt_blas_update_triangles(r.ctx, empty.value, None, 0, st) == 0
    finally:
        r.close()


@pytest.mark.parametrize("n_tris", [1, 2, 3, 5, 1027])
def test_every_alignment_and_tail_of_the_copy(hrt, oracle, gpu_available, n_tris):
    """The kernel takes four triangles at a time in 16-byte words where the pointers allow: every source alignment a float pointer can
    have, triangle counts that leave every tail -- the updated BLAS traces like a scene built from those vertices."""
    import torch
    verts = hrt.scenes._random_triangles(n_tris, 0.8, 90 + n_tris)
    start = (verts * np.float32(0.5)).astype(np.float32)
    scene = {"name": "tails", "instances": [hrt.scenes._tri_instance(start, hrt.scenes.WHITE)], "camera": hrt.scenes._soup_camera(),
             "background": hrt.scenes.BACKGROUND.copy(), "width": 8, "height": 8, "spp": 1}
    if not gpu_available:
        pytest.skip("no GPU in this container")
    r = hrt.Renderer(0, 0)
    try:
        r.load_scene(scene)
        o, d = oracle.random_rays(3000, 5)
        scene["instances"][0] = hrt.scenes._tri_instance(verts, hrt.scenes.WHITE)
        ref = oracle.OracleScene(scene, force_brute=True).trace(o, d)
        handle = int(r._h_inst[0].traversableHandle)
        for offset in (0, 1, 2, 3):
            back = torch.zeros(9 * n_tris, dtype=torch.float32, device=r.device)
            assert r.lib.hrt_blas_update_triangles(r.ctx, handle, back.data_ptr(), 3 * n_tris, r._stream()) == 0      # (to a degenerate mesh and back)
            buf = torch.zeros(9 * n_tris + 8, dtype=torch.float32, device=r.device)
            buf[offset:offset + 9 * n_tris] = torch.from_numpy(verts.reshape(-1)).to(r.device)
            src = buf[offset:]
            assert src.data_ptr() % 16 == 4 * offset
            assert r.lib.hrt_blas_update_triangles(r.ctx, handle, src.data_ptr(), 3 * n_tris, r._stream()) == 0
            assert float(buf[offset + 9 * n_tris:].abs().sum()) == 0.0
            r.update_instances([hrt.scenes.IDENTITY])
            for a, c in zip(r.trace_rays(o, d), ref):
                assert np.array_equal(_bits(a), _bits(c)), offset
    finally:
        r.close()


def test_denoiser_drops_a_pending_link_and_keeps_a_history(hrt, gpu_available):
    r = _renderer(hrt, gpu_available, 0)
    try:
        verts = bc.state("deformed")[0]
        frame = lambda: (r.set_frame(bc.W, bc.H, bc.SALT), r.render(bc.SPP))      # noqa: E731
        # (a) without a pending link the history is kept: the call after the update blends with it
        frame(); r.denoise_temporal()
        r.update_blas_vertices(bc.INSTANCE_OF_BLAS[2], verts[2])
        r.update_instances(bc.state("base")[1])
        frame(); r.denoise_temporal()
        length = r.denoise_temporal_state()[1].cpu().numpy()
        assert length.max() >= 2.0 and r.stats().denoise_history_rebinds == 0
        # (b) a pending by-primitive link that reads the 96-triangle BLAS as its old geometry is dropped by an update of that BLAS
        j = bc.INSTANCE_OF_BLAS[0]
        other = r.build_tlas(vertices={j: verts[0]})
        r.denoise_temporal_rebind(other, by_primitive=True)
        assert r.stats().denoise_by_primitive_links == 1
        r.update_blas_vertices(j, bc.state("deformed_again")[0][0])
        r.use_tlas(other)
        frame()
        out = r.denoise_temporal().cpu().numpy()
        assert np.array_equal(_bits(out), _bits(r.denoise().cpu().numpy())), "no link: the call starts afresh, which is denoise()"
        assert r.stats().denoise_history_rebinds == 0
    finally:
        r.close()


def test_primary_hit_capture_is_invalidated(hrt, gpu_available):
    r = _renderer(hrt, gpu_available, hrt.CTX_CAPTURE_PRIMARY)
    try:
        r.update_instances(bc.state("base")[1])
        r.set_frame(bc.W, bc.H, bc.SALT)
        r.render(1)
        r.primary_hits()
        _deform_all(r, "deformed")
        r.primary_hits()                             # (the BLAS call alone changes no tree: the capture is still the stale TLAS's)
        r.update_instances(bc.state("deformed")[1])
        with pytest.raises(hrt.HrtError, match="status -5"):
            r.primary_hits()
        r.render(1)
        t, u, v, prim, inst = r.primary_hits()
        assert (prim != 0xFFFFFFFF).any()
    finally:
        r.close()
