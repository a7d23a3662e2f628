"""hrt_blas_update_spheres on the GPU: a sphere cloud that moves keeps its BLAS handle, and the next hrt_tlas_update of every TLAS over it
picks the new centres and radii up -- by a refit where the tree holds every primitive as a record of its own, by a rebuild elsewhere
(DESIGN.md section 3a).

"Equal" (_equal) is three things: the hit records (t, u, v, primitive, instance) of 20000 rays are bit-identical to the oracle's brute
force over the moved scene, in the oracle mode the tree structure is pinned to (two-level: INSTANCED, else FLATTENED); linear radiance,
colour and RNG states of a 48 x 32 frame at 2 spp are bit-identical to the oracle's render of it; and all of these are identical to a
fresh Renderer of the same flags that loaded the moved scene.  The frame also shows that SHADING follows: a sphere's normal is
(hit - centre) / radius, read from the buffers Renderer.update_blas_spheres rewrites, so a frame shaded with the old ones would differ.
The scene, the motions and the oracle's results (computed once per state and mode) are tests/sphere_update_cases.py's; four instances
stand over the three BLASes because the 700-sphere one is shared by two."""
import ctypes as C

import numpy as np
import pytest

import sphere_update_cases as sc

pytestmark = pytest.mark.gpu

MISS = 0xFFFFFFFF


def _renderer(hrt, gpu_available, flags=0, state="base"):
    if not gpu_available:
        pytest.skip("no GPU in this container")
    r = hrt.Renderer(0, flags)
    r.load_scene(sc.scene_of(state))
    return r


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _observe(r, rays=None):
    """hit records of the ray set, then a frame from fresh RNG states"""
    o, d = rays if rays is not None else sc.rays()
    hits = r.trace_rays(o, d)
    r.set_frame(sc.W, sc.H, sc.SALT, linear=True)
    r.render(sc.SPP)
    return {"hits": hits, "linear": r.linear.cpu().numpy(), "color": r.color.cpu().numpy(), "states": r.rng_states_numpy()}


def _same(got, ref, what):
    for k, name in enumerate(("t", "u", "v", "prim", "inst")):
        assert np.array_equal(_bits(got["hits"][k]), _bits(ref["hits"][k])), f"{what}: {name} of the hit records"
    for key in ("linear", "color", "states"):
        assert np.array_equal(_bits(got[key]), _bits(ref[key])), f"{what}: {key}"


def _equal(hrt, r, flags, state, nan_rays=False, fresh=True):
    got = _observe(r, sc.rays_at_nan_prim() if nan_rays else None)
    _same(got, sc.reference(state, bool(flags & hrt.CTX_TWO_LEVEL), nan_rays), "against the oracle")
    if fresh:
        other = hrt.Renderer(0, flags)
        try:
            other.load_scene(sc.scene_of(state))
            _same(got, _observe(other, sc.rays_at_nan_prim() if nan_rays else None), "against a fresh renderer")
        finally:
            other.close()
    return got


def _move_all(r, state):
    """every BLAS of the renderer's scene to `state`'s spheres, each named through one of its instances"""
    spheres, _ = sc.state(state)
    for b, i in enumerate(sc.INSTANCE_OF_BLAS):
        r.update_blas_spheres(i, *spheres[b])


def _counts(r):
    s = r.stats()
    return int(s.tlas_refits), int(s.tlas_rebuilds)


def _download(hrt, r):
    """(records in the tree, its bounds' bits)"""
    blob = hrt.BvhBlob()
    r._check(r.lib.hrt_tlas_download(r.ctx, r.tlas, C.byref(blob)), "hrt_tlas_download")
    out = int(blob.n_triangles), np.array(list(blob.bounds), dtype=np.float32).view(np.uint32)
    r.lib.hrt_host_free(C.byref(blob))
    return out


def _refit_cases(hrt, gpu_available, flags):
    """An update of unchanged transforms (the first refit after the build; under HRT_CTX_ASYNC_UPDATE the synchronous one that the
    asynchronous path follows), then motion + update: equal, and a REFIT; then the second motion with moved instances in the same update."""
    r = _renderer(hrt, gpu_available, flags)
    try:
        r.update_instances(sc.state("base")[1])
        before = _counts(r)
        _move_all(r, "moved")
        r.update_instances(sc.state("moved")[1])
        assert _counts(r) == (before[0] + 1, before[1]), "the update that picks the motion up is a refit"
        _equal(hrt, r, flags, "moved")
        before = _counts(r)
        _move_all(r, "moved_again")
        r.update_instances(sc.state("moved_again")[1])
        assert _counts(r) == (before[0] + 1, before[1])
        _equal(hrt, r, flags, "moved_again")
    finally:
        r.close()


def test_flattened_default_context_refits(hrt, gpu_available):
    _refit_cases(hrt, gpu_available, 0)


def test_asynchronous_update_refits(hrt, gpu_available):
    _refit_cases(hrt, gpu_available, hrt.CTX_ASYNC_UPDATE)


def test_two_level_refits_the_blas_subtrees_and_the_top_level(hrt, gpu_available):
    """... the 700-sphere BLAS, shared by two instances, moves in both (every instance's hits are compared)."""
    _refit_cases(hrt, gpu_available, hrt.CTX_TWO_LEVEL)
    ref = sc.reference("moved", True)["hits"]
    for i in (1, 2):
        assert (ref[4] == i).sum() > 100


def test_two_level_asynchronous_update_refits(hrt, gpu_available):
    _refit_cases(hrt, gpu_available, hrt.CTX_TWO_LEVEL | hrt.CTX_ASYNC_UPDATE)


@pytest.mark.parametrize("two_level", [False, True])
def test_a_stale_tlas_shows_the_old_spheres_bit_for_bit(hrt, gpu_available, two_level):
    flags = hrt.CTX_TWO_LEVEL if two_level else 0
    r = _renderer(hrt, gpu_available, flags)
    try:
        o, d = sc.rays()
        old = r.trace_rays(o, d)
        _move_all(r, "moved")
        stale = r.trace_rays(o, d)
        for a, b, c in zip(stale, old, sc.reference("base", two_level)["hits"]):
            assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(c))
        r.update_instances(sc.state("moved")[1])
        new = r.trace_rays(o, d)
        for a, c in zip(new, sc.reference("moved", two_level)["hits"]):
            assert np.array_equal(_bits(a), _bits(c))
    finally:
        r.close()


def test_a_flattened_tree_that_keeps_its_splits_refits(hrt, gpu_available):
    """HRT_CTX_FAST_TRACE | HRT_CTX_KEEP_SPLITS, 6440 primitives (above the split line): the update after a sphere update is a refit, every
    record of a sphere taking the sphere's whole box at its new place, and the result is the oracle's.  (No fresh renderer: a fresh split
    build is a different tree.)"""
    flags = hrt.CTX_FAST_TRACE | hrt.CTX_KEEP_SPLITS
    r = _renderer(hrt, gpu_available, flags)
    try:
        r.update_instances(sc.state("base")[1])
        before = _counts(r)
        _move_all(r, "moved")
        r.update_instances(sc.state("moved")[1])
        assert _counts(r) == (before[0] + 1, before[1]), "a refit"
        _equal(hrt, r, flags, "moved", fresh=False)
    finally:
        r.close()


@pytest.mark.parametrize("case", ["fast_trace", "fast_trace_two_level", "refit_off"])
def test_rebuild_branches(hrt, gpu_available, monkeypatch, case):
    """What a refit cannot follow rebuilds, and is counted so: a flattened tree with split references (which rebuilds at its first
    update anyway), a two-level tree whose 5000-sphere BLAS carries a split tree (after a plain update that refits), HRT_REFIT=0.
    fast_trace_two_level: whether the split phase gives the 5000-sphere BLAS a split tree shows in the tree's record count -- 5740 is one
    record per sphere of the three BLASes, a split tree has more -- and decides what the update must be: a rebuild with a split tree, a
    refit without.  On the MI355X the tree has 6865 records: the 5000-sphere BLAS carries a split tree, and the update is a rebuild.

    (This case found a defect that was not the update's: pixel (18, 28) of the 2 spp frame differed from the oracle's, in a fresh renderer
    too, because the pixel's second primary ray was bounded at the distance the first had found on a sphere of radius 0.016 -- a distance
    the sphere test puts in front of the sphere's box -- and came back a miss.  A primary hit on a sphere seeds no bound now, path_lane.h.)"""
    flags = {"fast_trace": hrt.CTX_FAST_TRACE, "fast_trace_two_level": hrt.CTX_FAST_TRACE | hrt.CTX_TWO_LEVEL, "refit_off": 0}[case]
    if case == "refit_off":
        monkeypatch.setenv("HRT_REFIT", "0")
    r = _renderer(hrt, gpu_available, flags)
    try:
        rebuilds = True
        if case == "fast_trace_two_level":
            n_records, _ = _download(hrt, r)
            assert n_records >= sum(sc.SIZES)
            rebuilds = n_records > sum(sc.SIZES)
            print(f"fast_trace_two_level: {n_records} records for {sum(sc.SIZES)} spheres: the update must be a {'rebuild' if rebuilds else 'refit'}")
            before = _counts(r)
            r.update_instances(sc.state("base")[1])
            assert _counts(r) == (before[0] + 1, before[1]), "moved instances alone: the two-level tree is refitted, split BLASes or not"
        before = _counts(r)
        _move_all(r, "moved")
        r.update_instances(sc.state("moved")[1])
        if rebuilds:
            assert _counts(r) == (before[0], before[1] + 1), "this update is a rebuild"
        else:
            assert _counts(r) == (before[0] + 1, before[1]), "no split tree in any BLAS: this update is a refit"
        _equal(hrt, r, flags, "moved")
    finally:
        r.close()


def test_quality_guard_rebuilds_after_a_motion_that_degrades_the_tree(hrt, gpu_available, monkeypatch):
    """The triangle test's protocol: the centres of the 700-sphere BLAS scattered over 30 x its extent are REFITTED; the following update
    sees the verdict and rebuilds."""
    monkeypatch.setenv("HRT_REFIT_REBUILD_RATIO", "1.2")
    r = _renderer(hrt, gpu_available, 0)
    try:
        xf = sc.state("base")[1]
        r.update_instances(xf)                       # first refit after the build: checked on the spot, fine
        assert _counts(r) == (1, 1)
        r.update_blas_spheres(sc.INSTANCE_OF_BLAS[1], *sc.state("scattered")[0][1])
        r.update_instances(xf)                       # refit, boxes grow a lot (checked at the next update)
        assert _counts(r) == (2, 1), r.stats().tlas_refit_ratio
        r.update_instances(xf)                       # sees the degraded tree -> rebuild
        s = r.stats()
        assert _counts(r) == (2, 2) and s.tlas_refit_ratio > 1.2, s.tlas_refit_ratio
        _equal(hrt, r, 0, "scattered")
    finally:
        r.close()


def test_non_finite_spheres_in_both_directions(hrt, gpu_available):
    """A sphere that was NaN at the build is left out of the tree: the update that makes it finite rebuilds, and it is hit.  A finite
    sphere that gets a NaN centre, or an infinite radius, is refitted away and never hit again.  Everything else is equal."""
    r = _renderer(hrt, gpu_available, 0, "nan_built")
    try:
        r.update_instances(sc.state("nan_built")[1])
        before = _counts(r)
        r.update_blas_spheres(sc.INSTANCE_OF_BLAS[0], *sc.state("base")[0][0])
        r.update_instances(sc.state("base")[1])
        assert _counts(r) == (before[0], before[1] + 1), "the tree had no record for the NaN sphere: a rebuild"
        got = _equal(hrt, r, 0, "base", nan_rays=True)
        assert ((got["hits"][3] == sc.NAN_PRIM) & (got["hits"][4] == 0)).sum() >= 1
        for name in ("nan_after", "inf_after"):      # the reverse
            before = _counts(r)
            r.update_blas_spheres(sc.INSTANCE_OF_BLAS[0], *sc.state(name)[0][0])
            r.update_instances(sc.state(name)[1])
            assert _counts(r) == (before[0] + 1, before[1]), name
            got = _equal(hrt, r, 0, name, nan_rays=True)
            assert not ((got["hits"][3] == sc.NAN_PRIM) & (got["hits"][4] == 0)).any(), name
    finally:
        r.close()


def test_one_blas_under_two_tlases(hrt, gpu_available):
    """Each TLAS picks the change up at its own update; the one not yet updated stays on the old spheres."""
    r = _renderer(hrt, gpu_available, 0)
    try:
        o, d = sc.rays()
        first = r.tlas
        second = r.build_tlas(transforms=sc.state("base_moved")[1])
        _move_all(r, "moved")
        r.update_instances(sc.state("moved")[1])

        def hits_are(state):
            for a, c in zip(r.trace_rays(o, d), sc.reference(state, False)["hits"]):
                assert np.array_equal(_bits(a), _bits(c)), state

        hits_are("moved")
        r.use_tlas(second)
        hits_are("base_moved")
        r.update_instances(sc.state("moved_old_instances")[1])
        hits_are("moved_old_instances")
        r.use_tlas(first)
        hits_are("moved")
    finally:
        r.close()


def test_refusals_change_nothing(hrt, gpu_available):
    r = _renderer(hrt, gpu_available, 0)
    try:
        import torch
        lib, st = r.lib, r._stream()
        before = _observe(r)
        n = sc.SIZES[0]
        c, rad = sc.state("moved")[0][0]
        d_c, d_r = r._dev(c), r._dev(rad)
        sph = int(r._h_inst[0].traversableHandle)
        tri = C.c_uint64()
        d_v = r._dev(np.zeros((3 * n, 3), np.float32))
        assert lib.hrt_blas_build_triangles(r.ctx, d_v.data_ptr(), 3 * n, st, C.byref(tri)) == 0
        update = lib.hrt_blas_update_spheres
        assert update(r.ctx, 0xDEAD, d_c.data_ptr(), d_r.data_ptr(), n, st) == -1                # an unknown handle
        assert update(r.ctx, r.tlas, d_c.data_ptr(), d_r.data_ptr(), n, st) == -1                # (a TLAS is not a BLAS)
        assert update(r.ctx, tri.value, d_c.data_ptr(), d_r.data_ptr(), n, st) == -1             # a triangle BLAS
        assert update(r.ctx, sph, d_c.data_ptr(), d_r.data_ptr(), n - 1, st) == -1               # a count off by one
        assert update(r.ctx, sph, d_c.data_ptr(), d_r.data_ptr(), n + 1, st) == -1
        assert update(r.ctx, sph, None, d_r.data_ptr(), n, st) == -1                             # NULL centres
        assert b"NULL" in lib.hrt_last_error(r.ctx)
        assert update(r.ctx, sph, d_c.data_ptr(), None, n, st) == -1                             # NULL radii
        assert update(r.ctx, sph, d_c.data_ptr() + 2, d_r.data_ptr(), n - 1, st) == -1           # (both wrong)
        assert update(r.ctx, sph, d_c.data_ptr() + 2, d_r.data_ptr(), n, st) == -1               # a pointer offset by 2 bytes
        assert b"aligned" in lib.hrt_last_error(r.ctx)
        assert update(r.ctx, sph, d_c.data_ptr(), d_r.data_ptr() + 2, n, st) == -1
        torch.cuda.synchronize()
        _same(_observe(r), before, "after the refused calls")
        counts = _counts(r)
        r.update_instances(sc.state("base")[1])
        assert _counts(r) == (counts[0] + 1, counts[1]), "nothing changed: the plain first refit"
        got = _observe(r)
        _same(got, before, "after the refused calls and an update")
        _same(got, sc.reference("base", False), "against the oracle")
        # a BLAS of zero primitives with n_spheres == 0 is fine
        empty = C.c_uint64()
        assert lib.hrt_blas_build_spheres(r.ctx, None, None, 0, st, C.byref(empty)) == 0
        assert update(r.ctx, empty.value, None, None, 0, st) == 0
    finally:
        r.close()


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 8, 9, 1023, 1025])
def test_every_alignment_and_tail_of_the_copy(hrt, oracle, gpu_available, n):
    """The kernel takes four spheres at a time in 16-byte words where a source array allows, chosen per array: every alignment a float
    pointer can have for centres and radii independently (both the vector and the word variant of each), sphere counts that leave every
    tail -- the updated BLAS traces like a scene built from those arrays, in a flattened tree and in a two-level one, whose top level
    stands on the BLAS's recomputed bounds.  Then the bounds themselves: a TLAS built over the updated BLAS has bit for bit the bounds and
    the hits of a renderer that built the BLAS from the same arrays (hrt_tlas_download's `bounds` is the tree's as built: a refit does
    not renew it, so a build over the updated BLAS is what is compared)."""
    import torch
    S = hrt.scenes
    c = S.uniform_f32(9300 + n, 3 * n, -0.5, 0.5).reshape(n, 3)
    rad = S.uniform_f32(9400 + n, n, 0.2 if n < 16 else 0.01, 0.4 if n < 16 else 0.05)
    start_c, start_r = (c * np.float32(0.5)).astype(np.float32), (rad * np.float32(0.5)).astype(np.float32)

    def scene(cc, rr):
        return {"name": "tails", "instances": [S._sphere_instance(cc, rr, S.WHITE)], "camera": S._soup_camera(),
                "background": S.BACKGROUND.copy(), "width": 8, "height": 8, "spp": 1}

    if not gpu_available:
        pytest.skip("no GPU in this container")
    o, d = oracle.random_rays(2000, 5)
    for flags in (0, hrt.CTX_TWO_LEVEL):
        ref = oracle.OracleScene(scene(c, rad), force_brute=True, instanced=bool(flags)).trace(o, d)
        assert (ref[3] != MISS).any()
        r = hrt.Renderer(0, flags)
        try:
            r.load_scene(scene(start_c, start_r))
            handle = int(r._h_inst[0].traversableHandle)
            back_c, back_r = r._dev(start_c), r._dev(start_r)
            for off_c in range(4):
                for off_r in range(4):
                    assert r.lib.hrt_blas_update_spheres(r.ctx, handle, back_c.data_ptr(), back_r.data_ptr(), n, r._stream()) == 0      # (to the start and back)
                    buf_c = torch.zeros(3 * n + 8, dtype=torch.float32, device=r.device)
                    buf_r = torch.zeros(n + 8, dtype=torch.float32, device=r.device)
                    buf_c[off_c:off_c + 3 * n] = torch.from_numpy(c.reshape(-1)).to(r.device)
                    buf_r[off_r:off_r + n] = torch.from_numpy(rad).to(r.device)
                    src_c, src_r = buf_c[off_c:], buf_r[off_r:]
                    assert src_c.data_ptr() % 16 == 4 * off_c and src_r.data_ptr() % 16 == 4 * off_r
                    assert r.lib.hrt_blas_update_spheres(r.ctx, handle, src_c.data_ptr(), src_r.data_ptr(), n, r._stream()) == 0
                    assert float(buf_c[off_c + 3 * n:].abs().sum()) == 0.0 and float(buf_r[off_r + n:].abs().sum()) == 0.0
                    r.update_instances([S.IDENTITY])
                    for a, b in zip(r.trace_rays(o, d), ref):
                        assert np.array_equal(_bits(a), _bits(b)), (flags, off_c, off_r)
            r.use_tlas(r.build_tlas())
            got, bounds = r.trace_rays(o, d), _download(hrt, r)[1]
            fresh = hrt.Renderer(0, flags)
            try:
                fresh.load_scene(scene(c, rad))
                assert np.array_equal(bounds, _download(hrt, fresh)[1]), (flags, "bounds")
                for a, b in zip(got, fresh.trace_rays(o, d)):
                    assert np.array_equal(_bits(a), _bits(b)), (flags, "a build over the updated BLAS")
            finally:
                fresh.close()
        finally:
            r.close()


def test_primary_hit_capture_is_invalidated(hrt, gpu_available):
    r = _renderer(hrt, gpu_available, hrt.CTX_CAPTURE_PRIMARY)
    try:
        r.update_instances(sc.state("base")[1])
        r.set_frame(sc.W, sc.H, sc.SALT)
        r.render(1)
        r.primary_hits()
        _move_all(r, "moved")
        r.primary_hits()                             # (the BLAS call alone changes no tree: the capture is still the stale TLAS's)
        r.update_instances(sc.state("moved")[1])
        with pytest.raises(hrt.HrtError, match="status -5"):
            r.primary_hits()
        r.render(1)
        t, u, v, prim, inst = r.primary_hits()
        assert (prim != MISS).any()
    finally:
        r.close()
