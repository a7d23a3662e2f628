"""The denoiser's history hand-over across rebuilt BLASes on the MI355X (include/hrt.h hrt_denoise_temporal_rebind_geometry,
csrc/denoise_link_prim.hip k_denoise_temporal_by_prim): sequences that move to a TLAS over deformed meshes bit for bit against the
numpy specification (tests/denoise_by_primitive_ref.py) over the oracle's primary hits, what the old call does there, the re-baked
identity, maps, the lifetime of the link and of the BLASes it reads, the primary-hit capture, and hrt_mesh_render's file boundary.
Figures: profiles/r25_denoise_by_primitive.txt."""
import importlib
import subprocess
from pathlib import Path

import numpy as np
import pytest

import denoise_by_primitive_cases as cases
import denoise_by_primitive_ref as pref
import denoise_handoff_ref as href
import denoise_ref as ref

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
NO = int(href.NO_INSTANCE)


@pytest.fixture(scope="module")
def hrt_gpu(hrt):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return hrt


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want):
    """Bit-identical float32 arrays, NaN where the other has NaN."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    gn, wn = np.isnan(got), np.isnan(want)
    return np.array_equal(gn, wn) and np.array_equal(_bits(np.where(gn, 0, got)), _bits(np.where(wn, 0, want)))


def _where_differs(got, want):
    return np.argwhere(_bits(np.nan_to_num(got)) != _bits(np.nan_to_num(want)))[:8]


def _call(r, variance):
    """render(1) and one temporal / variance-guided call: (the colour buffer it took, {"out", "A", "L", "motion", ("M", "var")})."""
    r.render(1)
    color = r.color.cpu().numpy()
    out = (r.denoise_variance() if variance else r.denoise_temporal()).cpu().numpy()
    A, L, motion = (x.cpu().numpy() for x in r.denoise_temporal_state())
    got = {"out": out, "A": A, "L": L, "motion": motion}
    if variance:
        got["M"], got["var"] = (x.cpu().numpy() for x in r.denoise_variance_state())
    return color, got


def _compare(k, got, want):
    for what in want:
        assert _same(got[what], want[what]), (k, what, _where_differs(got[what], want[what]))


def _spec_link(prev_scene, next_scene, prev_instance=None, prev_order=None, next_order=None):
    link, by_prim = pref.make_link(pref.blas_info(prev_scene, prev_order), pref.blas_info(next_scene, next_order), prev_instance)
    return link, by_prim, pref.scene_verts(prev_scene)


def _build(hrt, r, sc, order, tf, deformed):
    """build_tlas(order, tf) with the deformed mesh, in a BLAS of its own, for every instance j whose source order[j] is in `deformed`;
    returns (handle, the scene it traces)."""
    verts = {j: cases.deform(sc["instances"][k]["vertices"]) for j, k in enumerate(order) if k in deformed}
    normals = {j: hrt.scenes.face_normals(v) for j, v in verts.items()}
    t = r.build_tlas(order, tf, vertices=verts, normals=normals)
    return t, pref.with_vertices(href.sub_scene(sc, order, tf), verts, normals, ("tlas", t))


FLAGS = {"production": lambda hrt: 0, "counting": lambda hrt: hrt.CTX_COUNT, "two_level": lambda hrt: hrt.CTX_TWO_LEVEL}
ALL = list(range(cases.N_PARTICLES + 1))


def _sequence(hrt, oracle, r, sc, cam, w, h, variance, by_primitive, instanced=False):
    """cases.SEQUENCE on `r`: frames 0-2 on load_scene's TLAS A, a rebind (by primitive or not) to B over the deformed meshes, frames
    3-4 on B, every frame compared with the specification.  Returns (what frame 3 gave, its history, the link)."""
    hist, on, prev, at3 = None, "A", None, None
    for k, (tlas, pose) in enumerate(cases.SEQUENCE):
        link = None
        if tlas != on:
            b, cur = _build(hrt, r, sc, ALL, cases.poses(hrt, pose), set(cases.DEFORMED))
            r.denoise_temporal_rebind(b, by_primitive=by_primitive)
            r.use_tlas(b)
            link = _spec_link(prev, cur)
            if not by_primitive:                       # the old call: another BLAS, no history
                link = (np.where(link[1], href.NO_INSTANCE, link[0]).astype(np.uint32), np.zeros_like(link[1]), link[2])
            on = tlas
        else:
            if k > 0 and pose != cases.SEQUENCE[k - 1][1]:
                r.update_instances(cases.poses(hrt, pose))
            cur = cases.scene_b(hrt, sc, pose) if tlas == "B" else href.sub_scene(sc, None, cases.poses(hrt, pose))
        color, got = _call(r, variance)
        want, hist = cases.spec_frame(oracle, variance, hist, link, color, cur, cam, w, h, instanced=instanced)
        _compare(k, got, want)
        if link is not None:
            at3 = (got, hist, link)
        prev = cur
    return at3


@pytest.mark.parametrize("size", cases.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("variance", [False, True], ids=["temporal", "variance"])
@pytest.mark.parametrize("mode", ["production", "counting", "two_level"])
def test_by_primitive_bit_exact(hrt_gpu, oracle, mode, variance, size):
    """cases.SEQUENCE: frames 0-2 on TLAS A with one update_instances, then hrt_denoise_temporal_rebind_geometry to TLAS B -- the
    deformed half of the particles in BLASes of their own, the others in their shared BLAS, the ground sphere -- and frames 3-4 on B
    with an update before frame 4.  Output, A, L, motion (moments and variance in the variance-guided mode) of every frame equal the
    specification's over the oracle's hits; on frame 3 more than 0.3 of the hit pixels linked by primitive have L > 1; one call counts
    as begun from a linked history, and the deformed instances as linked by primitive."""
    hrt = hrt_gpu
    w, h = size
    sc = cases.scene(hrt, w, h)
    cam = cases.camera(hrt, sc)
    r = hrt.Renderer(0, FLAGS[mode](hrt))
    try:
        r.load_scene(sc)
        r.set_frame(w, h, hrt.scenes.SEED_SALT)
        got, hist, link = _sequence(hrt, oracle, r, sc, cam, w, h, variance, True, instanced=(mode == "two_level"))
        px = cases.by_primitive_pixels(hist, link[1])
        share = (got["L"][px] > 1).sum() / max(px.sum(), 1)
        print(f"{mode} {w}x{h}: {px.sum()} by-primitive hit pixels on frame 3, with history {share:.3f}")
        assert px.any() and share > 0.3
        s = r.stats()
        assert s.denoise_history_rebinds == 1 and s.denoise_by_primitive_links == len(cases.DEFORMED)
    finally:
        r.close()


@pytest.mark.parametrize("size", cases.SIZES, ids=lambda s: "%dx%d" % s)
def test_it_is_the_new_call_that_carries(hrt_gpu, oracle, size):
    """The same sequence with hrt_denoise_temporal_rebind: the deformed instances' pixels have L = 1 and NaN motion on frame 3 -- that
    call's behaviour, unchanged, and still the specification's bit for bit -- where the new call has L > 1 on more than 0.3 of them."""
    hrt = hrt_gpu
    w, h = size
    sc = cases.scene(hrt, w, h)
    cam = cases.camera(hrt, sc)
    shares = {}
    for by_primitive in (False, True):
        r = hrt.Renderer(0, 0)
        try:
            r.load_scene(sc)
            r.set_frame(w, h, hrt.scenes.SEED_SALT)
            got, hist, link = _sequence(hrt, oracle, r, sc, cam, w, h, False, by_primitive)
            hit = hist["inst"] != href.MISS
            px = np.zeros_like(hit)
            px[hit] = np.isin(hist["inst"][hit], cases.DEFORMED)
            assert px.any()
            if not by_primitive:
                assert np.all(got["L"][px] == 1) and np.isnan(got["motion"][px]).all()
                assert r.stats().denoise_by_primitive_links == 0
            shares[by_primitive] = (got["L"][px] > 1).sum() / px.sum()
            assert (got["L"][hit & ~px] > 1).any()
        finally:
            r.close()
    assert shares[False] == 0 and shares[True] > 0.3, shares


@pytest.mark.parametrize("size", cases.SIZES, ids=lambda s: "%dx%d" % s)
def test_rebaked_identity(hrt_gpu, size):
    """The particles baked differently on a flattened tree: vertices x 2 in BLASes of their own, transforms x 0.5 (both exact), a
    static camera and scene.  Across the rebind every by-primitive hit pixel's motion lies within 0.01 pixel of its own centre (the
    rounding is about 1e-4 pixel), and L grows by one per frame on the pixels that had history."""
    hrt = hrt_gpu
    w, h = size
    sc = cases.scene(hrt, w, h)
    cam = cases.camera(hrt, sc)
    dirs = ref.primary_directions(w, h, *cam[1:])
    r = hrt.Renderer(0, 0)
    try:
        r.load_scene(sc)
        r.set_frame(w, h, hrt.scenes.SEED_SALT)
        r.update_instances(cases.poses(hrt, 1))
        L = [_call(r, False)[1]["L"] for _ in range(2)]
        assert set(np.unique(L[1])) <= {0.0, 2.0}
        subset = list(range(1, cases.N_PARTICLES + 1))
        tf = cases.poses(hrt, 1).copy()
        tf[subset] = (tf[subset].reshape(-1, 3, 4) * np.array([0.5, 0.5, 0.5, 1.0], np.float32)).reshape(-1, 12)
        verts = {j: (sc["instances"][j]["vertices"] * np.float32(2)).astype(np.float32) for j in subset}
        b = r.build_tlas(None, tf, vertices=verts, normals={j: sc["instances"][j]["normals"] for j in subset})
        r.denoise_temporal_rebind(b, by_primitive=True)
        r.use_tlas(b)
        assert r.stats().denoise_by_primitive_links == len(subset)
        for k in range(2):
            _, got = _call(r, False)
            inst = r.trace_rays(np.broadcast_to(cam[0], dirs.shape), dirs)[4].reshape(h, w)
            px = (inst != href.MISS) & (inst != 0)             # the particles' pixels: every one of them is linked by primitive
            assert px.sum() > 20
            ys, xs = np.nonzero(px)
            off = np.abs(got["motion"][px].astype(np.float64) - np.stack([xs, ys], axis=1)).max()
            print(f"re-baked identity {w}x{h} frame {k}: {px.sum()} particle pixels, motion off centre max {off:.3g} px")
            assert off <= 0.01
            # (L = (sum w L_prev) / (sum w) + 1 over up to four taps that all hold 2 + k: exact for the powers of two, and within the
            # four products', three sums', the division's and the addition's roundings -- 8 ulp -- of 3 + k otherwise)
            want = np.float32(3 + k)
            assert np.all(np.abs(got["L"][L[1] == 2] - want) <= 8 * np.spacing(want)) and np.all(L[1][px] == 2)
    finally:
        r.close()


@pytest.mark.parametrize("variance", [False, True], ids=["temporal", "variance"])
def test_all_blases_shared_is_the_old_call(hrt_gpu, variance):
    """Between TLASes that share every BLAS the new call links nothing by primitive, runs k_denoise_temporal_linked and gives
    hrt_denoise_temporal_rebind's bits: output, A, L, motion."""
    hrt = hrt_gpu
    w, h = cases.SIZES[1]
    sc = cases.scene(hrt, w, h)
    rs = [hrt.Renderer(0, 0), hrt.Renderer(0, 0)]
    try:
        got = []
        for r, by_primitive in zip(rs, (False, True)):
            r.load_scene(sc)
            r.set_frame(w, h, hrt.scenes.SEED_SALT)
            for _ in range(2):
                _call(r, variance)
            b = r.build_tlas(None, cases.poses(hrt, 1))
            r.denoise_temporal_rebind(b, by_primitive=by_primitive)
            r.use_tlas(b)
            got.append([_call(r, variance)[1] for _ in range(2)])
            s = r.stats()
            assert s.denoise_history_rebinds == 1 and s.denoise_by_primitive_links == 0
        for k in range(2):
            _compare(k, got[1][k], got[0][k])
            assert (got[0][k]["L"] > 1).any()
    finally:
        for r in rs:
            r.close()


def _chain(hrt, oracle, r, sc, cam, w, h, steps, variance):
    """steps: (order, pose, how, deformed) per frame -- the frame runs on a TLAS over scene instances `order` at cases.poses(pose)[order]
    with the sources in `deformed` deformed.  how: "same" (the TLAS of the frame before, updated if the pose differs), "fresh" (a new
    TLAS, no rebind), None (rebind by primitive with the NULL map) or the map.  Every frame is compared with the specification; the
    instances the link does not carry have L = 1 and NaN motion on their pixels.  Returns the by-primitive links the specification counts."""
    hist, prev, prev_step, links = None, None, None, 0
    for k, (order, pose, how, deformed) in enumerate(steps):
        tf = cases.poses(hrt, pose)[order]
        link = None
        if how == "same":
            assert (order, deformed) == (prev_step[0], prev_step[3])
            if pose != prev_step[1]:
                r.update_instances(tf)
            cur = dict(prev, instances=[dict(it, transform=m.copy()) for it, m in zip(prev["instances"], tf)])
        else:
            t, cur = _build(hrt, r, sc, order, tf, set(deformed))
            if how == "fresh":
                hist = None
            else:
                r.denoise_temporal_rebind(t, how, by_primitive=True)
                link = _spec_link(prev, cur, how, prev_step[0], order)
                links += int(link[1].sum())
            r.use_tlas(t)
        color, got = _call(r, variance)
        want, hist = cases.spec_frame(oracle, variance, hist, link, color, cur, cam, w, h)
        _compare(k, got, want)
        if link is not None:
            hit = hist["inst"] != href.MISS
            new = np.zeros_like(hit)
            new[hit] = link[0][hist["inst"][hit]] == NO
            assert np.all(got["L"][new] == 1) and np.isnan(got["motion"][new]).all(), k
            assert (got["L"][cases.by_primitive_pixels(hist, link[1])] > 1).any() or not link[1].any(), k
        prev, prev_step = cur, (order, pose, how, deformed)
    return links


_PERM = [int(k) for k in np.random.default_rng(7).permutation(len(ALL))]
# one instance taken out of the middle (the map shifts) and appended again as a body that was not there
_DROP = ALL[:12] + ALL[13:] + [12]
_DROP_MAP = ALL[:12] + ALL[13:] + [NO]
# new instances with the same predecessor, instance 1 of A (shape 0): scene instances 7 and 1 (shape 0, both deformed on B) by
# primitive, instance 4 (shape 0, not deformed: the shared BLAS) on the rigid path
_DUP = [0, 7, 1, 4, 2]
_DUP_MAP = [0, 1, 1, 1, 2]
# ineligible predecessors: deformed instance 1 after the ground sphere, deformed instance 7 (shape 0) after instance 2 (shape 1:
# another count), the ground sphere after triangles; deformed instance 5 stays eligible
_BAD = [1, 7, 0, 5]
_BAD_MAP = [0, 2, 1, 5]
D = cases.DEFORMED
MAP_CASES = {
    "permuted": [(ALL, 0, "fresh", []), (ALL, 1, "same", []), (_PERM, 2, _PERM, D), (_PERM, 3, "same", D)],
    "removed_and_appended": [(ALL, 0, "fresh", []), (ALL, 1, "same", []), (_DROP, 2, _DROP_MAP, D), (_DROP, 3, "same", D)],
    "duplicates": [(ALL, 0, "fresh", []), (ALL, 1, "same", []), (_DUP, 2, _DUP_MAP, D), (_DUP, 3, "same", D)],
    "ineligible": [(ALL, 0, "fresh", []), (ALL, 1, "same", []), (_BAD, 2, _BAD_MAP, D), (_BAD, 3, "same", D)],
    # deformed to deformed again (two BLASes of their own with the same vertices) and back to the shared BLAS, under the NULL map
    "rebuilt_twice_and_back": [(ALL, 0, "fresh", D), (ALL, 1, None, D), (ALL, 2, None, [])],
}
MAP_LINKS = {"permuted": len(D), "removed_and_appended": len(D), "duplicates": 2, "ineligible": 1, "rebuilt_twice_and_back": 2 * len(D)}


@pytest.mark.parametrize("variance", [False, True], ids=["temporal", "variance"])
@pytest.mark.parametrize("case", sorted(MAP_CASES))
def test_by_primitive_maps(hrt_gpu, oracle, case, variance):
    hrt = hrt_gpu
    w, h = cases.SIZES[1]
    sc = cases.scene(hrt, w, h)
    cam = cases.camera(hrt, sc)
    r = hrt.Renderer(0, 0)
    try:
        r.load_scene(sc)
        r.set_frame(w, h, hrt.scenes.SEED_SALT)
        links = _chain(hrt, oracle, r, sc, cam, w, h, MAP_CASES[case], variance)
        s = r.stats()
        assert links == MAP_LINKS[case] and s.denoise_by_primitive_links == links
        assert s.denoise_history_rebinds == sum(1 for st in MAP_CASES[case] if st[2] not in ("same", "fresh"))
    finally:
        r.close()


def _own_tlas(hrt, r, sc, pose, deform):
    """A TLAS at `pose` whose DEFORMED instances have BLASes of their own: the scene's vertices, or the deformed ones."""
    verts = {j: (cases.deform if deform else np.asarray)(sc["instances"][j]["vertices"]) for j in cases.DEFORMED}
    return r.build_tlas(None, cases.poses(hrt, pose), vertices=verts)


@pytest.mark.parametrize("variance", [False, True], ids=["temporal", "variance"])
def test_old_objects_may_go_between_rebind_and_launch(hrt_gpu, variance):
    """After the rebind and before the launch, TLAS A and the BLASes of its that the link reads are destroyed: the linked frame's
    bits, and the next frame's, equal those of a run that destroys nothing."""
    hrt = hrt_gpu
    w, h = cases.SIZES[1]
    sc = cases.scene(hrt, w, h)
    got = []
    for destroy in (False, True):
        r = hrt.Renderer(0, 0)
        try:
            r.load_scene(sc)
            r.set_frame(w, h, hrt.scenes.SEED_SALT)
            a = _own_tlas(hrt, r, sc, 0, False)
            r.use_tlas(a)
            for _ in range(2):
                _call(r, variance)
            b = _own_tlas(hrt, r, sc, 1, True)
            r.denoise_temporal_rebind(b, by_primitive=True)
            r.use_tlas(b)
            if destroy:
                r.destroy_tlas(a)
                r.destroy_built_blases(a)
            got.append([_call(r, variance)[1] for _ in range(2)])
            s = r.stats()
            assert s.denoise_history_rebinds == 1 and s.denoise_by_primitive_links == len(cases.DEFORMED)
        finally:
            r.close()
    for k in range(2):
        _compare(k, got[1][k], got[0][k])
    hit = got[0][0]["L"] > 0
    assert (got[0][0]["L"][hit] > 1).sum() > 0.3 * hit.sum()


@pytest.mark.parametrize("variance", [False, True], ids=["temporal", "variance"])
def test_by_primitive_link_lifetime(hrt_gpu, variance):
    """What drops a link (test_handoff_link_lifetime's list: a launch on a third handle, a reset, a new frame size, the other mode, no
    history to begin with, the target destroyed, a second rebind) drops a by-primitive one too: the next call is a fresh start -- no
    motion, L = 1 on every hit pixel, the bits of a call after hrt_denoise_temporal_reset.  A second rebind replaces a by-primitive
    link, and the linked call counts once."""
    hrt = hrt_gpu
    w, h = cases.SIZES[1]
    sc = cases.scene(hrt, w, h)
    r = hrt.Renderer(0, 0)

    def call(var=variance):
        return (r.denoise_variance() if var else r.denoise_temporal()).cpu().numpy()

    def fresh(var=variance):
        out = call(var)
        _, L, motion = (x.cpu().numpy() for x in r.denoise_temporal_state())
        assert np.isnan(motion).all() and set(np.unique(L)) <= {0.0, 1.0} and (L == 1).any()
        r.denoise_temporal_reset()
        assert np.array_equal(_bits(out), _bits(call(var)))

    def carried():
        call()
        return (r.denoise_temporal_state()[1].cpu().numpy() > 1).any()

    def history_on(t):
        r.use_tlas(t)
        r.denoise_temporal_reset()
        r.render(1)
        call()
        assert carried()

    def rebind(t):
        r.denoise_temporal_rebind(t, by_primitive=True)

    try:
        r.load_scene(sc)
        r.set_frame(w, h, hrt.scenes.SEED_SALT)
        a = r.tlas
        b, c = _own_tlas(hrt, r, sc, 0, True), _own_tlas(hrt, r, sc, 0, True)
        rebinds = lambda: r.stats().denoise_history_rebinds      # noqa: E731
        links = lambda: r.stats().denoise_by_primitive_links     # noqa: E731
        n = len(cases.DEFORMED)
        history_on(a)
        rebind(b)
        assert links() == n
        r.use_tlas(c)                                  # a launch on a third handle
        fresh()
        r.use_tlas(b)
        fresh()                                        # ... which has dropped the link to B as well
        history_on(a)
        rebind(b)
        r.denoise_temporal_reset()                     # a reset
        r.use_tlas(b)
        fresh()
        history_on(a)
        rebind(b)
        r.use_tlas(b)
        r.set_frame(w // 2, h // 2, hrt.scenes.SEED_SALT)      # a new frame size
        r.render(1)
        fresh()
        r.set_frame(w, h, hrt.scenes.SEED_SALT)
        r.render(1)
        history_on(a)
        rebind(b)
        r.use_tlas(b)
        fresh(not variance)                            # the other mode
        r.denoise_temporal_reset()
        before = links()
        rebind(a)                                      # no history: HRT_OK, nothing linked, nothing counted
        assert links() == before
        r.use_tlas(a)
        fresh()
        assert rebinds() == 0
        history_on(a)
        d = _own_tlas(hrt, r, sc, 0, True)
        rebind(d)
        r.destroy_tlas(d)                              # the link's TLAS destroyed: the history stays A's
        r.destroy_built_blases(d)
        assert carried() and rebinds() == 0
        rebind(c)
        rebind(b)                                      # another rebind replaces the by-primitive link
        r.use_tlas(c)
        fresh()
        history_on(a)
        rebind(b)
        r.use_tlas(b)
        assert carried() and rebinds() == 1            # the linked call
        assert carried() and rebinds() == 1            # the second call on B: ordinary, with history
        rebind(c)                                      # B -> C: two BLASes of their own per deformed instance
        r.use_tlas(c)
        assert carried() and rebinds() == 2
        r.use_tlas(a)                                  # back to A with no rebind
        fresh()
        assert rebinds() == 2
    finally:
        r.close()


@pytest.mark.parametrize("variance", [False, True], ids=["temporal", "variance"])
def test_by_primitive_takes_the_primary_capture(hrt_gpu, variance):
    """Under HRT_CTX_CAPTURE_PRIMARY the first frame on B takes its guides, and its u and v, from the render launch's capture --
    guide_passes_captured rises by one -- and gives the bits of a context without the flag."""
    hrt = hrt_gpu
    w, h = cases.SIZES[1]
    sc = cases.scene(hrt, w, h)
    rs = [hrt.Renderer(0, hrt.CTX_CAPTURE_PRIMARY), hrt.Renderer(0, 0)]
    try:
        got = []
        for r in rs:
            r.load_scene(sc)
            r.set_frame(w, h, hrt.scenes.SEED_SALT)
            for _ in range(2):
                _call(r, variance)
            b = _own_tlas(hrt, r, sc, 1, True)
            r.denoise_temporal_rebind(b, by_primitive=True)
            r.use_tlas(b)
            before = r.stats()
            got.append(_call(r, variance)[1])
            after = r.stats()
            captured = after.guide_passes_captured - before.guide_passes_captured
            assert captured == (1 if r is rs[0] else 0) and after.denoise_history_rebinds == 1
            assert after.guide_passes_traced - before.guide_passes_traced == 1 - captured
            assert after.denoise_by_primitive_links == len(cases.DEFORMED)
        _compare(0, got[0], got[1])
        hit = got[0]["L"] > 0
        assert (got[0]["L"][hit] > 1).sum() > 0.3 * hit.sum()
    finally:
        for r in rs:
            r.close()


def _mesh_data(cfg_path, w, h):
    """io.mesh_mode_scene's dict with the particle ids per file ("ids") added; the frame counts are the driver's own expression."""
    io = importlib.import_module("nvidia-optix-ray-tracer_amd.io")
    mm = io.mesh_mode_scene(cfg_path, width=w, height=h)
    cfg = mm["config"]
    per_file = [int(np.float32(d) * np.float32(cfg["fps"] * cfg["render-speed-ratio"])) for d in mm["durations"]]      # RendererMesh.cu:366-367
    assert per_file == mm["frame_counts"]
    cache = Path(cfg_path).parent.parent / "cache"
    mm["ids"] = [[p["id"] for p in io.read_mesh_cache(str(cache / f"particle{k}.cache"))] for k in range(len(per_file))]
    return mm


def _mesh_enter_file(hrt, r, mm, f, w, h, handoff):
    """hrt_mesh_render's step onto file f through the Python host: file 0 is the loaded scene; every later file is a TLAS over a BLAS
    of its own per particle, from the file's vertices, with the material of its id, and the extra spheres' shared BLASes -- linked by
    particle id, by primitive, if `handoff`."""
    n_extra, ids = mm["n_extra"], mm["ids"]
    if f == 0:
        r.load_scene(mm["scenes"][0])
        r.set_frame(w, h, hrt.scenes.SEED_SALT)
        return
    first = {pid: n_extra + p for p, pid in enumerate(ids[0])}       # (the record of an id: file 0's instance with it)
    particles = mm["scenes"][f]["instances"][n_extra:]
    t = r.build_tlas(list(range(n_extra)) + [first[pid] for pid in ids[f]],
                     vertices={n_extra + p: it["vertices"] for p, it in enumerate(particles)},
                     normals={n_extra + p: it["normals"] for p, it in enumerate(particles)})
    if handoff:
        last = {pid: n_extra + p for p, pid in enumerate(ids[f - 1])}
        r.denoise_temporal_rebind(t, list(range(n_extra)) + [last.get(pid, NO) for pid in ids[f]], by_primitive=True)
    r.use_tlas(t)


def _mesh_pose(r, mm, f, frame):
    cfg = mm["config"]
    st = np.zeros((len(mm["velocities"][f]), 12), np.float32)
    st[:, 7:10] = mm["velocities"][f]
    r.pose_instances(st, st, float(mm["durations"][f]), frame, mm["frame_counts"][f], first_instance=mm["n_extra"],
                     offset=cfg["particle-shift"], scale=cfg["particle-scale"], mesh_mode=True)


def _mesh_sequence(hrt, cfg_path, w, h, frames, handoff):
    """hrt_mesh_render's loop through the Python host for `frames` Mesh-mode frames in all, with or without the hand-over at the file
    boundaries.  Returns the 8-bit image of the last frame, the history length it ended on, the history rebinds and the by-primitive
    links."""
    mm = _mesh_data(cfg_path, w, h)
    r = hrt.Renderer(0, 0)
    try:
        done = 0
        for f in range(len(mm["scenes"])):
            if done == frames:
                break
            _mesh_enter_file(hrt, r, mm, f, w, h, handoff)
            for frame in range(mm["frame_counts"][f]):
                if done == frames:
                    break
                _mesh_pose(r, mm, f, frame)
                r.render(1)
                r.denoise_temporal(out=r.color)
                done += 1
        s = r.stats()
        return r.to_rgba8().cpu().numpy()[..., :3], r.denoise_temporal_state()[1].cpu().numpy(), s.denoise_history_rebinds, s.denoise_by_primitive_links
    finally:
        r.close()


def test_mesh_driver_hands_the_history_over(hrt_gpu, tmp_path):
    """hrt_mesh_render --denoise-temporal on io.write_mesh_mode_sample's data set (3 files of 12 particles whose ids are permuted per
    file) at 120x80, for the frames of file 0 -- the driver's frame-count expression -- and two of file 1: its image is the Python
    sequence's with the by-primitive rebind by particle id at the boundary, and with --no-history-handoff the sequence's without one.
    The two differ, and only the first ends on a history longer than the two frames of file 1."""
    hrt = hrt_gpu
    io = importlib.import_module("nvidia-optix-ray-tracer_amd.io")
    w, h = 120, 80
    cfg_path = io.write_mesh_mode_sample(tmp_path, n_files=3, n_particles=12, width=w, height=h)
    exe = ROOT / "nvidia-optix-ray-tracer_amd" / "lib" / "hrt_mesh_render"
    assert exe.exists(), "run `make tools`"
    images = {}
    for handoff in (True, False):
        per_file = _mesh_data(cfg_path, w, h)["frame_counts"]
        frames = per_file[0] + 2
        assert per_file[1] >= 2
        want, L, rebinds, links = _mesh_sequence(hrt, cfg_path, w, h, frames, handoff)
        out = tmp_path / f"frame{int(handoff)}.ppm"
        extra = [] if handoff else ["--no-history-handoff"]
        subprocess.run([str(exe), str(cfg_path), str(tmp_path / "bin"), str(frames), str(out), str(w), str(h), "--denoise-temporal", *extra],
                       check=True, timeout=300)
        raw = out.read_bytes()
        header = f"P6\n{w} {h}\n255\n".encode()
        assert raw.startswith(header)
        got = np.frombuffer(raw[len(header):], np.uint8).reshape(h, w, 3)
        assert np.array_equal(got, want), handoff
        assert rebinds == (1 if handoff else 0) and links == (12 if handoff else 0)
        assert (L.max() > 2) == handoff, (handoff, L.max())
        images[handoff] = got
    assert not np.array_equal(images[True], images[False])


def test_by_primitive_quality_at_the_file_boundary(hrt_gpu, tmp_path):
    """io.write_mesh_mode_sample's data set at 120x80 and 1 spp, hrt_mesh_render's loop up to the first frame of file 1, denoised
    there with the by-primitive hand-over and as the fresh start it used to be, against 4096 spp of that pose: the hand-over's MSE is
    at most BOUND times the reset's.  The specification over the oracle's hits measures 0.5619 on the CPU
    (tools/denoise_by_primitive_spec.py, profiles/r25_denoise_by_primitive.txt; the GPU gives the same frames bit for bit); BOUND is
    halfway between that and 1.  Next to guide edges -- test_temporal_quality_animation's mask -- the hand-over's error does not
    exceed the raw frame's: nothing ghosts across the boundary."""
    BOUND = 0.7809
    from test_denoise_temporal_gpu import _edge_pixels
    hrt = hrt_gpu
    io = importlib.import_module("nvidia-optix-ray-tracer_amd.io")
    w, h = 120, 80
    cfg_path = io.write_mesh_mode_sample(tmp_path, n_files=3, n_particles=12, width=w, height=h)
    mm = _mesh_data(cfg_path, w, h)
    results = {}
    for handoff in (True, False):
        r = hrt.Renderer(0, 0)
        try:
            _mesh_enter_file(hrt, r, mm, 0, w, h, handoff)
            for frame in range(mm["frame_counts"][0]):
                _mesh_pose(r, mm, 0, frame)
                r.render(1)
                r.denoise_temporal()
            _mesh_enter_file(hrt, r, mm, 1, w, h, handoff)
            _mesh_pose(r, mm, 1, 0)
            r.render(1)
            raw = r.color.cpu().numpy()[..., :3].astype(np.float64)
            results[handoff] = r.denoise_temporal().cpu().numpy()[..., :3].astype(np.float64)
            L = r.denoise_temporal_state()[1].cpu().numpy()
            assert (L.max() > 1) == handoff
            edge = _edge_pixels(r.denoise_guides().cpu().numpy().view(np.uint16))
        finally:
            r.close()
    r = hrt.Renderer(0, 0)
    try:
        _mesh_enter_file(hrt, r, mm, 0, w, h, False)
        _mesh_enter_file(hrt, r, mm, 1, w, h, False)
        _mesh_pose(r, mm, 1, 0)
        r.render(4096)
        conv = r.color.cpu().numpy()[..., :3].astype(np.float64)
    finally:
        r.close()
    mse_h, mse_r = ((results[True] - conv) ** 2).mean(), ((results[False] - conv) ** 2).mean()
    e_raw, e_h = ((raw - conv) ** 2)[edge].mean(), ((results[True] - conv) ** 2)[edge].mean()
    print(f"Mesh-mode file boundary: mse reset {mse_r:.6g} hand-over {mse_h:.6g} ratio {mse_h / mse_r:.4f}; "
          f"edges ({edge.sum()} px) raw {e_raw:.6g} hand-over {e_h:.6g} ratio {e_h / e_raw:.4f}")
    assert BOUND < 1
    assert mse_h <= BOUND * mse_r
    assert e_h <= e_raw
