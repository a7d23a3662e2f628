"""HRT_CTX_FAST_TRACE | HRT_CTX_KEEP_SPLITS: the flattened tree the device builds with spatial splits is REFITTED by hrt_tlas_update and
keeps its split references -- every triangle record's part of its triangle as ranges of the triangle's own barycentric coordinates,
which hold under any affine map and after hrt_blas_update_triangles; instances that have not moved keep their as-built clip boxes.

Parity bar as for every flattened tree: image, RNG states, ray counts and hit records BIT-EXACT against the oracle's flattened mode
(duplicate references cannot change the canonical hit), and the downloaded tree walked on the CPU finds what brute force finds, random
rays and the adversarial rays of ray_cases.py (exact vertices and edge points of the MOVED scene: the rays a clip box a hair too small
would lose).  What is new is checked on the structure: the update is a refit, node and record counts stay, an update that moves
nothing leaves every byte, a rebuild inside an update builds a split tree again.

Scenes just above the 4096-primitive line under which the device does not split.  Where instances turn, the rebuild ratio is
switched off (HRT_REFIT_REBUILD_RATIO, as in test_update_instances_refit_matches_oracle): the instances are interleaved soups, whose
nodes grow under any rotation, and it is the refitted tree that is under test; the animation test keeps the default verdict."""
import ctypes as C
import importlib

import numpy as np
import pytest

import ray_cases as rc
from blas_update_cases import deform

pytestmark = pytest.mark.gpu

W, H, SPP = 96, 64, 2
N_RANDOM, N_WALK, N_ADVERSARIAL = 20000, 4000, 3000
MISS = 0xFFFFFFFF
_hrt = importlib.import_module("nvidia-optix-ray-tracer_amd")
S = _hrt.scenes


# ---- scenes ----
def _mixed():
    """Three triangle instances of 2000 triangles and two sphere instances: the scene test_fast_trace_tree_with_spatial_splits splits."""
    return S.mixed_test_scene(6000, 30, 5, W, H, SPP)


def _thin_triangles(n, seed):
    """Long, thin triangles: one edge of 0.3 .. 0.5, the other half of it plus 0.02 across."""
    c = S.uniform_f32(seed * 1000 + 1, 3 * n, -1.0, 1.0).reshape(n, 3)
    d = S.uniform_f32(seed * 1000 + 2, 3 * n, -1.0, 1.0).reshape(n, 3).astype(np.float64)
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-6)
    e1 = d * S.uniform_f32(seed * 1000 + 3, n, 0.3, 0.5).astype(np.float64)[:, None]
    e2 = 0.5 * e1 + S.uniform_f32(seed * 1000 + 4, 3 * n, -0.02, 0.02).reshape(n, 3)
    v0 = c - (e1 + e2) / 3.0
    return np.stack([v0, v0 + e1, v0 + e2], axis=1).astype(np.float32)


def _thin_soup(sphere=None):
    """About 6000 long thin triangles dealt into four instances under distinct transforms; `sphere`: (centre, radius) of one more instance."""
    v = _thin_triangles(6000, 21)
    xf = [S.IDENTITY.copy(), S.rigid_transform((0.05, 0.0, -0.05), (0.2, 1.0, 0.1), 0.2), S.rigid_transform((0.0, -0.05, 0.0), (1.0, 0.0, 0.3), -0.3, 0.9),
          S.rigid_transform((-0.05, 0.05, 0.0), (0.0, 0.3, 1.0), 0.5, 1.1)]
    mats = ((S.WHITE, "rough", 0.0), (S.STEEL, "metal", 0.1), (S.RED, "rough", 0.0), (S.GREEN, "rough", 0.0))
    inst = [S._tri_instance(v[k::4], mats[k][0], mats[k][1], mats[k][2], xf[k]) for k in range(4)]
    if sphere is not None:
        inst.append(S._sphere_instance([sphere[0]], [sphere[1]], S.SAND, "rough", 0.0, S.IDENTITY.copy()))
    return {"name": "thin-soup", "instances": inst, "camera": S._soup_camera(), "background": S.BACKGROUND.copy(), "width": W, "height": H, "spp": SPP}


GROUND = ((0.05, -0.1, 0.0), 0.8)         # a sphere in the middle of the soup, far larger than a cell: it straddles every early plane and the split phase cuts it


def _scene(name):
    return {"mixed": _mixed, "thin": _thin_soup, "ground": lambda: _thin_soup(GROUND)}[name]()


def _n_prims(scene, visible=None):
    return sum(len(it["vertices"]) if it["geometry"] == "triangles" else len(it["radii"])
               for i, it in enumerate(scene["instances"]) if visible is None or visible[i])


def _squash(m, diag):
    """The transform m with a non-uniform scale of the object's axes in front."""
    m = np.asarray(m, np.float64).reshape(3, 4).copy()
    m[:, :3] = m[:, :3] @ np.diag(diag)
    return m.astype(np.float32).reshape(12)


def _pose(scene, step):
    """Transforms of animation step `step` (0: as built): the odd instances turn and shift a little further every step, those of
    triangles are scaled unevenly too; the even ones stay bit-identical."""
    out = []
    for i, it in enumerate(scene["instances"]):
        m = np.asarray(it["transform"], np.float32).copy()
        if step and i % 2 == 1:
            t = S.rigid_transform((0.03 * step, -0.02 * step, 0.015 * step * (i - 2)), (0.3, 1.0, 0.2 * i), 0.06 * step)
            a, b = t.reshape(3, 4).astype(np.float64), m.reshape(3, 4).astype(np.float64)
            c = np.concatenate([a[:, :3] @ b[:, :3], (a[:, :3] @ b[:, 3] + a[:, 3])[:, None]], axis=1)
            m = _squash(c, [1.0 + 0.04 * step, 1.0 - 0.03 * step, 1.0] if it["geometry"] == "triangles" else [1.0, 1.0, 1.0])
        out.append(m)
    return out


def _moved(scene, xf):
    out = dict(scene, instances=[dict(it, transform=np.asarray(m, np.float32)) for it, m in zip(scene["instances"], xf)])
    return out


# ---- the renderer and its tree ----
def _renderer(hrt, gpu_available, flags, monkeypatch=None, ratio_off=True):
    if not gpu_available:
        pytest.skip("no GPU in this container")
    if monkeypatch is not None and ratio_off:
        monkeypatch.setenv("HRT_REFIT_REBUILD_RATIO", "1e30")
    return hrt.Renderer(0, flags)


def _flags(hrt, update="synchronous"):
    return hrt.CTX_FAST_TRACE | hrt.CTX_KEEP_SPLITS | (hrt.CTX_ASYNC_UPDATE if update == "asynchronous" else 0)


def _download(hrt, r):
    blob = hrt.BvhBlob()
    r._check(r.lib.hrt_tlas_download(r.ctx, r.tlas, C.byref(blob)), "hrt_tlas_download")
    nodes = np.ctypeslib.as_array(C.cast(blob.nodes, C.POINTER(C.c_uint8)), shape=(blob.n_nodes * 80,)).copy()
    prims = np.ctypeslib.as_array(C.cast(blob.triangles, C.POINTER(C.c_uint8)), shape=(max(blob.n_triangles, 1) * 48,)).copy()
    n_nodes, n_records = int(blob.n_nodes), int(blob.n_triangles)
    r.lib.hrt_host_free(C.byref(blob))
    return nodes, prims, n_nodes, n_records


def _record_ids(prims, n_records):
    w = prims[: 48 * n_records].view(np.uint32).reshape(-1, 12)
    return w[:, 3], w[:, 7], w[:, 11]             # primitive, instance, kind


def _is_split(prims, n_records, n_primitives, moved_instances):
    """The preconditions: the tree holds duplicated references, and an instance the test moves owns a primitive with two records or more."""
    assert n_records >= 1.05 * n_primitives, (n_records, n_primitives)
    prim, inst, _ = _record_ids(prims, n_records)
    key = (inst.astype(np.uint64) << np.uint64(32)) | prim.astype(np.uint64)
    ids, count = np.unique(key, return_counts=True)
    owners = set((ids[count >= 2] >> np.uint64(32)).astype(np.int64).tolist())
    assert owners & set(moved_instances), (sorted(owners), moved_instances)


def _frame_is_the_oracles(oracle, r, scene, salt):
    r.set_frame(W, H, salt, linear=True)
    r.reset_stats()
    r.render(SPP)
    lin, col, states, rays = r.linear.cpu().numpy(), r.color.cpu().numpy(), r.rng_states_numpy(), int(r.stats().rays)
    ref_states = oracle.rng_init(W, H, salt)
    ref = oracle.OracleScene(scene).render(W, H, ref_states, SPP)
    assert np.array_equal(lin.view(np.uint32), ref["linear"].view(np.uint32)), "linear radiance must be bit-exact"
    assert np.array_equal(col.view(np.uint32), ref["color"].view(np.uint32)), "the colour image must be bit-exact"
    assert np.array_equal(states, ref_states), "the RNG streams must end where the oracle's end"
    assert rays == ref["rays"]


def _hits_are_brute_forces(oracle, r, scene, n=N_RANDOM, seed=31):
    o, d = oracle.random_rays(n, seed)
    want = oracle.OracleScene(scene, force_brute=True).trace(o, d)
    assert (want[3] != MISS).mean() >= 0.5                                  # (precondition: the rays do see the scene)
    got = r.trace_rays(o, d)
    diff = rc.records_differ(got, want)
    assert not diff.any(), (int(diff.sum()), int(np.argmax(diff)))
    any_got = r.trace_rays(o, d, any_hit=True)
    assert np.array_equal(any_got[3] != MISS, want[3] != MISS)


def _inverse_tables(scene):
    """World -> object per instance and the identity flags, which the CPU walk takes for the spheres of a one-level tree: the oracle's
    invert_affine restated (cofactors in double, each entry rounded once), so that the walk's records are brute force's bit for bit."""
    inv, ident = [], []
    for it in scene["instances"]:
        m = np.asarray(it["transform"], np.float32).astype(np.float64)
        a, b, c, d, e, f, g, h, i = m[0], m[1], m[2], m[4], m[5], m[6], m[8], m[9], m[10]
        A, B, Cc = e * i - f * h, -(d * i - f * g), d * h - e * g
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.float64(1.0) / (a * A + b * B + c * Cc)
            n = [[A * r, -(b * i - c * h) * r, (b * f - c * e) * r], [B * r, (a * i - c * g) * r, -(a * f - c * d) * r], [Cc * r, -(a * h - b * g) * r, (a * e - b * d) * r]]
            tx, ty, tz = m[3], m[7], m[11]
            inv.append(np.float32([[row[0], row[1], row[2], -(row[0] * tx + row[1] * ty + row[2] * tz)] for row in n]).reshape(12))
        ident.append(int(np.array_equal(np.asarray(it["transform"], np.float32).view(np.uint32), S.IDENTITY.view(np.uint32))))
    return np.ascontiguousarray(np.stack(inv), np.float32), np.asarray(ident, np.uint32)


def _cpu_walk_is_brute_forces(hrt, oracle, r, scene, seed=77, aim=None):
    """The downloaded tree under oracle.bvh8_trace: random rays, and adversarial rays aimed at the scene's edges and vertices as they are
    now (`aim`: the scene the rays are aimed at, where `scene` itself holds a NaN)."""
    aim = scene if aim is None else aim
    blob = hrt.BvhBlob()
    r._check(r.lib.hrt_tlas_download(r.ctx, r.tlas, C.byref(blob)), "hrt_tlas_download")
    try:
        brute = oracle.OracleScene(scene, force_brute=True)
        inv, ident = _inverse_tables(scene)
        o, d = oracle.random_rays(N_WALK, seed)
        ao, ad, _ = rc.adversarial_rays(aim, N_ADVERSARIAL, seed + 1, rc.scene_extent(aim))
        for oo, dd, what in ((o, d, "random"), (ao, ad, "adversarial")):
            want = brute.trace(oo, dd)
            got = oracle.bvh8_trace(blob.nodes, blob.triangles, oo, dd, inst_inv=inv, inst_identity=ident)
            diff = rc.records_differ(got[:5], want)
            assert not diff.any(), (what, int(diff.sum()), int(np.argmax(diff)))
            dev = r.trace_rays(oo, dd)
            diff = rc.records_differ(dev, want)
            assert not diff.any(), (what, "device", int(diff.sum()), int(np.argmax(diff)))
    finally:
        r.lib.hrt_host_free(C.byref(blob))


def _update(r, xf, update, twice_from=None):
    """One update; an asynchronous context's first update after a build is synchronous, so `twice_from` (a pose on the way) goes first there:
    the update under test then takes the asynchronous path.  Returns the number of updates made."""
    n = 0
    if update == "asynchronous" and twice_from is not None:
        r.update_instances(twice_from)
        n += 1
    r.update_instances(xf)
    return n + 1


# ---- 1, 4: moved instances ----
@pytest.mark.parametrize("update", ["synchronous", "asynchronous"])
@pytest.mark.parametrize("name", ["mixed", "thin"])
def test_moved_instances_are_refitted_and_the_tree_keeps_its_splits(hrt, oracle, gpu_available, monkeypatch, name, update):
    """The test that fails without the feature: there the update counts a rebuild and the record count falls to the primitive count."""
    scene = _scene(name)
    r = _renderer(hrt, gpu_available, _flags(hrt, update), monkeypatch)
    try:
        r.load_scene(scene)
        _, prims0, n_nodes, n_records = _download(hrt, r)
        xf = _pose(scene, 2)
        movers = [i for i, (it, m) in enumerate(zip(scene["instances"], xf)) if not np.array_equal(np.asarray(it["transform"], np.float32), m)]
        assert 2 * len(movers) >= len(xf) - 1 and len(movers) < len(xf)
        _is_split(prims0, n_records, _n_prims(scene), movers)
        before = r.stats()
        made = _update(r, xf, update, twice_from=_pose(scene, 1))
        after = r.stats()
        assert after.tlas_rebuilds == before.tlas_rebuilds and after.tlas_refits == before.tlas_refits + made
        _, prims1, n_nodes1, n_records1 = _download(hrt, r)
        assert (n_nodes1, n_records1) == (n_nodes, n_records)
        ids0, ids1 = _record_ids(prims0, n_records), _record_ids(prims1, n_records)
        assert all(np.array_equal(a, b) for a, b in zip(ids0, ids1))        # the same records in the same order
        now = _moved(scene, xf)
        _frame_is_the_oracles(oracle, r, now, 99)
        _hits_are_brute_forces(oracle, r, now)
        _cpu_walk_is_brute_forces(hrt, oracle, r, now)
    finally:
        r.close()


# ---- 2: nothing moved ----
@pytest.mark.parametrize("update", ["synchronous", "asynchronous"])
def test_an_update_that_moves_nothing_leaves_every_byte(hrt, gpu_available, update):
    scene = _scene("ground")
    r = _renderer(hrt, gpu_available, _flags(hrt, update))
    try:
        r.load_scene(scene)
        nodes0, prims0, _, n_records = _download(hrt, r)
        _is_split(prims0, n_records, _n_prims(scene), range(len(scene["instances"])))
        before = r.stats()
        xf = _pose(scene, 0)
        for k in (1, 2, 3):                                                  # (asynchronous: the second and third take the device's comparison)
            r.update_instances(xf)
            nodes1, prims1, _, _ = _download(hrt, r)
            assert np.array_equal(prims0, prims1) and np.array_equal(nodes0, nodes1), k
        after = r.stats()
        assert after.tlas_refits == before.tlas_refits + 3 and after.tlas_rebuilds == before.tlas_rebuilds
    finally:
        r.close()


# ---- 3, 4: an animation, then a rebuild ----
@pytest.mark.parametrize("update", ["synchronous", "asynchronous"])
def test_five_frames_of_an_animation_then_a_rebuild_that_splits_again(hrt, oracle, gpu_available, update):
    """Small steps under the default quality verdict: every update a refit, every frame the oracle's.  Then a visibility bit flips: the
    update rebuilds (an asynchronous one learns it from the device and rebuilds at the next update) -- a split tree again."""
    scene = _scene("thin")
    r = _renderer(hrt, gpu_available, _flags(hrt, update))
    try:
        r.load_scene(scene)
        _, prims0, n_nodes, n_records = _download(hrt, r)
        _is_split(prims0, n_records, _n_prims(scene), [1, 3])
        built = r.stats()
        for step in (1, 2, 3, 4, 5):
            xf = _pose(scene, 0)
            xf[1] = _squash(S.rigid_transform((0.05 + 0.004 * step, -0.002 * step, -0.05), (0.2, 1.0, 0.1), 0.2 + 0.004 * step), [1.0 + 0.002 * step, 1.0, 1.0 - 0.002 * step])
            r.update_instances(xf)
            st = r.stats()
            assert st.tlas_refits == built.tlas_refits + step and st.tlas_rebuilds == built.tlas_rebuilds, (step, int(st.tlas_refits), int(st.tlas_rebuilds), float(st.tlas_refit_ratio))
            _, _, n_nodes1, n_records1 = _download(hrt, r)
            assert (n_nodes1, n_records1) == (n_nodes, n_records)
            now = _moved(scene, xf)
            _frame_is_the_oracles(oracle, r, now, 100 + step)
            _hits_are_brute_forces(oracle, r, now, 6000, step)
        r._h_inst[2].visibilityMask = 0
        r.update_instances(xf)
        if update == "asynchronous":
            r.update_instances(xf)
        st = r.stats()
        assert st.tlas_rebuilds == built.tlas_rebuilds + 1, (int(st.tlas_rebuilds), int(st.tlas_refits))
        _, prims1, _, n_records1 = _download(hrt, r)
        visible = [True, True, False, True]
        assert n_records1 >= 1.05 * _n_prims(scene, visible), (n_records1, _n_prims(scene, visible))
        assert not (_record_ids(prims1, n_records1)[1] == 2).any()
        refits = int(st.tlas_refits)
        r.update_instances(xf)                                               # ... and the rebuilt tree is refitted like the first
        st = r.stats()
        assert st.tlas_refits == refits + 1 and st.tlas_rebuilds == built.tlas_rebuilds + 1
        assert _download(hrt, r)[3] == n_records1
    finally:
        r.close()


# ---- 5: a deformed mesh ----
@pytest.mark.parametrize("update", ["synchronous", "asynchronous"])
def test_a_deformed_mesh_is_followed_by_a_refit(hrt, oracle, gpu_available, monkeypatch, update):
    scene = _scene("thin")
    r = _renderer(hrt, gpu_available, _flags(hrt, update), monkeypatch)
    try:
        r.load_scene(scene)
        _, prims0, n_nodes, n_records = _download(hrt, r)
        _is_split(prims0, n_records, _n_prims(scene), [1])
        xf = _pose(scene, 0)
        if update == "asynchronous":
            r.update_instances(xf)                                           # (the first update after the build: synchronous)
        before = r.stats()
        v = deform(scene["instances"][1]["vertices"], 1)
        r.update_blas_vertices(1, v)
        r.update_instances(xf)
        after = r.stats()
        assert after.tlas_refits == before.tlas_refits + 1 and after.tlas_rebuilds == before.tlas_rebuilds
        assert _download(hrt, r)[2:] == (n_nodes, n_records)
        now = _moved(scene, xf)
        now["instances"][1] = dict(now["instances"][1], vertices=v, normals=S.face_normals(v))
        _frame_is_the_oracles(oracle, r, now, 7)
        _hits_are_brute_forces(oracle, r, now)
        _cpu_walk_is_brute_forces(hrt, oracle, r, now)
        o, d = oracle.random_rays(N_RANDOM, 5)
        got = r.trace_rays(o, d)
        fresh = hrt.Renderer(0, 0)
        try:
            fresh.load_scene(now)
            assert not rc.records_differ(got, fresh.trace_rays(o, d)).any()
        finally:
            fresh.close()
    finally:
        r.close()


# ---- 6: spheres ----
def _leaf_boxes_of(nodes, n_nodes, records):
    """Decoded boxes of the leaf slots that hold nothing but the given records: {first record: (lo, hi, grid step)}."""
    nb = nodes.reshape(n_nodes, 80)
    words = nb.view(np.uint32).reshape(n_nodes, 20)
    origin = nb[:, :12].copy().view(np.float32).reshape(n_nodes, 3)
    records = set(int(x) for x in records)
    out = {}
    for n in range(n_nodes):
        if words[n, 3] == 0:
            continue
        scale = (nb[n, 12:15].astype(np.uint32) << 23).view(np.float32).astype(np.float64)
        for slot in range(8):
            meta = int(nb[n, 24 + slot])
            if meta == 0 or (meta & 0x18) == 0x18:
                continue
            first = int(words[n, 5]) + (meta & 0x1F)
            mine = [first + k for k in range(bin(meta >> 5).count("1"))]
            if not all(x in records for x in mine):
                continue
            lo = origin[n].astype(np.float64) + nb[n, [32 + slot, 40 + slot, 48 + slot]].astype(np.float64) * scale
            hi = origin[n].astype(np.float64) + nb[n, [56 + slot, 64 + slot, 72 + slot]].astype(np.float64) * scale
            out[first] = (lo, hi, scale)
    return out


def test_a_split_sphere_that_stays_put_keeps_its_built_boxes(hrt, oracle, gpu_available, monkeypatch):
    scene = _scene("ground")
    r = _renderer(hrt, gpu_available, _flags(hrt), monkeypatch)
    try:
        r.load_scene(scene)
        nodes0, prims0, n_nodes, n_records = _download(hrt, r)
        prim, inst, kind = _record_ids(prims0, n_records)
        sphere = np.flatnonzero(inst == 4)
        assert len(sphere) >= 2 and (kind[sphere] == 1).all(), len(sphere)       # the build did cut the sphere
        _is_split(prims0, n_records, _n_prims(scene), [1, 3])
        xf = _pose(scene, 2)
        before = r.stats()
        r.update_instances(xf)
        after = r.stats()
        assert after.tlas_refits == before.tlas_refits + 1 and after.tlas_rebuilds == before.tlas_rebuilds
        nodes1, prims1, n_nodes1, n_records1 = _download(hrt, r)
        assert (n_nodes1, n_records1) == (n_nodes, n_records)
        rec0, rec1 = prims0.reshape(-1, 48), prims1.reshape(-1, 48)
        assert np.array_equal(rec0[sphere], rec1[sphere])                    # (centre and radius: the records hold no box, this line cannot tell the paths apart -- the lines below do)
        # its leaves' boxes: the as-built clip box again, stored on the node's grid as it is now -- within a grid step of before and after
        # of what it was, not the sphere's whole box (1.6 across)
        was, now_ = _leaf_boxes_of(nodes0, n_nodes, sphere), _leaf_boxes_of(nodes1, n_nodes, sphere)
        assert was.keys() == now_.keys() and len(was) >= 1
        for first, (lo0, hi0, s0) in was.items():
            lo1, hi1, s1 = now_[first]
            assert (np.abs(lo1 - lo0) <= s0 + s1).all() and (np.abs(hi1 - hi0) <= s0 + s1).all(), (first, lo0, lo1, hi0, hi1)
        assert min(float((hi - lo).min()) for lo, hi, _ in now_.values()) < 1.2   # (a part of the sphere, not all of it)
        now = _moved(scene, xf)
        _frame_is_the_oracles(oracle, r, now, 12)
        _hits_are_brute_forces(oracle, r, now)
        _cpu_walk_is_brute_forces(hrt, oracle, r, now)
    finally:
        r.close()


def test_a_split_sphere_that_moves_is_still_hit(hrt, oracle, gpu_available, monkeypatch):
    """The limitation: every record of a moved sphere takes the sphere's whole box.  Correct all the same."""
    scene = _scene("ground")
    r = _renderer(hrt, gpu_available, _flags(hrt), monkeypatch)
    try:
        r.load_scene(scene)
        _, prims0, _, n_records = _download(hrt, r)
        assert (_record_ids(prims0, n_records)[1] == 4).sum() >= 2
        xf = _pose(scene, 1)
        xf[4] = S.rigid_transform((0.1, 0.15, -0.1), (1.0, 0.2, 0.0), 0.3)
        before = r.stats()
        r.update_instances(xf)
        after = r.stats()
        assert after.tlas_refits == before.tlas_refits + 1 and after.tlas_rebuilds == before.tlas_rebuilds
        now = _moved(scene, xf)
        _hits_are_brute_forces(oracle, r, now)
        _cpu_walk_is_brute_forces(hrt, oracle, r, now)
        _frame_is_the_oracles(oracle, r, now, 13)
    finally:
        r.close()


# ---- 7: hostile inputs ----
@pytest.mark.parametrize("case", ["singular-transform", "zero-area-triangle", "nan-vertex"])
def test_hostile_inputs_after_one_update(hrt, oracle, gpu_available, monkeypatch, case):
    scene = _scene("thin")
    if case == "zero-area-triangle":                                         # in the tree from the build on, in an instance that moves
        v = scene["instances"][1]["vertices"].copy()
        v[5, 1] = v[5, 0]                                                    # two corners coincide
        v[9, 2] = (0.5 * v[9, 0].astype(np.float64) + 0.5 * v[9, 1].astype(np.float64)).astype(np.float32)      # three on a line (or as near as floats are)
        scene["instances"][1] = dict(scene["instances"][1], vertices=v, normals=S.face_normals(v))
    r = _renderer(hrt, gpu_available, _flags(hrt), monkeypatch)
    try:
        r.load_scene(scene)
        _, prims0, n_nodes, n_records = _download(hrt, r)
        _is_split(prims0, n_records, _n_prims(scene), [1, 3])
        xf = _pose(scene, 2)
        now = aim = _moved(scene, xf)
        if case == "singular-transform":
            xf[1] = _squash(xf[1], [1.0, 0.0, 1.0])                          # an axis of the object scaled to 0
            now = aim = _moved(scene, xf)
        if case == "nan-vertex":
            v = scene["instances"][1]["vertices"].copy()
            prim, inst, _ = _record_ids(prims0, n_records)
            ids, count = np.unique(prim[inst == 1], return_counts=True)
            victim = int(ids[np.argmax(count)])                              # a triangle the build cut
            assert count.max() >= 2
            v[victim, 2, 1] = np.nan
            r.update_blas_vertices(1, v)
            now = _moved(scene, xf)
            now["instances"][1] = dict(now["instances"][1], vertices=v, normals=S.face_normals(v))
        before = r.stats()
        r.update_instances(xf)
        after = r.stats()
        assert after.tlas_refits == before.tlas_refits + 1 and after.tlas_rebuilds == before.tlas_rebuilds
        assert _download(hrt, r)[2:] == (n_nodes, n_records)
        _hits_are_brute_forces(oracle, r, now)
        _cpu_walk_is_brute_forces(hrt, oracle, r, now, aim=aim)
        _frame_is_the_oracles(oracle, r, now, 21)
        if case == "nan-vertex":                                             # its triangle is never hit, as the update's contract says
            o, d = oracle.random_rays(N_RANDOM, 31)
            got = r.trace_rays(o, d)
            assert not ((got[3] == victim) & (got[4] == 1)).any()
    finally:
        r.close()


# ---- 8: without the flag ----
def test_without_the_flag_the_first_update_still_rebuilds(hrt, gpu_available):
    scene = _scene("mixed")
    r = _renderer(hrt, gpu_available, hrt.CTX_FAST_TRACE)
    try:
        r.load_scene(scene)
        n_records = _download(hrt, r)[3]
        assert n_records >= 1.05 * _n_prims(scene)
        before = r.stats()
        r.update_instances(_pose(scene, 1))
        after = r.stats()
        assert after.tlas_rebuilds == before.tlas_rebuilds + 1 and after.tlas_refits == before.tlas_refits
        assert _download(hrt, r)[3] == _n_prims(scene)
    finally:
        r.close()
