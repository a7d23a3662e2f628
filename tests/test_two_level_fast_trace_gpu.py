"""HRT_CTX_FAST_TRACE | HRT_CTX_TWO_LEVEL: the reference's own configuration -- every GAS built with PREFER_FAST_TRACE
(src/Global/RendererImpl.cu:94,118,144) under an IAS that is updated every frame (:180, :210-242) -- as a two-level tree whose shared BLAS
trees carry spatial splits.  The object space of a BLAS is where a split is valid for ever: hrt_tlas_update refits the top level only.

Parity bar as for every two-level tree: hit records and frames BIT-EXACT against the oracle's INSTANCED mode (duplicate references cannot
change the canonical hit).  What is new is checked on the structure: it is two-level AND split, it stays so through updates and rebuilds,
BLASes too small for the split phase are byte for byte what HRT_CTX_TWO_LEVEL alone builds, every combination that cannot have the tree
falls back to what it had before, and the split tree costs fewer node visits plus primitive tests than the unsplit one (CPU walk)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_TRI, EDGE, N_BODIES = 60000, 0.06, 6          # the soup of test_fast_trace_tree_with_spatial_splits: long thin triangles, references get duplicated
W, H, SPP = 112, 72, 2


def _body_transform(hrt, k, step=0):
    """Body k of the scene at animation step `step`: a rotation about its own axis, a place in a 3 x 2 grid, scale 0.4 -- one of them scaled
    unevenly -- and from step to step a little further along and around."""
    axis = np.array([np.cos(1.3 * k), np.sin(2.1 * k) + 0.2, np.cos(0.7 * k + 1.0)])
    pos = np.array([-0.95 + 0.95 * (k % 3), -0.5 + 1.0 * (k // 3), -0.2 + 0.1 * k]) + step * np.array([0.02, -0.015 * (1 + k % 2), 0.01])
    m = hrt.scenes.rigid_transform(pos, axis, 0.5 + 0.9 * k + 0.07 * step, 0.4).reshape(3, 4).astype(np.float64)
    if k == 2:
        m[:, :3] = m[:, :3] @ np.diag([1.3, 0.75, 1.0])
    return m.astype(np.float32).reshape(12)


def _bodies_scene(hrt, n_bodies=N_BODIES, small=0, small_first=True):
    """One triangle BLAS -- the vertices of random_soup(60000, 0.06) -- instanced n_bodies times with distinct rotations, translations and
    one non-uniform scale, plus a sphere BLAS; `small` more instances of two small shared shapes (far below 4096 primitives)."""
    sc = hrt.scenes
    v = sc.random_soup(N_TRI, EDGE, 9, W, H, SPP)["instances"][0]["vertices"]
    base = sc._tri_instance(v, sc.WHITE)
    bodies = []
    for k in range(n_bodies):
        it = dict(base)
        it["shape"] = "soup"
        it["transform"] = _body_transform(hrt, k)
        it["albedo"] = (sc.WHITE, sc.RED, sc.GREEN, sc.SAND)[k % 4]
        if k % 3 == 1:
            it["material"], it["albedo"], it["fuzz"] = "metal", sc.STEEL, 0.1 * k
        bodies.append(it)
    shapes = [sc._tri_instance(sc._blob_shape(2, 0.09, s), sc.SAND) for s in (1, 2)]
    smalls = []
    for k in range(small):
        it = dict(shapes[k % 2])
        it["shape"] = "blob%d" % (k % 2)
        it["transform"] = sc.rigid_transform([-1.2 + 2.4 * k / max(small - 1, 1), 0.0, 0.75], [0.3, 1.0, 0.2 * k], 0.4 * k, 1.0 + 0.1 * (k % 3))
        smalls.append(it)
    spheres = sc._sphere_instance([[-0.45, 0.0, -0.6], [0.5, 0.05, -0.7], [0.0, -0.9, 0.3]], [0.3, 0.25, 0.2], sc.STEEL, "metal", 0.05,
                                  np.array([1, 0, 0, 0.02, 0, 1, 0, 0.0, 0, 0, 1, -0.05], dtype=np.float32))
    inst = (smalls + bodies if small_first else bodies + smalls) + [spheres]
    return {"name": "soup-bodies", "instances": inst, "camera": sc._soup_camera(), "background": sc.BACKGROUND.copy(), "width": W, "height": H, "spp": SPP}


def _unique_prims(scene):
    seen, n = set(), 0
    for it in scene["instances"]:
        key = it.get("shape", id(it))
        if key in seen:
            continue
        seen.add(key)
        n += len(it["vertices"]) if it["geometry"] == "triangles" else len(it["radii"])
    return n


def _renderer(hrt, gpu_available, flags):
    if not gpu_available:
        pytest.skip("no GPU in this container")
    return hrt.Renderer(0, flags)


def _load(r, scene):
    """load_scene, and one ray: the statistics describe the tree that was traced last."""
    r.load_scene(scene)
    r.trace_rays(np.array([[0, 0, 5]], np.float32), np.array([[0, 0, -1]], np.float32))
    return r.stats()


def _tree_stats(hrt, gpu_available, scene, flags):
    r = _renderer(hrt, gpu_available, flags)
    try:
        s = _load(r, scene)
        return int(s.bvh_nodes), int(s.bvh_bytes), int(s.bvh_depth)
    finally:
        r.close()


def _frame(r, w, h, salt, spp):
    r.set_frame(w, h, salt, linear=True)
    r.reset_stats()
    r.render(spp)
    return r.linear.cpu().numpy().copy(), r.color.cpu().numpy().copy(), r.rng_states_numpy().copy(), int(r.stats().rays)


def _frame_is_the_oracles(oracle, r, scene, salt, instanced=True, w=W, h=H, spp=SPP):
    lin, col, states, rays = _frame(r, w, h, salt, spp)
    ref_states = oracle.rng_init(w, h, salt)
    ref = oracle.OracleScene(scene, instanced=instanced).render(w, h, ref_states, spp)
    assert np.array_equal(lin.view(np.uint32), ref["linear"].view(np.uint32)), "linear radiance must be bit-exact"
    assert np.array_equal(col.view(np.uint32), ref["color"].view(np.uint32)), "the colour image must be bit-exact"
    assert np.array_equal(states, ref_states), "the RNG streams must end where the oracle's end"
    assert rays == ref["rays"]
    return lin


def _hits_are_the_oracles(oracle, r, scene, n_rays, seed, brute=False, instanced=True):
    o, d = oracle.random_rays(n_rays, seed)
    osc = oracle.OracleScene(scene, force_brute=brute, instanced=instanced)
    got = r.trace_rays(o, d)
    ref = osc.trace(o, d)
    for g, x in zip(got[:3], ref[:3]):
        assert np.array_equal(g.view(np.uint32), x.view(np.uint32))
    assert np.array_equal(got[3], ref[3]) and np.array_equal(got[4], ref[4])
    assert (got[3] != 0xFFFFFFFF).mean() > 0.2
    any_got = r.trace_rays(o, d, any_hit=True)
    assert np.array_equal(any_got[3] != 0xFFFFFFFF, ref[3] != 0xFFFFFFFF)      # (which hit an any-hit query reports is the traversal's business)
    return got


def _is_split_two_level(stats, unique_prims, flat_nodes):
    payload = int(stats.bvh_bytes) - 80 * int(stats.bvh_nodes)
    return int(stats.bvh_nodes) < flat_nodes / 3 and payload > 48 * unique_prims * 1.05


def test_both_flags_build_a_two_level_tree_whose_blas_is_split(hrt, oracle, gpu_available):
    """Checks 1 and 2 of the issue.  Six instances of one BLAS: the tree has less than a third of the flattened fast-trace tree's nodes, and
    its records outnumber the unique primitives by more than 5 % (the flattened split test's criterion).  Hit records (t, u, v, primitive,
    instance; closest and any hit), linear radiance, colour, RNG end states and ray counts against the oracle's instanced mode, no
    tolerance; and the same hits as the tree HRT_CTX_TWO_LEVEL alone builds."""
    scene = _bodies_scene(hrt)
    unique = _unique_prims(scene)
    assert unique == N_TRI + 3
    flat_nodes, flat_bytes, _ = _tree_stats(hrt, gpu_available, scene, hrt.CTX_FAST_TRACE)
    assert flat_bytes - 80 * flat_nodes > 48 * (N_BODIES * N_TRI + 3) * 1.05         # (the flattened tree of this geometry does duplicate references)
    r = _renderer(hrt, gpu_available, hrt.CTX_FAST_TRACE | hrt.CTX_TWO_LEVEL)
    try:
        s = _load(r, scene)
        payload = int(s.bvh_bytes) - 80 * int(s.bvh_nodes)
        print("two-level split: %d nodes, %d records for %d unique primitives (x %.3f), depth %d; flattened split: %d nodes"
              % (s.bvh_nodes, payload // 48, unique, payload / 48 / unique, s.bvh_depth, flat_nodes))
        assert s.bvh_nodes < flat_nodes / 3
        assert payload > 48 * unique * 1.05
        assert s.bvh_triangles == N_TRI and s.bvh_spheres == 3                       # (primitives, not references)
        got = _hits_are_the_oracles(oracle, r, scene, 40000, 31)
        _hits_are_the_oracles(oracle, r, scene, 3000, 32, brute=True)
        _frame_is_the_oracles(oracle, r, scene, 77)
        assert r.stats().fused_fallback_launches == 0
    finally:
        r.close()
    r = _renderer(hrt, gpu_available, hrt.CTX_TWO_LEVEL)
    try:
        s = _load(r, scene)
        assert int(s.bvh_bytes) - 80 * int(s.bvh_nodes) == 48 * unique               # HRT_CTX_TWO_LEVEL alone: a record per primitive, as ever
        o, d = oracle.random_rays(40000, 31)
        plain = r.trace_rays(o, d)
        for a, b in zip(got, plain):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    finally:
        r.close()


@pytest.mark.parametrize("update", ["synchronous", "asynchronous"])
def test_the_split_blas_survives_updates_and_rebuilds(hrt, oracle, gpu_available, update):
    """Check 3.  Instances move and turn, several updates in a row: every one is a refit (of the top level), none a rebuild, node and
    record counts stay, every frame is the oracle's of the new transforms.  A forced rebuild (a visibility bit changes, and changes
    back) builds a two-level tree again out of the BLAS's cached split tree: the same node and record counts as the first build."""
    scene = _bodies_scene(hrt)
    unique = _unique_prims(scene)
    flat_nodes, _, _ = _tree_stats(hrt, gpu_available, scene, hrt.CTX_FAST_TRACE)
    r = _renderer(hrt, gpu_available, hrt.CTX_FAST_TRACE | hrt.CTX_TWO_LEVEL | (hrt.CTX_ASYNC_UPDATE if update == "asynchronous" else 0))
    try:
        built = _load(r, scene)
        assert _is_split_two_level(built, unique, flat_nodes)
        start = [it["transform"].copy() for it in scene["instances"]]
        before = built
        for step in (1, 2, 3, 4):
            xf = [_body_transform(hrt, k, step) for k in range(N_BODIES)] + [start[-1]]
            r.update_instances(xf)
            for it, m in zip(scene["instances"], xf):
                it["transform"] = m
            now = r.stats()
            assert now.tlas_refits == before.tlas_refits + 1 and now.tlas_rebuilds == built.tlas_rebuilds, (step, int(now.tlas_refits), int(now.tlas_rebuilds))
            assert now.bvh_nodes == built.bvh_nodes and now.bvh_bytes == built.bvh_bytes
            _frame_is_the_oracles(oracle, r, scene, 100 + step)
            _hits_are_the_oracles(oracle, r, scene, 6000, step)
            before = r.stats()
        # a visibility bit changes: the update has to rebuild (an asynchronous one learns it from the device and rebuilds at the next update)
        def update_that_rebuilds():
            r.update_instances(start)
            if update == "asynchronous":
                r.update_instances(start)
        r._h_inst[1].visibilityMask = 0
        update_that_rebuilds()
        hidden = r.stats()
        assert hidden.tlas_rebuilds == built.tlas_rebuilds + 1
        assert hidden.bvh_bytes - 80 * hidden.bvh_nodes == built.bvh_bytes - 80 * built.bvh_nodes      # the same records: the cached split tree
        assert hidden.bvh_nodes < built.bvh_nodes                                                        # (one transform node fewer, at least)
        r._h_inst[1].visibilityMask = 1
        update_that_rebuilds()
        again = r.stats()
        assert again.tlas_rebuilds == built.tlas_rebuilds + 2
        assert again.bvh_nodes == built.bvh_nodes and again.bvh_bytes == built.bvh_bytes and again.bvh_depth == built.bvh_depth
        for it, m in zip(scene["instances"], start):
            it["transform"] = m
        _frame_is_the_oracles(oracle, r, scene, 200)
        # ... and the rebuilt tree is refitted like the first one
        xf = [_body_transform(hrt, k, 1) for k in range(N_BODIES)] + [start[-1]]
        r.update_instances(xf)
        for it, m in zip(scene["instances"], xf):
            it["transform"] = m
        after = r.stats()
        assert after.tlas_refits == again.tlas_refits + 1 and after.tlas_rebuilds == again.tlas_rebuilds and after.bvh_bytes == built.bvh_bytes
        _frame_is_the_oracles(oracle, r, scene, 201)
        assert r.stats().fused_fallback_launches == 0
    finally:
        r.close()


def _download(hrt, r):
    blob = hrt.BvhBlob()
    assert r.lib.hrt_tlas_download(r.ctx, r.tlas, C.byref(blob)) == 0
    nodes = np.ctypeslib.as_array(C.cast(blob.nodes, C.POINTER(C.c_uint8)), shape=(blob.n_nodes * 80,)).copy()
    prims = np.ctypeslib.as_array(C.cast(blob.triangles, C.POINTER(C.c_uint8)), shape=(max(blob.n_triangles, 1) * 48,)).copy()
    r.lib.hrt_host_free(C.byref(blob))
    return nodes, prims


def _signature(nodes, prims):
    """What two builds of one tree have in common: the emission hands out child and record blocks from atomic cursors, so the ORDER of the
    blocks differs from build to build; what they hold does not -- nodes without their two block offsets, and records, as sorted rows
    (test_device_split_build_is_deterministic_and_fast)."""
    nd = nodes.reshape(-1, 80).copy(); nd[:, 16:24] = 0
    pr = prims.reshape(-1, 48)
    return nd[np.lexsort(nd.T[::-1])], pr[np.lexsort(pr.T[::-1])]


def test_small_blases_are_untouched(hrt, oracle, gpu_available):
    """Check 4.  The particle cloud of test_two_level_gpu.py (shapes far below 4096 primitives): both flags give the node count, the
    bytes, the image -- and the very nodes and records -- of HRT_CTX_TWO_LEVEL alone.  A scene that mixes small BLASes with the large one:
    the large one is split, and everything in front of its tree -- the top level and the small BLASes' nodes and records, whose boxes the
    pack's refit now takes from the clip array -- is what HRT_CTX_TWO_LEVEL alone builds, bit for bit; the image is the same, and the
    oracle's."""
    cloud = hrt.scenes.particle_cloud(500, 96, 64, 1)
    out = {}
    for name, flags in (("two", hrt.CTX_TWO_LEVEL), ("both", hrt.CTX_TWO_LEVEL | hrt.CTX_FAST_TRACE)):
        r = _renderer(hrt, gpu_available, flags)
        try:
            s = _load(r, cloud)
            out[name] = (int(s.bvh_nodes), int(s.bvh_bytes), int(s.bvh_alloc_bytes), int(s.bvh_depth)) + _signature(*_download(hrt, r)) + (_frame(r, 96, 64, 3, 1)[0],)
        finally:
            r.close()
    assert out["two"][:4] == out["both"][:4]
    for a, b in zip(out["two"][4:], out["both"][4:]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))

    mixed = _bodies_scene(hrt, n_bodies=2, small=9)           # instances 0-8: two small shapes; 9, 10: the soup; 11: the spheres
    small_records = 2 * 8 * 4 ** 2
    out = {}
    for name, flags in (("two", hrt.CTX_TWO_LEVEL), ("both", hrt.CTX_TWO_LEVEL | hrt.CTX_FAST_TRACE)):
        r = _renderer(hrt, gpu_available, flags)
        try:
            s = _load(r, mixed)
            nodes, prims = _download(hrt, r)
            lin = _frame_is_the_oracles(oracle, r, mixed, 5)
            # the BLAS trees lie behind the top level in the order their BLASes first appear: the small shapes, the soup, the spheres
            w = nodes.view(np.uint32).reshape(-1, 20)
            xform = w[w[:, 3] == 0]
            assert len(xform) == 12
            body_root, sphere_root = int(xform[xform[:, 5] == 9][0, 4]), int(xform[xform[:, 5] == 11][0, 4])
            assert 12 < body_root < sphere_root == int(s.bvh_nodes) - 1
            out[name] = (int(s.bvh_nodes), int(s.bvh_bytes), lin, body_root, _signature(nodes[:80 * body_root], prims[:48 * small_records]),
                         _signature(nodes[80 * sphere_root:], prims[-48 * 3:]))
        finally:
            r.close()
    two, both = out["two"], out["both"]
    assert two[1] - 80 * two[0] == 48 * _unique_prims(mixed)
    assert both[1] - 80 * both[0] > 48 * _unique_prims(mixed) * 1.05      # the large BLAS is split ...
    assert np.array_equal(two[2].view(np.uint32), both[2].view(np.uint32))
    # ... the small ones, in front of it and behind it, are not
    assert two[3] == both[3]
    for k in (4, 5):
        for a, b in zip(two[k], both[k]):
            assert np.array_equal(a, b)


def test_combinations_that_cannot_have_the_tree_fall_back(hrt, oracle, gpu_available, monkeypatch):
    """Check 5.  A counting context, the host's fast-trace builder, HRT_TWO_LEVEL=-1 and two levels chosen by size leave
    HRT_CTX_FAST_TRACE what it was: the flattened split tree, node for node.  HRT_TWO_LEVEL=1 asks as the flag does.  A combined tree too
    deep for the path kernel's stack -- the split BLAS under a lowered HRT_FUSED_MAX_DEPTH, and a geometric chain whose BLAS no stack
    could hold -- is built flattened instead (build_two_level: flatten_instead) and renders bit-exact against the oracle's FLATTENED mode."""
    scene = _bodies_scene(hrt, n_bodies=5)
    both = hrt.CTX_FAST_TRACE | hrt.CTX_TWO_LEVEL

    def nodes_of(flags):
        return _tree_stats(hrt, gpu_available, scene, flags)[0]
    flat = nodes_of(hrt.CTX_FAST_TRACE)
    split_two = nodes_of(both)
    assert split_two < flat / 2.5                                # (five instances here)
    assert nodes_of(both | hrt.CTX_COUNT) == nodes_of(hrt.CTX_FAST_TRACE | hrt.CTX_COUNT) == flat
    monkeypatch.setenv("HRT_TWO_LEVEL", "-1")
    assert nodes_of(hrt.CTX_FAST_TRACE) == flat
    assert nodes_of(both) == split_two                           # (the context flag asks for two levels whatever the environment says: include/hrt.h)
    monkeypatch.setenv("HRT_TWO_LEVEL", "0")
    monkeypatch.setenv("HRT_TWO_LEVEL_MIN_PRIMS", "1000")
    assert nodes_of(0) < flat / 2.5                              # by size (threshold lowered): two levels ...
    assert nodes_of(hrt.CTX_FAST_TRACE) == flat                  # ... but HRT_CTX_FAST_TRACE flattens, as before
    monkeypatch.delenv("HRT_TWO_LEVEL_MIN_PRIMS")
    monkeypatch.setenv("HRT_TWO_LEVEL", "1")
    assert nodes_of(hrt.CTX_FAST_TRACE) == split_two             # asked for through the environment
    monkeypatch.delenv("HRT_TWO_LEVEL")
    monkeypatch.setenv("HRT_FUSED", "0")
    assert nodes_of(both) == flat                                # the wavefront kernels do not walk two-level trees
    monkeypatch.delenv("HRT_FUSED")
    monkeypatch.setenv("HRT_FAST_TRACE_BUILD", "host")
    host_flat = nodes_of(hrt.CTX_FAST_TRACE)
    assert nodes_of(both) == host_flat and host_flat > 2 * split_two
    monkeypatch.delenv("HRT_FAST_TRACE_BUILD")
    # too deep: the flattened split tree instead
    monkeypatch.setenv("HRT_FUSED_MAX_DEPTH", "5")
    r = _renderer(hrt, gpu_available, both)
    try:
        assert _load(r, scene).bvh_nodes == flat
        _frame_is_the_oracles(oracle, r, scene, 9, instanced=False)
    finally:
        r.close()
    monkeypatch.delenv("HRT_FUSED_MAX_DEPTH")
    chain = hrt.scenes.growing_chain(393, 1.0728, 96, 64, 2)
    r = _renderer(hrt, gpu_available, both)
    try:
        r.load_scene(chain)
        _frame_is_the_oracles(oracle, r, chain, 11, instanced=False, w=96, h=64, spp=2)
        st = r.stats()
        assert st.bvh_depth <= 12 and st.bvh_triangles == 393
    finally:
        r.close()


def _camera_rays(scene, nx, ny):
    cam = scene["camera"]
    c, t, up = (np.asarray(cam[k], dtype=np.float64) for k in ("center", "target", "up"))
    fwd = (t - c) / np.linalg.norm(t - c)
    right = np.cross(fwd, up); right /= np.linalg.norm(right)
    upv = np.cross(right, fwd)
    x, y = np.meshgrid(np.linspace(-0.55, 0.55, nx), np.linspace(-0.35, 0.35, ny))
    d = fwd[None, :] + x.reshape(-1, 1) * right[None, :] + y.reshape(-1, 1) * upv[None, :]
    return np.broadcast_to(c, d.shape).astype(np.float32).copy(), d.astype(np.float32)


def test_the_split_tree_costs_less_to_walk(hrt, oracle, gpu_available):
    """Check 6: a condition, not a measurement.  The split and the unsplit two-level tree of the same scene, downloaded and walked on the
    CPU by the oracle's bvh8_walk (which knows transform nodes) over the same 120 000 camera and random rays: the split tree costs
    strictly fewer node visits plus primitive tests per ray and finds identical hits.  No ratio is fixed in advance; the figures are
    printed (tools/two_level_split_counts.py prints them next to the flattened default / split pair of the same soup)."""
    scene = _bodies_scene(hrt)
    inv = np.stack([np.linalg.inv(np.vstack([it["transform"].reshape(3, 4).astype(np.float64), [0, 0, 0, 1]]))[:3].reshape(12)
                    for it in scene["instances"]]).astype(np.float32)
    ident = np.array([int(np.array_equal(it["transform"], hrt.scenes.IDENTITY)) for it in scene["instances"]], dtype=np.uint32)
    co, cd = _camera_rays(scene, 300, 200)
    ro, rd = oracle.random_rays(60000, 41)
    o, d = np.concatenate([co, ro]), np.concatenate([cd, rd])
    assert len(o) >= 100000
    res = {}
    for name, flags in (("unsplit", hrt.CTX_TWO_LEVEL), ("split", hrt.CTX_TWO_LEVEL | hrt.CTX_FAST_TRACE)):
        r = _renderer(hrt, gpu_available, flags)
        try:
            r.load_scene(scene)
            nodes, prims = _download(hrt, r)
            res[name] = oracle.bvh8_trace(nodes.ctypes.data, prims.ctypes.data, o, d, inst_inv=inv, inst_identity=ident)
            gpu = r.trace_rays(o, d)
            assert np.array_equal(gpu[3], res[name][3]) and np.array_equal(gpu[4], res[name][4])      # (the walk is of the tree the GPU traces)
        finally:
            r.close()
    n = len(o)
    a, b = res["unsplit"], res["split"]
    print("per ray, unsplit: %.3f node visits + %.3f primitive tests; split: %.3f + %.3f; (visits + tests) split / unsplit = %.4f; hit fraction %.2f"
          % (a[5] / n, a[6] / n, b[5] / n, b[6] / n, (b[5] + b[6]) / (a[5] + a[6]), (a[3] != 0xFFFFFFFF).mean()))
    for x, y in zip(a[:5], b[:5]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert (a[3] != 0xFFFFFFFF).mean() > 0.3
    assert b[5] + b[6] < a[5] + a[6]
