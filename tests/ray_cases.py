"""Adversarial rays, one deterministic generator (a plain module like denoise_cases.py, shared by test_adversarial_rays_cpu.py,
test_adversarial_rays_gpu.py and tools/stress_rays.py).

The rays for which a box is culled by one ULP, a clip box of a spatial split is a hair too small or a tie between two leaves is resolved
differently: aimed at exact vertices and exact edge points of the scene's WORLD-SPACE triangles (xf_point's float32 operation order, i.e.
the stored vertex), tangent to its spheres and a hair inside / outside, through sphere centres, from inside spheres, from origins on the
surfaces, with directions scaled by 1e-30 .. 1e30 and components replaced by signed zeros and denormals; a block of axis-parallel rays
whose hit distances coincide bit for bit, from which the two "bound" windows (1e-6, t*) and (t*, 1e16) are made: both comparisons of the
canonical intersector are strict, so every ray at t* loses that hit.

Nothing here knows the product: the classes are judged on the brute-force reference alone (test_adversarial_rays_cpu.py)."""
import numpy as np

VERTEX, EDGE, INTERIOR, TANGENT, CENTRE, INSIDE, PLANE = range(7)
CLASS_NAMES = ("vertex", "edge", "interior", "tangent", "centre", "inside", "plane")
MISS = 0xFFFFFFFF

DISTANCES = (0.0, 1e-6, 0.3, 2.0, 10.0)                    # x extent / 2: the envelope DESIGN.md section 3 states; beyond it nothing is asserted
DIRECTION_SCALES = (1.0, 1.0, 1e-30, 1e30, 1e-3, 37.0)
COMPONENT_VALUES = (0.0, -0.0, 1e-40, -1e-40, 1e-25)
TANGENT_FACTORS = (0.999, 1.0, 1.001)
PLANE_SPEEDS = (-1.0, 1.0, -0.5, 2.0)
OPEN = (1e-6, 1e16)
WINDOWS = (OPEN, (0.0, 1e16), (1e-6, 0.5), (0.25, 3.0))


def _xf_points(m, p):
    """xf_point of oracle.c / the product: ((m0*x + m1*y) + m2*z) + m3, every operation rounded to float32."""
    m = np.asarray(m, np.float32)
    p = np.asarray(p, np.float32)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    return np.stack([((m[4 * r] * x + m[4 * r + 1] * y) + m[4 * r + 2] * z) + m[4 * r + 3] for r in range(3)], axis=-1).astype(np.float32)


def _is_identity(m):
    return np.array_equal(np.asarray(m, np.float32), np.float32([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]))


def world_triangles(scene):
    """(n, 3, 3) float32 world-space vertices as the flattened oracle and the product store them, with the (n,) primitive and instance
    indices.  Identity instances keep their vertices."""
    tris, prim, inst = [np.zeros((0, 3, 3), np.float32)], [np.zeros(0, np.uint32)], [np.zeros(0, np.uint32)]
    for i, it in enumerate(scene["instances"]):
        if it["geometry"] != "triangles":
            continue
        v = np.ascontiguousarray(it["vertices"], np.float32).reshape(-1, 3, 3)
        tris.append(v if _is_identity(it["transform"]) else _xf_points(it["transform"], v))
        prim.append(np.arange(len(v), dtype=np.uint32))
        inst.append(np.full(len(v), i, np.uint32))
    return np.concatenate(tris), np.concatenate(prim), np.concatenate(inst)


def object_spheres(scene):
    """Centres (n, 3) and radii (n,) in OBJECT space (where both canonical modes intersect them), the (n, 12) instance transforms,
    and the primitive and instance indices."""
    c, r, m, prim, inst = [np.zeros((0, 3))], [np.zeros(0)], [np.zeros((0, 12))], [np.zeros(0, np.uint32)], [np.zeros(0, np.uint32)]
    for i, it in enumerate(scene["instances"]):
        if it["geometry"] != "spheres":
            continue
        k = len(it["radii"])
        c.append(np.asarray(it["centers"], np.float64).reshape(-1, 3))
        r.append(np.asarray(it["radii"], np.float64))
        m.append(np.repeat(np.asarray(it["transform"], np.float64).reshape(1, 12), k, 0))
        prim.append(np.arange(k, dtype=np.uint32))
        inst.append(np.full(k, i, np.uint32))
    return np.concatenate(c), np.concatenate(r), np.concatenate(m), np.concatenate(prim), np.concatenate(inst)


def scene_extent(scene):
    """The largest edge of the scene's world-space bounding box."""
    tris = world_triangles(scene)[0].reshape(-1, 3).astype(np.float64)
    c, r, m = object_spheres(scene)[:3]
    pts = [tris]
    for sx in (-1, 1):
        for sy in (-1, 1):
            for sz in (-1, 1):
                pts.append(_to_world(m, c + r[:, None] * np.array([sx, sy, sz])))
    pts = np.concatenate(pts)
    return float((pts.max(0) - pts.min(0)).max())


def _to_world(m, p):
    m = m.reshape(-1, 3, 4)
    return np.einsum("nij,nj->ni", m[:, :, :3], p) + m[:, :, 3]


def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _perpendicular(rng, u):
    d = np.cross(u, _unit(rng, len(u)))
    return d / np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-30)


def _plane_block(scene, n, rng):
    """Axis-parallel rays whose hit distances coincide bit for bit.  Where the scene has an axis-aligned face (three vertices sharing a
    coordinate exactly; the largest such plane wins, of equal ones the last: the Cornell box's back wall z = 1) the origins lie in a parallel plane at a dyadic
    distance (0.75: z = 0.25), spread over the face's extent, d = s x axis with s in PLANE_SPEEDS: t = 0.75 / s exactly, whichever
    triangle of the plane is hit.  A scene without such a face (a soup) gets the ray along the dominant axis of its largest triangle's
    normal through that triangle's centroid instead, from 0.75 away, with the same speeds and every combination of signed zeros in the
    other two components: equal distances by construction, for the window test only."""
    tris = world_triangles(scene)[0].astype(np.float64)
    speeds = np.asarray(PLANE_SPEEDS)[rng.integers(0, len(PLANE_SPEEDS), n)]
    best = None
    for axis in range(3):
        flat = (tris[:, 0, axis] == tris[:, 1, axis]) & (tris[:, 0, axis] == tris[:, 2, axis])
        if not flat.any():
            continue
        area = 0.5 * np.linalg.norm(np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]), axis=1)
        for value in np.unique(tris[flat, 0, axis]):
            sel = flat & (tris[:, 0, axis] == value)
            if best is None or area[sel].sum() >= best[0]:             # (of equal planes the last: the back wall)
                best = (area[sel].sum(), axis, value, tris[sel].reshape(-1, 3))
    o = np.zeros((n, 3))
    d = np.zeros((n, 3))
    if best is not None:
        _, axis, value, pts = best
        lo, hi = pts.min(0), pts.max(0)
        o[:] = rng.uniform(lo + 0.02 * (hi - lo), hi - 0.02 * (hi - lo), (n, 3))
        inside = value > 0.5 * (tris[..., axis].min() + tris[..., axis].max())       # the origins go to the side the scene is on
        o[:, axis] = value - 0.75 if inside else value + 0.75
        d[np.arange(n), axis] = speeds if inside else -speeds
    else:
        nrm = np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0])
        k = int(np.argmax(np.linalg.norm(nrm, axis=1)))
        axis = int(np.argmax(np.abs(nrm[k])))
        o[:] = tris[k].mean(0).astype(np.float32)
        o[:, axis] -= 0.75
        d[:] = rng.choice([0.0, -0.0], (n, 3))
        d[np.arange(n), axis] = speeds
    return o, d


def adversarial_rays(scene, n, seed, extent=None, distances=DISTANCES, details=False):
    """n rays: (o (n, 3) float32, d (n, 3) float32, class label (n,) uint8); with details=True also a dict of per-ray arrays:
    target_prim / target_inst (the primitive aimed at; MISS for classes without one), dist (the origin's distance from its target, in
    units of extent / 2), scale (the direction's scale), replaced (a component was replaced), tiny (by a value other than zero), factor (tangent rays: 0.999 / 1 / 1.001)."""
    rng = np.random.default_rng(seed)
    extent = scene_extent(scene) if extent is None else float(extent)
    tris, tprim, tinst = world_triangles(scene)
    tris = tris.astype(np.float64)
    sc, sr, sm, sprim, sinst = object_spheres(scene)
    n_plane = (2 * n) // 15
    rest = n - n_plane
    shares = (0.3, 0.2, 0.1, 0.24, 0.08, 0.08) if len(sr) else (0.3, 0.3, 0.4, 0.0, 0.0, 0.0)
    if not len(tris):
        shares = (0.0, 0.0, 0.0, 0.6, 0.2, 0.2)
    counts = [int(rest * s) for s in shares]
    counts[INTERIOR if len(tris) else TANGENT] += rest - sum(counts)
    cls = np.concatenate([np.full(c, k, np.uint8) for k, c in enumerate(counts)] + [np.full(n_plane, PLANE, np.uint8)])
    target = np.zeros((n, 3))
    d = _unit(rng, n)
    target_prim = np.full(n, MISS, np.uint32)
    target_inst = np.full(n, MISS, np.uint32)
    factor = np.ones(n)

    tri_rays = np.flatnonzero(cls <= INTERIOR)
    if len(tri_rays):
        i = rng.integers(0, len(tris), len(tri_rays))
        w = rng.dirichlet([0.3, 0.3, 0.3], len(tri_rays))                   # interior points that like vertices and edges
        c = cls[tri_rays]
        w[c == VERTEX] = np.eye(3)[rng.integers(0, 3, int((c == VERTEX).sum()))]                       # exactly a vertex
        e = np.flatnonzero(c == EDGE)
        w[e, rng.integers(0, 3, len(e))] = 0.0                                                       # exactly on an edge
        w[e] /= np.maximum(w[e].sum(1, keepdims=True), 1e-30)
        target[tri_rays] = (tris[i] * w[:, :, None]).sum(1)
        target_prim[tri_rays], target_inst[tri_rays] = tprim[i], tinst[i]

    sph_rays = np.flatnonzero((cls >= TANGENT) & (cls <= INSIDE))
    if len(sph_rays):
        i = rng.integers(0, len(sr), len(sph_rays))
        c = cls[sph_rays]
        u = _unit(rng, len(sph_rays))
        lin = sm[i].reshape(-1, 3, 4)[:, :, :3]
        f = np.where(c == TANGENT, rng.choice(TANGENT_FACTORS, len(sph_rays)), np.where(c == CENTRE, 0.0, rng.uniform(0.0, 0.98, len(sph_rays))))
        target[sph_rays] = _to_world(sm[i], sc[i] + (sr[i] * f)[:, None] * u)       # the tangent point, the centre, a point inside
        tan = c == TANGENT
        dw = np.einsum("nij,nj->ni", lin[tan], _perpendicular(rng, u[tan]))         # perpendicular to u in object space, where the sphere is one
        d[sph_rays[tan]] = dw / np.linalg.norm(dw, axis=1, keepdims=True)
        target_prim[sph_rays], target_inst[sph_rays] = sprim[i], sinst[i]
        factor[sph_rays] = np.where(tan, f, 1.0)

    dist = rng.choice(np.asarray(distances, np.float64), n)
    dist[cls == INSIDE] = 0.0                                                    # the origin is the point inside
    o = target - d * (dist * 0.5 * extent)[:, None]
    scale = rng.choice(np.asarray(DIRECTION_SCALES), n)
    d = d * scale[:, None]
    z = rng.random((n, 3)) < 0.08
    d[z] = rng.choice(np.asarray(COMPONENT_VALUES), int(z.sum()))
    tiny = (z & (d != 0)).any(1)                                                 # 1e-40, -1e-40 or 1e-25 among the components
    plane = cls == PLANE
    if n_plane:
        o[plane], d[plane] = _plane_block(scene, n_plane, rng)
        dist[plane], scale[plane], z[plane], tiny[plane] = 0.0, 1.0, False, False
    o = o.astype(np.float32)
    with np.errstate(over="ignore", under="ignore"):
        d = d.astype(np.float32)
    d[(d == 0).all(1)] = np.float32([0, 0, 1])
    if not details:
        return o, d, cls
    return o, d, cls, {"target_prim": target_prim, "target_inst": target_inst, "dist": dist, "scale": scale, "replaced": z.any(1), "tiny": tiny, "factor": factor}


def bound_windows(t, prim):
    """The two windows made from the reference's open-window records: t* is the most frequent bit pattern among the hit distances (the
    smallest of equally frequent ones).  Returns ((1e-6, t*), (t*, 1e16)), t* and the mask of rays at t*."""
    hit = np.asarray(prim) != MISS
    bits, count = np.unique(np.asarray(t, np.float32)[hit].view(np.uint32), return_counts=True)
    star = np.uint32(bits[np.argmax(count)]).view(np.float32)
    at = hit & (np.asarray(t, np.float32).view(np.uint32) == star.view(np.uint32))
    return ((OPEN[0], float(star)), (float(star), OPEN[1])), float(star), at


def six_windows(t_open, prim_open):
    return WINDOWS + bound_windows(t_open, prim_open)[0]


def scaled(scene, k):
    """Every vertex, centre, radius, translation and the camera multiplied by 2^k: exact in float32."""
    s = np.float32(2.0 ** k)
    out = dict(scene, instances=[], camera=dict(scene["camera"]))
    for it in scene["instances"]:
        it = dict(it)
        for key in ("vertices", "centers", "radii"):
            if key in it:
                it[key] = (np.asarray(it[key], np.float32) * s).astype(np.float32)
        m = np.asarray(it["transform"], np.float32).copy()
        m[[3, 7, 11]] *= s
        it["transform"] = m
        out["instances"].append(it)
    for key in ("center", "target"):
        out["camera"][key] = (np.asarray(scene["camera"][key], np.float32) * s).astype(np.float32)
    return out


def translated(scene, v):
    """Every instance transform's translation, and the camera, moved by v: the object-space geometry stays, the world goes elsewhere."""
    v = np.asarray(v, np.float32)
    out = dict(scene, instances=[], camera=dict(scene["camera"]))
    for it in scene["instances"]:
        it = dict(it)
        m = np.asarray(it["transform"], np.float32).copy()
        m[[3, 7, 11]] = (m[[3, 7, 11]] + v).astype(np.float32)
        it["transform"] = m
        out["instances"].append(it)
    for key in ("center", "target"):
        out["camera"][key] = (np.asarray(scene["camera"][key], np.float32) + v).astype(np.float32)
    return out


def tame(info):
    """Rays whose every intermediate of the canonical intersector stays a normal float when the scene is scaled by 2^+-20: directions
    of scale 1e-3 .. 37 without a denormal or 1e-25 component (zeros are exact at every scale).  For these the scaled scene's record is
    the unscaled one's with t x 2^k, bit for bit: every operation of isect_tri / isect_sph / xf_point is homogeneous in the scale."""
    return np.isin(info["scale"], (1.0, 1e-3, 37.0)) & ~info["tiny"]


def records_differ(got, want):
    """Closest-hit records (t, u, v, prim, inst), bit for bit: the mask of differing rays."""
    diff = (np.asarray(got[3]) != np.asarray(want[3])) | (np.asarray(got[4]) != np.asarray(want[4]))
    for k in range(3):
        diff |= np.asarray(got[k], np.float32).view(np.uint32) != np.asarray(want[k], np.float32).view(np.uint32)
    return diff


# ---- the scenes both test files use (s = the package's scenes module) ----
BODY_TRIANGLES, BODY_EDGE, BODY_INSTANCES = 6000, 0.2, 4


def bodies_scene(s):
    """One shared triangle BLAS -- the vertices of random_soup(6000, 0.2): long triangles, so that a split build duplicates references --
    instanced four times with rigid_transform, one of them scaled unevenly, plus a sphere instance under a transform: _bodies_scene of
    test_two_level_fast_trace_gpu.py in small.  Four instances, not three: that file's criterion for "two-level" is fewer than a third of the
    flattened tree's nodes, which a tree over three instances of one BLAS cannot have at any edge length (measured at 0.2 / 0.3 / 0.4: 0.343,
    0.347, 0.344 of the flattened tree's nodes, records x 1.9 each time); the edge length stays 0.2."""
    v = s.random_soup(BODY_TRIANGLES, BODY_EDGE, 9, 64, 64, 1)["instances"][0]["vertices"]
    base = s._tri_instance(v, s.WHITE)
    inst = []
    for k in range(BODY_INSTANCES):
        it = dict(base)
        it["shape"] = "soup"
        m = s.rigid_transform([-0.6 + 1.2 * (k % 2), -0.45 + 0.9 * (k // 2), 0.1 * k], [np.cos(1.3 * k), np.sin(2.1 * k) + 0.2, np.cos(0.7 * k + 1.0)], 0.5 + 0.9 * k, 0.4)
        if k == 2:
            m = m.reshape(3, 4).astype(np.float64)
            m[:, :3] = m[:, :3] @ np.diag([1.3, 0.75, 1.0])
            m = m.astype(np.float32).reshape(12)
        it["transform"] = m
        inst.append(it)
    inst.append(s._sphere_instance([[-0.45, 0.0, -0.6], [0.5, 0.05, -0.7], [0.0, -0.9, 0.3]], [0.3, 0.25, 0.2], s.STEEL, "metal", 0.05,
                                   s.rigid_transform([0.02, 0.0, -0.05], [0.2, 1.0, 0.1], 0.4, 1.1)))
    return {"name": "soup-bodies-small", "instances": inst, "camera": s._soup_camera(), "background": s.BACKGROUND.copy(), "width": 64, "height": 64, "spp": 1}


def moved(s, scene, step):
    """Every instance of the scene moved by a small rigid step: a turn about an axis of its own and a shift, in front of its transform."""
    out = dict(scene, instances=[dict(it) for it in scene["instances"]])
    for k, it in enumerate(out["instances"]):
        a = np.vstack([s.rigid_transform([0.03 * step, -0.02 * step * (1 + k % 2), 0.01 * step], [0.3 + k, 1.0, 0.2 * k], 0.05 * step * (1 + k % 3)).reshape(3, 4).astype(np.float64), [0, 0, 0, 1]])
        b = np.vstack([np.asarray(it["transform"], np.float64).reshape(3, 4), [0, 0, 0, 1]])
        it["transform"] = (a @ b)[:3].astype(np.float32).reshape(12)
    return out


def _mixed(s):
    return s.mixed_test_scene(2500, 50, 13)


# name -> (scene, rays, seed).  The first three are the host builder's (test_adversarial_rays_cpu.py), the others the device's.
CASES = {
    "soup-3000": (lambda s: s.random_soup(3000, 0.15, 5, 64, 64, 1), 20000, 3),
    "soup-200": (lambda s: s.random_soup(200, 0.3, 7, 64, 64, 1), 20000, 3),
    "cornell": (lambda s: s.cornell_box(64, 64, 1), 20000, 3),
    "mixed": (_mixed, 12000, 3),                                                       # spheres, transforms, all four programs
    "cornell-12k": (lambda s: s.cornell_box(64, 64, 1), 12000, 3),                     # triangles only
    "soup-6000": (lambda s: s.random_soup(6000, 0.15, 5, 64, 64, 1), 12000, 3),        # above the device build's 4096-primitive threshold
    "bodies": (bodies_scene, 12000, 3),
    "mixed-moved": (lambda s: moved(s, moved(s, _mixed(s), 1), 2), 12000, 3),          # after two updates
    "mixed-far": (lambda s: translated(_mixed(s), (1000, -500, 250)), 12000, 3),
}
