"""HRT_CTX_KEEP_SPLITS, the geometry on the CPU: hrt_host_clip_barycentric gives the part of a triangle inside a box as ranges of the
triangle's own barycentric coordinates (csrc/bvh8_geom.h: clip_triangle_barycentric, what a flattened split tree keeps per record), and
the refit's rule turns the ranges into a world box wherever the triangle has gone since (bary_hexagon_box, restated here in numpy).

Checked: every point of the triangle inside the box has its barycentrics inside the ranges (no tolerance: the ranges carry their own
slack, below 0 and above 1 too); under 50 affine maps per case, singular ones among them, the image of every such point lies inside
the hexagon's box; an empty intersection and a box around the whole triangle give the full ranges; and a plain case gives the ranges
one computes by hand."""
import numpy as np

N_CASES, N_POINTS, N_MAPS = 400, 96, 50
SLACK = 1.0e-6                      # kBaryClipSlack


def _clip(lib, tri, box):
    tri = np.ascontiguousarray(tri, np.float32).reshape(9)
    box = np.ascontiguousarray(box, np.float32).reshape(6)
    out = np.zeros(6, np.float32)
    assert lib.hrt_host_clip_barycentric(tri.ctypes.data, box.ctypes.data, out.ctypes.data) == 0
    return out


def _record(tri):
    """(v0, e1, e2) as the builders hold a triangle: the edges rounded to float."""
    tri = np.asarray(tri, np.float32).reshape(3, 3)
    return tri[0].astype(np.float64), (tri[1] - tri[0]).astype(np.float32).astype(np.float64), (tri[2] - tri[0]).astype(np.float32).astype(np.float64)


def _cases(seed=5):
    """Triangles -- ordinary, thin, degenerate (a segment, a point) and huge -- each with a box that cuts it somewhere."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(N_CASES):
        kind = ("ordinary", "thin", "degenerate", "huge")[k % 4]
        c = rng.uniform(-1, 1, 3)
        e1, e2 = rng.uniform(-0.4, 0.4, 3), rng.uniform(-0.4, 0.4, 3)
        if kind == "thin":
            e2 = e1 * rng.uniform(0.2, 1.5) + rng.uniform(-1e-4, 1e-4, 3)
        if kind == "degenerate":
            e2 = e1 * rng.uniform(-0.5, 1.5) if k % 8 < 4 else np.zeros(3)
            if k % 16 == 2:
                e1 = np.zeros(3)
        tri = np.stack([c, c + e1, c + e2])
        if kind == "huge":
            tri = tri * 10.0 ** rng.uniform(4, 30)
        tri = tri.astype(np.float32)
        v0, f1, f2 = _record(tri)
        w = rng.dirichlet([1, 1, 1])
        p = v0 + w[1] * f1 + w[2] * f2                                   # a point of the triangle the box is put around
        ext = np.maximum(np.abs(f1), np.abs(f2)) + 1e-3 * max(np.abs(v0).max(), 1e-3)
        half = ext * rng.uniform(0.05, 0.8, 3)
        if k % 5 == 0:
            half[rng.integers(0, 3)] = np.inf                              # a slab: the cell of a first split
        box = np.concatenate([p - half * rng.uniform(0.2, 1.0, 3), p + half * rng.uniform(0.2, 1.0, 3)]).astype(np.float32)
        out.append((kind, tri, box))
    return out


def _points_inside(tri, box, rng):
    """Points of the triangle (record form) inside the closed box, by rejection: (u, v) and the points."""
    v0, e1, e2 = _record(tri)
    w = rng.dirichlet([0.6, 0.6, 0.6], N_POINTS)
    w[:3] = np.eye(3)                                                     # the corners too
    u, v = w[:, 1], w[:, 2]
    with np.errstate(over="ignore", invalid="ignore"):
        p = v0 + u[:, None] * e1 + v[:, None] * e2
        keep = ((p >= box[:3].astype(np.float64)) & (p <= box[3:].astype(np.float64))).all(1)
    return u[keep], v[keep]


def _hexagon_box(g, v0, e1, e2):
    """The refit's rule (csrc/bvh8_geom.h: bary_hexagon_box) in double, without its widening: the box of the eight candidate points, or
    the whole primitive's where an interval comes out empty."""
    g = g.astype(np.float64)
    s0, s1 = 1.0 - g[5], 1.0 - g[4]
    pts, ok = [], True
    for j in (0, 1):
        u = g[j]
        a, b = max(g[2], s0 - u), min(g[3], s1 - u)
        ok = ok and a <= b
        pts += [(u, a), (u, b)]
        v = g[2 + j]
        a, b = max(g[0], s0 - v), min(g[1], s1 - v)
        ok = ok and a <= b
        pts += [(a, v), (b, v)]
    if not ok:
        pts = [(0.0, 0.0), (1.0, 0.0), (0.0, 1.0)]
    p = np.array([v0 + a * e1 + b * e2 for a, b in pts])
    return p.min(0), p.max(0), ok


def _random_map(rng, k):
    a = rng.normal(size=(3, 3)) * 10.0 ** rng.uniform(-1, 1)
    if k % 5 == 1:
        a[:, rng.integers(0, 3)] = 0.0                                    # an axis scaled to 0
    elif k % 5 == 2:
        a = np.outer(rng.normal(size=3), rng.normal(size=3))              # rank 1
    elif k % 5 == 3:
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        a = q @ np.diag(rng.uniform(0.2, 3.0, 3))                         # a rotation with non-uniform scale
    return a, rng.uniform(-2, 2, 3)


def test_points_inside_the_box_are_inside_the_ranges_and_stay_inside_the_hexagon_box(hrt):
    lib = hrt.load_library()
    rng = np.random.default_rng(11)
    with_points = clipped = empty_intervals = maps_of_huge = 0
    for kind, tri, box in _cases():
        g = _clip(lib, tri, box)
        assert (g >= -SLACK).all() and (g <= 1 + SLACK).all() and (g[0::2] <= g[1::2]).all(), (kind, g)
        u, v = _points_inside(tri, box, rng)
        if not len(u):
            continue
        with_points += 1
        clipped += int((g[1::2] - g[0::2]).min() < 0.999)
        w = 1.0 - u - v
        for q, x in enumerate((u, v, w)):
            assert (x >= g[2 * q]).all() and (x <= g[2 * q + 1]).all(), (kind, q, g, x.min(), x.max())
        src = tri.astype(np.float64)
        for k in range(N_MAPS):
            a, t = _random_map(rng, k)
            if kind == "huge":
                a, t = a * 1e-2, t * np.abs(src).max()                   # (coordinates up to 1e30: the image stays a float, the shift is of the triangle's size)
            with np.errstate(over="ignore"):
                moved = (src @ a.T + t).astype(np.float32)
            if not np.isfinite(moved).all():
                continue
            maps_of_huge += int(kind == "huge")
            v0, e1, e2 = _record(moved)
            lo, hi, ok = _hexagon_box(g, v0, e1, e2)
            empty_intervals += int(not ok)
            p = v0 + u[:, None] * e1 + v[:, None] * e2
            tol = 1e-12 * (np.abs(v0) + np.abs(e1) + np.abs(e2))         # (double rounding of the candidate points and of p)
            assert (p >= lo - tol).all() and (p <= hi + tol).all(), (kind, k, g)
    assert with_points >= 300 and clipped >= 150 and maps_of_huge >= 3000, (with_points, clipped, maps_of_huge)
    assert empty_intervals == 0, empty_intervals                          # ranges that come from a polygon leave no interval empty


def test_empty_intersection_and_containing_box_give_full_ranges(hrt):
    lib = hrt.load_library()
    tri = np.float32([[0, 0, 0], [1, 0.5, 0.25], [0.25, 1, 0.5]])
    full = np.float32([0, 1, 0, 1, 0, 1])
    assert np.array_equal(_clip(lib, tri, np.float32([2, 2, 2, 3, 3, 3])), full)                  # the box is elsewhere
    assert np.array_equal(_clip(lib, tri, np.float32([-1, -1, -1, 2, 2, 2])), full)               # the box holds the triangle
    assert np.array_equal(_clip(lib, tri, np.float32([-np.inf] * 3 + [np.inf] * 3)), full)
    assert np.array_equal(_clip(lib, tri, np.float32([0, 0, np.nan, 1, 1, 1])), full)             # a NaN plane: the whole primitive
    nan_tri = tri.copy(); nan_tri[1, 2] = np.nan
    assert np.array_equal(_clip(lib, nan_tri, np.float32([0, 0, 0, 0.5, 0.5, 0.5])), full)        # a non-finite vertex too
    inf_tri = tri.copy(); inf_tri[2, 0] = np.inf
    assert np.array_equal(_clip(lib, inf_tri, np.float32([0, 0, 0, 0.5, 0.5, 0.5])), full)
    assert lib.hrt_host_clip_barycentric(None, None, None) == -1


def test_a_slab_through_the_unit_triangle_gives_the_ranges_computed_by_hand(hrt):
    lib = hrt.load_library()
    tri = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]])                   # p = (u, v, 0)
    g = _clip(lib, tri, np.float32([0.25, -1, -1, 0.5, 2, 2]))            # 0.25 <= u <= 0.5
    want = np.float32([0.25, 0.5, 0.0, 0.75, 0.0, 0.75])
    assert np.abs(g - want).max() <= 2 * SLACK, g
    assert g[0] <= 0.25 and g[1] >= 0.5 and g[2] < 0 and g[3] >= 0.75 and g[4] < 0 and g[5] >= 0.75      # (slack where the part touches an edge too)
    # a degenerate triangle (a segment along x) cut in the middle: the corners' barycentrics are exact, only the cut is interpolated
    seg = np.float32([[0, 0, 0], [2, 0, 0], [1, 0, 0]])
    g = _clip(lib, seg, np.float32([-1, -1, -1, 0.5, 1, 1]))              # x = 2 u + v <= 0.5
    assert g[1] <= 0.25 + 2 * SLACK and g[3] <= 0.5 + 2 * SLACK and g[4] >= 0.5 - 2 * SLACK, g
