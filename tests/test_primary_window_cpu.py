"""The argument behind HRT_SEED_PRIMARY=2 (csrc/trav_common.h: kSeedWindow, TravState::tlo), on the CPU.  A pixel's
repeat primary ray is the ray that found a hit at t before, so it may be bounded from BOTH sides: the culling bound starts at t (level 1,
tests/test_primary_seed_cpu.py) and the node step's interval begins at t (1 - delta) instead of the launch's tmin, because the identical ray
has proved that nothing lies before t.  Three parts, none needs a GPU:
  1. on the oracle's canonical walker the windowed walk ends in the same record, bit for bit, for every ray, in no more visits per ray than
     the walk bounded above only and fewer in all;
  2. a float32 emulation of node_slab_test<true> (tests/test_slab_interval_cpu.py's, with the lower end per ray) never culls a box that
     holds the hit point, for the ray classes of tests/ray_cases.py at three scene scales and origins up to 12 extents away;
  3. static: the one-level kernels' LDS stays at 10240 bytes or less (16 waves per CU) with the seed's word in it, and the knob is a level.
delta is read from the source, so the test follows the constant."""
import ctypes as C
import re
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import pytest

import ray_cases as rc
import test_slab_interval_cpu as si
from test_host_cpu import _build

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "nvidia-optix-ray-tracer_amd" / "csrc"
f32, f64 = np.float32, np.float64


def _delta():
    m = re.search(r"constexpr float kSeedWindow = 0x1p-(\d+)f;", (CSRC / "trav_common.h").read_text())
    assert m, "kSeedWindow: a power of two in trav_common.h"
    return 2.0 ** -int(m.group(1))


def test_delta_is_far_above_everything_that_rounds_and_no_wider_than_it_pays():
    """The window must dwarf the slack (2^-20) that keeps bt below the clamp, hence the ulps of v_rcp_f32 and of the FMAs: a factor of 2^8
    at least; above 2^-6 the CPU walks lose most of the gain."""
    assert 2.0 ** -12 <= _delta() <= 2.0 ** -6
    assert f32(1.0) - f32(_delta()) < f32(1.0)


# ---------------------------------------------------------------- 1. the walker ----------------------------------------------------------------
N_TRIANGLES, N_RAYS = 3000, 1500


@pytest.mark.parametrize("sbvh", ["0", "1"])
def test_a_walk_inside_the_window_under_its_known_hit_finds_it_again_in_fewer_visits(hrt, oracle, monkeypatch, sbvh):
    """Every hit ray again with tmax = nextafter(t) (the culling bound of level 1, test_primary_seed_cpu.py) and again with tmin = t (1 - delta)
    as well.  (The walker's tmin also bounds its primitive test, which the kernels' window does not: the old hit, at t > tmin, is still
    accepted, and whatever the raised tmin rejects had t below the hit's -- the complete walk found nothing there.)"""
    monkeypatch.setenv("HRT_SBVH", sbvh)
    delta = f32(_delta())
    scene = hrt.scenes.random_soup(N_TRIANGLES, 0.12, 17)
    lib, blob = _build(hrt, scene["instances"][0]["vertices"])
    try:
        assert blob.n_triangles > N_TRIANGLES if sbvh == "1" else blob.n_triangles == N_TRIANGLES
        o, d = oracle.random_rays(N_RAYS, 5)
        t, u, v, prim, inst, _, _ = oracle.bvh8_trace(blob.nodes, blob.triangles, o, d)
        hit = np.flatnonzero(prim != 0xFFFFFFFF)
        assert 0.3 * N_RAYS < len(hit) < N_RAYS
        above_visits = window_visits = above_tests = window_tests = checked = 0
        for i in hit:
            bound = float(np.nextafter(t[i], f32(np.inf)))
            lower = float(max(f32(1e-6), f32(t[i] * (f32(1.0) - delta))))
            _, _, _, aprim, _, av, at = oracle.bvh8_trace(blob.nodes, blob.triangles, o[i], d[i], tmax=bound)
            wt, wu, wv, wprim, winst, wn, wtests = oracle.bvh8_trace(blob.nodes, blob.triangles, o[i], d[i], tmin=lower, tmax=bound)
            assert aprim[0] == prim[i]
            assert wprim[0] == prim[i] and winst[0] == inst[i], (i, prim[i], wprim[0])      # never a miss, never a neighbour
            assert wt.view(np.uint32)[0] == t.view(np.uint32)[i] and wu.view(np.uint32)[0] == u.view(np.uint32)[i] and wv.view(np.uint32)[0] == v.view(np.uint32)[i]
            assert wn <= av, (i, wn, av)
            above_visits += av; window_visits += wn; above_tests += at; window_tests += wtests
            checked += 1
        assert checked == len(hit)                                                         # no ray left out
        assert window_visits < above_visits
        print(f"HRT_SBVH={sbvh}: {checked} hits, node visits {above_visits} -> {window_visits}, primitive tests {above_tests} -> {window_tests}")
    finally:
        lib.hrt_host_free(C.byref(blob))


# ---------------------------------------------------------------- 2. the emulation ----------------------------------------------------------------
# origins: the distances of ray_cases (x half an extent), and 12 and 24 half extents = 6 and 12 extents away
DISTANCES = tuple(rc.DISTANCES) + (12.0, 24.0)


def window_lo(d, seed, tmin, delta):
    """trav_common.h: seed_window_lo -- max(tmin, seed (1 - delta)); tmin for a direction that lies wholly below safe_rcp_dir's floor (the slab
    test then sees every plane 1e10 times nearer than it is: no bound from below can rest on that)"""
    plain = np.abs(d).max(1) >= f32(1e-20)
    return np.where(plain, np.maximum(f32(tmin), (seed * (f32(1.0) - delta)).astype(f32)), f32(tmin)).astype(f32)


@pytest.fixture(scope="module")
def window_cases():
    """test_slab_interval_cpu.hit_cases with the farther origins: rays with a valid hit at t* and a padded, quantised box that contains the
    hit point o + t* d (float64)."""
    rng = np.random.default_rng(22)
    out = []
    for scale in si.SCALES:
        for tmin, tmax in si.WINDOWS + ((1e-6 * scale, 1e16 * scale),):
            n = 40000
            d, _, dscale = si.make_rays(rng, n, scale)
            dist = rng.choice(np.asarray(DISTANCES), n) * scale
            target = rng.uniform(-scale, scale, (n, 3))
            dn = d.astype(f64) / np.maximum(np.linalg.norm(d.astype(f64), axis=1, keepdims=True), 1e-300)
            o = (target - dn * dist[:, None]).astype(f32)
            with np.errstate(all="ignore"):
                tstar = (dist / np.linalg.norm(d.astype(f64), axis=1)).astype(f32)
            tstar = np.where(rng.random(n) < 0.3, f32(tmin) + np.abs(tstar) * f32(1e-3), tstar).astype(f32)      # ... and hits just behind tmin
            valid = (tstar > f32(tmin)) & (tstar < f32(tmax)) & np.isfinite(tstar)
            d, o, tstar, dist = d[valid], o[valid], tstar[valid], dist[valid]
            H = o.astype(f64) + d.astype(f64) * tstar.astype(f64)[:, None]
            ok = np.abs(H).max(1) < 16 * scale
            d, o, tstar, dist, H = d[ok], o[ok], tstar[ok], dist[ok], H[ok]
            m = len(d)
            a = scale * 10.0 ** rng.uniform(-5, 0, (m, 3)) * (rng.random((m, 3)) < 0.6)
            b = scale * 10.0 ** rng.uniform(-5, 0, (m, 3)) * (rng.random((m, 3)) < 0.6)
            lo = np.nextafter((H - a).astype(f32), f32(-np.inf)); hi = np.nextafter((H + b).astype(f32), f32(np.inf))
            lo = np.minimum(lo, H.astype(f32)); hi = np.maximum(hi, H.astype(f32))
            pad = f32(4e-6) * f32(max(1.0, scale))
            lo, hi = (lo - pad).astype(f32), (hi + pad).astype(f32)
            p, e, ql, qh = si.boxes_in_nodes(rng, lo, hi, scale)
            out.append(dict(scale=scale, tmin=tmin, tmax=tmax, o=o, d=d, tstar=tstar, dist=dist / scale, p=p, e=e, ql=ql, qh=qh, ulps=rng.integers(-1, 2, (m, 4))))
    return out


def test_the_cases_reach_twelve_extents_and_every_scale(window_cases):
    assert {c["scale"] for c in window_cases} == set(si.SCALES) and len(window_cases) == 12
    for c in window_cases:
        assert len(c["d"]) > 10000
        for far in (12.0, 24.0):
            assert (c["dist"] == far).sum() > 500, (c["scale"], far)


def test_no_box_that_holds_the_hit_point_is_culled_by_the_window(window_cases):
    """bt = the seed and tlo = max(tmin, seed (1 - delta)) as fused_body.h makes them, the seed at the hit distance and one ulp above it (the
    primitive test's t and the box's geometry do not round alike).  Every case counts."""
    delta = f32(_delta())
    checked = 0
    for c in window_cases:
        idx, bt0 = si.ray_start(c["d"], c["tmax"], c["ulps"][:, :3], True)
        assert (bt0 > c["tstar"]).all()
        for which, seed in (("t*", c["tstar"]), ("t* + ulp", np.nextafter(c["tstar"], f32(np.inf)))):
            seed = seed.astype(f32)
            tlo = window_lo(c["d"], seed, c["tmin"], delta)
            assert (tlo > f32(c["tmin"])).sum() > len(seed) // 2          # the window IS raised in most cases (not where t* is within delta of tmin)
            hit = si.slab(c["o"], c["d"], idx, seed, tlo, c["p"], c["e"], c["ql"], c["qh"], True, c["ulps"][:, 3])
            bad = np.flatnonzero(~hit)
            assert len(bad) == 0, (c["scale"], c["tmin"], which, len(bad), len(hit), c["o"][bad[0]], c["d"][bad[0]], c["tstar"][bad[0]])
            checked += len(hit)
    assert checked == 2 * sum(len(c["d"]) for c in window_cases)
    print(f"{checked} boxes, none culled")


def test_the_window_culls_what_ends_before_it(window_cases):
    """... and it is not vacuous: a small box round the ray at half the hit distance passes the interval from tmin and is culled by the window."""
    delta = f32(_delta())
    c = next(c for c in window_cases if c["scale"] == 1.0 and c["tmin"] == 1e-6)
    keep = (c["dist"] >= 0.3) & (np.abs(c["d"]) >= np.abs(c["d"]).max(1, keepdims=True) * f32(2.0 ** -10)).all(1)
    o, d, tstar = c["o"][keep], c["d"][keep], c["tstar"][keep]
    rng = np.random.default_rng(23)
    mid = o.astype(f64) + d.astype(f64) * (0.5 * tstar.astype(f64))[:, None]
    h = 0.01 * np.linalg.norm(d.astype(f64), axis=1, keepdims=True) * tstar.astype(f64)[:, None]
    lo, hi = (mid - h).astype(f32), (mid + h).astype(f32)
    p, e, ql, qh = si.boxes_in_nodes(rng, lo, hi, 1.0)
    ulps = rng.integers(-1, 2, (len(d), 4))
    idx, _ = si.ray_start(d, c["tmax"], ulps[:, :3], True)
    tlo = window_lo(d, tstar, c["tmin"], delta)
    from_tmin = si.slab(o, d, idx, tstar, c["tmin"], p, e, ql, qh, True, ulps[:, 3])
    windowed = si.slab(o, d, idx, tstar, tlo, p, e, ql, qh, True, ulps[:, 3])
    # (not "none": the bytes of a small box in a large parent node round outwards by up to a cell of the parent, which can reach the window)
    assert from_tmin.mean() > 0.9 and windowed.mean() < 0.01, (from_tmin.mean(), windowed.mean())


# ---------------------------------------------------------------- 3. static ----------------------------------------------------------------
def _metadata(stem):
    sys.path.insert(0, str(ROOT / "tools"))
    import path_kernels
    with tempfile.TemporaryDirectory() as tmp:
        return {name: k["meta"] for name, k in path_kernels.compile_unit(stem, Path(tmp) / f"{stem}.s").items()}


def test_one_level_kernels_keep_sixteen_waves_of_lds():
    """s_nodes + s_leaves + the mailboxes are 9984 bytes; the seed's word per lane makes it 10240 = 160 KB / 16 exactly, no more."""
    with ThreadPoolExecutor(3) as pool:
        metas = list(pool.map(_metadata, ("fused", "fused_blocks", "fused_capture")))
    one_level = {}
    for meta in metas:
        for name, m in meta.items():
            flags = re.findall(r"Lb(\d)E", name)
            instanced = flags[1] == "1" if ("k_fused" in name or "k_path_capture" in name) else False
            if not instanced:
                one_level[name] = m["group_segment_fixed_size"]
    assert len(one_level) == 4 + 2 + 2, sorted(one_level)
    assert all(v <= 10240 for v in one_level.values()), one_level
    assert any(v == 10240 for v in one_level.values()), one_level          # the seed is in LDS somewhere


def test_the_knob_is_a_level():
    knobs = (CSRC / "knobs.def").read_text()
    line = next(l for l in knobs.splitlines() if l.startswith('HRT_KNOB("HRT_SEED_PRIMARY"'))
    assert line.startswith('HRT_KNOB("HRT_SEED_PRIMARY", "2",')
    assert "v >= 0 && v <= 2" in line and "ctx->seed_primary = v" in line
    assert re.search(r"ta\.seed_primary = ctx->seed_primary;", (CSRC / "hrt_api.cpp").read_text())
    assert re.search(r"int seed_primary = 2;", (CSRC / "hrt_internal.hpp").read_text())
    body = (CSRC / "fused_body.h").read_text()
    assert "a.seed_primary >= 2" in body                                                    # the window: level 2 only
    assert re.search(r"a\.seed_primary\) \*seed = bt", (CSRC / "path_lane.h").read_text())      # the upper end: levels 1 and 2
