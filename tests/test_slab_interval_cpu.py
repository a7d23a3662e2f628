"""The node step's interval form (csrc/trav_common.h: node_slab_test<true>): the ray's interval [tmin, bt] is mapped
onto [0, 1] once per node step and the clamp rides on the z axis' FMAs as their `clamp` output modifier.

Two halves, neither needs a GPU.  The assembly the Makefile's flags produce is pinned (the clamps are there, the loop is no larger than the
figures DESIGN.md states, k_traverse is untouched, DX10 clamp is on: a NaN clamps to 0).  And a float32 emulation of both forms in numpy
(FMA through float64, v_rcp_f32 as the rounded reciprocal moved by -1 / 0 / +1 ulp) over the ray classes of tests/ray_cases.py, against
boxes padded and quantised as the builders do (4e-6 * max(1, scale), bvh8_geom.h: node_exponent / quantise_axis):
  1. neither form culls a box that contains a valid hit point, with bt at the hit distance, one ulp above it and at tmax;
  2. on unrelated boxes the new form's answer is the float64 interval test's wherever that test is decided by more than the forms' rounding."""
import os
import re
import sys
from pathlib import Path

import numpy as np
import pytest

import ray_cases as rc

ROOT = Path(__file__).resolve().parent.parent
CSRC = "nvidia-optix-ray-tracer_amd/csrc/"
sys.path.insert(0, str(ROOT / "tools"))
import loop_stats, path_kernels          # noqa: E402
f32, f64 = np.float32, np.float64


# ---------------------------------------------------------------- assembly pins ----------------------------------------------------------------
def _compile(tmp, stem, tag):
    """{kernel: {"lines": the first traversal loop, "text": the kernel's body, "meta": its metadata}} and the whole assembly text"""
    asm = tmp / f"{stem}_{tag}.s"
    kernels = path_kernels.compile_unit(stem, asm)
    return {name: {"lines": k["lines"], "text": "\n".join(k["body"]), "meta": k["meta"]} for name, k in kernels.items()}, asm.read_text()


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("slab_interval")
    out = {}
    for stem in ("fused", "fused_blocks", "fused_queue", "kernels"):
        out[stem] = _compile(tmp, stem, "default")
    saved = os.environ.get("EXTRA_HIPFLAGS")
    os.environ["EXTRA_HIPFLAGS"] = "-DHRT_SLAB_INTERVAL01=0"          # (the Makefile's HIPFLAGS end with it: tools/audit_asm_loads.py reads them through make)
    try:
        out["kernels_form0"] = _compile(tmp, "kernels", "form0")
    finally:
        if saved is None:
            del os.environ["EXTRA_HIPFLAGS"]
        else:
            os.environ["EXTRA_HIPFLAGS"] = saved
    return out


def _counts(lines):
    from collections import Counter
    cs, ops = Counter(), Counter()
    for op, _ in loop_stats.instructions(lines):
        cs[loop_stats.kind(op)] += 1
        ops[op] += 1
    return cs, ops


def _clamped_fmas(lines):
    return [l for l in lines if re.match(r"\s*v_fma_f32\b.*\bclamp\b", l)]


@pytest.mark.parametrize("stem, fragment", [("fused", "k_fusedILb0ELb0ELb0E"), ("fused_blocks", "k_path_blocksILb0E")])
def test_the_flagship_loops_carry_sixteen_clamped_fmas_and_are_no_larger_than_stated(compiled, stem, fragment):
    k = path_kernels.one(compiled[stem][0], fragment)
    cs, ops = _counts(k["lines"])
    print(fragment, dict(cs))
    assert len(_clamped_fmas(k["lines"])) == 16
    assert sum(cs.values()) <= 432 and cs["valu_complex"] <= 149, dict(cs)
    assert not any(op.startswith("scratch_") or op.startswith("buffer_") for op in ops), sorted(ops)
    # the clamp to [tmin, bt] is gone from the loop: eight max3 / min3 and nothing else of that family
    assert ops["v_max3_f32"] == 8 and ops["v_min3_f32"] == 8 and ops["v_max_f32"] == 0 and ops["v_min_f32"] == 0, dict(ops)


def test_k_path_blocks_spills_at_most_six_registers(compiled):
    meta = path_kernels.one(compiled["fused_blocks"][0], "k_path_blocksILb0E")["meta"]
    assert meta["vgpr_spill_count"] <= 6 and meta["sgpr_spill_count"] == 0 and meta["vgpr_count"] <= 128, meta


def test_every_loop_that_runs_traverse_to_regen_has_the_clamps(compiled):
    """k_fused (8), k_path_blocks (2), k_trace_queue (2): 16 per copy of the loop (the copy for the drained phase included)."""
    n = 0
    for stem in ("fused", "fused_blocks", "fused_queue"):
        for name, k in compiled[stem][0].items():
            total = len(_clamped_fmas(k["text"].split("\n")))
            assert total >= 32 and total % 16 == 0, (name, total)
            n += 1
    assert n == 12


def test_k_traverse_keeps_the_exact_form(compiled):
    """No clamp anywhere in any instantiation, and the loops' counts are those of a build with the interval form switched off."""
    default, form0 = compiled["kernels"][0], compiled["kernels_form0"][0]
    assert len(default) == 6 and sorted(default) == sorted(form0), sorted(default)
    for name, k in default.items():
        assert " clamp" not in k["text"], name
        assert k["lines"] and _counts(k["lines"])[1] == _counts(form0[name]["lines"])[1], name


def test_dx10_clamp_is_on_in_every_path_kernel(compiled):
    for stem in ("fused", "fused_blocks", "fused_queue"):
        text = compiled[stem][1]
        values = re.findall(r"\.amdhsa_dx10_clamp\s+(\d)", text)
        assert len(values) == len(compiled[stem][0]) and set(values) == {"1"}, (stem, values)


# ---------------------------------------------------------------- the emulation ----------------------------------------------------------------
SLACK = f32(1.0) - f32(2.0 ** -20)
FLOOR, REACH, RATIO = f32(2.0 ** -36), f32(2.0 ** 64), f32(2.0 ** 40)


def fma(a, b, c):
    with np.errstate(all="ignore"):
        return (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)


def rcp(x, ulps):
    """v_rcp_f32: the rounded reciprocal, moved by `ulps` in {-1, 0, 1}"""
    with np.errstate(all="ignore"):
        r = (1.0 / x.astype(f64)).astype(f32)
        up = np.nextafter(r, f32(np.inf)); dn = np.nextafter(r, f32(-np.inf))
    return np.where(ulps > 0, up, np.where(ulps < 0, dn, r)).astype(f32)


def ray_start(d, tmax, ulps, interval):
    """safe_rcp_dir + lean_start's slab_cap_rcp and reach bound (the cap, the slack folded into the reciprocals): (idx (n, 3), first culling bound (n,))"""
    lim = f32(1e-20)
    dd = np.where(np.abs(d) < lim, np.copysign(lim, d + f32(0.0)), d).astype(f32)
    idx = rcp(dd, ulps)
    if not interval:
        return idx, np.full(len(d), tmax, f32)
    with np.errstate(all="ignore"):
        m = np.abs(idx).min(1)
        cap = (m * RATIO).astype(f32)
        idx = np.copysign((np.minimum(np.abs(idx), cap[:, None]) * SLACK).astype(f32), idx).astype(f32)
        bt = np.minimum(f32(tmax), (REACH * m).astype(f32)).astype(f32)
    return idx, bt


def slab(o, d, idx, bt, tmin, node_p, node_e, qlo, qhi, interval, kulp=None):
    """node_slab_test for one child per ray: node origin (n, 3), biased exponents (n, 3) uint8, the child's bytes (n, 3) each."""
    with np.errstate(all="ignore"):
        neg = d < 0
        qn = np.where(neg, qhi, qlo).astype(f32); qf = np.where(neg, qlo, qhi).astype(f32)
        es = (node_e.astype(np.uint32) << 23).view(f32)
        tmin = f32(tmin)
        if interval:
            k = rcp(((bt - tmin).astype(f32) + FLOOR).astype(f32), kulp)
            kk = (idx * k[:, None]).astype(f32)
            c0 = (-(tmin * k)).astype(f32)
            ai = (es * kk).astype(f32)
            ao = fma((node_p - o).astype(f32), kk, np.broadcast_to(c0[:, None], kk.shape))
        else:
            ai = (es * idx).astype(f32)
            ao = ((node_p - o).astype(f32) * idx).astype(f32)
        tn, tf = fma(qn, ai, ao), fma(qf, ai, ao)
        if interval:
            clamp = lambda x: np.where(np.isnan(x), f32(0), np.minimum(np.maximum(x, f32(0)), f32(1))).astype(f32)      # DX10 clamp
            tn[:, 2], tf[:, 2] = clamp(tn[:, 2]), clamp(tf[:, 2])
            return np.fmax(np.fmax(tn[:, 0], tn[:, 1]), tn[:, 2]) < np.fmin(np.fmin(tf[:, 0], tf[:, 1]), tf[:, 2])
        tlo = np.fmax(np.fmax(tn[:, 0], tn[:, 1]), np.fmax(tn[:, 2], tmin))
        thi = np.fmin(np.fmin(tf[:, 0], tf[:, 1]), np.fmin(tf[:, 2], bt))
        return tlo <= thi


def node_exponent(ext):
    """bvh8_geom.h, vectorised"""
    bits = ext.astype(f32).view(np.uint32)
    E = ((bits >> 23) & 0xff).astype(np.int64); M = bits & 0x7fffff
    e = np.where(M <= 0x7f0000, E - 127 - 7, E - 127 - 6)
    e = np.clip(e, -126, 127) + 127
    e = np.where(~(ext > 0) | (E == 0), 1, np.where(E == 255, 254, e))
    return e.astype(np.uint8)


def quantise(p, e, clo, chi):
    """quantise_axis, vectorised: outward-rounded bytes whose float decode p + q * 2^(e - 127) stays outside [clo, chi]"""
    fs = (e.astype(np.uint32) << 23).view(f32)
    with np.errstate(all="ignore"):
        ql = np.clip(np.floor((clo.astype(f64) - p.astype(f64)) / fs.astype(f64)), 0, 255).astype(np.int64)
        qh = np.clip(np.ceil((chi.astype(f64) - p.astype(f64)) / fs.astype(f64)), 0, 255).astype(np.int64)
        for _ in range(3):
            ql = np.where((ql > 0) & ((p + (ql.astype(f32) * fs).astype(f32)).astype(f32) > clo), ql - 1, ql)
            qh = np.where((qh < 255) & ((p + (qh.astype(f32) * fs).astype(f32)).astype(f32) < chi), qh + 1, qh)
    return ql.astype(np.uint8), qh.astype(np.uint8)


def boxes_in_nodes(rng, lo, hi, scale):
    """Child boxes [lo, hi] (float32, already padded) in random parent nodes: origin, exponents, bytes.  The parent reaches a random
    amount beyond the child on either side, so that the bytes fall anywhere in 0 .. 255."""
    n = len(lo)
    ext = (hi - lo).astype(f64)
    grow = ext * 10.0 ** rng.uniform(-2, 1.5, (n, 3)) + scale * 10.0 ** rng.uniform(-6, 0, (n, 3)) * (rng.random((n, 3)) < 0.5)
    share = rng.random((n, 3))
    p = (lo.astype(f64) - grow * share).astype(f32)
    p = np.minimum(p, lo)
    top = np.maximum((hi.astype(f64) + grow * (1 - share)).astype(f32), hi)
    e = node_exponent((top - p).astype(f32))
    # (an extent rounded down can leave 255 cells a hair short: the builders take the next exponent then)
    fs = (e.astype(np.uint32) << 23).view(f32)
    short = (p + (f32(255) * fs).astype(f32)).astype(f32) < hi
    e = np.where(short, e + 1, e).astype(np.uint8)
    ql, qh = quantise(p, e, lo, hi)
    fs = (e.astype(np.uint32) << 23).view(f32)
    assert ((p + ql.astype(f32) * fs).astype(f32) <= lo).all() and ((p + qh.astype(f32) * fs).astype(f32) >= hi).all()
    return p, e, ql, qh


def make_rays(rng, n, scale):
    """Directions of every scale and with replaced components as ray_cases.adversarial_rays makes them, the distance of the origin from
    its target in units of the scene's half extent."""
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    axis = rng.random(n) < 0.15                                          # axis-parallel, like the plane block
    d[axis] = np.eye(3)[rng.integers(0, 3, int(axis.sum()))] * rng.choice(rc.PLANE_SPEEDS, int(axis.sum()))[:, None]
    d[axis] = np.where(d[axis] == 0, rng.choice([0.0, -0.0], (int(axis.sum()), 3)), d[axis])
    dscale = rng.choice(np.asarray(rc.DIRECTION_SCALES), n)
    d = d * dscale[:, None]
    z = (rng.random((n, 3)) < 0.08) & ~axis[:, None]
    d[z] = rng.choice(np.asarray(rc.COMPONENT_VALUES), int(z.sum()))
    with np.errstate(all="ignore"):
        d = d.astype(f32)
    d[(d == 0).all(1)] = f32([0, 0, 1])
    dist = rng.choice(np.asarray(rc.DISTANCES), n) * scale
    return d, dist, dscale


WINDOWS = ((1e-6, 1e16), (0.0, 1e16), (1e-30, 1e16))
SCALES = (2.0 ** -20, 1.0, 2.0 ** 20)


@pytest.fixture(scope="module")
def hit_cases():
    """Rays with a valid hit at t* and a padded, quantised box that contains the hit point o + t* d (computed in float64)."""
    rng = np.random.default_rng(20)
    out = []
    for scale in SCALES:
        for tmin, tmax in WINDOWS + ((1e-6 * scale, 1e16 * scale),):
            n = 60000
            d, dist, dscale = make_rays(rng, n, scale)
            target = rng.uniform(-scale, scale, (n, 3))
            dn = d.astype(f64) / np.maximum(np.linalg.norm(d.astype(f64), axis=1, keepdims=True), 1e-300)
            o = (target - dn * dist[:, None]).astype(f32)
            with np.errstate(all="ignore"):
                tstar = (dist / np.linalg.norm(d.astype(f64), axis=1)).astype(f32)
            tstar = np.where(rng.random(n) < 0.3, f32(tmin) + np.abs(tstar) * f32(1e-3), tstar).astype(f32)      # ... and hits just behind tmin
            valid = (tstar > f32(tmin)) & (tstar < f32(tmax)) & np.isfinite(tstar)
            d, o, tstar, dscale = d[valid], o[valid], tstar[valid], dscale[valid]
            m = len(d)
            H = o.astype(f64) + d.astype(f64) * tstar.astype(f64)[:, None]
            ok = np.abs(H).max(1) < 16 * scale                             # (a 1e-30 direction with a replaced component can leave the scene: not a case)
            d, o, tstar, dscale, H = d[ok], o[ok], tstar[ok], dscale[ok], H[ok]
            m = len(d)
            # the primitive's box: the hit point on a face (vertex / edge rays: extent 0 on that side) or inside
            a = scale * 10.0 ** rng.uniform(-5, 0, (m, 3)) * (rng.random((m, 3)) < 0.6)
            b = scale * 10.0 ** rng.uniform(-5, 0, (m, 3)) * (rng.random((m, 3)) < 0.6)
            lo = np.nextafter((H - a).astype(f32), f32(-np.inf)); hi = np.nextafter((H + b).astype(f32), f32(np.inf))
            lo = np.minimum(lo, H.astype(f32)); hi = np.maximum(hi, H.astype(f32))
            pad = f32(4e-6) * f32(max(1.0, scale))
            lo, hi = (lo - pad).astype(f32), (hi + pad).astype(f32)
            p, e, ql, qh = boxes_in_nodes(rng, lo, hi, scale)
            ulps = rng.integers(-1, 2, (m, 4))
            out.append(dict(scale=scale, tmin=tmin, tmax=tmax, o=o, d=d, tstar=tstar, dscale=dscale, p=p, e=e, ql=ql, qh=qh, ulps=ulps))
    return out


def test_the_generator_covers_the_classes(hit_cases):
    d = np.concatenate([c["d"] for c in hit_cases]); ds = np.concatenate([c["dscale"] for c in hit_cases])
    assert len(d) > 300000
    assert ((d == 0).sum(1) == 2).sum() > 10000                                     # axis-parallel
    assert (np.signbit(d) & (d == 0)).any(1).sum() > 5000                           # negative zeros
    assert ((np.abs(d) > 0) & (np.abs(d) < 1.2e-38)).any(1).sum() > 1000            # denormal components
    for s in (1e-3, 1.0, 37.0, 1e30):
        assert (ds == s).sum() > 1000, s
    assert {c["scale"] for c in hit_cases} == set(SCALES)


@pytest.mark.parametrize("interval", [False, True], ids=["clamped-form", "interval-form"])
def test_no_box_with_a_valid_hit_point_is_culled(hit_cases, interval):
    """Condition 1, with bt at the hit distance (a tie with a lower primitive id must still be found), one ulp above it and at tmax."""
    for c in hit_cases:
        idx, bt0 = ray_start(c["d"], c["tmax"], c["ulps"][:, :3], interval)
        assert (bt0 > c["tstar"]).all(), (c["scale"], c["tmin"])            # the reach guard is beyond every hit of the envelope
        for which, bt in (("t*", c["tstar"]), ("t* + ulp", np.nextafter(c["tstar"], f32(np.inf))), ("tmax", bt0)):
            hit = slab(c["o"], c["d"], idx, bt.astype(f32), c["tmin"], c["p"], c["e"], c["ql"], c["qh"], interval, c["ulps"][:, 3])
            bad = np.flatnonzero(~hit)
            assert len(bad) == 0, (c["scale"], c["tmin"], which, len(bad), len(hit), c["o"][bad[0]], c["d"][bad[0]], c["tstar"][bad[0]])


def test_unrelated_boxes_get_the_float64_interval_tests_answer():
    """Condition 2, over every direction scale and with every v_rcp_f32 moved by -1 / 0 / +1 ulp.  The reference is the slab test in float64
    on the decoded box with the reciprocals the kernel holds (slack and perturbation included), over [tmin, bt + 2^-36], the interval the
    form maps onto [0, 1].  The two can differ only by the float32 roundings of the form, so they are compared outside a band:
      * a plane's distance fma(byte, 2^e idx k, fma(p - o, idx k, -tmin k)) carries the roundings of p - o, idx k, the two FMAs and -tmin k
        (2^e idx k is exact), each at most 2^-24 of the largest term: 5 roundings, taken as 16 (`tol`);
      * at the bt end the clamp at 1 stands for t = bt + 2^-36 up to k's own error, one ulp of v_rcp_f32 and half an ulp each of the subtract
        and the add, 2 ulps = 4 * 2^-24 of the interval's length, taken as 8 (`tol_end`).  That is half of the 2^-20 = 16 * 2^-24 by which
        the slack keeps bt itself below the clamp: the band never reaches a plane at bt.
    Where the reference accepts or rejects by more than the band the interval form says the same; inside it either answer is a correct cull,
    and of the rays without a tiny component under 1 % of the boxes fall inside."""
    rng = np.random.default_rng(21)
    undecided = total = accepted = 0
    for scale in SCALES:
        for tmin, tmax in ((1e-6 * scale, 1e16 * scale), (0.0, 1e16)):
            n = 150000
            d, dist, dscale = make_rays(rng, n, scale)
            o = rng.uniform(-scale, scale, (n, 3)).astype(f32)
            c = o.astype(f64) + rng.normal(size=(n, 3)) * scale * 10.0 ** rng.uniform(-3, 0.5, (n, 1))
            h = scale * 10.0 ** rng.uniform(-4, 0, (n, 3))
            lo, hi = (c - h).astype(f32), (c + h).astype(f32)
            p, e, ql, qh = boxes_in_nodes(rng, lo, hi, scale)
            ulps = rng.integers(-1, 2, (n, 4))
            idx, bt0 = ray_start(d, tmax, ulps[:, :3], True)
            far = np.linalg.norm(c - o.astype(f64), axis=1) / np.linalg.norm(d.astype(f64), axis=1)
            with np.errstate(all="ignore"):
                bt = np.where(rng.random(n) < 0.5, bt0, np.minimum(far * rng.uniform(0.3, 3.0, n), 1e30).astype(f32)).astype(f32)
            bt = np.maximum(bt, np.nextafter(f32(tmin), f32(np.inf)))
            got = slab(o, d, idx, bt, tmin, p, e, ql, qh, True, ulps[:, 3])
            with np.errstate(all="ignore"):
                fs = (e.astype(np.uint32) << 23).view(f32).astype(f64)
                blo, bhi = p.astype(f64) + ql * fs, p.astype(f64) + qh * fs
                i64, o64 = idx.astype(f64), o.astype(f64)
                t0, t1 = (blo - o64) * i64, (bhi - o64) * i64
                tn, tf = np.minimum(t0, t1), np.maximum(t0, t1)
                N, F = tn.max(1), tf.min(1)
                end = bt.astype(f64) + float(FLOOR)          # (the slack is in idx: t0 / t1 carry it)
                mag = (np.abs(p.astype(f64) - o64) * np.abs(i64) + 255 * fs * np.abs(i64)).max(1) + abs(tmin)
                tol = 16 * 2.0 ** -24 * mag                              # of a plane's distance
                tol_end = tol + 8 * 2.0 ** -24 * (end - tmin)            # of the clamp at 1, in t: k's roundings
                sure_hit = (N + tol < F - tol) & (F - tol > tmin) & (N + tol < end - tol_end)
                sure_miss = (N - tol > F + tol) | (F + tol < tmin) | (N - tol > end + tol_end)
            assert not (got & sure_miss).any(), (scale, tmin, int((got & sure_miss).sum()))
            assert not (~got & sure_hit).any(), (scale, tmin, int((~got & sure_hit).sum()))
            # (a component below 2^-30 of the largest: its planes' distances are 2^30 .. 2^40 times the others', and so is the band)
            plain = (np.abs(d) >= np.abs(d).max(1, keepdims=True) * f32(2.0 ** -30)).all(1)
            undecided += int((~sure_hit & ~sure_miss & plain).sum()); total += int(plain.sum()); accepted += int(got.sum())
    print("condition 2: %d boxes of rays without a tiny component, %d within the rounding band; %d accepted in all" % (total, undecided, accepted))
    assert total > 300000 and accepted > total // 50 and undecided < total // 100
