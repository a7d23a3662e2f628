"""The denoiser's edge cases (tests/denoise_cases.py) without a GPU: on the numpy specifications and the oracle alone, every case reaches
the expression it is for -- so that a later edit of a scene or a default cannot quietly turn a case back into a benign one -- and what
the specification does with non-finite colour is pinned.  tests/test_denoise_edges_gpu.py runs the kernels on the same cases.

Counts are "at least 50 pixels (or taps)" unless the frame is smaller, where they are "at least one"."""
import numpy as np
import pytest

import denoise_cases as dc
import denoise_ref as ref
import denoise_temporal_ref as tref

f32 = np.float32


def _enough(count, pixels):
    return count >= (50 if pixels >= 2000 else 1)


# ---- the filter -----------------------------------------------------------------------------
def _first_pass_terms(color, guides, params, step=1):
    """Of every tap of a pass at `step` over the case's input that counts (inside the frame, centre and tap on geometry): the normal
    weight after its squarings and the colour distance dc2, as the specification computes them."""
    n, _, z = ref.unpack_guides(guides)
    squarings = ref.pass_constants(params)[1]
    hit = (z > 0) & (z < np.inf)
    H, W = z.shape
    wn_all, dc2_all = [], []
    with np.errstate(all="ignore"):
        for j in range(5):
            for i in range(5):
                dy, dx = (j - 2) * step, (i - 2) * step
                y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
                if y0 >= y1 or x0 >= x1:
                    continue
                P, Q = (slice(y0, y1), slice(x0, x1)), (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
                d = color[Q][..., :3] - color[P][..., :3]
                dc2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                wn = np.fmax(ref._dot(n[P], n[Q]), f32(0))
                for _ in range(squarings):
                    wn = wn * wn
                m = hit[P] & hit[Q]
                wn_all.append(wn[m])
                dc2_all.append(dc2[m])
    return np.concatenate(wn_all), np.concatenate(dc2_all)


def _hit(guides):
    z = ref.unpack_guides(guides)[2]
    return (z > 0) & (z < np.inf)


def test_case_lists_hold_the_sizes_asked_for():
    sizes = {dc.filter_case_size(name) for name in dc.FILTER_CASES}
    for w in (15, 16, 17, 31, 32, 33):
        for h in (1, 16, 17):
            assert (w, h) in sizes
    assert (1, 300) in sizes and (300, 1) in sizes
    its = {}
    for name in dc.FILTER_CASES:
        if name.startswith(("outer-tap", "deep")):
            c, g, p = dc.filter_case(name)
            its.setdefault(p["iterations"], []).append((c.shape[1], c.shape[0]))
    for it, s in ((3, 4), (5, 16), (7, 64)):                  # the last pass's outer tap x + 2 s: just outside at width 2 s, the last pixel at 2 s + 1
        assert 1 << (it - 1) == s and (2 * s, 3) in its[it] and (2 * s + 1, 3) in its[it]
    for it in (9, 12, 16):                                    # from step 32 on only the centre tap lies in a 17 x 5 frame
        assert (17, 5) in its[it]
    assert (523, 3) in its[9] and 523 > 2 * 256               # step 256 finds x + 256 and x + 512
    sizes = [(w, h) for _, w, h in dc.GUIDE_CASES]
    assert {(97, 61), (1, 1), (1, 37), (255, 1), (257, 3)} <= set(sizes)
    assert all((w * h) % 256 and (w * h) % 64 for w, h in sizes)
    assert max(w / h for w, h in sizes) >= 85 and min(w / h for w, h in sizes) <= 1 / 37


def test_npow8_weights_walk_through_the_subnormals():
    c, g, p = dc.filter_case("npow8")
    assert p["normal_power_log2"] == 8
    wn, _ = _first_pass_terms(c, g, p)
    sub = (wn > 0) & (wn < dc.FLT_MIN)
    print(f"npow8: taps {wn.size}, subnormal {sub.sum()}, zero {(wn == 0).sum()}, normal {(wn >= dc.FLT_MIN).sum()}")
    assert sub.sum() >= 50 and (wn == 0).sum() >= 50 and (wn >= dc.FLT_MIN).sum() >= 50
    out = ref.atrous(c, g, p)
    assert not np.array_equal(dc.bits(out[..., :3]), dc.bits(c[..., :3]))


def test_dark_frame_stays_subnormal():
    c, g, p = dc.filter_case("dark")
    out = ref.atrous(c, g, p)
    hit = _hit(g)
    rgb = out[..., :3][hit]
    assert np.all(np.abs(c[..., :3]) < dc.FLT_MIN) and np.all(c[..., :3] > 0)
    assert np.all(np.abs(rgb) < dc.FLT_MIN) and (rgb > 0).sum() >= 50
    assert (dc.bits(out[..., :3])[hit] != dc.bits(c[..., :3])[hit]).sum() >= 50              # ... and filtered, not copied


def test_hdr_colour_distances_overflow():
    c, g, p = dc.filter_case("hdr")
    _, dc2 = _first_pass_terms(c, g, p)
    assert np.isinf(dc2).sum() >= 50 and np.isfinite(dc2).sum() >= 50
    assert (c[..., :3] < 0).sum() >= 50 and np.isfinite(c[..., :3]).all()
    out = ref.atrous(c, g, p)
    assert np.isfinite(out[..., :3][_hit(g)]).sum() >= 50


def _dilate(mask, hit, iterations):
    """The hit pixels that a chain of taps (5 x 5, 1 << pass apart) over hit pixels connects to `mask` within the passes."""
    reach = mask & hit
    H, W = mask.shape
    for i in range(iterations):
        s = 1 << i
        grown = np.zeros_like(reach)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                y0, y1, x0, x1 = max(0, -dy * s), min(H, H - dy * s), max(0, -dx * s), min(W, W - dx * s)
                if y0 < y1 and x0 < x1:
                    grown[y0:y1, x0:x1] |= reach[y0 + dy * s: y1 + dy * s, x0 + dx * s: x1 + dx * s]
        reach = grown & hit
    return reach


@pytest.mark.parametrize("iterations", dc.FIREFLY_ITERATIONS)
def test_fireflies_spread_as_nan_and_leave_the_rest_finite(iterations):
    """What a non-finite colour does, pinned on the specification.  In one pass, for a pixel on geometry:
      * a NaN among its taps' colours (its own included) makes that tap's weight and so the weight sum NaN, `sw > 0` is false, and
        the pixel keeps its colour: unfiltered, not NaN.  A pixel that is itself infinite has inf - inf = NaN at its centre tap and
        keeps its colour likewise -- a firefly is never removed;
      * otherwise an infinite tap has an infinite colour distance and the weight 0, and 0 * inf = NaN in the channels that are
        infinite: those channels of the output are NaN, the others are finite.
    Later passes repeat this, so after k passes every difference lies among the pixels that chains of taps connect to a firefly
    (at most 2 (2^k - 1) columns and rows away); outside them the output equals, bit for bit, the filter's over the frame with the
    fireflies replaced.  Background pixels keep their colour, and the alpha channel is the input's bits untouched."""
    c, g, p = dc.filter_case(f"fireflies-{iterations}")
    assert p["iterations"] == iterations
    rgb = c[..., :3]
    bad = ~np.isfinite(rgb).all(axis=-1)
    assert 0 < bad.sum() < 0.01 * bad.size
    kinds = rgb[~np.isfinite(rgb)]
    assert np.isposinf(kinds).any() and np.isneginf(kinds).any() and np.isnan(kinds).any()
    out = ref.atrous(c, g, p)
    hit = _hit(g)
    nan_px = np.isnan(out[..., :3]).any(axis=-1)
    fin_px = np.isfinite(out[..., :3]).all(axis=-1)
    print(f"fireflies, {iterations} passes: NaN pixels {nan_px.sum()}, finite hit pixels {(fin_px & hit).sum()} of {hit.sum()} hit pixels")
    assert (nan_px & hit).sum() >= 50 and (fin_px & hit).sum() >= 50
    assert np.array_equal(dc.bits(out[~hit]), dc.bits(c[~hit]))                              # background: a copy
    assert np.array_equal(dc.bits(out[..., 3]), dc.bits(c[..., 3]))                          # alpha: a copy
    assert np.array_equal(dc.bits(out[bad]), dc.bits(c[bad]))                                # a firefly stays as it is
    reach = _dilate(bad, hit, iterations)
    assert not (nan_px & ~reach & hit).any()
    clean = c.copy()
    clean[..., :3][~np.isfinite(rgb)] = 0.25
    calm = ref.atrous(clean, g, p)
    rest = hit & ~reach
    assert rest.sum() >= 50 and np.array_equal(dc.bits(out[..., :3])[rest], dc.bits(calm[..., :3])[rest])
    if iterations == 1:
        nan_tap = _dilate(np.isnan(rgb).any(axis=-1), hit, 1)
        assert np.array_equal(dc.bits(out[nan_tap]), dc.bits(c[nan_tap])) and nan_tap.sum() > np.isnan(rgb).any(axis=-1).sum()
        for ch in range(3):
            inf_tap = _dilate(np.isinf(rgb[..., ch]), hit, 1) & ~nan_tap & ~bad
            assert inf_tap.sum() >= 10 and np.isnan(out[..., ch][inf_tap]).all()
            assert np.isfinite(out[..., ch][hit & ~nan_tap & ~bad & ~inf_tap]).all()


def test_alpha_is_a_copy_of_the_inputs_bits():
    """Random bit patterns in the alpha channel, signalling and quiet NaNs with payloads among them, leave every filter case as they
    entered it."""
    seen_snan = seen_qnan = False
    for name in ("npow8", "hdr", "hostile-depth", "hostile-normals", "ringed-hit", "deep-16-17x5", "tile-17x17"):
        c, g, p = dc.filter_case(name)
        a = dc.bits(c[..., 3])
        nan = (a & 0x7F800000 == 0x7F800000) & (a & 0x007FFFFF != 0)
        seen_snan |= bool((nan & (a & 0x00400000 == 0)).any())
        seen_qnan |= bool((nan & (a & 0x00400000 != 0)).any())
        assert np.array_equal(dc.bits(ref.atrous(c, g, p)[..., 3]), a)
    assert seen_snan and seen_qnan


def test_hostile_depths_are_present_and_split_into_hits_and_background():
    c, g, p = dc.filter_case("hostile-depth")
    z = ref.unpack_guides(g)[2]
    zb = dc.bits(z)
    for v in dc.HOSTILE_DEPTHS:
        assert (zb == dc.bits(np.array([v]))[0]).sum() >= 1, v
    hit = _hit(g)
    for v, is_hit in zip(dc.HOSTILE_DEPTHS, (False, False, False, False, True, True, True, True)):
        assert np.all(hit[zb == dc.bits(np.array([v]))[0]] == is_hit), v
    out = ref.atrous(c, g, p)
    changed = (dc.bits(out[..., :3]) != dc.bits(c[..., :3])).any(axis=-1)
    assert not changed[~hit].any()
    for lo, hi in ((0, 6), (6, 10)):                           # in the strips of extreme but comparable depths the filter does filter
        assert changed[lo:hi].sum() >= 50
    with np.errstate(all="ignore"):
        szs = ref.pass_constants(p)[0][0][3]
        inv_z = f32(1) / (szs * z)
    assert np.isinf(inv_z[hit]).any() and ((inv_z[hit] > 0) & (inv_z[hit] < dc.FLT_MIN)).any()      # a subnormal depth; FLT_MAX: a subnormal quotient


def test_hostile_normals_and_albedos_are_present():
    c, g, p = dc.filter_case("hostile-normals")
    n, a, z = ref.unpack_guides(g)
    ln = np.sqrt((n.astype(np.float64) ** 2).sum(-1))
    assert (ln == 0).sum() >= 50 and (np.abs(ln - 3) < 0.01).sum() >= 50
    assert np.isnan(n).any(axis=-1).sum() >= 50 and np.isinf(n).any(axis=-1).sum() >= 50
    assert (a == 65504).sum() >= 50 and np.isinf(a).sum() >= 50
    with np.errstate(all="ignore"):
        d = ref._dot(n[:, 1:], n[:, :-1])
    assert (d < 0).sum() >= 50
    out = ref.atrous(c, g, p)
    assert (dc.bits(out[..., :3]) != dc.bits(c[..., :3])).any(axis=-1).sum() >= 50


def test_background_cases():
    c, g, p = dc.filter_case("all-background")
    assert not _hit(g).any() and np.array_equal(dc.bits(ref.atrous(c, g, p)), dc.bits(c))
    c, g, p = dc.filter_case("single-hit")
    assert _hit(g).sum() == 1 and np.array_equal(dc.bits(ref.atrous(c, g, p)), dc.bits(c))      # its only tap is itself: c w / w
    c, g, p = dc.filter_case("ringed-hit")
    hit = _hit(g)
    ringed = [(y, x) for y in range(1, hit.shape[0] - 1) for x in range(1, hit.shape[1] - 1)
              if hit[y, x] and hit[y - 1: y + 2, x - 1: x + 2].sum() == 1]
    assert len(ringed) == 3
    out = ref.atrous(c, g, p)
    assert any(not np.array_equal(dc.bits(out[y, x]), dc.bits(c[y, x])) for y, x in ringed)        # the later passes jump the ring


def test_late_refusal_constants_leave_the_finite_range_at_a_later_pass_only():
    for bad in dc.LATE_REFUSALS:
        with np.errstate(all="ignore"):
            deep, _ = ref.pass_constants(dict(bad, iterations=16))
            shallow, _ = ref.pass_constants(dict(bad, iterations=5))
        assert all(np.isfinite(k) and k > 0 for step, kc, ka, szs in shallow for k in (kc, ka, szs))
        assert any(not np.isfinite(k) for step, kc, ka, szs in deep[5:] for k in (kc, ka, szs))
        assert all(np.isfinite(k) for step, kc, ka, szs in deep[:5] for k in (kc, ka, szs))


# ---- the guide pass ---------------------------------------------------------------------------
def test_degenerate_normals_take_the_fallback_on_one_side_of_the_threshold(hrt, oracle):
    for name, w, h in dc.GUIDE_CASES:
        if name != "degenerate":
            continue
        scene = dc.scene_by_name(hrt, name, w, h)
        assert scene["camera"]["opengl"] is False
        cam = dc.cam_of(hrt, scene["camera"])
        osc = oracle.OracleScene(scene)
        with np.errstate(all="ignore"):                         # (0 * inf under the fallback, 1e5 -> half infinity)
            g = ref.primary_guides(osc, scene, cam, w, h)
        dirs = ref.primary_directions(w, h, *cam[1:])
        t, u, v, prim, inst = osc.trace(np.broadcast_to(cam[0], dirs.shape).copy(), dirs)
        osc.close()
        n, a, z = ref.unpack_guides(g)
        inst = inst.reshape(h, w)
        fallback = (n == np.array([0, 0, 1], np.float32)).all(axis=-1) & np.isfinite(z)
        px = w * h
        assert np.all(fallback[(inst == 0) | (inst == 1)]) and _enough(fallback[inst == 0].sum(), px) and _enough(fallback[inst == 1].sum(), px)
        assert not fallback[inst == 2].any() and _enough((inst == 2).sum(), px)                     # 1e-5 long: normalised
        assert _enough(fallback[inst == 3].sum(), px) and _enough((~fallback[inst == 3]).sum(), px)  # the threshold inside a triangle
        assert not fallback[inst == 4].any()
        assert _enough(np.isinf(a[inst == 2]).sum(), px) and np.isfinite(a[inst != 2]).all()        # albedo 1e5, 7e4: half infinities


# ---- the temporal mode -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def walked(hrt, oracle):
    """Every sequence (but the full-size one) through the specification, once: id -> list of frames with their diagnostics."""
    out = {}
    for name, seq in dc.temporal_sequences(hrt).items():
        if not seq.get("gpu_only"):
            out[name] = (seq, list(dc.walk_sequence(hrt, oracle, name, seq, with_diag=True)))
    return out


def _frames_with_history(frames):
    return [f for f in frames if f["diag"]]


def test_temporal_sizes_fill_no_block(hrt):
    sizes = {s["size"] for s in dc.temporal_sequences(hrt).values()}
    assert {(97, 61), (1, 1), (1, 37), (255, 1), (257, 3)} <= sizes
    assert sum(1 for w, h in sizes if (w * h) % 256 and (w * h) % 64) >= 5


def test_small_alpha_min_takes_the_reciprocal(walked):
    seq, frames = walked["alpha-small"]
    am = f32(seq["tparams"]["alpha_min"])
    assert seq["in_place"] and seq["params"] != None and am <= 0.05           # noqa: E711
    for f in _frames_with_history(frames):
        L = f["L"]
        assert ((L > 1) & (f32(1) / np.where(L > 0, L, 1) > am)).sum() >= 50
    assert len(_frames_with_history(frames)) >= 4
    # the size sequences run the same parameters on frames that fill no block
    for name, (s2, fr2) in walked.items():
        if name.startswith("size-"):
            assert any((f["L"] > 1).sum() >= 1 for f in fr2), name


@pytest.mark.parametrize("name,cap,n_frames", [("cap-3", 3, 6), ("cap-default-static", 32, 40)])
def test_history_length_reaches_its_cap(walked, name, cap, n_frames):
    seq, frames = walked[name]
    assert len(frames) >= n_frames
    tp = dict(tref.DEFAULTS)
    tp.update(seq["tparams"] or {})
    assert tp["max_history"] == cap
    if name == "cap-default-static":
        assert seq["tparams"] is None
    above = below = 0
    px = seq["size"][0] * seq["size"][1]
    for f in _frames_with_history(frames):
        d = f["diag"]
        blended = d["sw"] > 0
        above += int((d["unclamped"][blended] > cap).sum())
        below += int((d["unclamped"][blended] < cap).sum())
        assert f["L"].max() <= cap
    last = frames[-1]["diag"]
    assert _enough(int((last["unclamped"][last["sw"] > 0] > cap).sum()), px)
    assert _enough(above, px) and _enough(below, px)


def test_turned_camera_leaves_points_behind_the_previous_one(walked):
    seq, frames = walked["turn"]
    behind = [int((f["diag"]["s"] <= 0).sum()) for f in _frames_with_history(frames)]
    ahead = [int((f["diag"]["s"] > 0).sum()) for f in _frames_with_history(frames)]
    print(f"turn: hit pixels behind the previous camera per frame {behind}, in front {ahead}")
    assert behind[0] >= 50 and ahead[0] >= 50 and sum(1 for b in behind if b >= 50) >= 2
    f = frames[1]
    d = f["diag"]
    L = f["L"].reshape(-1)[d["sel"]]
    assert np.all(L[d["s"] <= 0] == 1) and np.isnan(f["motion"].reshape(-1, 2)[d["sel"]][d["s"] <= 0]).all()


def test_pan_zoom_roll_reach_every_kind_of_tap_set(walked):
    """Taps inside the frame: 0, 1, 2 and 4 of them.  (Three cannot be: a tap is inside if its column and its row are, so the count is
    a product of two numbers from 0..2.)  Taps taken -- inside, the same primitive, the depth agreeing: every count from 0 to 4."""
    seq, frames = walked["pan-zoom-roll"]
    assert any(f["camera"]["opengl"] is False for f in frames)
    inside = np.zeros(5, np.int64)
    taken = np.zeros(5, np.int64)
    for f in _frames_with_history(frames):
        d = f["diag"]
        proj = d["s"] > 0
        inside += np.bincount(d["inside"][proj].sum(axis=1), minlength=5)
        taken += np.bincount(d["taken"][proj].sum(axis=1), minlength=5)
    print(f"pan-zoom-roll: pixels by taps inside {inside.tolist()}, by taps taken {taken.tolist()}")
    assert inside[3] == 0
    assert inside[0] >= 50 and inside[2] >= 50 and inside[4] >= 50 and inside[1] >= 1
    assert all(taken[k] >= 50 for k in (0, 1, 2, 3, 4))


def test_a_reprojection_can_be_non_finite(walked):
    """Both cameras at the origin with |W| = 1e19, turned by 90 degrees: s is of the order 1e-39 and x' overflows."""
    seq, frames = walked["nonfinite"]
    n_inf = n_nan_frac = 0
    for f in _frames_with_history(frames):
        d = f["diag"]
        proj = d["s"] > 0
        with np.errstate(all="ignore"):
            n_inf += int((~np.isfinite(d["xp"][proj])).sum())
            fx = d["xp"][proj] - np.floor(d["xp"][proj])
        n_nan_frac += int(np.isnan(fx).sum())
        m = f["motion"].reshape(-1, 2)[d["sel"]][proj]
        assert np.array_equal(np.isinf(m[:, 0]), np.isinf(d["xp"][proj]))
    print(f"nonfinite: projected pixels with a non-finite x' {n_inf}, with fx = NaN {n_nan_frac}")
    assert n_inf >= 1 and n_nan_frac >= 1


def test_depth_tolerance_alone_decides(walked):
    seq, frames = walked["depth-tight"]
    assert seq["tparams"]["depth_tolerance"] <= 1e-6
    by_depth = 0
    for f in _frames_with_history(frames):
        d = f["diag"]
        by_depth += int((d["inside"] & d["same_id"] & ~d["depth_ok"]).sum())
    assert by_depth >= 50
    seq, frames = walked["depth-loose"]
    assert seq["tparams"]["depth_tolerance"] >= 1
    kept = 0
    for f in _frames_with_history(frames):
        d = f["diag"]
        assert not (d["inside"] & d["same_id"] & ~d["depth_ok"]).any()
        kept += int(d["taken"].sum())
    assert kept >= 50
    assert walked["depth-tight"][0]["frames"] is seq["frames"]               # the same motion under both tolerances


def test_instance_transforms_reject_by_id_and_keep_history(walked):
    seq, frames = walked["instances"]
    changed = [sorted(f["changed"]) for f in frames]
    assert changed == [[], [3], [0], [2], [1]]
    for f in _frames_with_history(frames):
        d = f["diag"]
        by_id = (d["inside"] & ~d["same_id"]).sum()
        inst = f["hist"]["inst"].reshape(-1)[d["sel"]]
        L = f["L"].reshape(-1)[d["sel"]]
        moved = np.isin(inst, list(f["changed"]))
        print(f"instances frame {f['k']}: taps rejected by id {by_id}, pixels of the moved instance {moved.sum()}, with history {(L[moved] > 1).sum()}")
        assert by_id >= 50
        assert moved.sum() >= 50 and (L[moved] > 1).sum() >= 50
    # the 90 degree turn and the uneven scales are what they say
    lin = lambda k, i: np.asarray(frames[k]["changed"][i], np.float64).reshape(3, 4)[:, :3]      # noqa: E731
    base = lambda i: np.asarray(frames[0]["scene"]["instances"][i]["transform"], np.float64)       # noqa: E731
    r = lin(2, 0)
    assert np.allclose(r @ r.T, np.eye(3), atol=1e-6) and abs(np.trace(r) - 1) < 1e-6                # a rotation by 90 degrees
    sv = np.linalg.svd(lin(3, 2), compute_uv=False)
    assert sv.max() / sv.min() > 1.5


def test_hostile_colour_in_the_history(walked):
    """Pinned on the specification: a non-finite colour enters the accumulated colour as it is on its first frame (A = C without
    history, H + alpha (C - H) with), and once in the history it makes NaN of every pixel that takes it as a tap, weight 0 included."""
    seq, frames = walked["hostile-color"]
    assert seq["color"] == "hostile"
    assert np.isfinite(frames[0]["A"][..., :3]).all() and (np.abs(frames[0]["A"][..., :3]) > 1e30).sum() >= 50
    nan_counts = [int(np.isnan(f["A"][..., :3]).any(axis=-1).sum()) for f in frames]
    print(f"hostile-color: pixels with NaN in A per frame {nan_counts}")
    assert nan_counts[-1] >= 1 and nan_counts[-1] < 0.5 * frames[-1]["L"].size
    for f in frames:
        assert np.array_equal(dc.bits(f["A"][..., 3]), dc.bits(f["color"][..., 3]))
        assert np.array_equal(dc.bits(f["want"][..., 3]), dc.bits(f["color"][..., 3]))
        assert np.isfinite(f["L"]).all()
