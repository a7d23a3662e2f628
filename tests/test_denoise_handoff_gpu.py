"""The denoiser's history hand-over across TLAS handles on the MI355X (include/hrt.h hrt_denoise_temporal_rebind, csrc/denoise_link.hip
k_denoise_temporal_linked): sequences that change TLAS bit for bit against the numpy specification (tests/denoise_handoff_ref.py) over
the oracle's primary hits, maps that permute, drop, add and re-shape instances, the lifetime of the link, the argument checks, the
primary-hit capture, and hrt_time_render's file boundary.  Figures: profiles/r21_denoise_handoff.txt."""
import importlib
import subprocess
from pathlib import Path

import numpy as np
import pytest

import denoise_handoff_cases as cases
import denoise_handoff_ref as href

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
SAMPLE = ROOT / "tests" / "golden" / "files" / "config.json"
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


FLAGS = {"production": lambda hrt: 0, "counting": lambda hrt: hrt.CTX_COUNT, "two_level": lambda hrt: hrt.CTX_TWO_LEVEL}


@pytest.mark.parametrize("size", cases.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("variance", [False, True], ids=["temporal", "variance"])
@pytest.mark.parametrize("mode", ["production", "counting", "two_level"])
def test_handoff_bit_exact(hrt_gpu, oracle, mode, variance, size):
    """cases.SEQUENCE: frames 0-2 on TLAS A with one update_instances, then hrt_denoise_temporal_rebind to TLAS B -- the same BLASes at
    the next poses, from build_tlas -- and frames 3-4 on B with an update before frame 4.  Output, A, L, motion (moments and variance
    in the variance-guided mode) of every frame equal the specification's over the oracle's hits; frame 3 blends with the history on
    more than 0.3 of its hit pixels (test_temporal_bit_exact's figure); exactly one call counts as begun from a linked history."""
    hrt = hrt_gpu
    w, h = size
    sc = cases.scene(hrt, w, h)
    cam = cases.camera(hrt, sc)
    r = hrt.Renderer(0, FLAGS[mode](hrt))
    try:
        r.load_scene(sc)
        r.set_frame(w, h, hrt.scenes.SEED_SALT)
        hist, on = None, "A"
        for k, (tlas, pose) in enumerate(cases.SEQUENCE):
            link = None
            if tlas != on:
                b = r.build_tlas(None, cases.poses(hrt, pose))
                r.denoise_temporal_rebind(b)
                r.use_tlas(b)
                link = href.make_link(href.blas_ids(sc), href.blas_ids(sc))
                on = tlas
            elif k > 0 and pose != cases.SEQUENCE[k - 1][1]:
                r.update_instances(cases.poses(hrt, pose))
            color, got = _call(r, variance)
            cur = href.sub_scene(sc, None, cases.poses(hrt, pose))
            want, hist = cases.spec_frame(oracle, variance, hist, link, color, cur, cam, w, h, instanced=(mode == "two_level"))
            _compare(k, got, want)
            if k > 0:
                assert (want["L"] > 1).sum() > 0.3 * (want["L"] > 0).sum(), k
        assert r.stats().denoise_history_rebinds == 1
    finally:
        r.close()


@pytest.mark.parametrize("variance", [False, True], ids=["temporal", "variance"])
def test_handoff_to_an_identical_tlas_changes_nothing(hrt_gpu, variance):
    """Two renderers with the same seeds: one stays on TLAS A, the other rebinds to a second TLAS built from the identical instance
    array.  Output, A, L and motion of the two following frames are the same bits."""
    hrt = hrt_gpu
    w, h = cases.SIZES[1]
    sc = cases.scene(hrt, w, h)
    rs = [hrt.Renderer(0, 0), hrt.Renderer(0, 0)]
    try:
        for r in rs:
            r.load_scene(sc)
            r.set_frame(w, h, hrt.scenes.SEED_SALT)
            for _ in range(2):
                _call(r, variance)
        b = rs[1].build_tlas()
        rs[1].denoise_temporal_rebind(b)
        rs[1].use_tlas(b)
        for k in range(2):
            (_, stay), (_, moved) = _call(rs[0], variance), _call(rs[1], variance)
            _compare(k, moved, stay)
            assert (stay["L"] > 1).any()
        assert [r.stats().denoise_history_rebinds for r in rs] == [0, 1]
    finally:
        for r in rs:
            r.close()


def _chain(hrt, oracle, r, sc, cam, w, h, steps, variance):
    """steps: (order, pose, how) per frame -- the frame runs on build_tlas(order) at cases.poses(pose)[order].  how: "same" (the TLAS of
    the frame before, updated if the pose differs), "fresh" (a new TLAS, no rebind), None (rebind with the NULL map) or the map.
    Every frame is compared with the specification; the instances the link does not carry have L = 1 and NaN motion on their pixels."""
    hist, order_prev, pose_prev = None, None, None
    for k, (order, pose, how) in enumerate(steps):
        tf = cases.poses(hrt, pose)[order]
        link = None
        if how == "same":
            assert order == order_prev
            if pose != pose_prev:
                r.update_instances(tf)
        else:
            t = r.build_tlas(order, tf)
            if how == "fresh":
                hist = None
            else:
                r.denoise_temporal_rebind(t, how)
                link = href.make_link(href.blas_ids(sc, order_prev), href.blas_ids(sc, order), how)
            r.use_tlas(t)
        color, got = _call(r, variance)
        want, hist = cases.spec_frame(oracle, variance, hist, link, color, href.sub_scene(sc, order, tf), cam, w, h)
        _compare(k, got, want)
        if link is not None:
            hit = hist["inst"] != href.MISS
            new = np.zeros_like(hit)
            new[hit] = link[hist["inst"][hit]] == NO
            assert np.all(got["L"][new] == 1) and np.isnan(got["motion"][new]).all(), k
            assert (got["L"][hit & ~new] > 1).any() or not (link != NO).any(), k
        order_prev, pose_prev = order, pose
    return hist


ALL = list(range(cases.N_PARTICLES + 1))
_PERM = [int(k) for k in np.random.default_rng(7).permutation(len(ALL))]
# one instance taken out of the middle (the map shifts) and one appended that was not there
_DROP = ALL[:12] + ALL[13:] + [13]
_DROP_MAP = ALL[:12] + ALL[13:] + [NO]
# another BLAS at index 13: scene instance 14 (shape 1) where instance 13 (shape 0) was, under the NULL map
_SWAP = ALL[:13] + [14] + ALL[14:]
MAP_CASES = {
    "permuted": [(ALL, 0, "fresh"), (ALL, 1, "same"), (_PERM, 2, _PERM), (_PERM, 3, "same")],
    "removed_and_appended": [(ALL, 0, "fresh"), (ALL, 1, "same"), (_DROP, 2, _DROP_MAP), (_DROP, 3, "same")],
    "null_map_other_blas": [(ALL, 0, "fresh"), (ALL, 1, "same"), (_SWAP, 2, None), (_SWAP, 3, "same")],
    # instance counts 1 -> 3 -> 1 in a context whose history was first made for a single instance: the linked call reads the last
    # (only) entry of a one-entry table while the set it writes grows, twice through the same predecessor; back down, the map reads
    # the last entry of the three-entry table.  13, 16 and 19 share shape 0; 14 is shape 1.
    "one_three_one": [([13], 0, "fresh"), ([13], 1, "same"), ([16, 13, 14], 2, [0, 0, NO]), ([16, 13, 14], 3, "same"), ([14], 4, [2]),
                      ([14, 13], 5, None)],
}


@pytest.mark.parametrize("variance", [False, True], ids=["temporal", "variance"])
@pytest.mark.parametrize("case", sorted(MAP_CASES))
def test_handoff_maps(hrt_gpu, oracle, case, variance):
    hrt = hrt_gpu
    w, h = cases.SIZES[1]
    sc = cases.scene(hrt, w, h)
    cam = cases.camera(hrt, sc)
    r = hrt.Renderer(0, 0)
    try:
        r.load_scene(sc)
        r.set_frame(w, h, hrt.scenes.SEED_SALT)
        _chain(hrt, oracle, r, sc, cam, w, h, MAP_CASES[case], variance)
        assert r.stats().denoise_history_rebinds == sum(1 for s in MAP_CASES[case] if s[2] not in ("same", "fresh"))
    finally:
        r.close()


@pytest.mark.parametrize("variance", [False, True], ids=["temporal", "variance"])
def test_handoff_link_lifetime(hrt_gpu, variance):
    """What drops the link -- a launch on a third handle, a reset, a new frame size, the other mode, no history to begin with, going
    back without a rebind -- makes the next call a fresh start: no motion, L = 1 on every hit pixel, and the bits of a call after
    hrt_denoise_temporal_reset on the same colour buffer (hrt_denoise_launch's in the temporal mode).  The second call on B after a
    linked one carries history as usual, and denoise_history_rebinds counts the linked calls only."""
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
        if not var:
            assert np.array_equal(_bits(out), _bits(r.denoise().cpu().numpy()))

    def carried():
        call()
        return (r.denoise_temporal_state()[1].cpu().numpy() > 1).any()

    def history_on(t):
        r.use_tlas(t)
        r.denoise_temporal_reset()
        r.render(1)
        call()
        assert carried()

    try:
        r.load_scene(sc)
        r.set_frame(w, h, hrt.scenes.SEED_SALT)
        a = r.tlas
        b, c = r.build_tlas(), r.build_tlas()
        rebinds = lambda: r.stats().denoise_history_rebinds      # noqa: E731
        history_on(a)
        r.denoise_temporal_rebind(b)
        r.use_tlas(c)                                  # a launch on a third handle
        fresh()
        r.use_tlas(b)
        fresh()                                        # ... which has dropped the link to B as well
        history_on(a)
        r.denoise_temporal_rebind(b)
        r.denoise_temporal_reset()                     # a reset
        r.use_tlas(b)
        fresh()
        history_on(a)
        r.denoise_temporal_rebind(b)
        r.use_tlas(b)
        r.set_frame(w // 2, h // 2, hrt.scenes.SEED_SALT)      # a new frame size
        r.render(1)
        fresh()
        r.set_frame(w, h, hrt.scenes.SEED_SALT)
        r.render(1)
        history_on(a)
        r.denoise_temporal_rebind(b)
        r.use_tlas(b)
        fresh(not variance)                            # the other mode
        r.denoise_temporal_reset()
        r.denoise_temporal_rebind(a)                   # no history: HRT_OK, nothing linked
        r.use_tlas(a)
        fresh()
        assert rebinds() == 0
        history_on(a)
        d = r.build_tlas()
        r.denoise_temporal_rebind(d)
        r.destroy_tlas(d)                              # the link's TLAS destroyed: the history stays A's
        assert carried() and rebinds() == 0
        r.denoise_temporal_rebind(c)
        r.denoise_temporal_rebind(b)                   # another rebind replaces the link
        r.use_tlas(c)
        fresh()
        history_on(a)
        r.denoise_temporal_rebind(b)
        r.use_tlas(b)
        assert carried() and rebinds() == 1            # the linked call
        assert carried() and rebinds() == 1            # the second call on B: ordinary, with history
        r.use_tlas(a)                                  # back to A with no rebind
        fresh()
        assert rebinds() == 1
    finally:
        r.close()


def test_handoff_rejects_bad_arguments(hrt_gpu):
    hrt = hrt_gpu
    w, h = 16, 12
    sc = cases.scene(hrt, w, h)
    n = len(sc["instances"])
    r = hrt.Renderer(0, 0)
    try:
        r.load_scene(sc)
        r.set_frame(w, h, hrt.scenes.SEED_SALT)
        small = r.build_tlas([0, 13, 14])
        b = r.build_tlas()
        for _ in range(2):                             # with and without a history
            with pytest.raises(hrt.HrtError, match="status -1"):
                r.denoise_temporal_rebind(0xDEAD)                                  # not a TLAS
            with pytest.raises(hrt.HrtError, match="status -1"):
                r.denoise_temporal_rebind(b, list(range(n - 1)))                   # not its instance count
            with pytest.raises(hrt.HrtError, match="status -1"):
                r.denoise_temporal_rebind(small, [0, 1, 2, 3])
            r.use_tlas(small)
            r.render(1)
            r.denoise_temporal()
        for bad in ([0, 1, 3], [0, 1, n], [NO - 1, 1, 2]):                         # the history's TLAS has 3 instances
            with pytest.raises(hrt.HrtError, match="status -1"):
                r.denoise_temporal_rebind(b, bad + [NO] * (n - 3))
        r.denoise_temporal_rebind(b, [2, 2, 2, NO] + [0] * (n - 4))                # duplicates and the last entry are taken
        r.use_tlas(b)
        r.render(1)
        r.denoise_temporal()
        assert r.stats().denoise_history_rebinds == 1
    finally:
        r.close()


@pytest.mark.parametrize("variance", [False, True], ids=["temporal", "variance"])
def test_handoff_takes_the_primary_capture(hrt_gpu, variance):
    """Under HRT_CTX_CAPTURE_PRIMARY the first frame on B takes its guides from the render launch's capture -- guide_passes_captured
    rises by one -- and gives the bits of a context without the flag."""
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
            b = r.build_tlas(None, cases.poses(hrt, 1))
            r.denoise_temporal_rebind(b)
            r.use_tlas(b)
            before = r.stats()
            got.append(_call(r, variance)[1])
            after = r.stats()
            captured = after.guide_passes_captured - before.guide_passes_captured
            assert captured == (1 if r is rs[0] else 0) and after.denoise_history_rebinds == 1
            assert after.guide_passes_traced - before.guide_passes_traced == 1 - captured
        _compare(0, got[0], got[1])
        assert (got[0]["L"] > 1).any()
    finally:
        for r in rs:
            r.close()


def _time_sequence(hrt, w, h, frames, handoff):
    """hrt_time_render's loop through the Python host: the untimed launch, then `frames` Time-mode frames, a new TLAS per file (with or
    without the hand-over).  Returns the 8-bit image of the last frame and the history length it ended on."""
    io = importlib.import_module("nvidia-optix-ray-tracer_amd.io")
    tm = io.time_mode_scene(SAMPLE, width=w, height=h)
    cfg = tm["config"]
    per_file = [int(np.float32(d) * np.float32(cfg["fps"] * cfg["render-speed-ratio"])) for d in tm["durations"]]      # RendererTime.cu:427-428
    assert per_file[:2] == [9, 9] and per_file == tm["frame_counts"]
    r = hrt.Renderer(0, 0)
    try:
        r.load_scene(tm["scene"])
        r.set_frame(w, h, hrt.scenes.SEED_SALT)
        r.render(1)
        r.denoise_temporal(out=r.color)
        f, done = 0, 0
        while done < frames:
            if f > 0:
                t = r.build_tlas()                     # the file's own IAS, identity-posed like every one of the driver's
                if handoff:
                    r.denoise_temporal_rebind(t)
                r.use_tlas(t)
            nxt = tm["states"][min(f + 1, len(tm["states"]) - 1)]
            for frame in range(per_file[f]):
                if done == frames:
                    break
                r.pose_instances(tm["states"][f], nxt, float(tm["durations"][f]), frame, per_file[f], first_instance=tm["n_extra"],
                                 offset=cfg["particle-shift"], scale=cfg["particle-scale"])
                r.render(1)
                r.denoise_temporal(out=r.color)
                done += 1
            f += 1
        return r.to_rgba8().cpu().numpy()[..., :3], r.denoise_temporal_state()[1].cpu().numpy(), r.stats().denoise_history_rebinds
    finally:
        r.close()


def test_time_driver_hands_the_history_over(hrt_gpu, tmp_path):
    """hrt_time_render --denoise-temporal on the shipped sample at 120x80 for 11 frames, of which 9 -- the driver's frame-count
    expression over the sample's values -- lie in file 0 and two in file 1: its image is the Python sequence's with a rebind at the
    file boundary, and with --no-history-handoff the sequence's without one.  The two differ, and only the first ends on a history
    longer than the two frames of file 1."""
    hrt = hrt_gpu
    w, h = 120, 80
    exe = ROOT / "nvidia-optix-ray-tracer_amd" / "lib" / "hrt_time_render"
    assert exe.exists(), "run `make tools`"
    images = {}
    for handoff in (True, False):
        out = tmp_path / f"frame{int(handoff)}.ppm"
        extra = [] if handoff else ["--no-history-handoff"]
        subprocess.run([str(exe), str(SAMPLE), str(SAMPLE.parent), "11", str(out), str(w), str(h), "--denoise-temporal", *extra], check=True, timeout=300)
        raw = out.read_bytes()
        header = f"P6\n{w} {h}\n255\n".encode()
        assert raw.startswith(header)
        got = np.frombuffer(raw[len(header):], np.uint8).reshape(h, w, 3)
        want, L, rebinds = _time_sequence(hrt, w, h, 11, handoff)
        assert np.array_equal(got, want), handoff
        assert rebinds == (1 if handoff else 0)
        assert (L.max() > 2) == handoff, (handoff, L.max())
        images[handoff] = got
    assert not np.array_equal(images[True], images[False])


def test_handoff_quality_at_the_file_boundary(hrt_gpu):
    """The shipped sample at 120x80 and 1 spp, hrt_time_render's loop up to the first frame of file 1, denoised there with the
    hand-over and as the fresh start it used to be, against 4096 spp of that pose: the hand-over's MSE is at most BOUND times the
    reset's.  The specification over the oracle's hits measures 0.5748 on the CPU (tools/denoise_handoff_spec.py,
    profiles/r21_denoise_handoff.txt; the GPU gives the same frames bit for bit); BOUND is halfway between that and 1.  Next to
    guide edges -- test_temporal_quality_animation's mask -- the hand-over's error does not exceed the raw frame's: nothing ghosts
    across the boundary."""
    BOUND = 0.7874
    from test_denoise_temporal_gpu import _edge_pixels, _pose, _time_mode
    hrt = hrt_gpu
    w, h = 120, 80
    results = {}
    for handoff in (True, False):
        r = hrt.Renderer(0, 0)
        try:
            tm, cfg = _time_mode(hrt, r, w, h)
            per_file = tm["frame_counts"][0]
            r.render(1)
            r.denoise_temporal()
            for frame in range(per_file):
                _pose(r, tm, cfg, frame)
                r.render(1)
                r.denoise_temporal()
            t = r.build_tlas()
            if handoff:
                r.denoise_temporal_rebind(t)
            r.use_tlas(t)
            r.pose_instances(tm["states"][1], tm["states"][2], float(tm["durations"][1]), 0, tm["frame_counts"][1], first_instance=tm["n_extra"],
                             offset=cfg["particle-shift"], scale=cfg["particle-scale"])
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
        tm, cfg = _time_mode(hrt, r, w, h)
        r.pose_instances(tm["states"][1], tm["states"][2], float(tm["durations"][1]), 0, tm["frame_counts"][1], first_instance=tm["n_extra"],
                         offset=cfg["particle-shift"], scale=cfg["particle-scale"])
        r.render(4096)
        conv = r.color.cpu().numpy()[..., :3].astype(np.float64)
    finally:
        r.close()
    mse_h, mse_r = ((results[True] - conv) ** 2).mean(), ((results[False] - conv) ** 2).mean()
    e_raw, e_h = ((raw - conv) ** 2)[edge].mean(), ((results[True] - conv) ** 2)[edge].mean()
    print(f"sample file boundary: mse reset {mse_r:.6g} hand-over {mse_h:.6g} ratio {mse_h / mse_r:.4f}; "
          f"edges ({edge.sum()} px) raw {e_raw:.6g} hand-over {e_h:.6g} ratio {e_h / e_raw:.4f}")
    assert BOUND < 1
    assert mse_h <= BOUND * mse_r
    assert e_h <= e_raw
