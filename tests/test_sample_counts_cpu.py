"""The adaptive-sampling reference (tests/sample_counts_ref.py) against the CPU oracle, and the reach of the inputs the GPU tests feed the
allocator (hrt_sample_counts) and the end-to-end render: conditions that make those tests meaningful, checked where no GPU is needed."""
import numpy as np
import pytest

import sample_counts_ref as ref

W, H = 32, 24
TOTALS = (1, 2, 5, 8, 12)


def _scene(hrt, name):
    return {"c1": lambda: hrt.scenes.cornell_box(W, H, 1), "mixed": lambda: hrt.scenes.mixed_test_scene(width=W, height=H, transforms=True)}[name]()


@pytest.mark.parametrize("name", ["c1", "mixed"])
def test_accumulated_single_samples_are_the_oracles_render(hrt, oracle, name):
    """Per-sample linear radiance of successive spp = 1 renders, added in sample order with the first sample assigned and divided by n, is the
    oracle's spp = n linear frame bit for bit, and so are the RNG states -- over one launch after another of one sample each, from a sum
    that starts as garbage."""
    osc = oracle.OracleScene(_scene(hrt, name))
    try:
        states = oracle.rng_init(W, H, hrt.scenes.SEED_SALT)
        sum4 = np.full((W * H, 4), np.nan, np.float32); taken = np.zeros(W * H, np.uint32)
        for n in range(1, max(TOTALS) + 1):
            ref.accumulate(osc, W, H, states, 1, sum4, taken)
            if n not in TOTALS:
                continue
            want_states = oracle.rng_init(W, H, hrt.scenes.SEED_SALT)
            want = osc.render(W, H, want_states, n)
            assert np.all(taken == n)
            assert np.array_equal(ref.mean(sum4, taken).view(np.uint32), want["linear"].reshape(-1, 4)[:, :3].view(np.uint32)), n
            assert np.array_equal(states, want_states), n
    finally:
        osc.close()


def test_a_count_map_leaves_the_other_pixels_streams_alone(hrt, oracle):
    """min(counts, spp) per pixel: pixels of count 0 keep state and sum, the others hold the oracle's render of their total."""
    osc = oracle.OracleScene(_scene(hrt, "c1"))
    try:
        counts = (np.arange(W * H, dtype=np.uint32) * 7) % 5           # 0 .. 4, clamped to 3 below
        states = oracle.rng_init(W, H, hrt.scenes.SEED_SALT); first = states.copy()
        sum4 = np.full((W * H, 4), -3.0, np.float32); taken = np.zeros(W * H, np.uint32)
        c = ref.accumulate(osc, W, H, states, 3, sum4, taken, counts)
        assert np.array_equal(c, np.minimum(counts, 3)) and np.array_equal(taken, c)
        assert np.array_equal(states[c == 0], first[c == 0]) and np.all(sum4[c == 0] == -3.0)
        for n in (1, 2, 3):
            st = first.copy()
            want = osc.render(W, H, st, n)
            sel = c == n
            assert np.array_equal(ref.mean(sum4, taken)[sel].view(np.uint32), want["linear"].reshape(-1, 4)[sel, :3].view(np.uint32))
            assert np.array_equal(states[sel], st[sel])
    finally:
        osc.close()


def test_the_pilots_count_map_is_worth_rendering(hrt, oracle):
    """C1 at 32 x 24, pilot 8, the defaults with max_total = 64: between 0.3 and 0.9 of the pixels take no more samples and the others take
    at least 10 distinct counts -- what the end-to-end GPU test's map must look like to test anything."""
    osc = oracle.OracleScene(_scene(hrt, "c1"))
    try:
        states = oracle.rng_init(W, H, hrt.scenes.SEED_SALT)
        sum4 = np.zeros((W * H, 4), np.float32); taken = np.zeros(W * H, np.uint32)
        ref.accumulate(osc, W, H, states, 8, sum4, taken)
        counts = ref.sample_counts(sum4.reshape(H, W, 4), taken.reshape(H, W), **dict(ref.DEFAULTS, max_total=64))
        zero = float(np.mean(counts == 0))
        print(f"zero share {zero:.2f}, distinct {len(np.unique(counts))}, at the cap {int(np.sum(counts + 8 == 64))}")
        assert 0.3 <= zero <= 0.9 and len(np.unique(counts)) >= 10
    finally:
        osc.close()


@pytest.mark.parametrize("size", ref.SIZES)
def test_the_synthetic_frames_reach_every_branch(size):
    """taken 0 and 1, the NaN -> 0 of fmaxf, x at and above the cap, total <= taken: with radius 0, sigma 0.5 and max_total 8 every frame size
    reaches them all (a 1 x 1 frame: the N_KINDS frames of that size together)."""
    w, h = size
    p = dict(target_sigma=0.5, min_total=1, max_total=8, radius=0)
    reached = {}
    for seed in range(ref.N_KINDS if w * h < 3 * ref.N_KINDS else 1):
        for k, v in ref.branches(*ref.synthetic_frame(w, h, seed), **p).items():
            reached[k] = reached.get(k, False) or v
    assert all(reached.values()) and len(reached) == 7, reached


def test_the_allocator_by_hand():
    """a few pixels worked out by hand: v = 2 and sigma 0.5 want 8 samples; limits, the window and `nothing known yet`"""
    sum4 = np.zeros((1, 3, 4), np.float32); taken = np.array([[2, 2, 1]], np.uint32)
    sum4[0, 0] = (0, 0, 0, 4.0)                 # v = 2
    sum4[0, 1] = (0.0, 0.0, 0.0, 0.0)           # two black samples: v = 0
    p = dict(target_sigma=0.5, min_total=1, max_total=64)
    assert ref.sample_counts(sum4, taken, radius=0, **p).tolist() == [[6, 0, 63]]
    assert ref.sample_counts(sum4, taken, radius=1, **p).tolist() == [[6, 62, 63]]            # the middle pixel sees +inf next to it
    assert ref.sample_counts(sum4, taken, radius=0, target_sigma=0.5, min_total=5, max_total=7).tolist() == [[5, 3, 6]]
    assert ref.sample_counts(sum4, taken, radius=0, target_sigma=1e-30, min_total=1, max_total=64).tolist() == [[62, 0, 63]]   # sigma^2 == 0: inf, NaN
