"""The inputs of the accumulated mode's tests, built deterministically from seeds in the style of tests/denoise_cases.py and shared by
tests/test_denoise_accumulated_cpu.py (which asserts on the numpy specification that they reach the branches they are for) and
tests/test_denoise_accumulated_gpu.py (which runs the kernels on exactly these inputs): sums and sample totals as hrt_render_accumulate
leaves them, guides, and parameters for hrt_denoise_accumulated_filter.

No test functions here."""
from __future__ import annotations

import numpy as np

import denoise_cases as dc
import denoise_variance_cases as vc
import sample_counts_ref as sref

f32 = np.float32

# id -> (sum4 (H, W, 4) float32, taken (H, W) uint32, guides (H, W, 8) uint16, params, vparams, linear_out, var_out); the last two "set" or "null"
SIZES = ((1, 1), (2, 1), (5, 3), (17, 5), (37, 29))          # (width, height); 37 x 29: three 16 x 16 tiles each way, 1073 pixels = 4 x 256 + 49
PASSES = (1, 2, 3, 4, 5)
HISTORY_MIN = (1, 2, 4, 65536)                               # 1: the definition's max(.., 2) decides
TAKEN_MAPS = ("zero", "one", "hmin", "mixed", "stripe", "island", "young-edges")
MIXED = np.array([0, 1, 2, 3, 4, 64, (1 << 24) - 1], np.uint32)
SUMS = ("plain", "hdr", "subnormal")
GUIDES = ("holes", "all-hits", "holes", "all-background")


def young_positions(h, w):
    """The four corners and the middle of the four edges."""
    ys, xs = (0, h // 2, h - 1), (0, w // 2, w - 1)
    return sorted({(y, x) for y in ys for x in xs if y in (0, h - 1) or x in (0, w - 1)})


def stripe_rows(h):
    """The rows of the striped tile: the middle third, one row at least."""
    return range(h // 3, max(h // 3 + 1, (2 * h) // 3))


def taken_map(kind, rng, h, w, history_min):
    """-> (taken (H, W) uint32, the pixels whose guide must be a hit for the map to do what it is for)."""
    t = np.zeros((h, w), np.uint32)
    must_hit = []
    if kind == "one":
        t[:] = 1
    elif kind == "hmin":
        t[:] = history_min
    elif kind == "mixed":
        t = rng.choice(MIXED, (h, w))
        t.reshape(-1)[: len(MIXED)] = MIXED[: t.size]        # every value, where the frame has room
    elif kind == "stripe":
        rows = list(stripe_rows(h))
        t[rows] = rng.choice(MIXED[1:], (len(rows), w))
    elif kind == "island":
        t[h // 2, w // 2] = 1
        must_hit = [(h // 2, w // 2)]
    elif kind == "young-edges":
        t[:] = 64
        must_hit = young_positions(h, w)
        for y, x in must_hit:
            t[y, x] = 1
    return t.astype(np.uint32), must_hit


def sums(kind, rng, taken):
    """Sums that `taken` samples of a plausible pixel leave: radiance of mean 0..1 (squared uniform), luminance with a standard deviation
    of 0 to 0.5.  hdr: means up to 3e38 (sums and squares overflow) and negative ones.  subnormal: means of 1e-40 and below."""
    h, w = taken.shape
    mean = rng.uniform(0, 1, (h, w, 3)) ** 2
    sd = rng.choice(np.array([0.0, 0.01, 0.1, 0.5]), (h, w))
    if kind == "hdr":
        mean = mean * rng.choice([1.0, 1e10, 1e19, 3e38], size=(h, w, 1), p=[0.5, 0.2, 0.15, 0.15])
        mean = mean * rng.choice([1.0, -1.0], size=(h, w, 1), p=[0.8, 0.2])
    elif kind == "subnormal":
        mean = mean * 1e-40
        sd = sd * 1e-20
    n = taken.astype(np.float64)
    s = np.zeros((h, w, 4), np.float32)
    with np.errstate(all="ignore"):
        s[..., :3] = (mean * n[..., None]).astype(np.float32)
        lum = 0.2126 * mean[..., 0] + 0.7152 * mean[..., 1] + 0.0722 * mean[..., 2]
        s[..., 3] = (n * (lum ** 2 + sd ** 2)).astype(np.float32)
    s[taken == 0] = np.array([np.nan, 7.0, -1.0, np.inf], np.float32)          # whatever a sum without a sample holds is not read
    return s


def guides(kind, rng, h, w, must_hit=()):
    n, a, z = dc.random_guides(rng, h, w, background={"holes": 0.25, "all-hits": 0.0, "all-background": 1.0}[kind], arrays=True)
    if kind == "all-background":
        z[:] = np.inf
    else:
        for y, x in must_hit:
            z[y, x] = f32(1.5)
    return dc._pack(n, a, z)


# (sums, guides, history_min, passes) of the grid's cases that matter most: the largest frames filter plausible sums over real hits
CHOSEN = {"mixed-37x29": ("plain", "holes", 4, 5), "hmin-37x29": ("plain", "all-hits", 4, 3), "stripe-37x29": ("plain", "all-hits", 2, 4),
          "young-edges-37x29": ("plain", "all-hits", 4, 5), "one-37x29": ("hdr", "holes", 2, 2), "mixed-17x5": ("hdr", "holes", 1, 5),
          "one-17x5": ("plain", "holes", 4, 3), "hmin-17x5": ("subnormal", "all-hits", 65536, 4)}


def _grid(name, w, h, k, kind):
    """Case k of the grid: sums, guides, history_min and passes in turn, or what CHOSEN says."""
    rng = np.random.default_rng(dc._seed(name))
    needs_hits = kind in ("island", "young-edges")
    sums_kind, guides_kind, hmin, passes = CHOSEN.get(name, (SUMS[k % 3], ("holes", "all-hits")[k % 2] if needs_hits else GUIDES[(k // 2) % 4],
                                                             HISTORY_MIN[k % 4], PASSES[k % 5]))
    t, must_hit = taken_map(kind, rng, h, w, hmin)
    params = {"iterations": passes}
    vparams = {"history_min": hmin}
    if k % 3 == 1:
        params.update(vc.OTHER_PARAMS)
        vparams.update({"sigma_luminance": 1.5, "variance_floor": 1e-4})
    g = guides(guides_kind, rng, h, w, must_hit)
    return sums(sums_kind, rng, t), t, g, params, vparams, ("set", "null")[k % 2], ("set", "null")[(k // 2) % 2]


def _synthetic(name, hmin):
    """sample_counts_ref.synthetic_frame: totals 0 to 2^20 and, on every third pixel, a hostile one -- inf and NaN in xyz and in w, w
    smaller than m1^2 n, subnormal sums.  history_min 65536 sends every one of them through the 5x5 block as a tap."""
    w, h = 37, 29
    rng = np.random.default_rng(dc._seed(name))
    s, t = sref.synthetic_frame(w, h, 7 + hmin % 11)
    return s.copy(), t.astype(np.uint32), guides("holes" if hmin != 2 else "all-hits", rng, h, w), {"iterations": 3}, {"history_min": hmin}, "set", "set"


def _negative(name):
    """w smaller than m1^2 n on every pixel: a negative difference, 0, as the own variance of the pixels with four samples; the three
    with one sample take the block's estimate over a constant frame."""
    w, h = 5, 3
    rng = np.random.default_rng(dc._seed(name))
    t = np.full((h, w), 4, np.uint32)
    t[1, 1:4] = 1
    s = np.zeros((h, w, 4), np.float32)
    s[..., :3] = f32(8.0) * t[..., None].astype(np.float32)
    s[..., 3] = f32(0.5)
    return s, t, guides("all-hits", rng, h, w), {"iterations": 2}, None, "set", "set"


def _hostile_depth(name):
    """Depths that are no hit (-0, negative, NaN, -inf) and extreme ones, under pixels with and without samples."""
    w, h = 37, 29
    rng = np.random.default_rng(dc._seed(name))
    n, a, z = dc.random_guides(rng, h, w, arrays=True)
    kind = rng.integers(0, 3 * len(dc.HOSTILE_DEPTHS), (h, w))
    for k, v in enumerate(dc.HOSTILE_DEPTHS):
        z[kind == k] = v
    t, _ = taken_map("mixed", rng, h, w, 4)
    return sums("plain", rng, t), t, dc._pack(n, a, z), {"iterations": 3, "sigma_depth": 0.5}, None, "null", "set"


def _build():
    cases = {}
    k = 0
    for w, h in SIZES:
        for kind in TAKEN_MAPS:
            name = f"{kind}-{w}x{h}"
            cases[name] = (_grid, (name, w, h, k, kind))
            k += 1
    for hmin in HISTORY_MIN:
        name = f"synthetic-hmin{hmin}"
        cases[name] = (_synthetic, (name, hmin))
    cases["negative"] = (_negative, ("negative",))
    cases["hostile-depth"] = (_hostile_depth, ("hostile-depth",))
    return cases


_CASES = _build()
CASES = list(_CASES)
# one context through frames that grow and shrink
GROW_SHRINK = ("mixed-5x3", "synthetic-hmin4", "island-1x1", "young-edges-17x5", "stripe-37x29", "zero-2x1", "mixed-37x29")


def case(name):
    fn, args = _CASES[name]
    return fn(*args)


def full_frame(w, h, seed, history_min=4):
    """An all-hit frame with every total >= history_min: (sum4, taken, guides)."""
    rng = np.random.default_rng(seed)
    t = rng.choice(np.array([history_min, history_min + 1, 8, 64, 1 << 20], np.uint32), (h, w)).astype(np.uint32)
    return sums("plain", rng, t), t, guides("all-hits", rng, h, w)
