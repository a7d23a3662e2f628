"""Adaptive sampling restated in numpy, operation for operation (include/hrt.h: hrt_render_accumulate, hrt_sample_counts; csrc/path_lane.h
kCounts, csrc/kernels.hip k_finalize_counts / k_sample_counts).  Everything is float32; no product and sum is contracted into an fma.

The accumulation runs over the CPU oracle's successive spp = 1 renders: a pixel's samples are independent of every other pixel's and are
taken in order on its own RNG stream, so sample k of a pixel is what the k-th spp = 1 render of the frame gives it -- provided the pixel's
state advanced only when the pixel took the sample, which `accumulate` sees to.

NaN and special-value behaviour of every min / max / compare below:
  luminance(r)               plain products and sums; inf - inf and 0 * inf are NaN and stay NaN
  taken < 2                  integers
  fmaxf(0, m2 - m1 * m1)     np.fmax: a NaN operand is dropped, so a NaN difference gives 0; -inf gives 0; +inf stays
  fmaxf over the window      np.fmax of values that are >= 0 or +inf, never NaN: the order of the window does not matter
  V / (sigma * sigma)        IEEE: a sigma whose square underflows to 0 gives +inf (V > 0) or NaN (V == 0); one whose square overflows gives 0 or NaN
                             (V == +inf)
  x >= (float)max_total      false for NaN
  (uint32_t)ceilf(x)         taken only where 0 < x < max_total; a NaN x and x <= 0 (that is +-0) give 0
  max(total, min_total), total > taken, min(counts, spp)    integers
"""
import numpy as np

F = np.float32
KR, KG, KB = F(0.2126), F(0.7152), F(0.0722)
DEFAULTS = dict(target_sigma=0.05, min_total=1, max_total=64, radius=1)


def luminance(rgb):
    """l = (0.2126 r.x + 0.7152 r.y) + 0.0722 r.z of (..., 3+) float32 values"""
    rgb = np.asarray(rgb, F)
    with np.errstate(all="ignore"):
        return ((KR * rgb[..., 0] + KG * rgb[..., 1]) + KB * rgb[..., 2]).astype(F)


def effective_counts(n_pixels, spp, counts=None):
    """c = counts ? min(counts[p], spp) : spp, as (n_pixels,) uint32"""
    if counts is None:
        return np.full(n_pixels, spp, np.uint32)
    return np.minimum(np.asarray(counts, np.uint32).reshape(-1), np.uint32(spp))


def accumulate(osc, width, height, states, spp, sum4, taken, counts=None, rows=None):
    """hrt_render_accumulate over the oracle scene `osc`: every pixel of the tile (`rows`: frame rows, None = all) takes its c samples.
    states (H*W, 12) uint32, sum4 (H*W, 4) float32 and taken (H*W,) uint32 are updated in place; returns the effective counts (0 outside the tile)."""
    n = width * height
    c = effective_counts(n, spp, counts)
    if rows is not None:
        inside = np.zeros((height, width), bool)
        inside[np.asarray(rows, np.int64)] = True
        c = np.where(inside.reshape(-1), c, np.uint32(0)).astype(np.uint32)
    for k in range(int(c.max()) if n else 0):
        trial = states.copy()
        lin = osc.render(width, height, trial, 1)["linear"].reshape(n, 4)[:, :3].astype(F)
        l = luminance(lin)
        with np.errstate(all="ignore"):
            l2 = (l * l).astype(F)
        live = k < c
        first = live & (taken == 0)               # the first sample of a frame is assigned, not added: whatever the sum held is gone
        add = live & ~first
        sum4[first, :3] = lin[first]; sum4[first, 3] = l2[first]
        with np.errstate(all="ignore"):
            sum4[add, :3] = (sum4[add, :3] + lin[add]).astype(F); sum4[add, 3] = (sum4[add, 3] + l2[add]).astype(F)
        taken[live] += np.uint32(1)
        states[live] = trial[live]                # only a pixel that took the sample has drawn its random numbers
    return c


def mean(sum4, taken):
    """sum.xyz / (float)taken, k_finalize's arithmetic (no division for one sample); rows with taken == 0 are returned as they are"""
    out = np.array(sum4[..., :3], F)
    many = taken > 1
    with np.errstate(all="ignore"):
        out[many] = (out[many] / taken[many].astype(F)[..., None]).astype(F)
    return out


def variance(sum4, taken):
    """per pixel v: +inf below two samples, else fmaxf(0, m2 - m1 * m1)"""
    sum4 = np.asarray(sum4, F); taken = np.asarray(taken, np.uint32)
    with np.errstate(all="ignore"):
        n = taken.astype(F)
        m1 = (luminance(sum4) / n).astype(F)
        m2 = (sum4[..., 3] / n).astype(F)
        v = np.fmax(F(0.0), (m2 - (m1 * m1).astype(F)).astype(F)).astype(F)
    return np.where(taken < 2, F(np.inf), v).astype(F)


def sample_counts(sum4, taken, target_sigma=0.05, min_total=1, max_total=64, radius=1):
    """hrt_sample_counts: sum4 (H, W, 4) float32, taken (H, W) uint32 -> counts (H, W) uint32"""
    sum4 = np.asarray(sum4, F); taken = np.asarray(taken, np.uint32)
    h, w = taken.shape
    v = variance(sum4, taken)
    big = np.zeros((h, w), F)
    for dy in range(-radius, radius + 1):           # row-major over the window; pixels outside the frame are left out
        for dx in range(-radius, radius + 1):
            ys, xs = slice(max(0, -dy), min(h, h - dy)), slice(max(0, -dx), min(w, w - dx))
            yq, xq = slice(max(0, dy), min(h, h + dy)), slice(max(0, dx), min(w, w + dx))
            big[ys, xs] = np.fmax(big[ys, xs], v[yq, xq])
    s = F(target_sigma)
    with np.errstate(all="ignore"):
        x = (big / (s * s).astype(F)).astype(F)
        capped = x >= F(max_total)
        inner = (x > F(0.0)) & ~capped
        total = np.where(capped, np.uint32(max_total), np.uint32(0)).astype(np.uint32)
        total[inner] = np.ceil(x[inner]).astype(np.uint32)
    total = np.maximum(total, np.uint32(min_total))
    return np.where(total > taken, total - taken, np.uint32(0)).astype(np.uint32)


# ---- synthetic inputs of the allocator, shared by the CPU and the GPU tests ----
N_KINDS = 11
SIZES = [(1, 1), (5, 3), (37, 29), (64, 48)]
# (non-default sigma and limits; 0.5 and 8 put `at the cap` within reach: v = 2 gives x = 2 / 0.25 = 8 exactly)
PARAM_SETS = [dict(DEFAULTS), dict(target_sigma=0.5, min_total=1, max_total=8, radius=0), dict(target_sigma=0.02, min_total=4, max_total=65536, radius=1)]


def _hostile(kind):
    """(sum4, taken) of one hostile pixel"""
    inf, nan = F(np.inf), F(np.nan)
    return {0: ((nan, 7.0, -1.0, nan), 0),                      # nothing taken: whatever the sum holds is not read as a variance
            1: ((0.5, 0.5, 0.5, 0.25), 1),                      # one sample: nothing known yet
            2: ((inf, 1.0, 1.0, 5.0), 2),                       # m1 = inf, m2 finite: -inf, 0
            3: ((inf, 1.0, 1.0, inf), 2),                       # inf - inf: NaN, 0
            4: ((nan, nan, nan, nan), 3),                       # NaN all the way, 0
            5: ((1e-40, 1e-40, 1e-40, 1e-42), 2),               # subnormal sums
            6: ((8.0, 8.0, 8.0, 0.0), 2),                       # w smaller than m1 * m1: negative, 0
            7: ((0.0, 0.0, 0.0, 4.0), 2),                       # v = 2
            8: ((0.0, 0.0, 0.0, 400.0), 2),                     # v = 200
            9: ((2.0 ** 20, 2.0 ** 20, 2.0 ** 20, 2.0 ** 20 + 64.0), 1 << 20),      # 2^20 samples of luminance 1 and a little variance: total <= taken
            10: ((1.0, -inf, 1.0, 3.0), 2)}[kind]


def synthetic_frame(width, height, seed):
    """sum4 (H, W, 4) float32, taken (H, W) uint32: plausible pixels (samples of mean luminance 0..2, standard deviation 0..3, 0 to 2^20 of
    them) with a hostile pixel of kind (position + seed) % N_KINDS wherever position % 3 == 0"""
    n = width * height
    rng = np.random.default_rng(seed)
    taken = rng.choice(np.array([0, 1, 2, 2, 3, 8, 64, 1 << 20], np.uint32), n)
    mean = rng.uniform(0.0, 2.0, (n, 3))
    sd = rng.choice(np.array([0.0, 0.01, 0.1, 0.5, 3.0]), n)
    sum4 = np.zeros((n, 4), F)
    sum4[:, :3] = (mean * taken[:, None]).astype(F)
    sum4[:, 3] = (taken * (luminance(mean.astype(F)).astype(np.float64) ** 2 + sd ** 2)).astype(F)
    for p in range(0, n, 3):
        s, t = _hostile((p + seed) % N_KINDS)
        sum4[p] = np.array(s, F); taken[p] = t
    return sum4.reshape(height, width, 4), taken.reshape(height, width)


def branches(sum4, taken, target_sigma=0.05, min_total=1, max_total=64, radius=1):
    """which branches of the definition the frame reaches, for the tests to insist on"""
    taken = np.asarray(taken, np.uint32)
    with np.errstate(all="ignore"):
        n = taken.astype(F)
        m1 = (luminance(sum4) / n).astype(F); m2 = (np.asarray(sum4, F)[..., 3] / n).astype(F)
        raw = (m2 - (m1 * m1).astype(F)).astype(F)
        x = (variance(sum4, taken) / (F(target_sigma) * F(target_sigma))).astype(F) if radius == 0 else None
    counts = sample_counts(sum4, taken, target_sigma, min_total, max_total, radius)
    out = {"taken 0": bool((taken == 0).any()), "taken 1": bool((taken == 1).any()), "NaN -> 0": bool((np.isnan(raw) & (taken >= 2)).any()),
           "negative -> 0": bool(((raw < 0) & (taken >= 2)).any()), "total <= taken": bool(((counts == 0) & (taken >= 2)).any())}
    if x is not None:
        out["at the cap"] = bool((x == F(max_total)).any()); out["above the cap"] = bool((x > F(max_total)).any())
    return out
