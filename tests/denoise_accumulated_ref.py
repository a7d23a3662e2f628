"""Numpy specification of the denoiser's accumulated mode (include/hrt.h "Accumulated mode"; csrc/denoise_accum.hip
k_denoise_accumulated, then the variance-guided passes and colorToFloat4), operation for operation in float32, nothing contracted.

The inputs are what hrt_render_accumulate leaves with its caller -- sum (H, W, 4): the summed radiance and, in w, the summed squared
luminances; taken (H, W) uint32: the samples they hold -- and the frame's guides.  With n = taken[p] and
l(c) = (0.2126 c.x + 0.7152 c.y) + 0.0722 c.z (sample_counts_ref.luminance):

  mean     n == 0: (0, 0, 0);  n == 1: sum.xyz;  else sum.xyz / (float)n  (sample_counts_ref.mean, k_finalize_counts' arithmetic); alpha 1
  guides'  guides[p], the depth +inf where n == 0: a pixel without a sample is background to the filter -- never a tap, never
           filtered, black in the result.  A hit below is 0 < depth' < +inf
  var      the variance of the mean's luminance.  Background: 0.  A hit with n >= max(history_min, 2): fmaxf(0, m2 - m1 m1) / (float)n with
           m1 = l(sum.xyz) / n, m2 = sum.w / n: sample_counts_ref.variance over n.  Every other hit (a young pixel): over the 5x5 block
           around it, row-major, the taps inside the frame that are hits (the centre among them): k their count, s1 = sum l(mean_q),
           s2 = sum l(mean_q) l(mean_q), mu = s1 / k, var = fmaxf(0, s2 / k - mu mu); taps left out do not touch the sums (np.where)
  filter   denoise_variance_ref.filter_variance(mean, guides', var, params, vparams): on LINEAR radiance, unlike the other modes
  output   colorToFloat4 of the filtered frame (the oracle's, which the colour tests pin k_color_to_float4 to), alpha 1

Every min, max and compare, with what it does to a NaN:
  np.fmax(0, x)        both variances: fmaxf, a NaN x gives 0, -inf gives 0, +inf stays
  n >= max(hmin, 2)    integers
  z > 0 and z < inf    a hit; false for a NaN depth
  everything else      denoise_variance_ref's and the oracle's"""
from __future__ import annotations

import numpy as np

import denoise_ref as ref
import denoise_variance_ref as vref
import sample_counts_ref as sref

f32 = np.float32
DEFAULTS = vref.DEFAULTS


def _history_min(vparams):
    p = dict(DEFAULTS)
    p.update(vparams or {})
    return int(p["history_min"])


def prepare(sum4, taken, guides, vparams=None, diag=None):
    """k_denoise_accumulated: sum4 (H, W, 4) float32, taken (H, W) uint32, guides (H, W, 8) uint16 -> (mean (H, W, 4), var (H, W),
    guides' (H, W, 8) uint16).  diag receives the masks "unsampled", "one", "many" (the mean's three cases), "background" (of guides'),
    "turned" (a hit of the guides without a sample), "own", "spatial" (which variance a hit took), the spatial count "k", "clipped" (a
    spatial pixel whose block leaves the frame), and "nan_to_zero" / "negative_to_zero" (what fmax decided)."""
    sum4 = np.ascontiguousarray(sum4, dtype=np.float32)
    taken = np.ascontiguousarray(taken).view(np.uint32) if np.asarray(taken).dtype == np.int32 else np.asarray(taken, np.uint32)
    H, W = taken.shape
    believed = max(_history_min(vparams), 2)
    zero = f32(0)
    mean = np.zeros((H, W, 4), np.float32)
    mean[..., :3] = sref.mean(sum4, taken)
    mean[taken == 0, :3] = 0
    mean[..., 3] = 1
    g2 = np.ascontiguousarray(guides).view(np.uint16).copy()
    n_, a_, z = ref.unpack_guides(g2)
    z2 = np.where(taken == 0, f32(np.inf), z).astype(np.float32)
    g2[..., 6:8] = np.ascontiguousarray(z2).reshape(H, W, 1).view(np.uint16)
    hit = (z2 > 0) & (z2 < np.inf)
    with np.errstate(all="ignore"):
        n = taken.astype(np.float32)
        m1 = (sref.luminance(sum4) / n).astype(np.float32)
        m2 = (sum4[..., 3] / n).astype(np.float32)
        raw_o = (m2 - (m1 * m1).astype(np.float32)).astype(np.float32)
        var_o = (np.fmax(zero, raw_o) / n).astype(np.float32)                     # NaN -> 0
        lum = sref.luminance(mean)
        k = np.zeros((H, W), np.float32)
        s1, s2 = np.zeros_like(k), np.zeros_like(k)
        for dy in range(-2, 3):                                                   # row-major, dy outer
            for dx in range(-2, 3):
                y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
                if y0 >= y1 or x0 >= x1:
                    continue
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
                take = hit[Q]
                k[P] = np.where(take, k[P] + f32(1), k[P])
                s1[P] = np.where(take, s1[P] + lum[Q], s1[P])
                s2[P] = np.where(take, s2[P] + lum[Q] * lum[Q], s2[P])
        mu = s1 / k
        raw_s = (s2 / k - mu * mu).astype(np.float32)
        var_s = np.fmax(zero, raw_s)                                              # NaN -> 0
    own = hit & (taken >= believed)
    spatial = hit & ~own
    var = np.where(own, var_o, np.where(spatial, var_s, zero)).astype(np.float32)
    if diag is not None:
        ys, xs = np.mgrid[0:H, 0:W]
        raw = np.where(own, raw_o, raw_s)
        diag.update(unsampled=taken == 0, one=taken == 1, many=taken > 1, background=~hit,
                    turned=(z > 0) & (z < np.inf) & (taken == 0), own=own, spatial=spatial, k=k,
                    clipped=spatial & ((ys < 2) | (ys >= H - 2) | (xs < 2) | (xs >= W - 2)),
                    nan_to_zero=hit & np.isnan(raw), negative_to_zero=hit & (raw < 0))
    return mean, var, g2


def encode(linear):
    """colorToFloat4 over an (H, W, 4) frame: the oracle's conversion (alpha 1)."""
    import oracle_py
    src = np.ascontiguousarray(linear, dtype=np.float32)
    out = np.empty_like(src)
    oracle_py.lib().oracle_color_to_float4_n(src.ctypes.data, out.ctypes.data, src.shape[0] * src.shape[1])
    return out


def denoise_accumulated(sum4, taken, guides, params=None, vparams=None, diag=None):
    """hrt_denoise_accumulated_filter: -> (out (H, W, 4) encoded, linear (H, W, 4) filtered, var_out (H, W) filtered)."""
    mean, var, g2 = prepare(sum4, taken, guides, vparams, diag)
    linear, var_out = vref.filter_variance(mean, g2, var, params, vparams)
    return encode(linear), linear, var_out
