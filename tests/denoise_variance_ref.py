"""Numpy specification of the denoiser's variance-guided mode (include/hrt.h "Variance-guided mode", csrc/denoise.hip
k_denoise_temporal<true>, k_denoise_variance, k_denoise_pass_var), operation for operation in float32.  The reprojection, the taps and
the blend are tests/denoise_temporal_ref.py's (its `diag` hands out the taps it took), the guides and the pass constants
tests/denoise_ref.py's; what is new here is the luminance moments that ride through the blend, the variance made of them, and the
filter pass whose colour stop follows that variance.

Every min, max and compare, with what it does to a NaN:
  np.fmax(0, x)        variance: fmaxf(0, x), a NaN x gives 0 (np.maximum would give NaN)
  np.fmax(1 / L, a)    the blend weight, as the kernel's fmaxf (L is never NaN: it comes from finite history lengths)
  L >= history_min     false for a NaN L: the spatial estimate
  np.fmax(n . n', 0)   the normal stop, tests/denoise_ref.py's
  sw > 0               false for a NaN weight sum: the pixel keeps its colour and its variance
  z > 0 and z < inf    a hit; false for a NaN depth"""
from __future__ import annotations

import numpy as np

import denoise_ref as ref
import denoise_temporal_ref as tref

f32 = np.float32
MISS = tref.MISS
DEFAULTS = {"sigma_luminance": 4.0, "history_min": 4, "variance_floor": 1e-6}
G3 = np.array([0.25, 0.5, 0.25], np.float32)


def luminance(c):
    """l(c) = (0.2126 c.x + 0.7152 c.y) + 0.0722 c.z of an sRGB-encoded colour (..., >= 3)."""
    return (f32(0.2126) * c[..., 0] + f32(0.7152) * c[..., 1]) + f32(0.0722) * c[..., 2]


def _params(vparams):
    p = dict(DEFAULTS)
    p.update(vparams or {})
    return p


# ---- 1. moments -----------------------------------------------------------------------------
def moments_step(hist, color, hits, cam, inv, xf, width, height, tparams=None):
    """tref.temporal_step plus the moments M = (m1, m2) of the luminance (k_denoise_temporal<true>).  hist: the dict this returns
    (tref's history with "moments" (H, W, 2)) or None.  Returns (A, L, motion, M, history)."""
    n_px = width * height
    diag = {}
    A, L, motion, hist2 = tref.temporal_step(hist, color, hits, cam, inv, xf, width, height, tparams, diag)
    c = np.ascontiguousarray(color, dtype=np.float32).reshape(n_px, 4)
    inst = np.asarray(hits[4], np.uint32).reshape(-1)
    hit = inst != MISS
    with np.errstate(all="ignore"):
        lc = luminance(c)
        M = np.stack([lc, lc * lc], axis=1).astype(np.float32)
        M[~hit] = 0                                                               # background: (0, 0)
        if hist is not None:
            tp = dict(tref.DEFAULTS)
            tp.update(tparams or {})
            alpha_min = f32(tp["alpha_min"])
            one = f32(1)
            sel, xp, yp, taken, sw = diag["sel"], diag["xp"], diag["yp"], diag["taken"], diag["sw"]
            x0, y0 = np.floor(xp), np.floor(yp)
            fx, fy = xp - x0, yp - y0
            gx, gy = one - fx, one - fy
            w = [gx * gy, fx * gy, gx * fy, fx * fy]                               # the colour's weights, recomputed by its formula
            Mp = np.asarray(hist["moments"], np.float32).reshape(n_px, 2)
            sm = np.zeros((sel.size, 2), np.float32)
            for k in range(4):
                take = taken[:, k]
                qx, qy = x0 + f32(k & 1), y0 + f32(k >> 1)
                q = np.where(take, np.where(take, qy, 0).astype(np.int64) * width + np.where(take, qx, 0).astype(np.int64), 0)
                sm = np.where(take[:, None], sm + w[k][:, None] * Mp[q], sm)       # in tap order
            blend = (diag["s"] > 0) & (sw > 0)
            Hm = sm / sw[:, None]
            alpha = np.fmax(one / L.reshape(-1)[sel], alpha_min)                   # fmaxf; the colour's alpha
            Mb = Hm + alpha[:, None] * (M[sel] - Hm)
            b = sel[blend]
            M[b] = Mb[blend]
    hist2["moments"] = M.reshape(height, width, 2)
    return A, L, motion, hist2["moments"], hist2


# ---- 2. variance ----------------------------------------------------------------------------
def variance(M, L, inst, history_min, diag=None, fmax=np.fmax):
    """k_denoise_variance: (H, W, 2) moments, (H, W) history length, (H, W) uint32 instance (MISS on background) -> (H, W) variance.
    diag receives "temporal" / "spatial" (which branch a pixel took), "n" (the spatial count) and "nan_to_zero" (fmax turned a NaN into 0).
    fmax: the max(0, x) of both branches; the reach check puts np.maximum there to see which bits the NaN -> 0 decides."""
    M = np.asarray(M, np.float32)
    H, W = L.shape
    inst = np.asarray(inst, np.uint32)
    hit = inst != MISS
    m1, m2 = M[..., 0], M[..., 1]
    zero = f32(0)
    with np.errstate(all="ignore"):
        raw_t = m2 - m1 * m1
        var_t = fmax(zero, raw_t)                                                 # NaN -> 0
        n = np.zeros((H, W), np.float32)
        s1, s2 = np.zeros_like(n), np.zeros_like(n)
        for dy in range(-2, 3):                                                   # row-major, dy outer
            for dx in range(-2, 3):
                y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
                if y0 >= y1 or x0 >= x1:
                    continue
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
                take = hit[Q] & (inst[Q] == inst[P])
                n[P] = np.where(take, n[P] + f32(1), n[P])
                s1[P] = np.where(take, s1[P] + m1[Q], s1[P])
                s2[P] = np.where(take, s2[P] + m2[Q], s2[P])
        mu = s1 / n
        raw_s = s2 / n - mu * mu
        var_s = fmax(zero, raw_s)                                                 # NaN -> 0
        temporal = hit & (L >= f32(history_min))                                  # (a NaN L: spatial)
        spatial = hit & ~temporal
        var = np.where(temporal, var_t, np.where(spatial, var_s, zero)).astype(np.float32)
    if diag is not None:
        diag.update(temporal=temporal, spatial=spatial, n=n,
                    nan_to_zero=(temporal & np.isnan(raw_t)) | (spatial & np.isnan(raw_s)))
    return var


# ---- 3. the filter --------------------------------------------------------------------------
def smoothed_variance(var, hit, diag=None):
    """gv = (sum g var_q) / (sum g) over the 3x3 block's taps inside the frame that are hits, g = G3 x G3, row-major."""
    H, W = var.shape
    sgv, sgw = np.zeros((H, W), np.float32), np.zeros((H, W), np.float32)
    with np.errstate(all="ignore"):
        for j in range(3):
            dy = j - 1
            for i in range(3):
                dx = i - 1
                y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
                if y0 >= y1 or x0 >= x1:
                    continue
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
                g = G3[i] * G3[j]
                take = hit[Q]
                sgw[P] = np.where(take, sgw[P] + g, sgw[P])
                sgv[P] = np.where(take, sgv[P] + g * var[Q], sgv[P])
        gv = sgv / sgw
    if diag is not None:
        diag["sgw"] = sgw
    return gv


def pass_var(src, var, n, a, z, step, k_luminance, variance_floor, k_albedo, sz_step, squarings, diag=None):
    """One pass (k_denoise_pass_var): src (H, W, 4), var (H, W) -> (out (H, W, 4), var_out (H, W))."""
    H, W = z.shape
    hit = (z > 0) & (z < np.inf)
    one = f32(1)
    with np.errstate(all="ignore"):
        inv_z = one / (sz_step * z)
        gv = smoothed_variance(var, hit, diag)
        inv_v = one / (k_luminance * gv + variance_floor)
        lum = luminance(src)
        sw = np.zeros((H, W), np.float32)
        sr, sg, sb, sv = np.zeros_like(sw), np.zeros_like(sw), np.zeros_like(sw), np.zeros_like(sw)
        for j in range(5):
            dy = (j - 2) * step
            for i in range(5):
                dx = (i - 2) * step
                y0, y1 = max(0, -dy), min(H, H - dy)
                x0, x1 = max(0, -dx), min(W, W - dx)
                if y0 >= y1 or x0 >= x1:
                    continue
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
                cq = src[Q]
                dl = lum[Q] - lum[P]
                wn = np.fmax(ref._dot(n[P], n[Q]), f32(0))
                for _ in range(squarings):
                    wn = wn * wn
                da = a[P] - a[Q]
                da2 = ref._dot(da, da)
                rz = (z[P] - z[Q]) * inv_z[P]
                w = ((ref.H_B3[i] * ref.H_B3[j]) * wn) / (((one + (dl * dl) * inv_v[P]) * (one + da2 * k_albedo)) * (one + rz * rz))
                take = hit[Q]
                sw[P] = np.where(take, sw[P] + w, sw[P])
                sr[P] = np.where(take, sr[P] + w * cq[..., 0], sr[P])
                sg[P] = np.where(take, sg[P] + w * cq[..., 1], sg[P])
                sb[P] = np.where(take, sb[P] + w * cq[..., 2], sb[P])
                sv[P] = np.where(take, sv[P] + (w * w) * var[Q], sv[P])
        keep = ~(hit & (sw > 0))                                                  # (a NaN sw: kept)
        out = np.stack([sr / sw, sg / sw, sb / sw, src[..., 3]], axis=-1).astype(np.float32)
        var_out = (sv / (sw * sw)).astype(np.float32)
    out[keep] = src[keep]
    var_out[keep] = var[keep]
    return out, var_out


def filter_variance(color, guides, var, params=None, vparams=None, diag=None):
    """hrt_denoise_filter_variance: -> (out (H, W, 4), var_out (H, W)).  diag: the first pass's terms."""
    n, a, z = ref.unpack_guides(guides)
    passes, squarings = ref.pass_constants(params)
    vp = _params(vparams)
    sl = f32(vp["sigma_luminance"])
    k_luminance, floor = f32(sl * sl), f32(vp["variance_floor"])
    out = np.ascontiguousarray(color, dtype=np.float32)
    v = np.ascontiguousarray(var, dtype=np.float32)
    for k, (step, _, ka, szs) in enumerate(passes):
        out, v = pass_var(out, v, n, a, z, step, k_luminance, floor, ka, szs, squarings, diag if k == 0 else None)
    return out, v


# ---- a whole call ---------------------------------------------------------------------------
def variance_frame(hist, color, oscene, scene, cam, width, height, params=None, tparams=None, vparams=None, diag=None):
    """One hrt_denoise_variance_launch over the oracle's primary hits of `scene`: returns (output, A, L, motion, M, var, history).
    A call without history has L = 1 on every hit pixel, so the spatial variance applies on all of them."""
    center, U, V, W = cam
    dirs = ref.primary_directions(width, height, U, V, W)
    origins = np.broadcast_to(np.asarray(center, np.float32), dirs.shape).copy()
    hits = oscene.trace(origins, dirs)
    xf = np.array([np.asarray(it["transform"], np.float32).reshape(12) for it in scene["instances"]], np.float32).reshape(-1, 12)
    A, L, motion, M, hist2 = moments_step(hist, color, hits, cam, tref.world_to_object(oscene), xf, width, height, tparams)
    var = variance(M, L, hist2["inst"], _params(vparams)["history_min"], diag)
    guides = ref.guides_from_hits(scene, center, dirs, *hits, width, height)
    out, _ = filter_variance(A, guides, var, params, vparams)
    return out, A, L, motion, M, var, hist2
