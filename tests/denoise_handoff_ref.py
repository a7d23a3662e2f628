"""Numpy specification of the denoiser's history hand-over (include/hrt.h hrt_denoise_temporal_rebind, csrc/denoise_link.hip
k_denoise_temporal_linked), operation for operation in float32: the first temporal or variance-guided call on a TLAS whose history was
made for another TLAS of the same scene.  It is tests/denoise_temporal_ref.py's temporal_step and tests/denoise_variance_ref.py's
moments_step with the previous object -> world table indexed through the link, the previous ids compared through the link, and the
HRT_NO_INSTANCE rule; every other call of a sequence is those modules' own.  The history this leaves is theirs, labelled with this
TLAS's instance indices, so the next call is an ordinary one.

A hit pixel of instance i with primitive prim, pi = link[i]:
  pi == NO_INSTANCE   no history: A = C, L = 1, M = mc, motion (NaN, NaN)
  otherwise           P' = X_prev(pi) (X_inv(i) P); a tap counts if it is inside the frame, holds id (pi, prim) and passes the depth
                      test; blend, length and moments as in the unlinked step
The id kept for the next call is (i, prim)."""
from __future__ import annotations

import numpy as np

import denoise_ref as ref
import denoise_temporal_ref as tref
import denoise_variance_ref as vref

f32 = np.float32
MISS = tref.MISS
NO_INSTANCE = np.uint32(0xFFFFFFFF)


def make_link(prev_blas, next_blas, prev_instance=None):
    """The link hrt_denoise_temporal_rebind keeps: prev_instance (None: the identity over the instances both TLASes have, every
    further one new) with the entries whose BLAS differs from their predecessor's turned into NO_INSTANCE.  prev_blas / next_blas: one
    hashable BLAS identity per instance of the history's TLAS and of the next one."""
    n_prev, n_next = len(prev_blas), len(next_blas)
    if prev_instance is None:
        prev_instance = [i if i < n_prev else int(NO_INSTANCE) for i in range(n_next)]
    assert len(prev_instance) == n_next
    link = np.empty(n_next, np.uint32)
    for i, pi in enumerate(prev_instance):
        pi = int(pi)
        assert pi == int(NO_INSTANCE) or 0 <= pi < n_prev, (i, pi)                # (HRT_ERR_INVALID in the library)
        link[i] = pi if pi != int(NO_INSTANCE) and prev_blas[pi] == next_blas[i] else NO_INSTANCE
    return link


def handoff_step(hist, link, color, hits, cam, inv, xf, width, height, tparams=None, moments=False):
    """One linked call's reprojection and blend.  hist: the previous call's history (tref.temporal_step's dict, with "moments" if
    `moments`), made on the previous TLAS; link: (n_next,) uint32 (make_link).  The other arguments are temporal_step's, of this
    frame's TLAS.  Returns (A, L, motion, M or None, history)."""
    p = dict(tref.DEFAULTS)
    p.update(tparams or {})
    alpha_min, max_history, tol = f32(p["alpha_min"]), f32(p["max_history"]), f32(p["depth_tolerance"])
    n_px = width * height
    center, U, V, W = (np.asarray(x, np.float32) for x in cam)
    t, _, _, prim, inst = hits
    t = np.asarray(t, np.float32).reshape(-1)
    prim = np.asarray(prim, np.uint32).reshape(-1)
    inst = np.asarray(inst, np.uint32).reshape(-1)
    link = np.asarray(link, np.uint32).reshape(-1)
    c = np.ascontiguousarray(color, dtype=np.float32).reshape(n_px, 4)
    hit = inst != MISS
    acc = c.copy()
    length = np.where(hit, f32(1), f32(0)).astype(np.float32)
    motion = np.full((n_px, 2), np.nan, np.float32)
    one, half = f32(1), f32(0.5)
    with np.errstate(all="ignore"):
        lc = vref.luminance(c)
        M = np.stack([lc, lc * lc], axis=1).astype(np.float32)
        M[~hit] = 0
    # the hit pixels whose instance has a predecessor: the only ones that look into the history
    carried = hit.copy()
    carried[hit] = link[inst[hit].astype(np.int64)] != NO_INSTANCE
    sel = np.nonzero(carried)[0]
    ii = inst[sel].astype(np.int64)
    pi = link[ii]                                                                  # the instance's index in the history
    dirs = ref.primary_directions(width, height, U, V, W)
    hp = center + dirs[sel] * t[sel][:, None]                                      # hit_point
    pw = tref._xf_point(np.asarray(hist["xf"], np.float32)[pi.astype(np.int64)], tref._xf_point(np.asarray(inv, np.float32)[ii], hp))
    pc, pU, pV, pW = (np.asarray(x, np.float32) for x in hist["cam"])
    r = (pw - pc).astype(np.float32)
    with np.errstate(all="ignore"):
        s = tref._dot(r, pW) / tref._dot(pW, pW)
        proj = s > 0
        fw, fh = f32(width), f32(height)
        aspect = fw / fh
        ndcx = (tref._dot(r, pU) / tref._dot(pU, pU)) / (s * aspect)
        ndcy = (tref._dot(r, pV) / tref._dot(pV, pV)) / s
        xp = ((ndcx + one) * half) * fw - half
        yp = ((ndcy + one) * half) * fh - half
        zp = np.sqrt(tref._dot(r, r))
        x0, y0 = np.floor(xp), np.floor(yp)
        fx, fy = xp - x0, yp - y0
        gx, gy = one - fx, one - fy
        w = [gx * gy, fx * gy, gx * fy, fx * fy]
        sw = np.zeros(sel.size, np.float32)
        sa = np.zeros((sel.size, 3), np.float32)
        sl = np.zeros(sel.size, np.float32)
        sm = np.zeros((sel.size, 2), np.float32)
        h_acc = np.asarray(hist["accum"], np.float32).reshape(n_px, 4)
        h_len = np.asarray(hist["length"], np.float32).reshape(-1)
        h_z = np.asarray(hist["depth"], np.float32).reshape(-1)
        h_inst = np.asarray(hist["inst"], np.uint32).reshape(-1)
        h_prim = np.asarray(hist["prim"], np.uint32).reshape(-1)
        h_mom = np.asarray(hist["moments"], np.float32).reshape(n_px, 2) if moments else None
        for k in range(4):
            qx, qy = x0 + f32(k & 1), y0 + f32(k >> 1)
            inside = proj & (qx >= 0) & (qx <= fw - one) & (qy >= 0) & (qy <= fh - one)
            q = np.where(inside, np.where(inside, qy, 0).astype(np.int64) * width + np.where(inside, qx, 0).astype(np.int64), 0)
            same_id = (h_inst[q] == pi) & (h_prim[q] == prim[sel])               # the history's ids are the previous TLAS's
            depth_ok = np.abs(h_z[q] - zp) <= tol * zp
            take = inside & same_id & depth_ok
            sw = np.where(take, sw + w[k], sw)
            sa = np.where(take[:, None], sa + w[k][:, None] * h_acc[q, :3], sa)
            sl = np.where(take, sl + w[k] * h_len[q], sl)
            if moments:
                sm = np.where(take[:, None], sm + w[k][:, None] * h_mom[q], sm)
        blend = proj & (sw > 0)
        H = sa / sw[:, None]
        L = np.minimum(sl / sw + one, max_history)
        alpha = np.fmax(one / L, alpha_min)
        A = H + alpha[:, None] * (c[sel, :3] - H)
        Hm = sm / sw[:, None]
        Mb = Hm + alpha[:, None] * (M[sel] - Hm)
    b = sel[blend]
    acc[b, :3] = A[blend]
    length[b] = L[blend]
    if moments:
        M[b] = Mb[blend]
    m = sel[proj]
    motion[m, 0], motion[m, 1] = xp[proj], yp[proj]
    history = {"accum": acc.reshape(height, width, 4), "length": length.reshape(height, width),
               "depth": np.where(hit, t, f32(np.inf)).astype(np.float32).reshape(height, width),
               "inst": np.where(hit, inst, MISS).astype(np.uint32).reshape(height, width),
               "prim": np.where(hit, prim, 0).astype(np.uint32).reshape(height, width),
               "xf": np.asarray(xf, np.float32).reshape(-1, 12).copy(), "cam": tuple(np.asarray(x, np.float32).copy() for x in cam)}
    Mout = None
    if moments:
        history["moments"] = Mout = M.reshape(height, width, 2)
    return history["accum"], history["length"], motion.reshape(height, width, 2), Mout, history


def _frame_inputs(oscene, scene, cam, width, height):
    center, U, V, W = cam
    dirs = ref.primary_directions(width, height, U, V, W)
    origins = np.broadcast_to(np.asarray(center, np.float32), dirs.shape).copy()
    hits = oscene.trace(origins, dirs)
    xf = np.array([np.asarray(it["transform"], np.float32).reshape(12) for it in scene["instances"]], np.float32).reshape(-1, 12)
    guides = ref.guides_from_hits(scene, center, dirs, *hits, width, height)
    return hits, xf, guides


def handoff_temporal_frame(hist, link, color, oscene, scene, cam, width, height, params=None, tparams=None):
    """The hrt_denoise_temporal_launch that takes the link, over the oracle's primary hits of `scene` (the next TLAS's instances):
    returns tref.temporal_frame's (output, A, L, motion, history)."""
    hits, xf, guides = _frame_inputs(oscene, scene, cam, width, height)
    A, L, motion, _, hist2 = handoff_step(hist, link, color, hits, cam, tref.world_to_object(oscene), xf, width, height, tparams)
    return ref.atrous(A, guides, params), A, L, motion, hist2


def handoff_variance_frame(hist, link, color, oscene, scene, cam, width, height, params=None, tparams=None, vparams=None):
    """... and the hrt_denoise_variance_launch: returns vref.variance_frame's (output, A, L, motion, M, var, history)."""
    hits, xf, guides = _frame_inputs(oscene, scene, cam, width, height)
    A, L, motion, M, hist2 = handoff_step(hist, link, color, hits, cam, tref.world_to_object(oscene), xf, width, height, tparams, moments=True)
    var = vref.variance(M, L, hist2["inst"], vref._params(vparams)["history_min"])
    out, _ = vref.filter_variance(A, guides, var, params, vparams)
    return out, A, L, motion, M, var, hist2


def blas_ids(scene, order=None):
    """One BLAS identity per instance of the TLAS Renderer.build_tlas(order) makes of the loaded `scene` (None: load_scene's own), as
    load_scene shares BLASes: triangle instances with the same "shape" share one, every other instance has its own."""
    ids = [("shape", it["shape"]) if it.get("shape") is not None and it["geometry"] == "triangles" else ("own", k)
           for k, it in enumerate(scene["instances"])]
    return ids if order is None else [ids[k] for k in order]


def sub_scene(scene, order=None, transforms=None):
    """The scene Renderer.build_tlas(order, transforms) traces: instance j is `scene`'s instance order[j] with transforms[j]."""
    order = range(len(scene["instances"])) if order is None else order
    out = {k: v for k, v in scene.items() if k != "instances"}
    out["instances"] = []
    for j, k in enumerate(order):
        it = dict(scene["instances"][k])
        if transforms is not None:
            it["transform"] = np.asarray(transforms[j], np.float32).reshape(12).copy()
        out["instances"].append(it)
    return out
