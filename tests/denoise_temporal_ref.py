"""Numpy specification of the denoiser's temporal mode (include/hrt.h "Temporal mode", csrc/denoise.hip k_denoise_temporal), operation
for operation in float32: the reprojection of every hit pixel into the previous frame, the history lookup and blend, and the history a
call leaves behind.  The guides and the filter are tests/denoise_ref.py's; the world -> object table is the one the oracle's INSTANCED
mode applies (oracle.c invert_affine, the library's inverse restated), read out of the oracle's scene."""
from __future__ import annotations

import ctypes as C

import numpy as np

import denoise_ref as ref

f32 = np.float32
MISS = np.uint32(0xFFFFFFFF)
DEFAULTS = {"alpha_min": 0.8, "max_history": 32, "depth_tolerance": 0.02}


class _OracleSceneHead(C.Structure):
    """The first fields of oracle.c's oracle_scene: the instance count and the per-instance inverse transforms."""
    _fields_ = [("n_inst", C.c_int), ("inst", C.c_void_p), ("inv", C.POINTER(C.c_float))]


def world_to_object(oscene):
    """(n, 12) float32: the inverse of every instance transform as the oracle's INSTANCED mode computes it (oracle_py.OracleScene)."""
    head = C.cast(oscene.handle, C.POINTER(_OracleSceneHead)).contents
    n = int(head.n_inst)
    if n == 0:
        return np.zeros((0, 12), np.float32)
    return np.ctypeslib.as_array(head.inv, shape=(n * 12,)).reshape(n, 12).astype(np.float32).copy()


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _xf_point(m, p):
    """(n, 12) row-major 3x4 maps applied to (n, 3) points: ((m0 x + m1 y) + m2 z) + m3 per row (bvh8_geom.h xf_point)."""
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((m[:, 4 * r] * x + m[:, 4 * r + 1] * y) + m[:, 4 * r + 2] * z) + m[:, 4 * r + 3] for r in range(3)], axis=1)


def temporal_step(hist, color, hits, cam, inv, xf, width, height, tparams=None, diag=None):
    """One call's reprojection and blend.
    hist: the previous call's history (the dict this returns) or None (no history).  color: (H, W, 4) float32 colour buffer.
    hits: (t, u, v, prim, inst) of the frame's primary rays (oracle_py.OracleScene.trace, row-major pixels).  cam: (center, U, V, W).
    inv / xf: (n, 12) world -> object tables of this frame and object -> world tables (the instance transforms) of this frame.
    diag: a dict that receives, for a call with history, the terms the outputs are decided by (tests/test_denoise_edges_cpu.py asserts
    that its cases reach them): "sel" the hit pixels' indices and per hit pixel "s", "inside" / "same_id" / "depth_ok" / "taken"
    ((n, 4) bool, per tap), "sw" and "unclamped" (sl / sw + 1 before the max_history clamp).
    Returns (A (H, W, 4), L (H, W), motion (H, W, 2), history)."""
    p = dict(DEFAULTS)
    p.update(tparams or {})
    alpha_min, max_history, tol = f32(p["alpha_min"]), f32(p["max_history"]), f32(p["depth_tolerance"])
    n_px = width * height
    center, U, V, W = (np.asarray(x, np.float32) for x in cam)
    t, _, _, prim, inst = hits
    t = np.asarray(t, np.float32).reshape(-1)
    prim = np.asarray(prim, np.uint32).reshape(-1)
    inst = np.asarray(inst, np.uint32).reshape(-1)
    c = np.ascontiguousarray(color, dtype=np.float32).reshape(n_px, 4)
    hit = inst != MISS
    acc = c.copy()
    length = np.where(hit, f32(1), f32(0)).astype(np.float32)
    motion = np.full((n_px, 2), np.nan, np.float32)
    one, half = f32(1), f32(0.5)
    if hist is not None:
        dirs = ref.primary_directions(width, height, U, V, W)
        sel = np.nonzero(hit)[0]
        ii = inst[sel].astype(np.int64)
        hp = center + dirs[sel] * t[sel][:, None]                                   # hit_point
        pw = _xf_point(np.asarray(hist["xf"], np.float32)[ii], _xf_point(np.asarray(inv, np.float32)[ii], hp))
        pc, pU, pV, pW = (np.asarray(x, np.float32) for x in hist["cam"])
        r = (pw - pc).astype(np.float32)
        with np.errstate(all="ignore"):
            s = _dot(r, pW) / _dot(pW, pW)
            proj = s > 0
            fw, fh = f32(width), f32(height)
            aspect = fw / fh
            ndcx = (_dot(r, pU) / _dot(pU, pU)) / (s * aspect)
            ndcy = (_dot(r, pV) / _dot(pV, pV)) / s
            xp = ((ndcx + one) * half) * fw - half
            yp = ((ndcy + one) * half) * fh - half
            zp = np.sqrt(_dot(r, r))
            x0, y0 = np.floor(xp), np.floor(yp)
            fx, fy = xp - x0, yp - y0
            gx, gy = one - fx, one - fy
            w = [gx * gy, fx * gy, gx * fy, fx * fy]
            sw = np.zeros(sel.size, np.float32)
            sa = np.zeros((sel.size, 3), np.float32)
            sl = np.zeros(sel.size, np.float32)
            h_acc = np.asarray(hist["accum"], np.float32).reshape(n_px, 4)
            h_len = np.asarray(hist["length"], np.float32).reshape(-1)
            h_z = np.asarray(hist["depth"], np.float32).reshape(-1)
            h_inst = np.asarray(hist["inst"], np.uint32).reshape(-1)
            h_prim = np.asarray(hist["prim"], np.uint32).reshape(-1)
            taps = []
            for k in range(4):
                qx, qy = x0 + f32(k & 1), y0 + f32(k >> 1)
                inside = proj & (qx >= 0) & (qx <= fw - one) & (qy >= 0) & (qy <= fh - one)
                q = np.where(inside, np.where(inside, qy, 0).astype(np.int64) * width + np.where(inside, qx, 0).astype(np.int64), 0)
                same_id = (h_inst[q] == inst[sel]) & (h_prim[q] == prim[sel])
                depth_ok = np.abs(h_z[q] - zp) <= tol * zp
                take = inside & same_id & depth_ok
                taps.append((inside, same_id, depth_ok, take))
                sw = np.where(take, sw + w[k], sw)
                sa = np.where(take[:, None], sa + w[k][:, None] * h_acc[q, :3], sa)
                sl = np.where(take, sl + w[k] * h_len[q], sl)
            blend = proj & (sw > 0)
            H = sa / sw[:, None]
            L = np.minimum(sl / sw + one, max_history)
            alpha = np.maximum(one / L, alpha_min)
            A = H + alpha[:, None] * (c[sel, :3] - H)
            if diag is not None:
                diag.update(sel=sel, s=s, sw=sw, unclamped=sl / sw + one, xp=xp, yp=yp,
                            **{name: np.stack([t[i] for t in taps], axis=1) for i, name in enumerate(("inside", "same_id", "depth_ok", "taken"))})
        b = sel[blend]
        acc[b, :3] = A[blend]
        length[b] = L[blend]
        m = sel[proj]
        motion[m, 0], motion[m, 1] = xp[proj], yp[proj]
    history = {"accum": acc.reshape(height, width, 4), "length": length.reshape(height, width),
               "depth": np.where(hit, t, f32(np.inf)).astype(np.float32).reshape(height, width),
               "inst": np.where(hit, inst, MISS).astype(np.uint32).reshape(height, width),
               "prim": np.where(hit, prim, 0).astype(np.uint32).reshape(height, width),
               "xf": np.asarray(xf, np.float32).reshape(-1, 12).copy(), "cam": tuple(np.asarray(x, np.float32).copy() for x in cam)}
    return history["accum"], history["length"], motion.reshape(height, width, 2), history


def temporal_frame(hist, color, oscene, scene, cam, width, height, params=None, tparams=None, diag=None):
    """One whole hrt_denoise_temporal_launch over the oracle's primary hits of `scene` (whose instance transforms are this frame's):
    returns (output, A, L, motion, history)."""
    center, U, V, W = cam
    dirs = ref.primary_directions(width, height, U, V, W)
    origins = np.broadcast_to(np.asarray(center, np.float32), dirs.shape).copy()
    hits = oscene.trace(origins, dirs)
    xf = np.array([np.asarray(it["transform"], np.float32).reshape(12) for it in scene["instances"]], np.float32).reshape(-1, 12)
    A, L, motion, hist2 = temporal_step(hist, color, hits, cam, world_to_object(oscene), xf, width, height, tparams, diag)
    guides = ref.guides_from_hits(scene, center, dirs, *hits, width, height)
    return ref.atrous(A, guides, params), A, L, motion, hist2
