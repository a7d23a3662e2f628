"""Numpy specification of the denoiser's history hand-over across rebuilt BLASes (include/hrt.h hrt_denoise_temporal_rebind_geometry,
csrc/denoise_link_prim.hip k_denoise_temporal_by_prim), operation for operation in float32.  It is tests/denoise_handoff_ref.py's
handoff_step with one more input per instance: the object-space vertices of the BLAS the instance's predecessor had, where the
instance is linked by primitive.  Every other call of a sequence is denoise_temporal_ref's / denoise_variance_ref's own.

A hit pixel of instance i with primitive k, hit (t, u, v), pi = link[i], s = the predecessor's vertices if by_prim[i] else None:
  pi == NO_INSTANCE   no history: A = C, L = 1, M = mc, motion (NaN, NaN)
  s is None           Po = X_inv(i) (o + d t)                                       (the rigid path: denoise_handoff_ref)
  otherwise           a, b, c = s[k];  w = (1 - u) - v;  Po = (a w + b u) + c v     (hit_normal's order: u weighs the second vertex)
then P' = X_prev(pi) Po, and the projection, the four taps, the (pi, k) id test, the depth test, the blend and the moments of the
unlinked step.  The id kept for the next call is (i, k)."""
from __future__ import annotations

import numpy as np

import denoise_handoff_ref as href
import denoise_ref as ref
import denoise_temporal_ref as tref
import denoise_variance_ref as vref

f32 = np.float32
MISS = tref.MISS
NO_INSTANCE = href.NO_INSTANCE
TRIANGLES, SPHERES = "triangles", "spheres"


def make_link(prev, next, prev_instance=None):
    """What hrt_denoise_temporal_rebind_geometry keeps.  prev / next: per instance of the history's TLAS and of the next one a tuple
    (BLAS identity, kind, primitive count).  Returns (link, by_prim): link as denoise_handoff_ref.make_link's, except that an entry
    whose BLAS differs from its predecessor's stays where both are triangle BLASes of the same, non-zero count -- by_prim marks those."""
    n_prev, n_next = len(prev), len(next)
    if prev_instance is None:
        prev_instance = [i if i < n_prev else int(NO_INSTANCE) for i in range(n_next)]
    assert len(prev_instance) == n_next
    link = np.empty(n_next, np.uint32)
    by_prim = np.zeros(n_next, bool)
    for i, pi in enumerate(prev_instance):
        pi = int(pi)
        assert pi == int(NO_INSTANCE) or 0 <= pi < n_prev, (i, pi)
        if pi != int(NO_INSTANCE) and prev[pi][0] != next[i][0]:
            (_, kp, cp), (_, kn, cn) = prev[pi], next[i]
            if kp == TRIANGLES and kn == TRIANGLES and cp == cn and cn != 0:
                by_prim[i] = True
            else:
                pi = int(NO_INSTANCE)
        link[i] = pi
    return link, by_prim


def object_points(link, by_prim, prev_verts, hits, sel, hp, inv):
    """Po of the pixels `sel` (all carried hit pixels): the rigid path's X_inv(i) P, or the previous BLAS's material point."""
    t, u, v, prim, inst = hits
    ii = inst[sel].astype(np.int64)
    po = tref._xf_point(np.asarray(inv, np.float32)[ii], hp).astype(np.float32)
    bp = np.asarray(by_prim, bool)[ii]
    if bp.any():
        one = f32(1)
        for i in np.unique(ii[bp]):
            m = bp & (ii == i)
            s = np.asarray(prev_verts[int(link[i])], np.float32).reshape(-1, 3, 3)
            k = prim[sel][m].astype(np.int64)
            uu, vv = u[sel][m].astype(np.float32)[:, None], v[sel][m].astype(np.float32)[:, None]
            w = (one - uu) - vv
            po[m] = (s[k, 0] * w + s[k, 1] * uu) + s[k, 2] * vv
    return po


def step(hist, link, by_prim, prev_verts, color, hits, cam, inv, xf, width, height, tparams=None, moments=False, diag=None):
    """One linked call's reprojection and blend.  hist, link, color, hits, cam, inv, xf, width, height, tparams, moments: as
    denoise_handoff_ref.handoff_step's.  by_prim: (n_next,) bool (make_link); prev_verts: per instance of the HISTORY's TLAS its BLAS's
    object-space vertices (t, 3, 3), read for the predecessors of by-primitive entries only.  diag: a dict that receives "sel" (flat
    indices of the carried hit pixels), "po" and "by_prim" (per such pixel).  Returns (A, L, motion, M or None, history)."""
    p = dict(tref.DEFAULTS)
    p.update(tparams or {})
    alpha_min, max_history, tol = f32(p["alpha_min"]), f32(p["max_history"]), f32(p["depth_tolerance"])
    n_px = width * height
    center, U, V, W = (np.asarray(x, np.float32) for x in cam)
    t, u, v, prim, inst = hits
    t = np.asarray(t, np.float32).reshape(-1)
    u, v = np.asarray(u, np.float32).reshape(-1), np.asarray(v, np.float32).reshape(-1)
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
    carried = hit.copy()
    carried[hit] = link[inst[hit].astype(np.int64)] != NO_INSTANCE
    sel = np.nonzero(carried)[0]
    ii = inst[sel].astype(np.int64)
    pi = link[ii]
    dirs = ref.primary_directions(width, height, U, V, W)
    hp = center + dirs[sel] * t[sel][:, None]
    po = object_points(link, by_prim, prev_verts, (t, u, v, prim, inst), sel, hp, inv)
    if diag is not None:
        diag.update(sel=sel, po=po, by_prim=np.asarray(by_prim, bool)[ii])
    pw = tref._xf_point(np.asarray(hist["xf"], np.float32)[pi.astype(np.int64)], po)
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
            same_id = (h_inst[q] == pi) & (h_prim[q] == prim[sel])
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


def temporal_frame(hist, link, by_prim, prev_verts, color, oscene, scene, cam, width, height, params=None, tparams=None, diag=None):
    """The hrt_denoise_temporal_launch that takes the link, over the oracle's primary hits of `scene` (the next TLAS's instances):
    returns denoise_temporal_ref.temporal_frame's (output, A, L, motion, history)."""
    hits, xf, guides = href._frame_inputs(oscene, scene, cam, width, height)
    A, L, motion, _, hist2 = step(hist, link, by_prim, prev_verts, color, hits, cam, tref.world_to_object(oscene), xf, width, height, tparams,
                                  diag=diag)
    return ref.atrous(A, guides, params), A, L, motion, hist2


def variance_frame(hist, link, by_prim, prev_verts, color, oscene, scene, cam, width, height, params=None, tparams=None, vparams=None):
    """... and the hrt_denoise_variance_launch: returns denoise_variance_ref.variance_frame's (output, A, L, motion, M, var, history)."""
    hits, xf, guides = href._frame_inputs(oscene, scene, cam, width, height)
    A, L, motion, M, hist2 = step(hist, link, by_prim, prev_verts, color, hits, cam, tref.world_to_object(oscene), xf, width, height, tparams,
                                  moments=True)
    var = vref.variance(M, L, hist2["inst"], vref._params(vparams)["history_min"])
    out, _ = vref.filter_variance(A, guides, var, params, vparams)
    return out, A, L, motion, M, var, hist2


def blas_info(scene, order=None):
    """(identity, kind, primitive count) per instance of `scene` as Renderer.load_scene / build_tlas make its BLASes: triangle instances
    with the same "shape" share one; an instance with "own" (with_vertices) or without a shape has its own.  order: `scene` is
    sub_scene(loaded scene, order) -- instance j is the loaded scene's order[j], whose BLAS it keeps."""
    out = []
    for k, it in enumerate(scene["instances"]):
        k = k if order is None else int(order[k])
        tri = it["geometry"] == "triangles"
        ident = it["own"] if it.get("own") is not None else (("shape", it["shape"]) if tri and it.get("shape") is not None else ("own", k))
        out.append((ident, TRIANGLES if tri else SPHERES, len(it["vertices"]) if tri else len(it["radii"])))
    return out


def with_vertices(scene, vertices, normals, tag):
    """`scene` with the instances j of `vertices` ({j: (t, 3, 3)}) given those vertices, normals[j] and a BLAS of their own (identity
    (tag, j)): what Renderer.build_tlas(..., vertices=, normals=) traces."""
    out = {k: v for k, v in scene.items() if k != "instances"}
    out["instances"] = [dict(it) for it in scene["instances"]]
    for j, v in vertices.items():
        it = out["instances"][j]
        it["vertices"] = np.ascontiguousarray(v, np.float32).reshape(-1, 3, 3)
        it["normals"] = np.ascontiguousarray(normals[j], np.float32).reshape(-1, 3, 3)
        it["own"] = (tag, j)
    return out


def scene_verts(scene):
    """Per instance the object-space vertices of its BLAS (None for spheres): step's prev_verts of a history made on `scene`."""
    return [it["vertices"] if it["geometry"] == "triangles" else None for it in scene["instances"]]
