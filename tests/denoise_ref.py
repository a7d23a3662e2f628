"""Numpy specification of the denoiser (include/hrt.h "denoiser", csrc/denoise.hip), operation for operation in float32.

Guides are (H, W, 8) uint16 arrays laid out as HrtDenoiseGuide: normal[3] and albedo[3] as IEEE halves, then the depth as the two
halves of a float32.  ``atrous`` is the filter, ``primary_guides`` the guide pass over primary hits traced by the oracle, with the
shading arithmetic of oracle/oracle.c (closesthit_impl: :666-682 for the normal, :711 for its normalisation)."""
from __future__ import annotations

import numpy as np

f32 = np.float32
H_B3 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], dtype=np.float32)
DEFAULTS = {"iterations": 5, "sigma_color": 0.5, "sigma_albedo": 0.1, "sigma_depth": 0.02, "normal_power_log2": 3}
K_FLOAT_ZERO2 = f32(f32(1e-6) * f32(1e-6))


# ---- guide records ------------------------------------------------------------------------
def pack_guides(normal, albedo, depth):
    """(H, W, 3) float normal and albedo (rounded to half, RNE) + (H, W) float32 depth -> (H, W, 8) uint16 records."""
    h, w = depth.shape
    g = np.zeros((h, w, 8), np.uint16)
    g[..., 0:3] = np.asarray(normal, np.float32).astype(np.float16).view(np.uint16)
    g[..., 3:6] = np.asarray(albedo, np.float32).astype(np.float16).view(np.uint16)
    g[..., 6:8] = np.ascontiguousarray(depth, dtype=np.float32).reshape(h, w, 1).view(np.uint16)
    return g


def unpack_guides(g):
    g = np.ascontiguousarray(g).view(np.uint16)
    n = g[..., 0:3].view(np.float16).astype(np.float32)
    a = g[..., 3:6].view(np.float16).astype(np.float32)
    z = np.ascontiguousarray(g[..., 6:8]).view(np.float32)[..., 0]
    return n, a, z


# ---- the filter ---------------------------------------------------------------------------
def pass_constants(params=None):
    """The per-pass constants hrt_denoise.cpp derives from HrtDenoiseParams, in float32: (step, k_color, k_albedo, sigma_depth * step)."""
    p = dict(DEFAULTS)
    p.update(params or {})
    out = []
    for i in range(int(p["iterations"])):
        sc = f32(np.ldexp(f32(p["sigma_color"]), -i))
        sa = f32(p["sigma_albedo"])
        out.append((1 << i, f32(f32(1) / f32(sc * sc)), f32(f32(1) / f32(sa * sa)), f32(f32(p["sigma_depth"]) * f32(1 << i))))
    return out, int(p["normal_power_log2"])


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def atrous_pass(src, n, a, z, step, k_color, k_albedo, sz_step, squarings):
    """One pass: src (H, W, 4) float32 -> (H, W, 4) float32 (k_denoise_pass)."""
    H, W = z.shape
    hit = (z > 0) & (z < np.inf)
    one = f32(1)
    with np.errstate(all="ignore"):
        inv_z = one / (sz_step * z)
        sw = np.zeros((H, W), np.float32)
        sr, sg, sb = np.zeros_like(sw), np.zeros_like(sw), np.zeros_like(sw)
        for j in range(5):
            dy = (j - 2) * step
            for i in range(5):
                dx = (i - 2) * step
                y0, y1 = max(0, -dy), min(H, H - dy)       # pixels p whose tap q = p + (dx, dy) lies inside the frame
                x0, x1 = max(0, -dx), min(W, W - dx)
                if y0 >= y1 or x0 >= x1:
                    continue
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
                cp, cq = src[P], src[Q]
                dr, dg, db = cq[..., 0] - cp[..., 0], cq[..., 1] - cp[..., 1], cq[..., 2] - cp[..., 2]
                dc2 = (dr * dr + dg * dg) + db * db
                wn = np.fmax(_dot(n[P], n[Q]), f32(0))
                for _ in range(squarings):
                    wn = wn * wn
                da = a[P] - a[Q]
                da2 = _dot(da, da)
                rz = (z[P] - z[Q]) * inv_z[P]
                w = ((H_B3[i] * H_B3[j]) * wn) / (((one + dc2 * k_color) * (one + da2 * k_albedo)) * (one + rz * rz))
                take = hit[Q]
                sw[P] = np.where(take, sw[P] + w, sw[P])
                sr[P] = np.where(take, sr[P] + w * cq[..., 0], sr[P])
                sg[P] = np.where(take, sg[P] + w * cq[..., 1], sg[P])
                sb[P] = np.where(take, sb[P] + w * cq[..., 2], sb[P])
        keep = ~(hit & (sw > 0))
        out = np.stack([sr / sw, sg / sw, sb / sw, src[..., 3]], axis=-1).astype(np.float32)
    out[keep] = src[keep]
    return out


def atrous(color, guides, params=None):
    """hrt_denoise_filter: (H, W, 4) float32 colour + (H, W, 8) guides -> (H, W, 4) float32."""
    n, a, z = unpack_guides(guides)
    passes, squarings = pass_constants(params)
    out = np.ascontiguousarray(color, dtype=np.float32)
    for step, kc, ka, szs in passes:
        out = atrous_pass(out, n, a, z, step, kc, ka, szs, squarings)
    return out


# ---- the guide pass -----------------------------------------------------------------------
def _normalize3(v):
    len2 = (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]
    with np.errstate(all="ignore"):
        inv = f32(1) / np.sqrt(len2)
    out = v * inv[..., None]
    out[len2 <= K_FLOAT_ZERO2] = np.array([0, 0, 1], np.float32)
    return out


def primary_directions(width, height, U, V, Wv):
    """primary_direction (csrc/trav_common.h, Shader.cu:249-261) of every pixel, (H * W, 3) float32, row-major."""
    iy, ix = np.meshgrid(np.arange(height, dtype=np.float32), np.arange(width, dtype=np.float32), indexing="ij")
    ndcx = ((ix + f32(0.5)) / f32(width)) * f32(2) - f32(1)
    ndcy = ((iy + f32(0.5)) / f32(height)) * f32(2) - f32(1)
    aspect = f32(f32(width) / f32(height))
    U, V, Wv = (np.asarray(x, np.float32) for x in (U, V, Wv))
    d = (U * (ndcx * aspect)[..., None] + V * ndcy[..., None]) + Wv
    return _normalize3(d.astype(np.float32)).reshape(-1, 3)


def guides_from_hits(scene, origin, dirs, t, u, v, prim, inst, width, height):
    """HrtDenoiseGuide of every primary hit (oracle.c closesthit_impl's normal, normalised as its depth-1 AOV; the material's albedo)."""
    n_px = width * height
    normal = np.zeros((n_px, 3), np.float32)
    albedo = np.zeros((n_px, 3), np.float32)
    depth = np.full(n_px, np.inf, np.float32)
    o = np.asarray(origin, np.float32)
    insts = scene["instances"]
    for k, it in enumerate(insts):
        sel = np.nonzero(inst == k)[0]
        if sel.size == 0:
            continue
        d, tt, p = dirs[sel], t[sel][:, None], prim[sel].astype(np.int64)
        hp = o + d * tt
        if it["geometry"] == "triangles":
            nn = np.asarray(it["normals"], np.float32).reshape(-1, 3, 3)[p]
            uu, vv = u[sel][:, None], v[sel][:, None]
            w = (f32(1) - uu) - vv
            nv = (nn[:, 0] * w + nn[:, 1] * uu) + nn[:, 2] * vv
        else:
            c = np.asarray(it["centers"], np.float32).reshape(-1, 3)[p]
            r = np.asarray(it["radii"], np.float32).reshape(-1)[p][:, None]
            nv = (hp - c) / r
        front = _dot(d, nv) < 0
        nv = np.where(front[:, None], nv, -nv)
        normal[sel] = _normalize3(nv)
        albedo[sel] = np.asarray(it["albedo"], np.float32)
        depth[sel] = t[sel]
    return pack_guides(normal.reshape(height, width, 3), albedo.reshape(height, width, 3), depth.reshape(height, width))


def primary_guides(oscene, scene, cam, width, height):
    """The guides hrt_denoise_guides computes, from primary rays traced by the oracle (oracle_py.OracleScene, flattened or instanced).
    cam: (center, U, V, W) as the Renderer holds it."""
    center, U, V, Wv = cam
    dirs = primary_directions(width, height, U, V, Wv)
    origins = np.broadcast_to(np.asarray(center, np.float32), dirs.shape).copy()
    t, u, v, prim, inst = oscene.trace(origins, dirs)
    return guides_from_hits(scene, center, dirs, t, u, v, prim, inst, width, height)
