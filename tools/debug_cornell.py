#!/usr/bin/env python3
"""Why does cornell_box(64, 94, 3) with salt 525075280 differ from the oracle in one pixel?  (found by tools/stress_modes.py)"""
import importlib, sys, os
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import torch
hrt = importlib.import_module("nvidia-optix-ray-tracer_amd")
import oracle_py as oracle
w, h, spp, salt = 64, 94, 3, 525075280
scene = hrt.scenes.cornell_box(w, h, spp)
for mode in ("1", "0"):
    os.environ["HRT_FUSED"] = mode
    r = hrt.Renderer(0, 0)
    r.load_scene(scene); r.set_frame(w, h, salt, linear=True)
    st = oracle.rng_init(w, h, salt); osc = oracle.OracleScene(scene, force_brute=True)
    for s in range(spp):
        r.render(1)
        ref = osc.render(w, h, st, 1)
        got = r.linear.cpu().numpy()
        d = np.argwhere((got.view(np.uint32) != ref["linear"].view(np.uint32)).any(axis=2))
        print("HRT_FUSED", mode, "sample", s, "differing pixels", d.tolist()[:4], flush=True)
        for (y, x) in d[:2]:
            print("   gpu", got[y, x], "oracle", ref["linear"][y, x], flush=True)
    r.close()
os.environ["HRT_FUSED"] = "1"
r = hrt.Renderer(0, 0); r.load_scene(scene)
rng = np.random.default_rng(3)
tris = np.concatenate([it["vertices"].reshape(-1, 3, 3) for it in scene["instances"] if it["geometry"] == "triangles"]).astype(np.float64)
n = 2_000_000
k = rng.integers(0, len(tris), n); u = rng.random(n); v = rng.random(n); f = u + v > 1; u[f] = 1 - u[f]; v[f] = 1 - v[f]
edge = rng.random(n) < 0.2; v[edge] = 0.0                                    # some origins exactly on an edge
p = tris[k, 0] + u[:, None] * (tris[k, 1] - tris[k, 0]) + v[:, None] * (tris[k, 2] - tris[k, 0])
nrm = np.cross(tris[k, 1] - tris[k, 0], tris[k, 2] - tris[k, 0]); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
rv = rng.uniform(-1, 1, (n, 3)); rv /= np.linalg.norm(rv, axis=1, keepdims=True)
sign = np.where(rng.random(n) < 0.5, 1.0, -1.0)[:, None]
d = sign * nrm + rv
o = p.astype(np.float32); d = d.astype(np.float32)
t, uu, vv, prim, inst = r.trace_rays(o, d)
rt, ru, rv_, rprim, rinst = oracle.OracleScene(scene, force_brute=True).trace(o, d)
bad = np.argwhere((prim != rprim) | (inst != rinst) | (t.view(np.uint32) != rt.view(np.uint32))).ravel()
print("surface rays:", n, "mismatching hit records:", len(bad), flush=True)
for i in bad[:6]:
    print("  o", o[i], "d", d[i], "gpu", (t[i], prim[i], inst[i]), "oracle", (rt[i], rprim[i], rinst[i]), flush=True)
r.close()
