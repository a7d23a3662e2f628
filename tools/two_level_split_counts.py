#!/usr/bin/env python3
"""What spatial splits in a shared BLAS buy, counted on the CPU, for profiles/: the scene and the rays of
tests/test_two_level_fast_trace_gpu.py::test_the_split_tree_costs_less_to_walk (six instances of one soup of long thin triangles, a sphere
BLAS; camera and random rays) -- the two-level tree built with and without HRT_CTX_FAST_TRACE, downloaded and walked by the oracle's
bvh8_walk: node visits and primitive tests per ray -- next to the flattened default / split pair of the same soup alone.
    tools/two_level_split_counts.py"""
import importlib, sys
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
hrt = importlib.import_module("nvidia-optix-ray-tracer_amd")
import oracle_py as O
import test_two_level_fast_trace_gpu as T
sc = hrt.scenes
bodies = T._bodies_scene(hrt)
soup = sc.random_soup(T.N_TRI, T.EDGE, 9, T.W, T.H, T.SPP)
co, cd = T._camera_rays(bodies, 300, 200)
ro, rd = O.random_rays(60000, 41)
o, d = np.concatenate([co, ro]), np.concatenate([cd, rd]); n = len(o)


def walk(scene, flags):
    r = hrt.Renderer(0, flags)
    s = T._load(r, scene)
    nodes, prims = T._download(hrt, r)
    inv = np.stack([np.linalg.inv(np.vstack([it["transform"].reshape(3, 4).astype(np.float64), [0, 0, 0, 1]]))[:3].reshape(12) for it in scene["instances"]]).astype(np.float32)
    ident = np.array([int(np.array_equal(it["transform"], sc.IDENTITY)) for it in scene["instances"]], dtype=np.uint32)
    res = O.bvh8_trace(nodes.ctypes.data, prims.ctypes.data, o, d, inst_inv=inv, inst_identity=ident)
    r.close()
    return res, int(s.bvh_nodes), len(prims) // 48, int(s.bvh_depth)


print(f"{n} rays ({len(co)} camera, {len(ro)} random); soup of {T.N_TRI} triangles, edge {T.EDGE}")
for title, scene, pair in (("flattened, the soup alone", soup, (("default", 0), ("split (HRT_CTX_FAST_TRACE)", hrt.CTX_FAST_TRACE))),
                           (f"two-level, {T.N_BODIES} instances of the soup and a sphere BLAS", bodies,
                            (("unsplit (HRT_CTX_TWO_LEVEL)", hrt.CTX_TWO_LEVEL), ("split (| HRT_CTX_FAST_TRACE)", hrt.CTX_TWO_LEVEL | hrt.CTX_FAST_TRACE)))):
    got = []
    for name, flags in pair:
        res, nn, nr, depth = walk(scene, flags)
        got.append(res)
        print(f"{title}, {name}: {nn} nodes, {nr} records, depth {depth}; {res[5] / n:.3f} node visits + {res[6] / n:.3f} primitive tests per ray", flush=True)
    a, b = got
    print(f"  split / unsplit: node visits {b[5] / a[5]:.4f}, primitive tests {b[6] / a[6]:.4f}, visits + tests {(b[5] + b[6]) / (a[5] + a[6]):.4f}; same hits: {bool(np.array_equal(a[3], b[3]) and np.array_equal(a[0], b[0]))}", flush=True)
