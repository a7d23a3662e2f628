"""What tests/test_blas_update_cpu.py and tests/test_blas_update_gpu.py share: the scene, its deformations and the oracle's results for every
state a test brings a renderer to -- computed once per state and oracle mode, and never changed afterwards.

The scene: triangle BLASes of 96, 700 and 5000 triangles -- a single leaf group, several levels built by PLOC alone, and one above the
4096-primitive line where the top-down phase (and, under HRT_CTX_FAST_TRACE | HRT_CTX_TWO_LEVEL, the BLAS's split tree) begins -- under
distinct non-identity transforms; the 700-triangle BLAS is shared by two instances, which makes four instances over the three BLASes."""
import functools
import importlib

import numpy as np

import oracle_py

hrt = importlib.import_module("nvidia-optix-ray-tracer_amd")
scenes = hrt.scenes

W, H, SPP, SALT = 48, 32, 2, 0xB1A5
N_RAYS = 20000
SIZES = (96, 700, 5000)
BLAS_OF_INSTANCE = (0, 1, 1, 2)          # instance -> BLAS ("shape")
INSTANCE_OF_BLAS = (0, 1, 3)             # an instance to name each BLAS by (Renderer.update_blas_vertices takes either)


def base_vertices():
    return [scenes._random_triangles(96, 0.55, 41), scenes._random_triangles(700, 0.3, 42), scenes._random_triangles(5000, 0.14, 43)]


def transforms(moved=False):
    """Distinct non-identity transforms; moved: a small rigid step for every instance."""
    d = 0.07 if moved else 0.0
    return [scenes.rigid_transform((-0.25 + d, 0.2, 0.1), (1, 2, 0.5), 0.4 + d, 0.55),
            scenes.rigid_transform((0.3, -0.25 - d, -0.1), (0, 1, 1), -0.7 - d, 0.5),
            scenes.rigid_transform((-0.2, -0.3, 0.35 + d), (1, 0, 0.3), 1.9 + d, 0.45),
            scenes.rigid_transform((0.15 - d, 0.25, -0.2), (0.2, 1, 0), 2.6 - d, 0.6)]


def deform(v, which):
    """Every vertex displaced by a smooth function of its position, 2 % of the BLAS's extent (which: 1, 2: two different ones)."""
    v = np.asarray(v, dtype=np.float32)
    p = v.reshape(-1, 3).astype(np.float64)
    extent = float((p.max(axis=0) - p.min(axis=0)).max())
    k = np.array([[2.1, 0.7, -1.3], [-0.9, 2.4, 1.1], [1.6, -1.2, 2.2]]) * (1.0 + 0.5 * (which - 1))
    d = np.sin(p @ k.T + 0.4 * which)
    return (p + 0.02 * extent * d).astype(np.float32).reshape(v.shape)


def scatter(v, seed=7):
    """Every vertex somewhere in a box 30 x the BLAS's extent: what no refit survives."""
    p = np.asarray(v, dtype=np.float32).reshape(-1, 3)
    lo, hi = p.min(axis=0), p.max(axis=0)
    c, e = 0.5 * (lo + hi), 0.5 * (hi - lo)
    rng = np.random.default_rng(seed)
    return (c + 30.0 * e * rng.uniform(-1.0, 1.0, p.shape)).astype(np.float32).reshape(np.asarray(v).shape)


def make_scene(verts, xf):
    mats = (("rough", scenes.RED, 0.0), ("metal", scenes.STEEL, 0.2), ("rough", scenes.GREEN, 0.0), ("rough", scenes.WHITE, 0.0))
    inst = []
    for i, b in enumerate(BLAS_OF_INSTANCE):
        it = scenes._tri_instance(verts[b], mats[i][1], mats[i][0], mats[i][2], xf[i])
        it["shape"] = b
        inst.append(it)
    return {"name": "blas-update", "instances": inst, "camera": scenes._soup_camera(), "background": scenes.BACKGROUND.copy(),
            "width": W, "height": H, "spp": SPP}


# ---- the states: name -> (vertices per BLAS, transforms) ----
@functools.lru_cache(maxsize=None)
def state(name):
    base = base_vertices()
    if name == "base":
        return base, transforms()
    if name == "base_moved":             # (what a TLAS with other transforms over the same BLASes shows)
        return base, transforms(True)
    if name == "deformed":               # every BLAS deformed, the instances where they were
        return [deform(v, 1) for v in base], transforms()
    if name == "deformed_moved_old":     # ... seen through moved instances
        return [deform(v, 1) for v in base], transforms(True)
    if name == "deformed_again":         # another deformation, and moved instances in the same update
        return [deform(v, 2) for v in base], transforms(True)
    if name == "scattered":
        return [base[0], scatter(base[1]), base[2]], transforms()
    if name in ("nan_built", "nan_after"):      # triangle NAN_PRIM of the 96-triangle BLAS is NaN
        v = [x.copy() for x in base]
        v[0][NAN_PRIM] = np.nan
        return v, transforms()
    raise KeyError(name)


NAN_PRIM = 17


def scene_of(name):
    return make_scene(*state(name))


def rays(seed=3):
    return oracle_py.random_rays(N_RAYS, seed)


def rays_at_nan_prim():
    """... and a bundle aimed at triangle NAN_PRIM of instance 0 as the base scene has it."""
    o, d = rays()
    v, xf = state("base")
    m = xf[0].reshape(3, 4).astype(np.float64)
    c = v[0][NAN_PRIM].astype(np.float64).mean(axis=0)
    c = m[:, :3] @ c + m[:, 3]
    rng = np.random.default_rng(11)
    oo = (c + rng.normal(size=(400, 3)) * 0.02 + np.array([0.0, 0.0, 3.0])).astype(np.float32)
    dd = (c - oo.astype(np.float64) + rng.normal(size=(400, 3)) * 0.004).astype(np.float32)
    return np.concatenate([o, oo]), np.concatenate([d, dd])


@functools.lru_cache(maxsize=None)
def reference(name, instanced, nan_rays=False):
    """The oracle's word on a state, in the mode the tree structure is pinned to (two-level trees: INSTANCED, everything else: FLATTENED):
    brute-force hit records of the ray set, and the frame (linear radiance, colour, RNG states afterwards)."""
    scene = scene_of(name)
    o, d = rays_at_nan_prim() if nan_rays else rays()
    hits = oracle_py.OracleScene(scene, force_brute=True, instanced=instanced).trace(o, d)
    states = oracle_py.rng_init(W, H, SALT)
    frame = oracle_py.OracleScene(scene, instanced=instanced).render(W, H, states, SPP)
    for a in hits + (frame["linear"], frame["color"], states):
        a.setflags(write=False)
    return {"hits": hits, "linear": frame["linear"], "color": frame["color"], "states": states}
