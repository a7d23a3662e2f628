"""What tests/test_sphere_update_cpu.py and tests/test_sphere_update_gpu.py share: the scene, its motions and the oracle's results for every
state a test brings a renderer to -- computed once per state and oracle mode, and never changed afterwards.

The scene: sphere BLASes of 40, 700 and 5000 spheres -- a couple of leaf groups, several levels built by PLOC alone, and one above the
4096-primitive line where the top-down phase (and, under HRT_CTX_FAST_TRACE | HRT_CTX_TWO_LEVEL, the BLAS's split tree) begins -- under
tests/blas_update_cases.py's four distinct non-identity transforms; the 700-sphere BLAS is shared by two instances, which makes four
instances over the three BLASes."""
import functools
import importlib

import numpy as np

import blas_update_cases as bc
import oracle_py

hrt = importlib.import_module("nvidia-optix-ray-tracer_amd")
scenes = hrt.scenes

W, H, SPP, SALT = 48, 32, 2, 0xB1A5
N_RAYS = 20000
SIZES = (40, 700, 5000)
RADII = ((0.05, 0.14), (0.015, 0.05), (0.006, 0.02))
BLAS_OF_INSTANCE = (0, 1, 1, 2)          # instance -> BLAS ("shape")
INSTANCE_OF_BLAS = (0, 1, 3)             # an instance to name each BLAS by (Renderer.update_blas_spheres takes either)
NAN_PRIM = 17                            # of the 40-sphere BLAS

transforms = bc.transforms


def base_spheres():
    """Per BLAS: (centres (n, 3), radii (n,))."""
    out = []
    for k, (n, (r0, r1)) in enumerate(zip(SIZES, RADII)):
        out.append((scenes.uniform_f32(9100 + k, 3 * n, -0.5, 0.5).reshape(n, 3), scenes.uniform_f32(9200 + k, n, r0, r1)))
    return out


def move(c, r, which):
    """Every centre displaced by a smooth function of its position, 2 % of the cloud's extent (blas_update_cases.deform's), and every
    radius scaled by 1 + 0.1 sin(7 x + which) (which: 1, 2: two different motions)."""
    p = np.asarray(c, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    extent = float((p.max(axis=0) - p.min(axis=0)).max())
    k = np.array([[2.1, 0.7, -1.3], [-0.9, 2.4, 1.1], [1.6, -1.2, 2.2]]) * (1.0 + 0.5 * (which - 1))
    d = np.sin(p @ k.T + 0.4 * which)
    rr = np.asarray(r, dtype=np.float32).astype(np.float64) * (1.0 + 0.1 * np.sin(7.0 * p[:, 0] + which))
    return (p + 0.02 * extent * d).astype(np.float32), rr.astype(np.float32)


def scatter(c, seed=7):
    """Every centre somewhere in a box 30 x the cloud's extent: what no refit survives."""
    p = np.asarray(c, dtype=np.float32).reshape(-1, 3)
    lo, hi = p.min(axis=0), p.max(axis=0)
    mid, e = 0.5 * (lo + hi), 0.5 * (hi - lo)
    rng = np.random.default_rng(seed)
    return (mid + 30.0 * e * rng.uniform(-1.0, 1.0, p.shape)).astype(np.float32)


def make_scene(spheres, xf):
    mats = (("rough", scenes.RED, 0.0), ("metal", scenes.STEEL, 0.2), ("rough", scenes.GREEN, 0.0), ("rough", scenes.WHITE, 0.0))
    inst = []
    for i, b in enumerate(BLAS_OF_INSTANCE):
        it = scenes._sphere_instance(spheres[b][0], spheres[b][1], mats[i][1], mats[i][0], mats[i][2], xf[i])
        it["shape"] = b
        inst.append(it)
    return {"name": "sphere-update", "instances": inst, "camera": scenes._soup_camera(), "background": scenes.BACKGROUND.copy(),
            "width": W, "height": H, "spp": SPP}


# ---- the states: name -> (spheres per BLAS, transforms) ----
@functools.lru_cache(maxsize=None)
def state(name):
    base = base_spheres()
    if name == "base":
        return base, transforms()
    if name == "base_moved":             # (what a TLAS with other transforms over the same BLASes shows)
        return base, transforms(True)
    if name == "moved":                  # every BLAS in motion 1, the instances where they were
        return [move(c, r, 1) for c, r in base], transforms()
    if name == "moved_old_instances":    # ... seen through moved instances
        return [move(c, r, 1) for c, r in base], transforms(True)
    if name == "moved_again":            # the second motion, and moved instances in the same update
        return [move(c, r, 2) for c, r in base], transforms(True)
    if name == "scattered":
        return [base[0], (scatter(base[1][0]), base[1][1]), base[2]], transforms()
    if name in ("nan_built", "nan_after", "inf_after"):      # sphere NAN_PRIM of the 40-sphere BLAS: a NaN centre / an infinite radius
        c, r = base[0][0].copy(), base[0][1].copy()
        if name == "inf_after":
            r[NAN_PRIM] = np.inf
        else:
            c[NAN_PRIM] = np.nan
        return [(c, r), base[1], base[2]], transforms()
    raise KeyError(name)


def scene_of(name):
    return make_scene(*state(name))


def rays(seed=3):
    return oracle_py.random_rays(N_RAYS, seed)


def rays_at_nan_prim():
    """... and a bundle aimed at sphere NAN_PRIM of instance 0 as the base scene has it."""
    o, d = rays()
    s, xf = state("base")
    m = xf[0].reshape(3, 4).astype(np.float64)
    c = m[:, :3] @ s[0][0][NAN_PRIM].astype(np.float64) + m[:, 3]
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
