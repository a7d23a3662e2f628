#!/usr/bin/env python3
"""Random animations: a random scene, then a sequence of hrt_tlas_update calls with random transforms -- small steps (refits), now and then a jump across
the scene (the quality guard rebuilds), uneven scales and shears, an instance shrunk to nothing -- synchronous and asynchronous updates, flattened and
two-level trees, other execution modes; after every update the frame is compared bit for bit with the oracle's render of the moved scene.
--deform: between the instance updates a random triangle BLAS now and then gets new vertices in place (hrt_blas_update_triangles: a smooth
2 % deformation, at times a scatter that no refit survives), picked up by the update that follows; the scenes and transforms are the same
ones as without the option (the deformations draw from a generator of their own).
    tools/stress_updates.py [n_scenes=20] [seed=1] [--deform]"""
import importlib, os, sys, time, copy
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import torch
hrt = importlib.import_module("nvidia-optix-ray-tracer_amd")
import oracle_py as oracle

deform = "--deform" in sys.argv
argv = [a for a in sys.argv if a != "--deform"]
n_scenes = int(argv[1]) if len(argv) > 1 else 20
rng = np.random.default_rng(int(argv[2]) if len(argv) > 2 else 1)
drng = np.random.default_rng(1000 + (int(argv[2]) if len(argv) > 2 else 1))      # --deform's own
bad = deformed = 0

def deform_blas(r, scene, drng):
    """new vertices for the BLAS of a random triangle instance, in the renderer and in every instance of the scene that shares it"""
    tri = [i for i, it in enumerate(scene["instances"]) if it["geometry"] == "triangles"]
    if not tri: return 0
    i = int(drng.choice(tri)); it = scene["instances"][i]
    p = it["vertices"].reshape(-1, 3).astype(np.float64)
    ext = float((p.max(axis=0) - p.min(axis=0)).max()) or 1.0
    if drng.random() < 0.1: q = p.mean(axis=0) + 20.0 * ext * drng.uniform(-1, 1, p.shape)
    else: q = p + 0.02 * ext * np.sin(p @ drng.normal(0, 2.0 / ext, (3, 3)) + drng.uniform(0, 6.28, 3))
    v = q.astype(np.float32).reshape(it["vertices"].shape)
    r.update_blas_vertices(i, v)
    for jt in scene["instances"]:
        if jt is it or (jt["geometry"] == "triangles" and it.get("shape") is not None and jt.get("shape") == it.get("shape")):
            jt["vertices"] = v; jt["normals"] = hrt.scenes.face_normals(v)
    return 1

def jitter(m, rng, big):
    m = m.reshape(3, 4).astype(np.float64).copy()
    ang = rng.normal(0, 1.5 if big else 0.05); ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K
    lin = R @ m[:, :3]
    kind = rng.random()
    if kind < 0.1: lin = lin @ np.diag(rng.uniform(0.5, 1.8, 3))
    elif kind < 0.15: lin = lin @ np.array([[1, rng.uniform(-0.4, 0.4), 0], [0, 1, 0], [0, rng.uniform(-0.4, 0.4), 1]])
    elif kind < 0.17: lin = lin * 1e-9
    m[:, :3] = lin
    m[:, 3] += rng.normal(0, 1.0 if big else 0.02, 3)
    return m.astype(np.float32).reshape(12)

for k in range(n_scenes):
    w, h, spp = int(rng.integers(40, 120)), int(rng.integers(30, 90)), int(rng.integers(1, 4))
    kind = rng.integers(0, 3)
    if kind == 0: scene = hrt.scenes.mixed_test_scene(int(rng.integers(10, 2000)), int(rng.integers(1, 40)), int(rng.integers(1, 1000)), w, h, spp)
    elif kind == 1: scene = hrt.scenes.particle_cloud(int(rng.integers(4, 500)), w, h, spp, subdiv=int(rng.integers(0, 3)), seed=int(rng.integers(1, 100)))
    else: scene = hrt.scenes.particle_scene(int(rng.integers(1, 200)), w, h, spp, frame=int(rng.integers(0, 5)))
    flags = (hrt.CTX_TWO_LEVEL if rng.random() < 0.4 else 0) | (hrt.CTX_ASYNC_UPDATE if rng.random() < 0.5 else 0)
    mode = str(rng.choice(["1", "1", "1", "deep", "0"]))      # deep: k_fused's depth limit lowered to 1, round 1's path kernel takes the tree
    if flags & hrt.CTX_TWO_LEVEL: mode = "1"
    os.environ["HRT_FUSED"] = "1" if mode == "deep" else mode
    if mode == "deep": os.environ["HRT_FUSED_MAX_DEPTH"] = "1"
    else: os.environ.pop("HRT_FUSED_MAX_DEPTH", None)
    salt = int(rng.integers(1, 1 << 30))
    scene = copy.deepcopy(scene)
    r = hrt.Renderer(0, flags)
    st = None
    try:
        r.load_scene(scene); r.set_frame(w, h, salt, linear=True)
        states = oracle.rng_init(w, h, salt)
        for step in range(int(rng.integers(2, 7))):
            big = rng.random() < 0.2
            tr = [jitter(it["transform"], rng, big) if rng.random() < 0.8 else it["transform"] for it in scene["instances"]]
            for it, m in zip(scene["instances"], tr): it["transform"] = m
            if deform and drng.random() < 0.6: deformed += deform_blas(r, scene, drng)
            r.update_instances(tr)
            r.render(spp)
            got = r.linear.cpu().numpy().view(np.uint32)
            ref = oracle.OracleScene(scene, instanced=bool(flags & hrt.CTX_TWO_LEVEL)).render(w, h, states, spp)["linear"].view(np.uint32)
            if not np.array_equal(got, ref):
                bad += 1
                print("MISMATCH", scene["name"], (w, h, spp), "flags", flags, "HRT_FUSED", mode, "step", step, "big" if big else "", int((got != ref).sum()), "words", flush=True)
                break
        st = r.stats()
    except hrt.HrtError as e:
        bad += 1; print("ERROR", scene["name"], "flags", flags, "HRT_FUSED", mode, str(e)[:160], flush=True)
    finally:
        r.close()
    print(time.strftime("%H:%M:%S"), k, scene["name"], (w, h, spp), "flags", flags, "mode", mode, "refits", int(st.tlas_refits) if st else "-", "rebuilds", int(st.tlas_rebuilds) if st else "-", "ok" if not bad else f"{bad} bad so far", flush=True)
if deform: print("stress:", deformed, "BLAS updates")
print("stress:", "all frames bit-exact" if not bad else f"{bad} FAILURES")
sys.exit(1 if bad else 0)
