#!/usr/bin/env python3
"""HRT_CTX_KEEP_SPLITS on one MI355X: what a flattened split tree is worth after an update, and what the update costs.

Per scene (C4's soup as one instance; the 2000-particle scene) and motion (every instance turned by 0.2 rad about the world's y axis;
every instance shifted by 0.05) three trees are traced with the same frame:
  built     HRT_CTX_FAST_TRACE | HRT_CTX_KEEP_SPLITS, as built (no update: the instances already in the moved pose)
  kept      the same flags, built in the first pose, then ONE update to the moved pose: the split tree refitted
  default   HRT_CTX_FAST_TRACE alone, the same update: the first update rebuilds, a default tree (what the library did before the flag)
For each: node visits and primitive tests per ray (a context with HRT_CTX_COUNT), Mrays/s of a 1280 x 720 frame (HIP-event time of the
path kernel, median of --renders launches after a warm-up), the first update's wall time with its synchronisation, a second update's
(steady state: a refit in both), bvh_alloc_bytes.  The rebuild ratio and the moved-far check are switched off so that the refitted
tree is what is traced; the refit's area ratio is printed.  --repeats alternates the three; medians over the repeats.
One JSON line per (scene, motion, tree)."""
import argparse, importlib, json, os, statistics, sys, time
from pathlib import Path
import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
hrt = importlib.import_module("nvidia-optix-ray-tracer_amd")
S = hrt.scenes


def compose(a, b):
    a, b = np.asarray(a, np.float64).reshape(3, 4), np.asarray(b, np.float64).reshape(3, 4)
    return np.concatenate([a[:, :3] @ b[:, :3], (a[:, :3] @ b[:, 3] + a[:, 3])[:, None]], axis=1).astype(np.float32).reshape(12)


def moved(scene, motion, amount=1.0):
    t = S.rigid_transform((0, 0, 0), (0, 1, 0), 0.2 * amount) if motion == "rotate" else S.rigid_transform((0.05 * amount, 0, 0), (0, 1, 0), 0.0)
    return [compose(t, it["transform"]) for it in scene["instances"]]


def with_pose(scene, xf):
    return dict(scene, instances=[dict(it, transform=m) for it, m in zip(scene["instances"], xf)])


def one(scene, motion, tree, renders, count):
    import torch
    keep = tree != "default"
    flags = hrt.CTX_FAST_TRACE | (hrt.CTX_KEEP_SPLITS if keep else 0) | (hrt.CTX_COUNT if count else hrt.CTX_TIMING)
    r = hrt.Renderer(0, flags)
    out = {}
    try:
        final = moved(scene, motion)
        r.load_scene(with_pose(scene, final) if tree == "built" else scene)
        if tree != "built":
            torch.cuda.synchronize()
            t0 = time.perf_counter(); r.update_instances(final); torch.cuda.synchronize(); t1 = time.perf_counter()
            st = r.stats()
            out.update(first_update_ms=(t1 - t0) * 1e3, refits=int(st.tlas_refits), rebuilds=int(st.tlas_rebuilds), refit_ratio=float(st.tlas_refit_ratio))
        if count:
            r.set_frame(640, 360, 7, aov=False)
            r.reset_stats(); r.render(1)
            st = r.stats()
            out.update(node_visits_per_ray=st.node_visits / max(st.rays, 1), prim_tests_per_ray=st.prim_tests / max(st.rays, 1))
        else:
            r.set_frame(1280, 720, 7, aov=False)
            r.render(2)
            rates = []
            for _ in range(renders):
                r.reset_stats(); r.render(4)
                st = r.stats()
                rates.append(st.rays / (sum(st.kernel_ms[k] for k in range(hrt.K_COUNT) if k != hrt.K_REFIT) * 1e-3) / 1e6)
            out.update(mrays_per_s=statistics.median(rates), bvh_alloc_bytes=int(st.bvh_alloc_bytes), bvh_nodes=int(st.bvh_nodes),
                       records=(int(st.bvh_bytes) - 80 * int(st.bvh_nodes)) // 48)
            if tree != "built":                               # steady state: one more update, a refit in both
                again = moved(scene, motion, 1.02)
                torch.cuda.synchronize()
                t0 = time.perf_counter(); r.update_instances(again); torch.cuda.synchronize(); t1 = time.perf_counter()
                out.update(second_update_ms=(t1 - t0) * 1e3, refits_after=int(r.stats().tlas_refits))
    finally:
        r.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--renders", type=int, default=3)
    ap.add_argument("--scenes", default="soup-1m,particles-2000")
    a = ap.parse_args()
    os.environ["HRT_REFIT_REBUILD_RATIO"] = "1e30"
    os.environ["HRT_REFIT_MOVED_FAR"] = "0"
    for name in a.scenes.split(","):
        scene = S.soup_1m(1280, 720, 4) if name == "soup-1m" else S.random_soup(6000, 0.12, 3, 1280, 720, 4) if name == "soup-6000" else S.particle_scene(2000, 1280, 720, 1, 0, subdiv=3)
        for motion in ("rotate", "translate"):
            runs = {t: [] for t in ("built", "kept", "default")}
            for _ in range(a.repeats):
                for tree in runs:
                    runs[tree].append(one(scene, motion, tree, a.renders, False))
            counts = {t: one(scene, motion, t, 1, True) for t in runs}      # (deterministic: once)
            for tree, rs in runs.items():
                line = {"scene": name, "motion": motion, "tree": tree}
                for key in rs[0]:
                    vals = [x[key] for x in rs]
                    line[key] = round(statistics.median(vals), 4) if isinstance(vals[0], float) else vals[0]
                    if key in ("mrays_per_s", "first_update_ms", "second_update_ms"):
                        line[key + "_range"] = [round(min(vals), 4), round(max(vals), 4)]
                line["node_visits_per_ray"] = round(counts[tree]["node_visits_per_ray"], 3)
                line["prim_tests_per_ray"] = round(counts[tree]["prim_tests_per_ray"], 3)
                print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
