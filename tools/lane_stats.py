#!/usr/bin/env python3
"""Lane utilisation of the fused path kernel per phase (C4, 16 spp; `tools/lane_stats.py spp N`: N samples, e.g. 256 for the schedule bench.py
times, and HRT_SAMPLE_BLOCK=4 with 16 for a block render of few samples).  Needs a library built with the counters compiled in:
    touch nvidia-optix-ray-tracer_amd/csrc/kernels.hip && make lib HIPFLAGS="$(make -pn | sed -n 's/^HIPFLAGS := //p') -DHRT_LANE_STATS"
(the counters reuse HrtStats.debug[] and the two counting fields the production kernels leave at zero).
`tools/lane_stats.py spp 256 primary`, on `make stats EXTRA_HIPFLAGS=-DHRT_LANE_STATS_PRIMARY` through HRT_LIB: also what a pixel's repeat
primary rays cost -- how many there are, how many start at a node or are decided in the regeneration, the iterations they are alive and wait."""
import importlib, sys
sys.path[:0] = [str(__import__("pathlib").Path(__file__).resolve().parent.parent), str(__import__("pathlib").Path(__file__).resolve().parent)]
import path_kernels
hrt = importlib.import_module("nvidia-optix-ray-tracer_amd")
spp = 16
if len(sys.argv) > 1 and sys.argv[1] == "particles":       # tools/lane_stats.py particles N: the reference's kind of scene, 1200x800
    n_p = int(sys.argv[2])
    scene = hrt.scenes.particle_scene(n_p, 1200, 800, 16, subdiv=2 if n_p <= 100 else 3)
    r = hrt.Renderer(0, 0); r.load_scene(scene); r.set_frame(1200, 800, hrt.scenes.SEED_SALT, aov=False)
else:
    if len(sys.argv) > 2 and sys.argv[1] == "spp":
        spp = int(sys.argv[2])
    scene = hrt.scenes.soup_1m(1920, 1080, spp)
    r = hrt.Renderer(0, hrt.CTX_FAST_TRACE); r.load_scene(scene); r.set_frame(1920, 1080, hrt.scenes.SEED_SALT, aov=False)      # (the tree bench.py times)
r.render(2); r.reset_stats(); r.render(spp)
s = r.stats()
it, alive, node, prim = s.debug[0], s.debug[1], s.debug[2], s.debug[3]
ppass, regen = s.node_visits_closest, s.prim_tests_closest
print("rays", s.rays, "wave iterations", it, "regenerations", regen, "iters/ray-lane", it*64/s.rays)
print("alive lanes/iter %.1f  node lanes/iter %.1f  prim lanes/iter %.1f" % (alive/it, node/it, prim/it))
print("prim passes per iteration %.3f  lanes per prim pass %.1f  regens per iteration %.4f (every %.1f iterations)" % (ppass/it, prim/max(ppass,1), regen/it, it/max(regen,1)))
print("node steps per ray %.2f  prim tests per ray %.2f" % (node/s.rays, prim/s.rays))
if "primary" in sys.argv:
    # a library built with `make stats EXTRA_HIPFLAGS=-DHRT_LANE_STATS_PRIMARY` (trav_common.h: LaneStats): what a pixel's repeat primary rays cost.
    # The counters take the drained phase's slots (HrtStats.tail); a record tested in the regeneration (k_path_direct) counts as a primitive test.
    t = s.tail
    prim_rays, quick, q_alive, q_wait, direct = t[0], t[1], t[3], t[4], t[5]
    all_primary = prim_rays + direct + ((s.prim_tests - s.prim_tests_closest) >> 32)      # (walked, decided by their record, decided by the miss block: below)
    print("kernel", path_kernels.kernel_ran(s))
    print("primary rays", all_primary, "walked from the root", prim_rays - quick, "started at a node other than the root", quick, "decided in the regeneration", direct)
    print("h = share of primary rays with a record %.4f" % ((quick + direct) / max(all_primary, 1)))
    print("iterations the rays started at a node were alive", q_alive, "(%.2f each)  waited for their regeneration" % (q_alive / max(quick, 1)), q_wait, "(%.2f each)" % (q_wait / max(quick, 1)))
    print("their lane-slots %d of %d = %.2f %%" % (q_alive + q_wait, 64 * it, 100.0 * (q_alive + q_wait) / (64 * it)))
    # primary rays that came back from the loop a miss (depth 1), the iterations they were alive and waited for their regeneration, and the samples
    # k_path_direct's miss block decided without a walk (HRT_MISS_BLOCK): slots 6 and 7, and the two halves of prim_tests - prim_tests_closest
    packed = s.prim_tests - s.prim_tests_closest
    m_rays, ff, m_alive, m_wait = packed & 0xffffffff, packed >> 32, t[6], t[7]
    print("primary rays that came back a miss", m_rays, "iterations alive", m_alive, "(%.2f each)  waited" % (m_alive / max(m_rays, 1)), m_wait, "(%.2f each)" % (m_wait / max(m_rays, 1)))
    print("their lane-slots %d of %d = %.2f %%" % (m_alive + m_wait, 64 * it, 100.0 * (m_alive + m_wait) / (64 * it)))
    print("samples decided by the miss block", ff)
