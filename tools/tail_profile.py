#!/usr/bin/env python3
"""The end-of-frame tail of the fused path kernel on the frame bench.py times (C4: 1 M triangles, 1920x1080, HRT_CTX_FAST_TRACE): from
the first wave that finds the tile used up to the end of the kernel, how long is it and how many lane-slots stand idle in it.
Needs the instrumented build (its counters are HrtStats.tail, written by LaneStats::report at the end of the kernel):
    make stats && HRT_LIB=nvidia-optix-ray-tracer_amd/lib/libhrt_stats.so tools/tail_profile.py [spp ...]      (default: 256 64)
One launch per figure (the slots add up over launches): the frame is rendered once, warm, between a reset and a read of the statistics.
The clock is s_memrealtime, 100 MHz.  Idle lane-slots = 64 x (the time every wave is gone before the last one exits) + each wave's
span from draining to exit x the share of its lanes without a ray over its drained iterations; before a wave drains it is in steady
state and counts as full.  The kernel's lane-slots = its HIP-event time x waves x 64."""
import importlib, os, sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
hrt = importlib.import_module("nvidia-optix-ray-tracer_amd")

TICK_MS = 1e-5          # one tick of the 100 MHz clock
BIAS = 1 << 40          # LaneStats::report keeps clocks relative to the first reporting wave's, plus this


def schedule(s, spp):
    """the blocks the launch ran in: HrtStats.sample_block_schedule (a library from before it existed leaves the field zero) through hrt_sample_schedule"""
    import ctypes as C
    big, small, end, passes = (int(x) for x in getattr(s, "sample_block_schedule", (0, 0, 0, 0)))
    if int(s.sample_block_launches) == 0:
        return "no blocks"
    if big == 0:
        return "blocks (this library does not say which)"
    lib = hrt.load_library()
    if not hasattr(lib, "hrt_sample_schedule"):
        return f"largest {big}, smallest {small}, {passes} passes"
    first, n = (C.c_uint32 * (spp + 1))(), C.c_uint32(0)
    if lib.hrt_sample_schedule(spp, big, small if end else 0, first, spp + 1, C.byref(n)) != 0 or n.value != passes:
        return f"largest {big}, smallest {small}, {passes} passes"
    sizes = [first[i + 1] - first[i] for i in range(n.value)]
    return ("tapered " if end else "uniform ") + " ".join(str(k) for k in sizes) + f" ({passes} passes, {passes - 1} hand-overs per pixel)"


def profile(r, spp, width, height):
    r.set_frame(width, height, hrt.scenes.SEED_SALT, aov=False)
    r.render(2)
    r.set_frame(width, height, hrt.scenes.SEED_SALT, aov=False)
    r.reset_stats()
    r.render(spp)
    s = r.stats()
    t = list(s.tail)
    launches, kernel_ms = int(s.kernel_launches[hrt.K_PATHS]), float(s.kernel_ms[hrt.K_PATHS])
    if t[7] == 0:
        sys.exit("HrtStats.tail is empty: load the instrumented build (make stats; HRT_LIB=.../libhrt_stats.so)")
    if launches != 1:
        sys.exit(f"{launches} path-kernel launches between reset and read: the slots hold one launch (HRT_FUSED_MAX_SPP, HRT_FUSED_LPT?)")
    waves = t[7]
    first_drained = ((~t[3]) & 0xFFFFFFFFFFFFFFFF) - BIAS           # ticks, relative to the first wave's exit (negative: before it)
    last_exit = t[4] - BIAS
    span_ms = (last_exit - first_drained) * TICK_MS
    gone = 64 * (waves * t[4] - t[5])                               # lane-ticks of waves that have left before the kernel ends
    idle = gone + t[6]
    slots = kernel_ms / TICK_MS * waves * 64
    it_all, alive_all = s.debug[0], s.debug[1]
    print(f"C4 {width}x{height}, {spp} spp, sample_block {os.environ.get('HRT_SAMPLE_BLOCK', 'default')}, sample_taper {os.environ.get('HRT_SAMPLE_TAPER', 'default')}: "
          f"kernel {kernel_ms:.2f} ms, {waves} waves, {s.rays} rays")
    print(f"  schedule: {schedule(s, spp)}")
    print(f"  drained copy of the loop: {t[0]} of {it_all} wave iterations ({100.0 * t[0] / max(it_all, 1):.2f} %), "
          f"{t[1] / max(t[0], 1):.1f} lanes alive per iteration there against {alive_all / max(it_all, 1):.1f} over all")
    print(f"  first wave drained -> end of kernel: {span_ms:.2f} ms = {100.0 * span_ms / kernel_ms:.2f} % of the kernel's time")
    print(f"  idle lane-slots in that span: {100.0 * idle / slots:.2f} % of the kernel's lane-slots "
          f"(waves already gone {100.0 * gone / slots:.2f} %, lanes without a ray in drained waves {100.0 * t[6] / slots:.2f} %); "
          f"the whole span is {100.0 * span_ms / kernel_ms:.2f} %", flush=True)


if __name__ == "__main__":
    spps = [int(x) for x in sys.argv[1:]] or [256, 64]
    scene = hrt.scenes.soup_1m()
    r = hrt.Renderer(0, hrt.CTX_TIMING | hrt.CTX_FAST_TRACE)       # (the tree bench.py times)
    r.load_scene(scene)
    for spp in spps:
        profile(r, spp, scene["width"], scene["height"])
