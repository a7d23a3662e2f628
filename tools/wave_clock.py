#!/usr/bin/env python3
"""The clock the path kernel's waves run at, read inside the kernel (DESIGN.md section 4.1 "what bounds it"; profiles/r29_idle_lanes.txt).
The instrumented build stamps the shader clock's counter (s_memtime) beside the 100 MHz one (s_memrealtime) at a wave's first
regeneration and at its exit (trav_common.h: LaneStats); clock = cycles / ticks x 100 MHz, per wave, filed in HrtStats.wave_clock as a
histogram of 16 MHz bins.  The production kernels have no stamp.
    make stats && HRT_LIB=nvidia-optix-ray-tracer_amd/lib/libhrt_stats.so tools/wave_clock.py [C2|C3|C4|C5] [seconds of launches before the reading, default 2]
Renders the configuration of bench.py back to back for that long, then reads the waves of as many launches again.  Prints the median
over waves, the 5th and 95th percentile (to the bin: +-8 MHz), the mean (sum of cycles over sum of ticks) and which kernel ran."""
import importlib, json, sys, time
sys.path[:0] = [str(__import__("pathlib").Path(__file__).resolve().parent.parent), str(__import__("pathlib").Path(__file__).resolve().parent)]
import path_kernels
hrt = importlib.import_module("nvidia-optix-ray-tracer_amd")
LOW, STEP, BINS = 1600, 16, 56          # trav_common.h: kWaveClockLow, kWaveClockStep, kWaveClockBins


def percentile(hist, q):
    """the clock below which the share q of the waves lies, interpolated inside its bin"""
    total, seen = sum(hist), 0
    for k, n in enumerate(hist):
        if n and seen + n >= q * total:
            return LOW + STEP * (k + (q * total - seen) / n)
        seen += n
    return float("nan")


def main():
    config = sys.argv[1] if len(sys.argv) > 1 else "C4"
    seconds = float(sys.argv[2]) if len(sys.argv) > 2 else 2.0
    scene = hrt.scenes.BASELINE_CONFIGS[config]()
    W, H, spp = scene["width"], scene["height"], scene["spp"]
    r = hrt.Renderer(0, hrt.CTX_FAST_TRACE)
    r.load_scene(scene)
    r.set_frame(W, H, hrt.scenes.SEED_SALT, aov=False)
    r.render(spp, sync=True)
    launches, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        r.render(spp, sync=True)
        launches += 1
    r.reset_stats()
    t0 = time.perf_counter()
    for _ in range(launches):
        r.render(spp, sync=False)
    s = r.stats()
    dt = time.perf_counter() - t0
    wc = [int(x) for x in s.wave_clock]
    waves, cycles, ticks, hist = wc[0], wc[1], wc[2], wc[4:4 + BINS]
    if waves == 0:
        sys.exit("HrtStats.wave_clock is empty: load the instrumented build (make stats; HRT_LIB=.../libhrt_stats.so)")
    print(json.dumps({"config": config, "kernel": path_kernels.kernel_ran(s), "launches": launches, "ms_per_launch": round(dt / launches * 1e3, 3), "waves": waves,
                      "mhz_median": round(percentile(hist, 0.5), 1), "mhz_p05": round(percentile(hist, 0.05), 1), "mhz_p95": round(percentile(hist, 0.95), 1),
                      "mhz_mean": round(cycles / ticks * 100.0, 1), "below_range": hist[0], "above_range": hist[-1], "mean_wave_ms": round(ticks / waves / 1e5, 3),
                      "rays": int(s.rays)}))
    r.close()


if __name__ == "__main__":
    main()
