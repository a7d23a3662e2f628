"""The plan of a fused render (csrc/path_plan.h: plan_fused_render, plan_fused_launch -- everything hrt_api.cpp's render_fused decides before it
launches anything), as plain host code over a table of inputs.  A stand-alone program built against path_plan.h reads the rows below, prints
the plan of every render and of every one of its launches, and asks path_launch_admitted about each launch with the arguments the plan gives
and the plan's grid.  What the plan must be is restated here in Python -- the gates, the schedule, the ladder -- and not read from the C++.
No device is opened, nothing is launched, nothing is loaded into this process."""
import itertools
import random
import subprocess
from collections import namedtuple
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "nvidia-optix-ray-tracer_amd" / "csrc"

KERNELS = ("Fused", "FusedInstanced", "Capture", "Blocks", "OneGroup", "Restart", "Round1", "Counts", "MaskIdle", "Direct")      # enum class PathKernel, in order
SCENES = {"one instance of triangles": (1, 0), "two instances": (2, 0), "with spheres": (1, 1)}          # (n_instances, has_spheres): the choice test's three
TAPERS = {"64:8": (64, 8, 0), "4:2!": (4, 2, 1), "0": (0, 8, 0)}                                            # HRT_SAMPLE_TAPER: (big, min, forced)

# One render: what render_fused reads, by value (RenderPlanInput, in the order the program reads it), then whether the program prints the pass starts.
Row = namedtuple("Row", "n_cu fits two_level n_instances has_spheres has_records n full_frame spp reuse capture blocks_per_cu blocks_auto chunk "
                        "lpt sample_block taper_big taper_min taper_forced max_spp seed one_group primary_restart mask_idle primary_direct starts")
DEFAULT = Row(n_cu=256, fits=1, two_level=0, n_instances=1, has_spheres=0, has_records=1, n=0, full_frame=0, spp=1, reuse=0, capture=0, blocks_per_cu=20,
              blocks_auto=1, chunk=16, lpt=2, sample_block=-1, taper_big=64, taper_min=8, taper_forced=0, max_spp=512, seed=2,
              one_group=1, primary_restart=1, mask_idle=1, primary_direct=1, starts=0)

PIXELS = (48, 400, 448, 449, 512, 2257, 3072, 6144, 65535, 65536, 262143, 262144, 1048575, 1048576, 2073600)
SPP = (1, 2, 15, 16, 24, 63, 64, 65, 128, 256, 513, 1100)
SAMPLE_BLOCK = (-1, 0, 1, 2, 4, 32)


def ceil_div(a, b):
    return (a + b - 1) // b


def magic(d):
    return min((1 << 32) // d, (1 << 32) - 1) if d else 0


def schedule(now, r):
    """(k_big, k_min, taper_end or 0, pass starts) of a launch of `now` samples that may go in blocks: HRT_SAMPLE_BLOCK=N, uniform blocks of N;
    else HRT_SAMPLE_TAPER's -- K_big (halved until the launch has that many samples) up to the last whole window of K_big, which K_big / 2,
    K_big / 4 ... K_min, K_min fill, K_min behind it -- where samples x K_big stays below 2^31; else uniform blocks of 32."""
    if r.sample_block > 0 or r.taper_big <= 0 or now * r.taper_big >= 1 << 31:
        k = r.sample_block if r.sample_block > 0 else 32
        return k, k, 0, list(range(0, now, k))
    big = r.taper_big
    while big > 1 and big > now:
        big //= 2
    small = min(r.taper_min, big)
    end = now // big * big
    sizes = [big] * (end // big - 1)
    k = big // 2
    while k >= small:
        sizes.append(k)
        k //= 2
    sizes.append(small)
    assert sum(sizes) == end
    starts = [sum(sizes[:i]) for i in range(len(sizes))] + list(range(end, now, small))
    return big, small, end, [p for p in starts if p < now]


def expected(r):
    """The plan of render r: (the render's fields, one tuple per launch)."""
    # the tree's kernel and its waves per CU; fewer on a small tile (about 1.4 pixels per lane, 4 per CU at least); one-wave workgroups
    kernel, per_cu = ("Round1", r.blocks_per_cu) if not r.fits else ("FusedInstanced", min(r.blocks_per_cu, 12)) if r.two_level else ("Fused", min(r.blocks_per_cu, 16))
    fitted = min(per_cu, max(ceil_div(10 * r.n, 14 * 64 * r.n_cu), 4)) if r.blocks_auto else per_cu
    grid = min(r.n_cu * fitted, ceil_div(r.n, 64))
    slices = ceil_div(r.n, r.chunk)
    cache = bool(r.fits and r.spp > 1 and r.reuse)
    # the cost-order probe: many samples, at least 4096 slices, fewer than 4 pixels per lane; it takes precedence over the capture and over blocks
    probe = min(max(r.lpt, 1), r.spp // 4) if r.lpt and r.spp >= 16 and slices >= 4096 and r.n < 4 * 64 * grid else 0
    capture = bool(r.fits and not cache and r.full_frame and r.capture and not probe)
    want = forced = False
    # blocks: k_fused's one-level kernel, no cache, no probe, not switched off, and never on fewer waves than the 8 slice counters; `auto` where the
    # tile has 4 slices per slice in flight
    if kernel == "Fused" and not cache and not probe and r.sample_block != 0 and grid >= 8:
        forced = r.sample_block > 0 or (r.taper_big > 0 and bool(r.taper_forced))
        want = forced or slices * r.chunk >= 4 * 64 * grid
    launches, done = [], probe
    while done < r.spp:
        now = min(r.spp - done, r.max_spp)
        big, small, end, starts = schedule(now, r) if want else (0, 0, 0, [])
        blocks = len(starts) >= 2 and (forced or now >= 64) and len(starts) * slices * r.chunk < 1 << 32
        if not blocks:          # the tree's kernel; the capture in the render's first launch
            k = "Capture" if capture and done == 0 else kernel
        elif not r.one_group or (r.n_instances, r.has_spheres) != (1, 0):
            k = "Blocks"
        elif not r.primary_restart or r.seed != 2 or not r.has_records:
            k = "OneGroup"
        else:
            k = "Restart" if not r.mask_idle else "Direct" if r.primary_direct else "MaskIdle"
        tapered = blocks and end != 0
        launches.append(dict(now=now, continue_sum=int(done > 0), blocks=int(blocks), k_big=big, k_min=small, taper_end=end, passes=len(starts),
                             sample_block=big if blocks else 0, block_magic=magic(big) if blocks and not tapered else 0, block_min=small if tapered else 0,
                             block_taper_end=end if tapered else 0, block_slices=slices, block_slices_magic=magic(slices), block_chunk_magic=magic(r.chunk),
                             block_items=len(starts) * slices if blocks else 0, kernel=k, wants_table=int(k in ("Restart", "MaskIdle", "Direct")), starts=starts))
        done += now
    return dict(tree_kernel=kernel, round1=int(kernel == "Round1"), blocks_per_cu=per_cu, grid=grid, n_slices=slices, primary_cache=int(cache),
                probe_spp=probe, capture=int(capture), want_blocks=int(want), forced=int(forced and True)), launches


def table():
    """The grid of inputs: tile x samples x HRT_SAMPLE_BLOCK x HRT_SAMPLE_TAPER x HRT_FUSED_LPT x HRT_FUSED_MAX_SPP in full; over it, drawn from a
    fixed sequence, reuse, capture and full frame, the tree (levels, fits, scene, records) and the seed level; the four path knobs drawn only
    where a launch goes in blocks (nothing else reads them)."""
    rng = random.Random(32)
    rows = []
    for n, spp, sb, taper, lpt, max_spp in itertools.product(PIXELS, SPP, SAMPLE_BLOCK, TAPERS, (0, 2), (10, 512)):
        big, small, forced = TAPERS[taper]
        n_instances, has_spheres = SCENES[rng.choice(sorted(SCENES))]
        r = DEFAULT._replace(n=n, spp=spp, sample_block=sb, taper_big=big, taper_min=small, taper_forced=forced, lpt=lpt, max_spp=max_spp,
                             reuse=int(rng.random() < 0.2), capture=int(rng.random() < 0.3), full_frame=int(rng.random() < 0.5), two_level=int(rng.random() < 0.15),
                             fits=int(rng.random() < 0.9), n_instances=n_instances, has_spheres=has_spheres, has_records=int(rng.random() < 0.8), seed=rng.randrange(3))
        if any(l["blocks"] for l in expected(r)[1]):
            r = r._replace(one_group=rng.randrange(2), primary_restart=rng.randrange(2), mask_idle=rng.randrange(2), primary_direct=rng.randrange(2))
        rows.append(r)
    return rows


# The launches the GPU suite reaches through counters today: (what differs from DEFAULT; grid, slices, probe; the render's extras; per launch (now, blocks,
# K_big, K_min, taper_end or 0, passes, pass starts or None, kernel or None)).  Computed on the CPU from the arithmetic render_fused had before the plan.
K4 = dict(sample_block=4)
PINNED = [
    (dict(n=1920 * 1080, spp=256), 4096, 129600, 0, {}, [(256, 1, 64, 8, 256, 7, [0, 64, 128, 192, 224, 240, 248], "Direct")]),
    (dict(n=256 * 256, spp=64, lpt=0), 1024, 4096, 0, {}, [(64, 0)]),
    (dict(n=256 * 256, spp=64, lpt=0, sample_block=32), 1024, 4096, 0, {}, [(64, 1, 32, 32, 0, 2, [0, 32], None)]),
    (dict(n=256 * 256, spp=64, lpt=2, sample_block=32, capture=1, full_frame=1), 1024, 4096, 2, dict(capture=0), [(62, 0)]),
    (dict(n=1024 * 1024, spp=64), 4096, 65536, 0, {}, [(64, 1, 64, 8, 64, 4, [0, 32, 48, 56], None)]),
    (dict(n=1024 * 1024, spp=63), 4096, 65536, 0, {}, [(63, 0)]),
    (dict(n=8 * 6, spp=8, sample_block=2), 1, 3, 0, {}, [(8, 0)]),
    (dict(n=20 * 20, spp=24, sample_block=1), 7, 25, 0, {}, [(24, 0)]),
    (dict(n=32 * 16, spp=8, sample_block=2), 8, 32, 0, {}, [(8, 1, 2, 2, 0, 4, [0, 2, 4, 6], None)]),
    (dict(n=61 * 37, spp=8, taper_big=4, taper_min=2, taper_forced=1, lpt=0), 36, 142, 0, {}, [(8, 1, 4, 2, 8, 3, [0, 4, 6], None)]),
    (dict(n=64 * 48, spp=24, max_spp=10, **K4), 48, 192, 0, {}, [(10, 1, 4, 4, 0, 3, None, None), (10, 1, 4, 4, 0, 3, None, None), (4, 0)]),
    (dict(n=64 * 48, spp=5, reuse=1, **K4), 48, 192, 0, dict(primary_cache=1), [(5, 0)]),
    (dict(n=96 * 64, spp=8, sample_block=3, two_level=1), 96, 384, 0, dict(tree_kernel="FusedInstanced"), [(8, 0)]),
]
PINNED_ROWS = [DEFAULT._replace(starts=1, **p[0]) for p in PINNED]

PROGRAM = r"""
#include <hip/hip_runtime.h>
#include <cstdio>
#include "path_plan.h"
using namespace hrt;
static HitGroup hg; static uint32_t word; static float4 tuvp;
int main(int argc, char **argv) {
    std::FILE *f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int v[26];
    for (;;) {
        for (int i = 0; i < 26; ++i) if (std::fscanf(f, "%d", &v[i]) != 1) return i == 0 ? 0 : 3;
        RenderPlanInput in{};
        in.n_cu = v[0]; in.fits_fused = v[1]; in.two_level = v[2]; in.n_instances = (uint32_t)v[3]; in.has_spheres = v[4]; in.has_records = v[5];
        in.n = (uint32_t)v[6]; in.full_frame = v[7]; in.spp = (uint32_t)v[8]; in.reuse_primary = v[9]; in.capture_primary = v[10];
        in.fused_blocks_per_cu = v[11]; in.traverse_blocks_auto = v[12]; in.fused_fetch_chunk = v[13];
        in.fused_lpt = v[14]; in.sample_block = v[15]; in.taper_big = v[16]; in.taper_min = v[17]; in.taper_forced = v[18];
        in.fused_max_spp = v[19]; in.seed_primary = v[20]; in.knobs = PathKnobs{v[21] != 0, v[22] != 0, v[23] != 0, v[24] != 0};
        const RenderPlan r = plan_fused_render(in);
        std::printf("R %d %d %u %u %u %d %u %d %d %d\n", (int)r.tree_kernel, (int)r.round1, r.blocks_per_cu, r.grid, r.n_slices, (int)r.primary_cache, r.probe_spp,
                    (int)r.capture, (int)r.want_blocks, (int)r.forced);
        for (uint32_t done = r.probe_spp; done < in.spp;) {
            const LaunchPlan l = plan_fused_launch(r, in, done);
            // the arguments as render_fused fills them from the plan: the tables, the seed level, the cache, the probe's order, the block fields, the capture's arrays
            TraverseArgs a{}; a.seed_primary = in.seed_primary; a.fetch_chunk = (uint32_t)in.fused_fetch_chunk;
            PathArgs &p = a.path; p.hitgroups = &hg; p.inst_program = &word; p.spp = l.now; p.continue_sum = l.continue_sum;
            if (r.primary_cache) p.primary_cache = &tuvp;
            if (r.probe_spp) p.slice_order = &word;
            p.sample_block = l.sample_block; p.block_magic = l.block_magic; p.block_min = l.block_min; p.block_taper_end = l.block_taper_end;
            p.block_slices = l.block_slices; p.block_slices_magic = l.block_slices_magic; p.block_chunk_magic = l.block_chunk_magic; p.block_items = l.block_items;
            p.block_progress = l.blocks ? &word : nullptr;
            if (l.kernel == PathKernel::Capture) { p.trace_tuvp = &tuvp; p.trace_inst = &word; }
            const PathScene scene{!in.two_level, in.n_instances, in.has_spheres, l.wants_table ? &word : nullptr};      // (the table: made where the launch wants it)
            std::printf("L %u %u %d %u %u %u %u %u %u %u %u %u %u %u %u %d %d %d", l.now, l.continue_sum, (int)l.blocks, l.sc.k_big, l.sc.k_min, l.sc.tapered ? l.sc.taper_end : 0u, l.sc.passes,
                        l.sample_block, l.block_magic, l.block_min, l.block_taper_end, l.block_slices, l.block_slices_magic, l.block_chunk_magic, l.block_items,
                        (int)l.kernel, (int)l.wants_table, (int)path_launch_admitted(l.kernel, a, scene, r.grid));
            if (v[25]) for (uint32_t b = 0; b < l.sc.passes; ++b) std::printf(" %u", schedule_first(l.sc, b));
            std::printf("\n");
            done += l.now;
        }
    }
}
"""
RENDER_FIELDS = ("tree_kernel", "round1", "blocks_per_cu", "grid", "n_slices", "primary_cache", "probe_spp", "capture", "want_blocks", "forced")
LAUNCH_FIELDS = ("now", "continue_sum", "blocks", "k_big", "k_min", "taper_end", "passes", "sample_block", "block_magic", "block_min", "block_taper_end",
                 "block_slices", "block_slices_magic", "block_chunk_magic", "block_items", "kernel", "wants_table", "admitted")


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """[(row, the render's plan, its launches' plans)] for the table's rows, then the pinned ones"""
    tmp = tmp_path_factory.mktemp("render_plan")
    src, exe, inp = tmp / "plan.cpp", tmp / "plan", tmp / "rows.txt"
    rows = table() + PINNED_ROWS
    src.write_text(PROGRAM)
    inp.write_text("".join(" ".join(str(int(x)) for x in r) + "\n" for r in rows))
    # the host's compiler and the HIP headers, exactly as for device_types.h alone (test_path_launch_cpu.py)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{ROOT / 'include'}", f"-I{CSRC}", "-o", str(exe), str(src)])
    out, got = subprocess.run([str(exe), str(inp)], capture_output=True, text=True, check=True).stdout.splitlines(), []
    for line in out:
        tag, *nums = line.split()
        nums = [int(x) for x in nums]
        if tag == "R":
            render = dict(zip(RENDER_FIELDS, nums))
            render["tree_kernel"] = KERNELS[render["tree_kernel"]]
            got.append((render, []))
        else:
            launch = dict(zip(LAUNCH_FIELDS, nums), starts=nums[len(LAUNCH_FIELDS):])
            launch["kernel"] = KERNELS[launch["kernel"]]
            got[-1][1].append(launch)
    assert len(got) == len(rows)
    return [(r, render, launches) for r, (render, launches) in zip(rows, got)]


def test_the_table_reaches_every_axis_value():
    rows = table()
    assert 10000 <= len(rows) <= 40000, len(rows)
    for field, values in (("n", PIXELS), ("spp", SPP), ("sample_block", SAMPLE_BLOCK), ("lpt", (0, 2)), ("max_spp", (10, 512)), ("reuse", (0, 1)),
                          ("two_level", (0, 1)), ("fits", (0, 1)), ("has_records", (0, 1)), ("seed", (0, 1, 2))):
        assert {getattr(r, field) for r in rows} == set(values), field
    assert {(r.taper_big, r.taper_min, r.taper_forced) for r in rows} == set(TAPERS.values())
    assert {(r.capture, r.full_frame) for r in rows} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {(r.n_instances, r.has_spheres) for r in rows} == set(SCENES.values())
    in_blocks = [any(l["blocks"] for l in expected(r)[1]) for r in rows]
    for knob in ("one_group", "primary_restart", "mask_idle", "primary_direct"):
        assert {getattr(r, knob) for r, b in zip(rows, in_blocks) if b} == {0, 1}, knob
        assert all(getattr(r, knob) == 1 for r, b in zip(rows, in_blocks) if not b), knob


def test_the_plan_is_the_gates_restated(plans):
    wrong = []
    for r, render, launches in plans:
        want_render, want_launches = expected(r)
        if render != want_render:
            wrong.append((r, render, want_render))
        elif [{k: v for k, v in l.items() if k not in ("admitted", "starts")} for l in launches] != [{k: v for k, v in l.items() if k != "starts"} for l in want_launches]:
            wrong.append((r, launches, want_launches))
        elif r.starts and [l["starts"] for l in launches] != [l["starts"] for l in want_launches]:
            wrong.append((r, launches, want_launches))
    assert not wrong, (len(wrong), wrong[:3])
    chosen = {l["kernel"] for _, _, launches in plans for l in launches}
    print(f"{len(plans)} renders, {sum(len(l) for _, _, l in plans)} launches; kernels:", sorted(chosen))
    assert chosen == set(KERNELS) - {"Counts"}          # (hrt_render_accumulate names its kernel itself)


def test_every_render_keeps_the_plans_properties(plans):
    for r, render, launches in plans:
        what = (r, render, launches)
        assert sum(l["now"] for l in launches) == r.spp - render["probe_spp"], what
        for i, l in enumerate(launches):
            assert (l["continue_sum"] == 0) == (i == 0 and render["probe_spp"] == 0), what
            if l["blocks"]:
                assert render["grid"] >= 8 and not render["primary_cache"] and not render["probe_spp"] and render["tree_kernel"] == "Fused", what
                assert l["passes"] >= 2 and l["block_items"] == l["passes"] * render["n_slices"] and l["passes"] * render["n_slices"] * r.chunk < 1 << 32, what
                assert l["kernel"] in ("Blocks", "OneGroup", "Restart", "MaskIdle", "Direct"), what
            assert l["admitted"] == 1, what
            if l["kernel"] == "Capture":
                assert i == 0 and not l["blocks"] and not render["probe_spp"], what


@pytest.mark.parametrize("case", range(len(PINNED)))
def test_the_launches_the_gpu_suite_counts(plans, case):
    changes, grid, slices, probe, extras, want_launches = PINNED[case]
    r, render, launches = plans[len(plans) - len(PINNED) + case]
    assert r == PINNED_ROWS[case]
    assert (render["grid"], render["n_slices"], render["probe_spp"]) == (grid, slices, probe), render
    for field, value in dict(dict(tree_kernel="Fused", primary_cache=0, capture=0), **extras).items():
        assert render[field] == value, (field, render)
    assert len(launches) == len(want_launches), launches
    for l, want in zip(launches, want_launches):
        assert (l["now"], l["blocks"]) == want[:2] and l["admitted"] == 1, l
        if l["blocks"]:
            assert (l["k_big"], l["k_min"], l["taper_end"], l["passes"]) == want[2:6], l
            assert want[6] is None or l["starts"] == want[6], l
            assert want[7] is None or (l["kernel"] == want[7] and l["wants_table"] == 1), l
        else:
            assert l["kernel"] == render["tree_kernel"], l
