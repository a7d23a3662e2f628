"""The path kernels' one launch entry, as plain host code (device_types.h): the admission rule (path_launch_admitted, which launch_path_kernel
calls before it launches anything) -- for every kernel one launch that is admitted, and every single contradiction of what that kernel is
compiled to take for granted, refused -- and the choice of a launch's kernel (choose_path_launch, which the render's plan calls: path_plan.h,
tests/test_render_plan_cpu.py), over every combination of what decides it.  A stand-alone program built against device_types.h calls both over the tables below and prints the
verdicts -- no device is opened, nothing is launched, nothing is loaded into this process."""
import itertools
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "nvidia-optix-ray-tracer_amd" / "csrc"

# The admitted launch of each kernel: (scene = one_level, n_instances, has_spheres, leaf_parent; statements on the TraverseArgs `a`).
# Every launch has the material tables and a grid of 8 waves; the block kernels have a block size, a uniform schedule of it (block_magic = 2^32 / 32),
# the slices' progress words and items to hand out; the restart and the kernels built on it have the table and the window; the counts launch
# has the caller's sums and the samples they hold.
TABLES = "a.path.hitgroups = &hg; a.path.inst_program = &word;"
IN_BLOCKS = TABLES + " a.path.sample_block = 32u; a.path.block_magic = 0x08000000u; a.path.block_progress = &word; a.path.block_items = 2u;"
RESTART = ("{true, 1u, false, &word}", IN_BLOCKS + " a.seed_primary = 2;")
BASE = {
    "Fused":          ("{true, 3u, true, nullptr}", TABLES),
    "FusedInstanced": ("{false, 3u, true, nullptr}", TABLES),
    "Capture":        ("{true, 3u, true, nullptr}", TABLES + " a.path.trace_tuvp = &tuvp; a.path.trace_inst = &word;"),
    "Blocks":         ("{true, 3u, true, nullptr}", IN_BLOCKS),
    "OneGroup":       ("{true, 1u, false, nullptr}", IN_BLOCKS),
    "Restart":        RESTART,
    "Round1":         ("{true, 3u, true, nullptr}", TABLES),
    "Counts":         ("{true, 3u, true, nullptr}", TABLES + " a.path.spp = 4u; a.path.accum = &sum; a.path.trace_inst = &word;"),
    "MaskIdle":       RESTART,          # (the same launch as Restart's, and as each other's: the kernel alone differs)
    "Direct":         RESTART,
}
RESTART_KERNELS = ("Restart", "MaskIdle", "Direct")
ONE_GROUP_KERNELS = ("OneGroup",) + RESTART_KERNELS
BLOCK_KERNELS = ("Blocks",) + ONE_GROUP_KERNELS

# (kernel, what is changed about its admitted launch: statements on `a` and `scene`, admitted?)
CASES = [(k, "", True) for k in BASE]
# a launch in blocks: a block size, and none of what the block kernels' regeneration does not look at
CASES += [(k, "a.path.sample_block = 0u;", False) for k in BLOCK_KERNELS]
CASES += [(k, "a.path.trace_rays = &ray;", False) for k in BLOCK_KERNELS]
CASES += [(k, "a.path.slice_cost = &word;", False) for k in BLOCK_KERNELS]
CASES += [(k, "a.path.slice_order = &word;", False) for k in BLOCK_KERNELS]
# ... on a grid that gives every one of the 8 slice counters a wave whose home it is (fewer: the launch could wait for ever), with the hand-over's
# memory, and with a schedule that is purely uniform or purely tapered (powers of two, the halvings' end not in front of the first block)
TAPERED = "a.path.block_magic = 0u; a.path.block_min = 8u; a.path.block_taper_end = 64u;"
CASES += [(k, change, ok) for k in BLOCK_KERNELS for change, ok in
          [("grid = 7u;", False), ("grid = 0u;", False), ("grid = 8u;", True), ("grid = 4096u;", True),
           ("a.path.block_progress = nullptr;", False), ("a.path.block_items = 0u;", False),
           ("a.path.block_min = 8u;", False), ("a.path.block_taper_end = 64u;", False), ("a.path.block_magic = 0u;", False),        # mixed; mixed; neither
           (TAPERED, True), (TAPERED + " a.path.block_taper_end = 32u;", True), (TAPERED + " a.path.block_min = 32u;", True),
           (TAPERED + " a.path.block_taper_end = 31u;", False), (TAPERED + " a.path.block_min = 0u;", False), (TAPERED + " a.path.block_min = 6u;", False),
           (TAPERED + " a.path.sample_block = 48u; a.path.block_taper_end = 96u;", False)]]
# one hit group: a one-level tree of triangles over exactly one instance, whose table entries exist
CASES += [(k, "scene.n_instances = 2u;", False) for k in ONE_GROUP_KERNELS]
CASES += [(k, "scene.has_spheres = true;", False) for k in ONE_GROUP_KERNELS]
CASES += [(k, "scene.one_level = false;", False) for k in ONE_GROUP_KERNELS]
CASES += [(k, "a.path.hitgroups = nullptr;", False) for k in ONE_GROUP_KERNELS]
CASES += [(k, "a.path.inst_program = nullptr;", False) for k in ONE_GROUP_KERNELS]
# the restart, and k_path_idle and k_path_direct with it: the table, and the window (HRT_SEED_PRIMARY=2)
CASES += [(k, change, False) for k in RESTART_KERNELS for change in ("scene.leaf_parent = nullptr;", "a.seed_primary = 1;", "a.seed_primary = 0;")]
# the kernels without sample blocks: the caller names the block kernel it wants, nothing forwards
CASES += [(k, "a.path.sample_block = 32u;", False) for k in ("Fused", "FusedInstanced", "Capture")]
# the capture: trace_tuvp / trace_inst are its arrays, so no callers' rays; no primary-hit cache
CASES += [("Capture", "a.path.trace_rays = &ray;", False), ("Capture", "a.path.primary_cache = &tuvp;", False)]
# a kernel is compiled for the levels of its tree
CASES += [("Fused", "scene.one_level = false;", False), ("FusedInstanced", "scene.one_level = true;", False), ("Blocks", "scene.one_level = false;", False)]
# ... and what is none of a kernel's business stays admitted: hrt_trace_rays, the primary-hit cache, the cost probe and its order on k_fused;
# both kinds of tree with the capture; any scene in blocks; anything on round 1's kernel
CASES += [("Fused", s, True) for s in ("a.path.trace_rays = &ray;", "a.path.primary_cache = &tuvp;", "a.path.slice_cost = &word;", "a.path.slice_order = &word;",
                                       "scene.n_instances = 1u; scene.has_spheres = false;", "a.seed_primary = 0;")]
CASES += [("FusedInstanced", "a.path.trace_rays = &ray;", True), ("Capture", "scene.one_level = false;", True)]
CASES += [("Blocks", "scene.n_instances = 1u; scene.has_spheres = false;", True), ("Blocks", "a.seed_primary = 0;", True), ("OneGroup", "a.seed_primary = 0;", True)]
CASES += [("Round1", "a.path.trace_rays = &ray; a.path.slice_order = &word; scene.one_level = false;", True)]
# the counts launch (hrt_render_accumulate): slice_order carries the counts or NULL, any tree, any seed level; the caller's sums, the samples
# they hold and a sample count; no sample blocks, no callers' rays, no primary-hit cache, no cost probe
CASES += [("Counts", change, ok) for change, ok in
          [("a.path.slice_order = &word;", True), ("scene.one_level = false;", True), ("scene.n_instances = 1u; scene.has_spheres = false;", True),
           ("a.seed_primary = 0;", True),
           ("a.path.accum = nullptr;", False), ("a.path.trace_inst = nullptr;", False), ("a.path.spp = 0u;", False),
           ("a.path.sample_block = 32u;", False), ("a.path.trace_rays = &ray;", False), ("a.path.primary_cache = &sum;", False),
           ("a.path.slice_cost = &word;", False)]]

# The choice, exhaustively, in the order the program's loops run: what render_fused has decided by the time it launches.  `blocks` goes with
# Fused alone: render_fused cuts no other tree's launch into sample blocks.
TREE_KERNELS = ("Fused", "FusedInstanced", "Round1")
SCENES = ("one instance of triangles", "two instances", "with spheres")
CHOICES = [c for c in itertools.product(TREE_KERNELS, (0, 1), (0, 1), (0, 64), (0, 1, 2), (0, 1), (0, 1), (0, 1), (0, 1), SCENES, (False, True))
           if not c[2] or c[0] == "Fused"]          # (tree_kernel, capture, blocks, done_spp, seed_primary, one_group, primary_restart, mask_idle, primary_direct, scene, table)


def expected_kernel(tree_kernel, capture, blocks, done_spp, seed_primary, one_group, primary_restart, mask_idle, primary_direct, scene, table):
    """The ladder as DESIGN.md section 2.1 tells it, written down here and not read from the C++."""
    if not blocks:          # the tree's kernel; the capture in the render's first launch, and only outside blocks
        return "Capture" if capture and done_spp == 0 else tree_kernel
    if not one_group or scene != "one instance of triangles":
        return "Blocks"
    if not primary_restart or seed_primary != 2 or not table:          # (a tree without records has no table: k_path_one)
        return "OneGroup"
    if not mask_idle:
        return "Restart"
    return "Direct" if primary_direct else "MaskIdle"


PROGRAM = r"""
#include <hip/hip_runtime.h>
#include <cstdio>
#include "device_types.h"
using namespace hrt;
static HitGroup hg; static uint32_t word; static float4 tuvp, sum; static RayRec ray;
int main() {
%s
    // the choice: a line "kernel admitted" per combination, the TraverseArgs as render_fused builds them for that launch
    const PathKernel trees[] = {PathKernel::Fused, PathKernel::FusedInstanced, PathKernel::Round1};
    const PathScene scenes[] = {{true, 1u, false, nullptr}, {true, 2u, false, nullptr}, {true, 1u, true, nullptr}};
    for (int tree = 0; tree < 3; ++tree) for (int capture = 0; capture < 2; ++capture) for (int blocks = 0; blocks < 2; ++blocks)
    for (uint32_t done_spp = 0u; done_spp <= 64u; done_spp += 64u) for (int seed = 0; seed < 3; ++seed) for (int knob = 0; knob < 16; ++knob)
    for (int sc = 0; sc < 3; ++sc) for (int table = 0; table < 2; ++table) {
        if (blocks && tree != 0) continue;
        PathScene scene = scenes[sc]; scene.one_level = trees[tree] != PathKernel::FusedInstanced; scene.leaf_parent = table ? &word : nullptr;
        const PathKnobs knobs{(knob & 8) != 0, (knob & 4) != 0, (knob & 2) != 0, (knob & 1) != 0};
        const PathKernel kernel = choose_path_launch(trees[tree], capture != 0, blocks != 0, done_spp, seed, knobs, scene, table != 0);
        TraverseArgs a{}; a.path.hitgroups = &hg; a.path.inst_program = &word; a.seed_primary = seed;
        a.path.sample_block = blocks ? 32u : 0u;        // (a launch in blocks has no callers' rays, cost probe or slice order; it has a schedule and the hand-over's memory)
        if (blocks) { a.path.block_magic = 0x08000000u; a.path.block_progress = &word; a.path.block_items = 2u; }
        if (kernel == PathKernel::Capture) { a.path.trace_tuvp = &tuvp; a.path.trace_inst = &word; }
        std::printf("%%d %%d\n", (int)kernel, (int)path_launch_admitted(kernel, a, scene, 8u));
    }
    return 0;
}
"""
CASE = '    { TraverseArgs a{}; PathScene scene%s; uint32_t grid = 8u; %s %s std::printf("%%d\\n", (int)path_launch_admitted(PathKernel::%s, a, scene, grid)); }'


def enumerators():
    """every identifier of enum class PathKernel, whatever its layout"""
    body = (CSRC / "device_types.h").read_text().split("enum class PathKernel {")[1].split("};")[0]
    return re.findall(r"[A-Za-z_]\w*", re.sub(r"//[^\n]*|/\*.*?\*/", "", body, flags=re.S))


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    """(the admission verdicts of CASES, the (kernel, admitted) of CHOICES)"""
    tmp = tmp_path_factory.mktemp("path_launch")
    src, exe = tmp / "admitted.cpp", tmp / "admitted"
    src.write_text(PROGRAM % "\n".join(CASE % (BASE[k][0], BASE[k][1], change, k) for k, change, _ in CASES))
    # the host's compiler and the HIP headers: device_types.h needs their types, the program none of the runtime
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{ROOT / 'include'}", f"-I{CSRC}", "-o", str(exe), str(src)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(CASES) + len(CHOICES)
    names = enumerators()
    return [v == "1" for v in out[:len(CASES)]], [(names[int(l.split()[0])], l.split()[1] == "1") for l in out[len(CASES):]]


def test_every_kernel_has_an_admitted_launch_and_its_contradictions(output):
    named = enumerators()
    assert len(named) == 10 and named == list(BASE), named                        # the table knows every kernel there is
    for k in BASE:
        assert any(kk == k and ok for kk, _, ok in CASES) and (k == "Round1" or any(kk == k and not ok for kk, _, ok in CASES)), k


def test_the_verdicts_are_the_table(output):
    wrong = [(k, change, want, got) for (k, change, want), got in zip(CASES, output[0]) if want != got]
    assert not wrong, wrong


def test_the_counts_launch_is_admitted_and_its_contradictions_are_refused(output):
    got = [(change, want, ok) for (k, change, want), ok in zip(CASES, output[0]) if k == "Counts"]
    assert len(got) == 12 and all(want == ok for _, want, ok in got), got
    assert "case PathKernel::Counts: launch_path_counts(a, scene, grid_blocks, s); break;" in (CSRC / "fused.hip").read_text()


def test_the_entry_admits_for_mask_idle_and_direct_what_it_admits_for_restart(output):
    got = {k: [(change, ok) for (kk, change, _), ok in zip(CASES, output[0]) if kk == k] for k in RESTART_KERNELS}
    # the admitted launch, no table, seed_primary 0 and 1, callers' rays, a second instance -- and the rest of Restart's
    for needle in ("", "scene.leaf_parent = nullptr;", "a.seed_primary = 0;", "a.seed_primary = 1;", "a.path.trace_rays = &ray;", "scene.n_instances = 2u;"):
        assert any(change == needle for change, _ in got["Restart"]), needle
    assert got["MaskIdle"] == got["Direct"] == got["Restart"] == [(change, ok) for k, change, ok in CASES if k == "Restart"]


def test_the_chosen_kernel_is_the_ladders_and_is_admitted(output):
    """(a) what choose_path_launch returns is what the ladder above says; (b) path_launch_admitted admits it."""
    chosen = output[1]
    print(f"{len(CHOICES)} combinations; chosen:", {k: sum(c == k for c, _ in chosen) for k in BASE})
    assert len(CHOICES) == 4608
    wrong = [(c, expected_kernel(*c), got) for c, (got, _) in zip(CHOICES, chosen) if expected_kernel(*c) != got]
    assert not wrong, wrong[:8]
    refused = [(c, got) for c, (got, ok) in zip(CHOICES, chosen) if not ok]
    assert not refused, refused[:8]
    assert {c for c, _ in chosen} == set(BASE) - {"Counts"}          # (hrt_render_accumulate names its kernel itself)
    # the knob settings of tests/test_primary_direct_gpu.py::test_the_gate, a launch in blocks of a render with the window and the table:
    # (HRT_ONE_GROUP, HRT_PRIMARY_RESTART, HRT_MASK_IDLE, HRT_PRIMARY_DIRECT), HRT_SEED_PRIMARY, the scene
    one = "one instance of triangles"
    by_case = dict(zip(CHOICES, (k for k, _ in chosen)))
    for knobs, seed, scene, want in (((1, 1, 1, 1), 2, "two instances", "Blocks"), ((0, 1, 1, 1), 2, one, "Blocks"), ((1, 1, 1, 1), 1, one, "OneGroup"),
                                     ((1, 0, 1, 1), 2, one, "OneGroup"), ((1, 1, 0, 1), 2, one, "Restart"), ((1, 1, 1, 0), 2, one, "MaskIdle"),
                                     ((1, 1, 1, 1), 2, one, "Direct")):
        assert by_case[("Fused", 0, 1, 0, seed) + knobs + (scene, True)] == want, (knobs, seed, scene)
    # the capture: only when done_spp == 0, and not in blocks
    for tree in TREE_KERNELS:
        assert by_case[(tree, 1, 0, 0, 2, 1, 1, 1, 1, one, True)] == "Capture" and by_case[(tree, 1, 0, 64, 2, 1, 1, 1, 1, one, True)] == tree
    assert by_case[("Fused", 1, 1, 0, 2, 1, 1, 1, 1, one, True)] == "Direct"


def test_the_rule_is_written_once():
    """One entry, one rule, one choice: the translation units neither declare launch functions of their own by hand nor repeat either."""
    for path in sorted(CSRC.glob("*.hip")) + sorted(CSRC.glob("*.cpp")):
        text = path.read_text()
        assert "blocks_launch_admitted" not in text and "launch_fused" not in text.replace("launch_fused_as", "") and "launch_paths_v1" not in text, path.name
        assert ("path_launch_admitted(" in text) == (path.name == "fused.hip"), path.name          # called by the entry, and only there
        assert "choose_path_launch(" not in text, path.name          # called by the render's plan (below), and only there
    assert (CSRC / "path_plan.h").read_text().count("choose_path_launch(") == 1
    header = (CSRC / "device_types.h").read_text()
    assert header.count("bool launch_path_kernel(") == 1 and header.count("inline bool path_launch_admitted(") == 1 and header.count("inline PathKernel choose_path_launch(") == 1
