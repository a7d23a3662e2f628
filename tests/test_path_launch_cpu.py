"""The admission rule of the path kernels' one launch entry (device_types.h: path_launch_admitted, which launch_path_kernel calls before it
launches anything): for every kernel one launch that is admitted, and every single contradiction of what that kernel is compiled to
take for granted, refused.  The rule is plain host code: a stand-alone program built against device_types.h calls it over the table
below and prints the verdicts -- no device is opened, nothing is launched, nothing is loaded into this process."""
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "nvidia-optix-ray-tracer_amd" / "csrc"

# The admitted launch of each kernel: (scene = one_level, n_instances, has_spheres, leaf_parent; statements on the TraverseArgs `a`).
# Every launch has the material tables; the block kernels have a block size; the restart has its table and the window.
TABLES = "a.path.hitgroups = &hg; a.path.inst_program = &word;"
BASE = {
    "Fused":          ("{true, 3u, true, nullptr}", TABLES),
    "FusedInstanced": ("{false, 3u, true, nullptr}", TABLES),
    "Capture":        ("{true, 3u, true, nullptr}", TABLES + " a.path.trace_tuvp = &tuvp; a.path.trace_inst = &word;"),
    "Blocks":         ("{true, 3u, true, nullptr}", TABLES + " a.path.sample_block = 32u;"),
    "OneGroup":       ("{true, 1u, false, nullptr}", TABLES + " a.path.sample_block = 32u;"),
    "Restart":        ("{true, 1u, false, &word}", TABLES + " a.path.sample_block = 32u; a.seed_primary = 2;"),
    "Round1":         ("{true, 3u, true, nullptr}", TABLES),
}
BLOCK_KERNELS = ("Blocks", "OneGroup", "Restart")
ONE_GROUP_KERNELS = ("OneGroup", "Restart")

# (kernel, what is changed about its admitted launch: statements on `a` and `scene`, admitted?)
CASES = [(k, "", True) for k in BASE]
# a launch in blocks: a block size, and none of what the block kernels' regeneration does not look at
CASES += [(k, "a.path.sample_block = 0u;", False) for k in BLOCK_KERNELS]
CASES += [(k, "a.path.trace_rays = &ray;", False) for k in BLOCK_KERNELS]
CASES += [(k, "a.path.slice_cost = &word;", False) for k in BLOCK_KERNELS]
CASES += [(k, "a.path.slice_order = &word;", False) for k in BLOCK_KERNELS]
# one hit group: a one-level tree of triangles over exactly one instance, whose table entries exist
CASES += [(k, "scene.n_instances = 2u;", False) for k in ONE_GROUP_KERNELS]
CASES += [(k, "scene.has_spheres = true;", False) for k in ONE_GROUP_KERNELS]
CASES += [(k, "scene.one_level = false;", False) for k in ONE_GROUP_KERNELS]
CASES += [(k, "a.path.hitgroups = nullptr;", False) for k in ONE_GROUP_KERNELS]
CASES += [(k, "a.path.inst_program = nullptr;", False) for k in ONE_GROUP_KERNELS]
# the restart: the table, and the window (HRT_SEED_PRIMARY=2)
CASES += [("Restart", "scene.leaf_parent = nullptr;", False), ("Restart", "a.seed_primary = 1;", False), ("Restart", "a.seed_primary = 0;", False)]
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

PROGRAM = r"""
#include <hip/hip_runtime.h>
#include <cstdio>
#include "device_types.h"
using namespace hrt;
static HitGroup hg; static uint32_t word; static float4 tuvp; static RayRec ray;
int main() {
%s
    return 0;
}
"""
CASE = '    { TraverseArgs a{}; PathScene scene%s; %s %s std::printf("%%d\\n", (int)path_launch_admitted(PathKernel::%s, a, scene)); }'


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("path_launch")
    src, exe = tmp / "admitted.cpp", tmp / "admitted"
    src.write_text(PROGRAM % "\n".join(CASE % (BASE[k][0], BASE[k][1], change, k) for k, change, _ in CASES))
    # the host's compiler and the HIP headers: device_types.h needs their types, the program none of the runtime
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{ROOT / 'include'}", f"-I{CSRC}", "-o", str(exe), str(src)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert len(out) == len(CASES)
    return [v == "1" for v in out]


def test_every_kernel_has_an_admitted_launch_and_its_contradictions(verdicts):
    kernels = (CSRC / "device_types.h").read_text().split("enum class PathKernel {")[1].split("};")[0]
    named = re.findall(r"(\w+),", re.sub(r"//.*", "", kernels))
    assert named == list(BASE), named                        # the table knows every kernel there is
    for k in BASE:
        assert any(kk == k and ok for kk, _, ok in CASES) and (k == "Round1" or any(kk == k and not ok for kk, _, ok in CASES)), k


def test_the_verdicts_are_the_table(verdicts):
    wrong = [(k, change, want, got) for (k, change, want), got in zip(CASES, verdicts) if want != got]
    assert not wrong, wrong


def test_the_rule_is_written_once():
    """One entry, one rule: the translation units neither declare launch functions of their own by hand nor repeat the rule."""
    for path in sorted(CSRC.glob("*.hip")) + sorted(CSRC.glob("*.cpp")):
        text = path.read_text()
        assert "blocks_launch_admitted" not in text and "launch_fused" not in text.replace("launch_fused_as", "") and "launch_paths_v1" not in text, path.name
        assert ("path_launch_admitted(" in text) == (path.name == "fused.hip"), path.name          # called by the entry, and only there
    header = (CSRC / "device_types.h").read_text()
    assert header.count("bool launch_path_kernel(") == 1 and header.count("inline bool path_launch_admitted(") == 1
