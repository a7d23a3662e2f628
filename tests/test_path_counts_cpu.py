"""k_path_counts (csrc/fused_counts.hip: the path kernel of hrt_render_accumulate, every pixel with a sample count of its own) as compiled, read
from the assembly the Makefile's flags produce as tests/test_path_kernel_spills_cpu.py reads the other path kernels (tools/loop_stats.py),
compiled once for the module -- and the admission rule of its launch (device_types.h: path_launch_admitted), from a stand-alone host
program as in tests/test_path_launch_cpu.py, whose table lists the kernels that came before this one."""
import re
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = "nvidia-optix-ray-tracer_amd/csrc/"


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """{mangled kernel name: {"loop": Counter of kinds, "ops": Counter of the loop's opcodes, "body": [lines], "meta": {key: int}, "args": [...]}}"""
    sys.path.insert(0, str(ROOT / "tools"))
    import loop_stats
    tmp = tmp_path_factory.mktemp("path_counts")
    out = {}
    for stem, prefix in (("fused", "_ZN3hrt7k_fused"), ("fused_counts", "_ZN3hrt13k_path_counts")):
        asm = tmp / f"{stem}.s"
        loops = {name: (cs, ops) for name, cs, ops in loop_stats.loops(CSRC + f"{stem}.hip", prefix, asm=asm)}
        text = asm.read_text()
        bodies = {m.group(1): m.group(2).split("\n") for m in re.finditer(r"^(" + prefix + r"\w+):[^\n]*\n(.*?)s_endpgm", text, re.S | re.M)}
        for entry in text.split("amdhsa.kernels:")[1].split("\n  - .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", entry).group(1)
            if name not in bodies:
                continue
            meta = {k: int(v) for k, v in re.findall(r"^    \.(\w+):\s+(\d+)\s*$", entry, re.M)}
            args = re.findall(r"- \.offset:\s+(\d+)\n\s+\.size:\s+(\d+)\n\s+\.value_kind:\s+(\w+)", entry)
            out[name] = {"loop": loops[name][0], "ops": loops[name][1], "body": bodies[name], "meta": meta, "args": args}
    return out


def _counts(compiled):
    return {k: v for k, v in compiled.items() if "k_path_counts" in k}


def _opcodes(lines):
    import loop_stats
    return [op for op, _ in loop_stats.instructions(lines)]


def test_four_kernels_whose_only_argument_is_the_traverse_args(compiled):
    """<HAS_SPHERES, INSTANCED>: four instantiations, the by-value TraverseArgs at offset 0 their one explicit argument (fused_body.h:
    kernarg_traverse_args reads the regeneration's constants from there)."""
    counts = _counts(compiled)
    assert sorted(re.search(r"ILb(\d)ELb(\d)E", k).groups() for k in counts) == [("0", "0"), ("0", "1"), ("1", "0"), ("1", "1")], sorted(counts)
    for name, k in counts.items():
        explicit = [a for a in k["args"] if not a[2].startswith("hidden_")]
        assert len(explicit) == 1 and explicit[0][0] == "0" and explicit[0][2] == "by_value", (name, k["args"])


def test_the_loop_touches_no_scratch_and_nothing_is_a_flat_access(compiled):
    for name, k in _counts(compiled).items():
        assert not any(op.startswith("scratch_") or op.startswith("buffer_") for op in k["ops"]), (name, sorted(k["ops"]))
        ops = _opcodes(k["body"])
        assert not any(op.startswith("flat_") for op in ops), (name, sorted({op for op in ops if op.startswith("flat_")}))
        assert any(op.startswith("s_load_dword") for op in ops)


def test_the_one_level_kernels_keep_four_waves_per_simd(compiled):
    for name, k in _counts(compiled).items():
        if re.search(r"ILb\dELb0E", name):
            assert k["meta"]["vgpr_count"] <= 128, (name, k["meta"])


def test_the_loop_is_k_fuseds_within_the_block_kernels_allowance(compiled):
    """k_path_counts<false, false> against k_fused<false, false, false>: no more than 4 instructions on top, what k_path_blocks is allowed."""
    counts = [v for k, v in compiled.items() if "k_path_countsILb0ELb0E" in k]
    fused = [v for k, v in compiled.items() if "k_fusedILb0ELb0ELb0E" in k]
    assert len(counts) == 1 and len(fused) == 1
    assert sum(counts[0]["loop"].values()) <= sum(fused[0]["loop"].values()) + 4, (dict(counts[0]["loop"]), dict(fused[0]["loop"]))


def test_hand_issued_loads_are_not_touched_before_their_wait():
    sys.path.insert(0, str(ROOT / "tools"))
    import audit_asm_loads
    groups, bad = audit_asm_loads.audit(CSRC + "fused_counts.hip", "_ZN3hrt13k_path_counts")
    assert groups > 0 and bad == 0, (groups, bad)


def test_the_variant_is_the_plain_kernel_plus_the_counts_and_the_others_do_not_know_it():
    body = (ROOT / CSRC / "fused_counts.hip").read_text()
    variant = re.search(r"struct CountsVariant : (\w+<\w+>) \{([^}]*)\}", body)
    assert variant and variant.group(1) == "FusedBodyVariant<false>"
    assert re.sub(r"\s+", " ", variant.group(2)).strip() == "static constexpr bool kSpheres = HAS_SPHERES, kInstanced = INSTANCED, kCounts = true;"
    for stem in ("fused", "fused_blocks", "fused_one", "fused_restart", "fused_capture", "fused_queue", "kernels"):
        text = (ROOT / CSRC / f"{stem}.hip").read_text()
        assert "kCounts" not in text and "CountsLane" not in text, stem
        assert "k_path_counts" not in text or stem == "kernels", stem          # (kernels.hip has the launch's finalize kernel, which names it)


# ---- the admission rule: (statements on the admitted launch, admitted?) ----
ADMITTED = "a.path.hitgroups = &hg; a.path.inst_program = &word; a.path.spp = 4u; a.path.accum = &sum; a.path.trace_inst = &word;"
CASES = [("", True), ("a.path.slice_order = &word;", True), ("scene.one_level = false;", True), ("scene.n_instances = 1u; scene.has_spheres = false;", True),
         ("a.seed_primary = 0;", True),
         ("a.path.accum = nullptr;", False), ("a.path.trace_inst = nullptr;", False), ("a.path.spp = 0u;", False),
         ("a.path.sample_block = 32u;", False), ("a.path.trace_rays = &ray;", False), ("a.path.primary_cache = &sum;", False),
         ("a.path.slice_cost = &word;", False)]
PROGRAM = r"""
#include <hip/hip_runtime.h>
#include <cstdio>
#include "device_types.h"
using namespace hrt;
static HitGroup hg; static uint32_t word; static float4 sum; static RayRec ray;
int main() {
%s
    return 0;
}
"""
CASE = '    { TraverseArgs a{}; PathScene scene{true, 3u, true, nullptr}; %s %s std::printf("%%d\\n", (int)path_launch_admitted(PathKernel::Counts, a, scene)); }'


def test_the_counts_launch_is_admitted_and_its_contradictions_are_refused(tmp_path):
    src, exe = tmp_path / "admitted.cpp", tmp_path / "admitted"
    src.write_text(PROGRAM % "\n".join(CASE % (ADMITTED, change) for change, _ in CASES))
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{ROOT / 'include'}", f"-I{ROOT / CSRC}", "-o", str(exe), str(src)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    wrong = [(change, want, got) for (change, want), got in zip(CASES, out) if want != (got == "1")]
    assert len(out) == len(CASES) and not wrong, wrong
    fused = (ROOT / CSRC / "fused.hip").read_text()
    assert "case PathKernel::Counts: launch_path_counts(a, scene, grid_blocks, s); break;" in fused
