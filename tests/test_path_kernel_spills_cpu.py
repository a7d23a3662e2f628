"""What the compiled path kernels keep in registers (DESIGN.md sections 2.1 and 4.1): the regeneration phase reads its constants from the
kernel-argument segment with scalar loads where it uses them (fused_body.h: kernarg_traverse_args), so none of the 108 dwords of
TraverseArgs lives across the traversal loop, none is spilled into VGPR lanes and fetched back with v_readlane_b32, and nothing the
regeneration loads goes through flat_load.  tests/test_host_cpu.py holds k_fused's loop to its budget; this file holds k_path_blocks
(fused_blocks.hip, the flagship's kernel) to the same, and all one-level kernels to their spill counts.  Everything is read from the
assembly the Makefile's flags produce (tools/path_kernels.py), compiled once for the module."""
import re
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = "nvidia-optix-ray-tracer_amd/csrc/"
sys.path.insert(0, str(ROOT / "tools"))
import audit_asm_loads, loop_stats, path_kernels          # noqa: E402


TOOLS = ("kernel_table.py", "loop_stats.py", "audit_asm_loads.py", "loop_phases.py", "wave_clock.py", "lane_stats.py")


def _body_units():
    """the stems of the units that run fused_body"""
    return sorted(p.stem for p in (ROOT / CSRC).glob("*.hip") if '#include "fused_body.h"' in p.read_text())


@pytest.fixture(scope="module")
def every_unit(tmp_path_factory):
    """{mangled kernel name: what tools/path_kernels.py's compile_unit says of it} for every unit that runs fused_body"""
    from concurrent.futures import ThreadPoolExecutor
    tmp = tmp_path_factory.mktemp("path_kernels")
    with ThreadPoolExecutor(4) as pool:
        units = list(pool.map(lambda stem: path_kernels.compile_unit(stem, tmp / f"{stem}.s"), _body_units()))
    return {name: k for unit in units for name, k in unit.items()}


@pytest.fixture(scope="module")
def compiled(every_unit):
    """... for k_fused and k_path_blocks, the ten kernels this file holds to their budgets"""
    return {name: k for name, k in every_unit.items() if "k_fused" in name or "k_path_blocks" in name}


def test_twenty_two_kernels_whose_only_argument_is_the_traverse_args(every_unit, compiled):
    """kernarg_traverse_args() reads the TraverseArgs at offset 0 of the kernel-argument segment: every kernel that runs fused_body has it
    as its one explicit argument, by value, at offset 0 -- k_fused (8), k_path_blocks (2), k_path_one, k_path_restart, k_path_idle,
    k_path_direct, k_path_capture (4), k_path_counts (4)."""
    assert len(compiled) == 10, sorted(compiled)
    assert len(every_unit) == 22, sorted(every_unit)
    for name, k in every_unit.items():
        explicit = [a for a in k["args"] if not a[2].startswith("hidden_")]
        assert len(explicit) == 1 and explicit[0][0] == "0" and explicit[0][2] == "by_value", (name, k["args"])


def test_the_units_are_listed_once_for_makefile_tools_and_tests():
    """tools/path_kernels.py's list is the Makefile's PATH_UNITS and the units that run fused_body plus k_traverse's and k_trace_queue's, and
    no tool names a kernel's mangled prefix itself."""
    stems = [stem for stem, _, _ in path_kernels.UNITS]
    make = re.search(r"^PATH_UNITS := (.*)$", (ROOT / "Makefile").read_text(), re.M).group(1).split()
    assert stems == make, (stems, make)
    assert sorted(stems) == sorted(_body_units() + ["kernels", "fused_queue"])
    for stem, prefix, name in path_kernels.UNITS:
        assert prefix == f"_ZN3hrt{len(name)}{name}", (stem, prefix, name)
        assert (ROOT / CSRC / f"{stem}.hip").is_file()
    for tool in TOOLS:
        text = (ROOT / "tools" / tool).read_text()
        assert "_ZN3hrt" not in text and "path_kernels" in text, tool


@pytest.mark.parametrize("spheres", [0, 1])
def test_k_path_blocks_keeps_k_fuseds_loop_budget(compiled, spheres):
    """No scratch or buffer access in the traversal loop, 4 waves per SIMD (<= 128 VGPRs), and a loop no larger than the matching k_fused
    loop plus 4 instructions."""
    blocks = path_kernels.one(compiled, f"k_path_blocksILb{spheres}E")
    fused = path_kernels.one(compiled, f"k_fusedILb{spheres}ELb0ELb0E")
    assert not any(op.startswith("scratch_") or op.startswith("buffer_") for op in blocks["ops"]), sorted(blocks["ops"])
    assert blocks["meta"]["vgpr_count"] <= 128, blocks["meta"]
    assert sum(blocks["loop"].values()) <= sum(fused["loop"].values()) + 4, (dict(blocks["loop"]), dict(fused["loop"]))


# (SGPRs, VGPRs) spilled by the one-level kernels: what the build shows.  Before the regeneration read its constants from the segment these
# were (42, 11), (50, 14), (57, 20), (72, 20), (69, 23), (63, 34): anything above those is a failure whatever else has changed
SPILLS = {"k_fusedILb0ELb0ELb0E": (0, 2), "k_fusedILb1ELb0ELb0E": (0, 6), "k_fusedILb0ELb0ELb1E": (0, 12), "k_fusedILb1ELb0ELb1E": (0, 9),
          "k_path_blocksILb0E": (0, 12), "k_path_blocksILb1E": (0, 15)}


@pytest.mark.parametrize("fragment", sorted(SPILLS))
def test_spills_of_the_one_level_kernels(compiled, fragment):
    k = path_kernels.one(compiled, fragment)
    assert k["meta"]["sgpr_spill_count"] <= SPILLS[fragment][0] and k["meta"]["vgpr_spill_count"] <= SPILLS[fragment][1], k["meta"]


def _instanced(name):
    m = re.search(r"k_fusedILb\dELb(\d)ELb\dE", name)          # <HAS_SPHERES, INSTANCED, REUSE>
    return m is not None and m.group(1) == "1"


def test_the_instanced_kernels_spill_no_vector_register(compiled):
    """(compiled for 3 waves per SIMD: tests/test_host_cpu.py)"""
    two_level = [k for name, k in compiled.items() if _instanced(name)]
    assert len(two_level) == 4
    for k in two_level:
        assert k["meta"]["vgpr_spill_count"] == 0 and k["meta"]["sgpr_spill_count"] <= 4, k["meta"]


def test_no_constant_comes_back_from_a_vgpr_lane_or_through_a_flat_load(compiled):
    """The flagship's kernel, from the outer loop's header to the first traversal loop: no v_readlane_b32 (a spilled SGPR coming back).  In
    the whole of every kernel: only the handful of the wave reduction at its end (570 over both k_path_blocks kernels before), and no
    flat_load -- kernel arguments are read with s_load, scene data with global_load."""
    body = path_kernels.one(compiled, "k_path_blocksILb0E")["body"]
    outer = min(i for i, l in enumerate(body) if "Loop Header: Depth=1" in l)
    node_loads = min(i for i, l in enumerate(body) if "global_load_dwordx4" in l and "offset:64" in l)
    assert outer < node_loads
    assert "v_readlane_b32" not in loop_stats.opcodes(body[outer:node_loads])
    for name, k in compiled.items():
        ops = loop_stats.opcodes(k["body"])
        assert not any(op.startswith("flat_") for op in ops), (name, sorted({op for op in ops if op.startswith("flat_")}))
        assert any(op.startswith("s_load_dword") for op in ops)
        assert ops.count("v_readlane_b32") <= 4, (name, ops.count("v_readlane_b32"))


def test_hand_issued_loads_of_the_path_kernels_are_not_touched_before_their_wait():
    """tools/audit_asm_loads.py on the two files this change compiles differently: 0 hazards (tests/test_host_cpu.py runs it over all four)."""
    for stem in ("fused", "fused_blocks"):
        groups, bad = audit_asm_loads.audit(*path_kernels.source(stem))
        assert groups > 0 and bad == 0, (stem, groups, bad)
