"""What the compiled path kernels keep in registers (DESIGN.md sections 2.1 and 4.1): the regeneration phase reads its constants from the
kernel-argument segment with scalar loads where it uses them (fused_body.h: kernarg_traverse_args), so none of the 108 dwords of
TraverseArgs lives across the traversal loop, none is spilled into VGPR lanes and fetched back with v_readlane_b32, and nothing the
regeneration loads goes through flat_load.  tests/test_host_cpu.py holds k_fused's loop to its budget; this file holds k_path_blocks
(fused_blocks.hip, the flagship's kernel) to the same, and all one-level kernels to their spill counts.  Everything is read from the
assembly the Makefile's flags produce (tools/loop_stats.py), compiled once for the module."""
import re
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
    tmp = tmp_path_factory.mktemp("path_kernels")
    out = {}
    for stem, prefix in (("fused", "_ZN3hrt7k_fused"), ("fused_blocks", "_ZN3hrt13k_path_blocks")):
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


def _kernel(compiled, fragment):
    found = [v for k, v in compiled.items() if fragment in k]
    assert len(found) == 1, (fragment, sorted(compiled))
    return found[0]


def _opcodes(lines):
    import loop_stats
    return [op for op, _ in loop_stats.instructions(lines)]


def test_ten_kernels_whose_only_argument_is_the_traverse_args(compiled):
    """kernarg_traverse_args() reads the TraverseArgs at offset 0 of the kernel-argument segment: every kernel that runs fused_body has it
    as its one explicit argument, by value, at offset 0."""
    assert len(compiled) == 10, sorted(compiled)
    for name, k in compiled.items():
        explicit = [a for a in k["args"] if not a[2].startswith("hidden_")]
        assert len(explicit) == 1 and explicit[0][0] == "0" and explicit[0][2] == "by_value", (name, k["args"])


@pytest.mark.parametrize("spheres", [0, 1])
def test_k_path_blocks_keeps_k_fuseds_loop_budget(compiled, spheres):
    """No scratch or buffer access in the traversal loop, 4 waves per SIMD (<= 128 VGPRs), and a loop no larger than the matching k_fused
    loop plus 4 instructions."""
    blocks = _kernel(compiled, f"k_path_blocksILb{spheres}E")
    fused = _kernel(compiled, f"k_fusedILb{spheres}ELb0ELb0E")
    assert not any(op.startswith("scratch_") or op.startswith("buffer_") for op in blocks["ops"]), sorted(blocks["ops"])
    assert blocks["meta"]["vgpr_count"] <= 128, blocks["meta"]
    assert sum(blocks["loop"].values()) <= sum(fused["loop"].values()) + 4, (dict(blocks["loop"]), dict(fused["loop"]))


# (SGPRs, VGPRs) spilled by the one-level kernels: what the build shows.  Before the regeneration read its constants from the segment these
# were (42, 11), (50, 14), (57, 20), (72, 20), (69, 23), (63, 34): anything above those is a failure whatever else has changed
SPILLS = {"k_fusedILb0ELb0ELb0E": (0, 2), "k_fusedILb1ELb0ELb0E": (0, 6), "k_fusedILb0ELb0ELb1E": (0, 12), "k_fusedILb1ELb0ELb1E": (0, 9),
          "k_path_blocksILb0E": (0, 12), "k_path_blocksILb1E": (0, 15)}


@pytest.mark.parametrize("fragment", sorted(SPILLS))
def test_spills_of_the_one_level_kernels(compiled, fragment):
    k = _kernel(compiled, fragment)
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
    body = _kernel(compiled, "k_path_blocksILb0E")["body"]
    outer = min(i for i, l in enumerate(body) if "Loop Header: Depth=1" in l)
    node_loads = min(i for i, l in enumerate(body) if "global_load_dwordx4" in l and "offset:64" in l)
    assert outer < node_loads
    assert "v_readlane_b32" not in _opcodes(body[outer:node_loads])
    for name, k in compiled.items():
        ops = _opcodes(k["body"])
        assert not any(op.startswith("flat_") for op in ops), (name, sorted({op for op in ops if op.startswith("flat_")}))
        assert any(op.startswith("s_load_dword") for op in ops)
        assert ops.count("v_readlane_b32") <= 4, (name, ops.count("v_readlane_b32"))


def test_hand_issued_loads_of_the_path_kernels_are_not_touched_before_their_wait():
    """tools/audit_asm_loads.py on the two files this change compiles differently: 0 hazards (tests/test_host_cpu.py runs it over all four)."""
    sys.path.insert(0, str(ROOT / "tools"))
    import audit_asm_loads
    for stem, prefix in (("fused", "_ZN3hrt7k_fused"), ("fused_blocks", "_ZN3hrt13k_path_blocks")):
        groups, bad = audit_asm_loads.audit(CSRC + f"{stem}.hip", prefix)
        assert groups > 0 and bad == 0, (stem, groups, bad)
