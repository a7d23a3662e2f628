"""k_path_capture (csrc/fused_capture.hip: the path kernel that also keeps every pixel's primary hit, HRT_CTX_CAPTURE_PRIMARY) as compiled:
four kernels of their own whose traversal loops, registers and spills are those of the k_fused<S, I, false> they stand in for -- the
capture is two stores in the regeneration phase and costs the loop nothing.  Read from the assembly the Makefile's flags produce
(tools/loop_stats.py), fused.hip compiled next to it for the comparison; figures: profiles/r20_primary_capture.txt."""
import re
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = "nvidia-optix-ray-tracer_amd/csrc/"
sys.path.insert(0, str(ROOT / "tools"))
import audit_asm_loads, path_kernels          # noqa: E402


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """{mangled kernel name: {"loop": Counter of kinds, "ops": Counter of the loop's opcodes, "meta": {key: int}, "args": [...]}}"""
    tmp = tmp_path_factory.mktemp("capture_kernels")
    units = [path_kernels.compile_unit(stem, tmp / f"{stem}.s") for stem in ("fused", "fused_capture")]
    return {name: k for unit in units for name, k in unit.items() if k["lines"]}


def test_four_kernels_whose_only_argument_is_the_traverse_args(compiled):
    """kernarg_traverse_args() reads the TraverseArgs at offset 0 of the kernel-argument segment."""
    capture = {k: v for k, v in compiled.items() if "k_path_capture" in k}
    assert len(capture) == 4 and len(compiled) == 12, sorted(compiled)
    for name, k in capture.items():
        explicit = [a for a in k["args"] if not a[2].startswith("hidden_")]
        assert len(explicit) == 1 and explicit[0][0] == "0" and explicit[0][2] == "by_value", (name, k["args"])


# (SGPRs, VGPRs) spilled, as built (profiles/r20_primary_capture.txt): nothing, like the k_fused<S, I, false> beside them
SPILLS = {(0, 0): (0, 0), (1, 0): (0, 0), (0, 1): (0, 0), (1, 1): (0, 0)}


@pytest.mark.parametrize("spheres", [0, 1])
@pytest.mark.parametrize("instanced", [0, 1])
def test_the_capture_kernel_keeps_k_fuseds_loop_and_registers(compiled, spheres, instanced):
    """No scratch or buffer access in the traversal loop; a loop no larger than the matching k_fused<S, I, false> loop plus 4
    instructions; the parent's occupancy (<= 128 VGPRs one-level, 4 waves per SIMD; <= 168 instanced, 3 waves); the spills recorded."""
    capture = path_kernels.one(compiled, f"k_path_captureILb{spheres}ELb{instanced}E")
    fused = path_kernels.one(compiled, f"k_fusedILb{spheres}ELb{instanced}ELb0E")
    assert not any(op.startswith("scratch_") or op.startswith("buffer_") for op in capture["ops"]), sorted(capture["ops"])
    assert sum(capture["loop"].values()) <= sum(fused["loop"].values()) + 4, (dict(capture["loop"]), dict(fused["loop"]))
    assert capture["meta"]["vgpr_count"] <= (168 if instanced else 128), capture["meta"]
    assert capture["meta"]["vgpr_count"] <= fused["meta"]["vgpr_count"] + 2, (capture["meta"], fused["meta"])
    spilled = (capture["meta"]["sgpr_spill_count"], capture["meta"]["vgpr_spill_count"])
    assert spilled[0] <= SPILLS[(spheres, instanced)][0] and spilled[1] <= SPILLS[(spheres, instanced)][1], capture["meta"]


def test_hand_issued_loads_of_the_capture_kernels_are_not_touched_before_their_wait():
    """tools/audit_asm_loads.py on the new file: 0 hazards."""
    groups, bad = audit_asm_loads.audit(*path_kernels.source("fused_capture"))
    assert groups > 0 and bad == 0, (groups, bad)


def test_the_capture_is_compiled_into_its_own_kernels_only():
    """The flag is false in the variant every kernel starts from (trav_common.h: PathVariant): fused.hip, fused_blocks.hip and kernels.hip do not name it, so their
    kernels' instruction streams are what they were (tests/test_host_cpu.py and tests/test_path_kernel_spills_cpu.py pin them)."""
    for stem in ("fused", "fused_blocks", "kernels", "fused_queue"):
        text = (ROOT / CSRC / f"{stem}.hip").read_text()
        assert "CAPTURE" not in text and "kCapture" not in text and "k_path_capture" not in text, stem
    # ... and the file instantiates exactly the capture variant, with exactly the flags it had: the kernel's spheres and levels, the capture
    # -- no primary-hit cache, no sample blocks
    body = (ROOT / CSRC / "fused_capture.hip").read_text()
    assert re.findall(r"fused_body<([^;]*)>\(", body) == ["CaptureVariant<HAS_SPHERES, INSTANCED>"]
    variant = re.search(r"template <bool HAS_SPHERES, bool INSTANCED>\nstruct CaptureVariant : (\S+) \{(.*?)\};", body, re.S)
    assert variant.group(1) == "FusedBodyVariant<false>"
    assert re.sub(r"\s+", " ", variant.group(2)).strip() == "static constexpr bool kSpheres = HAS_SPHERES, kInstanced = INSTANCED, kCapture = true;"


def test_stats_mirror_and_entry_point(hrt):
    """The binding's HrtStats ends with the three counters the header appends, and declares the new entry point."""
    import ctypes as C
    names = [f[0] for f in hrt.Stats._fields_]
    assert names[-3:] == ["primary_capture_launches", "guide_passes_traced", "guide_passes_captured"]
    header = (ROOT / "include" / "hrt.h").read_text()
    struct = header.split("typedef struct HrtStats {")[1].split("} HrtStats;")[0]
    declared = re.findall(r"(\w+)(?:\[[^\]]*\])?\s*(?:,|;)", re.sub(r"/\*.*?\*/", "", struct, flags=re.S))
    assert declared == names, (declared, names)
    words = sum(int(n) if n.isdigit() else {"HRT_K_COUNT": hrt.K_COUNT}[n] for n in re.findall(r"\[(\w+)\]", struct)) + len(names) - len(re.findall(r"\[(\w+)\]", struct))
    assert C.sizeof(hrt.Stats) == 8 * words
    assert hrt.CTX_CAPTURE_PRIMARY == 0x40 and "hrt_primary_hits_get" in hrt.EXPORTS
