"""k_path_counts (csrc/fused_counts.hip: the path kernel of hrt_render_accumulate, every pixel with a sample count of its own) as compiled, read
from the assembly the Makefile's flags produce as tests/test_path_kernel_spills_cpu.py reads the other path kernels (tools/loop_stats.py),
compiled once for the module.  (The admission rule of its launch: tests/test_path_launch_cpu.py.)"""
import re
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = "nvidia-optix-ray-tracer_amd/csrc/"
sys.path.insert(0, str(ROOT / "tools"))
import audit_asm_loads, loop_stats, path_kernels          # noqa: E402


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """{mangled kernel name: what tools/path_kernels.py's compile_unit says of it} for k_fused and k_path_counts"""
    tmp = tmp_path_factory.mktemp("path_counts")
    return {**path_kernels.compile_unit("fused", tmp / "fused.s"), **path_kernels.compile_unit("fused_counts", tmp / "fused_counts.s")}


def _counts(compiled):
    return {k: v for k, v in compiled.items() if "k_path_counts" in k}


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
        ops = loop_stats.opcodes(k["body"])
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
    groups, bad = audit_asm_loads.audit(*path_kernels.source("fused_counts"))
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


# (the admission rule of the counts launch, twelve cases, and its case in fused.hip: tests/test_path_launch_cpu.py)
