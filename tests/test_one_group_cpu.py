"""k_path_one (fused_one.hip; DESIGN.md sections 2.1 and 4.1): k_path_blocks for a scene with one hit group, whose regeneration reads entry 0 of
the per-instance tables with scalar loads and keeps no albedo chain, and whose primitive test decides ties by the primitive id alone.  What
the compiler makes of that, read from ONE compilation of fused_one.hip with the Makefile's flags (tools/loop_stats.py, tools/loop_phases.py),
with k_path_blocks<0> compiled beside it for the comparison: the loop's first copy is held to what this build shows -- never more than
k_path_blocks' 408 instructions, 74 scalar ones, 1185 modelled cycles, and no more than 142 single-pipe instructions -- the kernel to its
registers, LDS and argument layout, and the regeneration to fewer vector loads than k_path_blocks<0> has."""
import re
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = "nvidia-optix-ray-tracer_amd/csrc/"
sys.path.insert(0, str(ROOT / "tools"))
import audit_asm_loads, loop_stats, path_kernels          # noqa: E402

# (instructions, scalar instructions, modelled cycles, single-pipe VALU instructions) of the first copy of k_path_one's loop: what the build
# shows.  k_path_blocks<0>: 408 / 74 / 1185 / 144.
LOOP = (401, 70, 1165, 142)
CEILING = (408, 74, 1185, 142)          # whatever the build shows, never above these
assert all(a <= b for a, b in zip(LOOP, CEILING))


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """{"one" / "blocks": {"loop": lines of the first loop copy, "body": lines of the kernel, "meta": {key: int}, "args": [...], "text": the file}}"""
    tmp = tmp_path_factory.mktemp("one_group")
    out = {}
    for key, stem, fragment in (("one", "fused_one", "k_path_one"), ("blocks", "fused_blocks", "k_path_blocksILb0E")):
        found = {name: k for name, k in path_kernels.compile_unit(stem, tmp / f"{stem}.s").items() if fragment in name and k["lines"]}
        assert len(found) == 1, sorted(found)
        name, k = next(iter(found.items()))
        out[key] = {"name": name, "loop": k["lines"], "body": k["body"], "meta": k["meta"], "args": k["args"], "text": (tmp / f"{stem}.s").read_text()}
    return out


def _regeneration(body):
    """from the outer loop's header to the first traversal loop's node loads (tests/test_block_regen_cpu.py)"""
    outer = min(i for i, l in enumerate(body) if "Loop Header: Depth=1" in l)
    node_loads = min(i for i, l in enumerate(body) if "global_load_dwordx4" in l and "offset:64" in l)
    assert outer < node_loads
    return body[outer:node_loads]


def test_one_kernel_in_the_file(compiled):
    assert len(re.findall(r"^\s*\.amdhsa_kernel\s", compiled["one"]["text"], re.M)) == 1


def test_the_loop_stays_within_what_this_build_shows(compiled):
    kinds = {}
    for op in loop_stats.opcodes(compiled["one"]["loop"]):
        kinds[loop_stats.kind(op)] = kinds.get(loop_stats.kind(op), 0) + 1
    total, salu, single = sum(kinds.values()), kinds.get("salu", 0), kinds.get("valu_complex", 0)
    cycles = loop_stats.model_cycles({k: kinds.get(k, 0) for k in ("valu_simple", "valu_complex", "salu")})
    print("k_path_one", total, salu, round(cycles), single, kinds)
    assert total <= LOOP[0] and salu <= LOOP[1] and cycles <= LOOP[2] + 0.5 and single <= LOOP[3], (total, salu, cycles, single)


def test_the_loop_is_no_larger_than_k_path_blocks(compiled):
    assert len(loop_stats.opcodes(compiled["one"]["loop"])) <= len(loop_stats.opcodes(compiled["blocks"]["loop"]))


def test_no_mask_save_behind_the_bookkeeping_sequence(compiled):
    import loop_phases
    _, scalar = loop_phases.phases(compiled["one"]["loop"])
    assert sum(scalar["exit"].values()) > 0 and "s_bcnt1_i32_b64" in scalar["exit"], dict(scalar["exit"])
    assert not any("saveexec" in op for op in scalar["exit"]), dict(scalar["exit"])


def test_registers_and_spills(compiled):
    meta = compiled["one"]["meta"]
    assert meta["vgpr_count"] <= 128 and meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, meta
    ops = loop_stats.opcodes(compiled["one"]["body"])
    assert not any(op.startswith("scratch_") or op.startswith("buffer_") for op in ops)
    # a spilled scalar register comes back with v_readlane_b32: no more of them than k_path_blocks<0> has (the wave reduction at its end)
    assert ops.count("v_readlane_b32") <= loop_stats.opcodes(compiled["blocks"]["body"]).count("v_readlane_b32") <= 4
    assert "v_readlane_b32" not in loop_stats.opcodes(_regeneration(compiled["one"]["body"]))


def test_lds_and_no_flat_instruction(compiled):
    assert compiled["one"]["meta"]["group_segment_fixed_size"] == 10240, compiled["one"]["meta"]
    assert not any(op.startswith("flat_") for op in loop_stats.opcodes(compiled["one"]["body"]))


def test_the_slab_tests_clamp(compiled):
    """the ray interval is folded into the slab test's FMAs (tests/test_slab_interval_cpu.py): DX10 clamping on, 16 clamped FMAs per loop copy"""
    text = compiled["one"]["text"]
    assert re.search(r"^\s*\.amdhsa_dx10_clamp 1\s*$", text, re.M)
    clamped = [l for op, l in loop_stats.instructions(compiled["one"]["loop"]) if op == "v_fma_f32" and re.search(r"\bclamp\b", l)]
    assert len(clamped) == 16, len(clamped)
    in_kernel = [l for op, l in loop_stats.instructions(compiled["one"]["body"]) if op == "v_fma_f32" and re.search(r"\bclamp\b", l)]
    assert len(in_kernel) == 32, len(in_kernel)          # two copies of the loop


def test_the_traverse_args_are_the_only_explicit_argument(compiled):
    """kernarg_traverse_args() (fused_body.h) reads the TraverseArgs at offset 0 of the kernel-argument segment"""
    explicit = [a for a in compiled["one"]["args"] if not a[2].startswith("hidden_")]
    assert len(explicit) == 1 and explicit[0][0] == "0" and explicit[0][2] == "by_value", compiled["one"]["args"]


def test_the_regeneration_has_fewer_vector_loads(compiled):
    """hitgroups[0], inst_program[0] and the albedos are scalar loads: at least five global_load fewer than k_path_blocks<0> between the outer
    loop's header and the first traversal loop, and more scalar loads instead"""
    one, blocks = loop_stats.opcodes(_regeneration(compiled["one"]["body"])), loop_stats.opcodes(_regeneration(compiled["blocks"]["body"]))
    n_one, n_blocks = sum(op.startswith("global_load") for op in one), sum(op.startswith("global_load") for op in blocks)
    print("global_load", n_one, n_blocks, "s_load", sum(op.startswith("s_load") for op in one), sum(op.startswith("s_load") for op in blocks))
    assert n_one <= n_blocks - 5, (n_one, n_blocks)
    assert sum(op.startswith("s_load") for op in one) > sum(op.startswith("s_load") for op in blocks)
    assert len(one) < len(blocks)


def test_the_other_translation_units_do_not_name_the_flag():
    for stem in ("fused", "fused_blocks", "fused_capture", "fused_queue", "kernels"):
        text = (ROOT / CSRC / f"{stem}.hip").read_text()
        assert "ONE_GROUP" not in text and "kOneGroup" not in text, stem


def test_hand_issued_loads_are_not_touched_before_their_wait():
    groups, bad = audit_asm_loads.audit(*path_kernels.source("fused_one"))
    assert groups > 0 and bad == 0, (groups, bad)
