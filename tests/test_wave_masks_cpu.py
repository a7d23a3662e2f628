"""The traversal loop of the path kernels keeps its lane flags and work masks as wave masks (trav_loop.h): what the
compiler makes of that, read from the assembly the Makefile's flags produce (tools/loop_stats.py, tools/loop_phases.py), compiled once
for the module.  The first copy of the loop -- one-level trees, work left to start -- of k_fused<0,0,0>, k_path_blocks<0> and
k_trace_queue<0> is held to the instruction counts this build shows, as upper bounds, and must not contain the two patterns a per-lane
bool costs: a mask save (s_and_saveexec_b64) behind the bookkeeping sequence, and a v_cndmask_b32 0 / 1 that feeds a v_cmp_ne -- a mask
turned into a per-lane value and back."""
import re
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = "nvidia-optix-ray-tracer_amd/csrc/"
sys.path.insert(0, str(ROOT / "tools"))
import loop_stats, path_kernels          # noqa: E402

# kernel -> (instructions, scalar instructions, modelled cycles) of the first copy of its loop: what the build shows.  Before the flags
# were masks: 432 / 89 / 1251, 432 / 89 / 1251 and 433 / 90 / 1254.
BUDGET = {"k_fusedILb0ELb0ELb0E": (408, 74, 1185), "k_path_blocksILb0E": (408, 74, 1185), "k_trace_queueILb0E": (410, 76, 1190)}


@pytest.fixture(scope="module")
def loops(tmp_path_factory):
    """{fragment of BUDGET: lines of the kernel's first loop, in layout order}"""
    tmp = tmp_path_factory.mktemp("wave_masks")
    out = {}
    for stem in ("fused", "fused_blocks", "fused_queue"):
        for name, k in path_kernels.compile_unit(stem, tmp / f"{stem}.s").items():
            for fragment in BUDGET:
                if fragment in name:
                    out[fragment] = k["lines"]
    assert sorted(out) == sorted(BUDGET)
    return out


@pytest.mark.parametrize("fragment", sorted(BUDGET))
def test_the_loop_stays_within_what_this_build_shows(loops, fragment):
    kinds = {}
    for op, _ in loop_stats.instructions(loops[fragment]):
        kinds[loop_stats.kind(op)] = kinds.get(loop_stats.kind(op), 0) + 1
    total, salu, cycles = sum(kinds.values()), kinds.get("salu", 0), loop_stats.model_cycles({k: kinds.get(k, 0) for k in ("valu_simple", "valu_complex", "salu")})
    print(fragment, total, salu, round(cycles), kinds)
    assert total <= BUDGET[fragment][0] and salu <= BUDGET[fragment][1] and cycles <= BUDGET[fragment][2] + 0.5, (total, salu, cycles)


@pytest.mark.parametrize("fragment", sorted(BUDGET))
def test_no_mask_save_behind_the_bookkeeping_sequence(loops, fragment):
    """`done`, `alive` and `waiting` are updated with scalar and / or / andn2; the exit is a population count, a compare and a branch"""
    import loop_phases
    _, scalar = loop_phases.phases(loops[fragment])
    assert sum(scalar["exit"].values()) > 0 and "s_bcnt1_i32_b64" in scalar["exit"], dict(scalar["exit"])
    assert not any("saveexec" in op for op in scalar["exit"]), dict(scalar["exit"])


@pytest.mark.parametrize("fragment", sorted(BUDGET))
def test_no_mask_goes_through_a_vector_register_and_back(loops, fragment):
    """No v_cndmask_b32 vN, 0, 1, <mask> whose vN a v_cmp_ne reads before it is written again"""
    ins = [l.strip() for _, l in loop_stats.instructions(loops[fragment])]
    found = []
    for i, l in enumerate(ins):
        m = re.match(r"v_cndmask_b32\w*\s+(v\d+), 0, 1, ", l)
        if not m:
            continue
        reg = re.compile(r"\b" + m.group(1) + r"\b")
        for later in ins[i + 1:]:
            if later.startswith("v_cmp_ne") and reg.search(later):
                found.append((l, later))
                break
            if re.match(r"\S+\s+" + m.group(1) + r"\b", later):        # written again
                break
    assert not found, found
