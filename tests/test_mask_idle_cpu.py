"""k_path_idle (csrc/fused_idle.hip; HRT_MASK_IDLE; DESIGN.md sections 2.1 and 4.1): k_path_restart whose loop runs the primitive test with
exec = the lanes that loaded a record and the node step with exec = the lanes that loaded a node, by plain moves to exec (shared with the
load groups, which already set those masks) in the loop copy where every lane is active.  What can be said without a GPU, from one
compilation of fused_idle.hip and one of fused_restart.hip with the Makefile's flags -- every bound is k_path_restart's own figure from
the same compiler, not a constant:
  (a) the budget: the first loop copy at most 3 instructions and 3 scalar instructions over k_path_restart's, the same 16 clamped FMAs, at
      most 128 VGPRs, nothing spilled, no scratch, no flat_ instruction, 10240 B of LDS, one kernel in the unit, no load hazard;
  (b) the moves: the primitive loads go out under the primitive mask, which is in exec again behind the node loads and untouched up to the
      primitives' wait, with no vector instruction on the way; in execution order from there, exec is written with the node mask in front
      of the nodes' wait and with -1 in front of the bookkeeping sequence's first mask -- and k_path_restart writes nothing there;
  (c) what runs with lanes off stays inside the lane's own stretch.  The compiler does not know that exec changes, so this is read from the
      assembly: a vector register written in the primitive stretch is either the best hit updated in place (v_cndmask_b32 with the
      destination as its first source: a lane that is off keeps its own) or is written again before anything reads it behind the stretch;
      a register written in the node stretch is read by the bookkeeping sequence at most (whose masks cover it: trav_lean.h) and written
      again before anything reads it behind that; and no vector instruction stands between the skip of an empty primitive pass and the
      node stretch's move, where exec may be either;
  (d) the launch entry admits for the enumerator exactly what it admits for Restart: tests/test_path_launch_cpu.py;
  (e) the flag, the knob and the counter are where the text says."""
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
    tmp = tmp_path_factory.mktemp("mask_idle")
    out = {}
    for key, stem in (("idle", "fused_idle"), ("restart", "fused_restart")):
        k = path_kernels.one(path_kernels.compile_unit(stem, tmp / f"{stem}.s"))
        out[key] = {"text": (tmp / f"{stem}.s").read_text(), "loop": [(op, l.strip()) for op, l in loop_stats.instructions(k["lines"])], "body": k["body"], "meta": k["meta"]}
    return out


# ---------------------------------------------------------------- (a) the budget ----------------------------------------------------------------
def test_the_budget_against_k_path_restart(compiled):
    idle, restart = compiled["idle"], compiled["restart"]
    n_i, n_r = len(idle["loop"]), len(restart["loop"])
    s_i, s_r = (sum(loop_stats.kind(op) == "salu" for op, _ in k["loop"]) for k in (idle, restart))
    print(f"loop: k_path_idle {n_i} instructions, {s_i} scalar; k_path_restart {n_r}, {s_r}")
    assert n_i <= n_r + 3 and s_i <= s_r + 3, (n_i, n_r, s_i, s_r)
    for k in (idle, restart):
        assert sum(op == "v_fma_f32" and re.search(r"\bclamp\b", l) is not None for op, l in k["loop"]) == 16
    meta = idle["meta"]
    print("k_path_idle", meta)
    assert len(re.findall(r"^\s*\.amdhsa_kernel\s", idle["text"], re.M)) == 1
    assert meta["group_segment_fixed_size"] == 10240, meta
    assert meta["vgpr_count"] <= 128 and meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, meta
    assert meta.get("private_segment_fixed_size", 0) == 0, meta
    ops = [op for op, _ in loop_stats.instructions(idle["body"])]
    assert not any(op.startswith("flat_") or op.startswith("scratch_") for op in ops)


def test_hand_issued_loads_are_not_touched_before_their_wait():
    groups, bad = audit_asm_loads.audit(*path_kernels.source("fused_idle"))
    assert groups > 0 and bad == 0, (groups, bad)


# ---------------------------------------------------------------- (b), (c) the moves and the stretches ----------------------------------------------------------------
def _from_the_loads(loop):
    """(the loop's instructions in execution order, beginning behind the node loads' group -- the five loads and the move to exec behind
    them --, that move's operand, the operand of the move in front of the primitive loads)"""
    last = [i for i, (_, l) in enumerate(loop) if l.startswith("global_load_dwordx4") and "offset:64" in l]
    assert len(last) == 1, last
    behind = re.fullmatch(r"s_mov_b64 exec, (\S+)", loop[last[0] + 1][1])
    first = [i for i, (_, l) in enumerate(loop) if l.startswith("global_load_dwordx4")][0]          # (the primitive group comes first in the layout too)
    before = re.fullmatch(r"s_mov_b64 exec, (\S+)", loop[first - 1][1])
    assert behind and before and first < last[0], (loop[first - 1], loop[last[0] + 1])
    return loop[last[0] + 2:] + loop[:last[0] + 2], behind.group(1), before.group(1)


def _exec_writes_up_to_the_bookkeeping(seq):
    """(index, line) of the instructions that write exec, up to the sequence's first mask"""
    out = []
    for i, (op, l) in enumerate(seq):
        if re.match(r"s_\w+ exec,", l):
            out.append((i, l))
            if op != "s_mov_b64":
                return out
    raise AssertionError("no bookkeeping sequence")


def _stretches(seq):
    """indices into seq: the primitives' wait, the node stretch's move, the move back to all lanes"""
    w = _exec_writes_up_to_the_bookkeeping(seq)
    assert len(w) == 3, w
    (inn, ln), (ia, la), (_, lb) = w
    assert re.fullmatch(r"s_mov_b64 exec, s\[\d+:\d+\]", ln) and seq[inn + 1][1] == "s_waitcnt vmcnt(0)", (ln, seq[inn + 1])
    assert la == "s_mov_b64 exec, -1" and lb.startswith("s_and_b64 exec,"), w
    waits = [i for i, (_, l) in enumerate(seq[:inn]) if l == "s_waitcnt vmcnt(5)"]
    assert len(waits) == 1, waits
    return waits[0], inn, ia


def test_exec_is_written_between_the_loads_and_the_bookkeeping(compiled):
    seq, behind, before = _from_the_loads(compiled["idle"]["loop"])
    # the primitive loads go out under a mask, the node loads under another, and the primitive mask is back in exec behind them ...
    assert re.fullmatch(r"s\[\d+:\d+\]", behind) and behind == before, (behind, before)
    ip, inn, ia = _stretches(seq)
    # ... the node stretch's mask is the one the node loads went out under
    node_mask = seq[inn][1]
    assert [l for _, l in compiled["idle"]["loop"]].count(node_mask) >= 2 and node_mask != f"s_mov_b64 exec, {behind}", node_mask
    # and nothing writes the primitive mask's registers, or any vector register, between the loads and the primitives' wait
    lo, hi = (int(x) for x in re.fullmatch(r"s\[(\d+):(\d+)\]", behind).groups())
    for op, l in seq[:ip]:
        assert not op.startswith("v_"), l
        dst = re.match(r"s_\w+ (s\[(\d+):(\d+)\]|s(\d+)),", l)
        if dst and not op.startswith("s_cmp"):
            a, b = (int(dst.group(2)), int(dst.group(3))) if dst.group(2) else (int(dst.group(4)), int(dst.group(4)))
            assert b < lo or a > hi, l
    # k_path_restart: the literal behind both groups, and nothing written to exec from there to the bookkeeping sequence
    rseq, rbehind, rbefore = _from_the_loads(compiled["restart"]["loop"])
    assert rbehind == "-1" and [l for _, l in _exec_writes_up_to_the_bookkeeping(rseq)][:-1] == []


def _vregs(tokens):
    out = set()
    for t in tokens:
        for a, b in re.findall(r"\bv\[(\d+):(\d+)\]", t):
            out |= set(range(int(a), int(b) + 1))
        out |= {int(a) for a in re.findall(r"(?<![\w\[:])v(\d+)\b", t)}
    return out


def _defs_uses(op, line):
    """vector registers an instruction writes and reads (what matters here: VALU, LDS and global memory instructions)"""
    parts = line.split(None, 1)
    operands = [o.strip() for o in parts[1].split(",")] if len(parts) > 1 else []
    if op.startswith("v_cmp") or op.startswith("v_readlane") or op.startswith("v_readfirstlane") or op.startswith("s_"):
        return set(), _vregs(operands)
    if op.startswith("v_") or op.startswith("ds_read") or op.startswith("global_load"):
        defs = _vregs(operands[:1])
        uses = _vregs(operands[1:])
        if "mac" in op or "UNUSED_PRESERVE" in line:
            uses |= defs
        return defs, uses
    return set(), _vregs(operands)


def _read_before_written(seq, regs):
    """the registers of `regs` that an instruction of `seq` reads before one has written them"""
    regs, bad = set(regs), set()
    for op, l in seq:
        defs, uses = _defs_uses(op, l)
        bad |= uses & regs
        regs -= defs
    return bad


def test_what_runs_with_lanes_off_stays_in_its_stretch(compiled):
    seq, _, _ = _from_the_loads(compiled["idle"]["loop"])
    ip, inn, ia = _stretches(seq)
    # the primitive stretch: in-place updates of the best hit, and temporaries
    temps, merged = set(), set()
    for op, l in seq[ip + 1:inn]:
        if op.startswith("s_cbranch") or op == "s_branch":
            continue
        defs, _ = _defs_uses(op, l)
        m = re.match(r"v_cndmask_b32_e\d+ (v\d+), (v\d+),", l)
        if m and m.group(1) == m.group(2):
            merged |= defs
        else:
            temps |= defs
    print("primitive stretch: updated in place", sorted(merged), "temporaries", sorted(temps))
    assert len(merged) == 5 and not (merged & temps), (merged, temps)          # t, u, v, the primitive, its record
    assert not _read_before_written(seq[inn:], temps)
    # no vector instruction where exec may be either mask: from the end of the primitive test's block (the branch back, or the label the skip
    # jumps to) to the node stretch's move.  The primitive block is the one that ends in the loop's only unconditional branch.
    tail = [i for i, (op, _) in enumerate(seq[:inn]) if op == "s_branch"]
    assert len(tail) <= 1, tail
    after = tail[0] + 1 if tail else max(i for i, (op, l) in enumerate(seq[:inn]) if op.startswith("v_")) + 1
    assert not any(op.startswith("v_") for op, _ in seq[after:inn]), seq[after:inn]
    # the node stretch: read by the bookkeeping sequence at most, which ends with the literal back in exec
    written = set()
    for op, l in seq[inn + 1:ia]:
        written |= _defs_uses(op, l)[0]
    end = next(i for i in range(ia + 1, len(seq)) if seq[i][1] == "s_mov_b64 exec, -1")
    assert not _read_before_written(seq[end + 1:] + seq[:ip], written)


# (d) the launch entry: tests/test_path_launch_cpu.py, whose table holds every case of Restart for MaskIdle and Direct as well


# ---------------------------------------------------------------- (e) the flag, the knob, the counter ----------------------------------------------------------------
def test_the_flag_the_knob_and_the_counter(hrt):
    for path in sorted((ROOT / CSRC).glob("*.hip")):
        assert ("kMaskIdle" in path.read_text()) == (path.name in ("fused_idle.hip", "fused_direct.hip")), path.name          # (k_path_direct is k_path_idle plus kDirect)
    body = (ROOT / CSRC / "fused_idle.hip").read_text()
    assert re.findall(r"fused_body<([^;]*)>\(", body) == ["MaskIdleVariant"]
    variant = re.search(r"struct MaskIdleVariant : (\S+) \{(.*?)\};", body, re.S)
    assert variant.group(1) == "FusedBodyVariant<false>"
    assert re.sub(r"\s+", " ", variant.group(2)).strip() == "static constexpr bool kBlocks = true, kOneGroup = true, kRestart = true, kMaskIdle = true;"
    assert "static constexpr bool kMaskIdle = false;" in (ROOT / CSRC / "trav_common.h").read_text()
    knobs = (ROOT / CSRC / "knobs.def").read_text()
    line = next(l for l in knobs.splitlines() if l.startswith('HRT_KNOB("HRT_MASK_IDLE"'))
    assert "ctx->mask_idle = std::atoi(e) != 0" in line
    names = [f[0] for f in hrt.Stats._fields_]
    assert names.index("mask_idle_launches") + 1 == names.index("restart_launches")
    assert ("fused_idle", "_ZN3hrt11k_path_idle", "k_path_idle") in path_kernels.UNITS
