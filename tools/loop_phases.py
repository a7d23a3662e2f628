#!/usr/bin/env python3
"""The traversal loop of k_fused (csrc/trav_loop.h, shared with k_trace_queue; tools/loop_stats.py: the same loop, the same counts) split into its phases, so that a change to one
phase can be checked against the others.  The phases are found by the markers the loop already has, in layout order:
    exit  the loop test and whatever follows the bookkeeping sequence (wherever the compiler lays the latch out)
    G     from the loop header to the first s_setprio: tail hand-over (kTail copy only), work masks, load issue
    C     to the next s_setprio: the primitives' wait and test
    A     to the next s_setprio: the nodes' wait and the node step
    B     to the end of the hand-written bookkeeping sequence (the asm block with ds_write2_b32)
Cycles are the cost model of DESIGN.md section 4.1 (4.1 per single-pipe VALU, 2.37 per dual-pipe VALU, 2.4 per SALU instruction).
Usage: tools/loop_phases.py [substring of the mangled kernel name, default: the C4 kernel ILb0ELb0ELb0E] [-v: the scalar opcodes]"""
import sys
from collections import Counter, defaultdict
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
from loop_stats import instructions, kind, loop_bodies, model_cycles
import path_kernels

PHASES = ("G", "C", "A", "B", "exit")


def phases(lines):
    """{phase: Counter of instruction kinds}, {phase: Counter of scalar opcodes} of one loop body (layout order)"""
    hdr = next(i for i, l in enumerate(lines) if "Loop Header: Depth=2" in l)
    # (the walk below starts at the header: the layout may put the rest of the body in front of it)
    top = max(i for i, l in enumerate(lines[:hdr + 1]) if l.startswith(".LBB"))
    lines, hdr = lines[top:] + lines[:top], hdr - top
    ends = [i for i, l in enumerate(lines) if "#ASMEND" in l and i > hdr]
    book = [i for i, l in enumerate(lines) if "ds_write2_b32" in l and i > hdr]
    if not book:
        raise SystemExit("no bookkeeping sequence in the loop")
    book_end = min(i for i in ends if i > book[0])
    cs, sops = defaultdict(Counter), defaultdict(Counter)
    phase = "exit"
    for i, l in enumerate(lines):
        if i == hdr:
            phase = "G"
        elif i == book_end + 1:
            phase = "exit"
        for op, _ in instructions([l]):
            cs[phase][kind(op)] += 1
            if kind(op) == "salu":
                sops[phase][op] += 1
            if op == "s_setprio" and phase in ("G", "C", "A"):
                phase = PHASES[PHASES.index(phase) + 1]
    return cs, sops


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "-v"]
    want = args[0] if args else "ILb0ELb0ELb0E"
    # (k_path_one, fused_one.hip, is no template: ask for it by name -- tools/loop_phases.py k_path_one)
    source = path_kernels.source("fused_one" if "k_path_one" in want else "fused")
    for name, lines in loop_bodies(*source):
        if want not in name:
            continue
        cs, sops = phases(lines)
        print(name)
        print(f"  {'phase':6s} {'total':>6s} {'dual':>6s} {'single':>6s} {'SALU':>6s} {'mem':>6s} {'cycles':>7s}")
        tot = Counter()
        for p in PHASES:
            c = cs[p]
            tot.update(c)
            print(f"  {p:6s} {sum(c.values()):6d} {c['valu_simple']:6d} {c['valu_complex']:6d} {c['salu']:6d} {c['mem']:6d} {model_cycles(c):7.0f}")
        print(f"  {'all':6s} {sum(tot.values()):6d} {tot['valu_simple']:6d} {tot['valu_complex']:6d} {tot['salu']:6d} {tot['mem']:6d} {model_cycles(tot):7.0f}")
        if "-v" in sys.argv:
            for p in PHASES:
                print(f"  {p}: " + ", ".join(f"{k} {v}" for k, v in sops[p].most_common()))
