#!/usr/bin/env python3
"""Instruction counts of the traversal loops (the inner loop around the hand-issued node loads) of every path / traverse kernel
instantiation, from the assembly the Makefile's flags produce: VALU split into the dual-pipe ("simple") and single-pipe ("complex")
kinds of profiles/r02_valu_pipes_microbench.txt, SALU, memory.  The SIMD issues about one instruction of ANY kind per 2.4 cycles
(profiles/r02_valu_issue_patterns_microbench.txt), so the total is what a loop iteration costs.
Usage: tools/loop_stats.py [substring of the mangled kernel name ...]"""
import re, subprocess, sys, tempfile
from collections import Counter
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
from audit_asm_loads import makefile_hipflags
SIMPLE = {"v_fma_f32", "v_add_f32", "v_mul_f32", "v_sub_f32", "v_subrev_f32", "v_fmac_f32", "v_and_b32", "v_or_b32", "v_xor_b32", "v_lshrrev_b32",
          "v_add_u32", "v_sub_u32", "v_subrev_u32", "v_mov_b32", "v_mov_b64", "v_cndmask_b32", "v_not_b32"}


def kind(op):
    """valu_simple / valu_complex / salu / mem of an opcode (encoding suffix stripped)"""
    if op.startswith("v_"):
        return "valu_simple" if op in SIMPLE else "valu_complex"
    return "salu" if op.startswith("s_") else "mem"


def instructions(lines):
    """(opcode without its encoding suffix, line) of the instructions among `lines` (labels, comments, asm markers skipped)"""
    for l in lines:
        t = l.strip().split()
        if not t or t[0].startswith(";") or t[0].endswith(":"):
            continue
        yield re.sub(r"_(e32|e64|sdwa|dpp)$", "", t[0]), l


def opcodes(lines):
    """the opcodes of the instructions among `lines`"""
    return [op for op, _ in instructions(lines)]


def loop_bodies(source, prefix, asm=None):
    """Compiles `source` to assembly at `asm` (default: hrt_loops_<stem>.s in the temporary directory) and yields (kernel, lines of
    its traversal loop in layout order).  The loop is the depth-2 loop whose header is the last one before the first copy's node loads;
    its lines are those of the basic blocks the compiler's own comments put into it ("in Loop: Header=..."), loops nested in it
    included, wherever the layout has placed them (the latch may come before the header or after it)."""
    asm = str(asm or Path(tempfile.gettempdir()) / f"hrt_loops_{Path(source).stem}.s")
    flags = [f for f in makefile_hipflags() if f != "-fPIC"]
    subprocess.check_call(["/opt/rocm/bin/hipcc", *flags, "-S", "--cuda-device-only", "-o", asm, source], cwd=ROOT, stderr=subprocess.DEVNULL)
    text = open(asm).read()
    for m in re.finditer(r"^(" + prefix + r"\w+):[^\n]*\n(.*?)s_endpgm", text, re.S | re.M):
        name, body = m.group(1), m.group(2).split("\n")
        loads = [i for i, l in enumerate(body) if "global_load_dwordx4" in l and "offset:64" in l]
        if not loads:
            continue
        hdrs = [i for i, l in enumerate(body) if "Loop Header: Depth=2" in l and i < loads[0]]
        if not hdrs:
            continue
        # basic blocks: (first line, label, header of the loop the block is in, headers of the loops round a block that is a header)
        blocks = []
        for i, l in enumerate(body):
            if l.startswith(".LBB") or l.startswith("; %bb."):
                inl = re.search(r"in Loop: Header=(BB\d+_\d+)", l)
                blocks.append([i, "BB" + l.split(":")[0][4:] if l.startswith(".LBB") else None, inl.group(1) if inl else None, re.findall(r"Parent Loop (BB\d+_\d+)", l)])
            elif blocks and l.lstrip().startswith(";") and "Parent Loop" in l:
                blocks[-1][3] += re.findall(r"Parent Loop (BB\d+_\d+)", l)
        header = max((b for b in blocks if b[0] <= hdrs[-1]), key=lambda b: b[0])[1]
        inside = {header} | {b[1] for b in blocks if b[1] and header in b[3]}
        lines = []
        for k, b in enumerate(blocks):
            if b[1] in inside or b[2] in inside:
                lines += body[b[0]:blocks[k + 1][0] if k + 1 < len(blocks) else len(body)]
        if lines:
            yield name, lines


def loops(source, prefix, asm=None):
    """Compiles `source` to assembly at `asm` (default: hrt_loops_<stem>.s in the temporary directory) and yields its loops."""
    for name, lines in loop_bodies(source, prefix, asm):
        cs, ops = Counter(), Counter()
        for op, _ in instructions(lines):
            ops[op] += 1
            cs[kind(op)] += 1
        yield name, cs, ops


def model_cycles(cs):
    """issue cycles of a loop iteration under the cost model of DESIGN.md section 4.1"""
    return 4.1 * cs["valu_complex"] + 2.37 * cs["valu_simple"] + 2.4 * cs["salu"]


if __name__ == "__main__":
    want = sys.argv[1:]
    import path_kernels          # (which imports this module: the list of units is needed here only)
    for stem, _, _ in path_kernels.UNITS[:-1]:          # (k_trace_queue's loop is k_fused's)
        src, prefix = path_kernels.source(stem)
        for name, cs, ops in loops(src, prefix):
            if want and not any(w in name for w in want):
                continue
            total = sum(cs.values())
            print(f"{name}: {total} instructions in the traversal loop: VALU {cs['valu_simple']} dual-pipe + {cs['valu_complex']} single-pipe, SALU {cs['salu']}, memory {cs['mem']}"
                  f" -- {model_cycles(cs):.0f} modelled cycles")
            if "-v" in want or len(want) == 1:
                print("   ", ", ".join(f"{k} {v}" for k, v in ops.most_common(24)))
