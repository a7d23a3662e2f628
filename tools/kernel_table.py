#!/usr/bin/env python3
"""The static table of the twenty kernels that run the lean traversal loop (k_fused, k_path_blocks, k_path_one, k_path_restart, k_path_idle, k_path_direct, k_path_capture, k_trace_queue), as the profile files
give it: tools/loop_stats.py's counts of the first loop copy, registers, spills and LDS from the code object's metadata, v_readlane_b32
in the whole kernel -- all from the assembly the Makefile's flags produce.
Usage: tools/kernel_table.py"""
import re, sys, tempfile
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import loop_stats

CSRC = "nvidia-optix-ray-tracer_amd/csrc/"
FILES = (("fused", "_ZN3hrt7k_fused"), ("fused_blocks", "_ZN3hrt13k_path_blocks"), ("fused_one", "_ZN3hrt10k_path_one"), ("fused_restart", "_ZN3hrt14k_path_restart"), ("fused_idle", "_ZN3hrt11k_path_idle"), ("fused_direct", "_ZN3hrt13k_path_direct"), ("fused_capture", "_ZN3hrt14k_path_capture"), ("fused_counts", "_ZN3hrt13k_path_counts"), ("fused_queue", "_ZN3hrt13k_trace_queue"))


def short(name):
    """k_fused<0,0,1> of _ZN3hrt7k_fusedILb0ELb0ELb1EEEvNS_12TraverseArgsE; k_path_one, which is no template, of _ZN3hrt10k_path_oneENS_12TraverseArgsE"""
    m = re.match(r"_ZN3hrt\d+(\w+?)I((?:Lb\dE)+)E", name)
    if m is None:
        return re.match(r"_ZN3hrt\d+(\w+?)ENS_", name).group(1)
    return m.group(1) + "<" + ",".join(re.findall(r"Lb(\d)E", m.group(2))) + ">"


def rows():
    for stem, prefix in FILES:
        asm = Path(tempfile.gettempdir()) / f"hrt_table_{stem}.s"
        counts = {name: cs for name, cs, _ in loop_stats.loops(CSRC + f"{stem}.hip", prefix, asm=asm)}
        text = asm.read_text()
        bodies = {m.group(1): m.group(2).split("\n") for m in re.finditer(r"^(" + prefix + r"\w+):[^\n]*\n(.*?)s_endpgm", text, re.S | re.M)}
        for entry in text.split("amdhsa.kernels:")[1].split("\n  - .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", entry).group(1)
            if name not in counts:
                continue
            meta = {k: int(v) for k, v in re.findall(r"^    \.(\w+):\s+(\d+)\s*$", entry, re.M)}
            readlanes = sum(1 for op, _ in loop_stats.instructions(bodies[name]) if op == "v_readlane_b32")
            yield short(name), counts[name], meta, readlanes


if __name__ == "__main__":
    print("  kernel                 instr cycles  dual single  SALU  mem | SGPRs s-spill VGPRs v-spill   LDS | v_readlane")
    for name, cs, meta, readlanes in rows():
        print(f"  {name:<22} {sum(cs.values()):>5} {loop_stats.model_cycles(cs):>6.0f} {cs['valu_simple']:>5} {cs['valu_complex']:>6} {cs['salu']:>5} {cs['mem']:>4} |"
              f" {meta['sgpr_count']:>5} {meta['sgpr_spill_count']:>6} {meta['vgpr_count']:>5} {meta['vgpr_spill_count']:>6} {meta['group_segment_fixed_size']:>6} | {readlanes}")
