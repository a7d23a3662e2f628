#!/usr/bin/env python3
"""The static table of the kernels that run the lean traversal loop (every unit of tools/path_kernels.py but k_traverse's), as the profile files
give it: tools/loop_stats.py's counts of the first loop copy, registers, spills and LDS from the code object's metadata, v_readlane_b32
in the whole kernel -- all from the assembly the Makefile's flags produce.
Usage: tools/kernel_table.py"""
import sys, tempfile
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import loop_stats
import path_kernels


def rows():
    for stem, _, _ in path_kernels.UNITS[1:]:
        for name, k in path_kernels.compile_unit(stem, Path(tempfile.gettempdir()) / f"hrt_table_{stem}.s").items():
            if k["lines"]:
                yield path_kernels.short(name), k["loop"], k["meta"], sum(1 for op, _ in loop_stats.instructions(k["body"]) if op == "v_readlane_b32")


if __name__ == "__main__":
    print("  kernel                 instr cycles  dual single  SALU  mem | SGPRs s-spill VGPRs v-spill   LDS | v_readlane")
    for name, cs, meta, readlanes in rows():
        print(f"  {name:<22} {sum(cs.values()):>5} {loop_stats.model_cycles(cs):>6.0f} {cs['valu_simple']:>5} {cs['valu_complex']:>6} {cs['salu']:>5} {cs['mem']:>4} |"
              f" {meta['sgpr_count']:>5} {meta['sgpr_spill_count']:>6} {meta['vgpr_count']:>5} {meta['vgpr_spill_count']:>6} {meta['group_segment_fixed_size']:>6} | {readlanes}")
