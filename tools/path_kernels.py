"""The path kernels' translation units, once, for the tools and the tests: which units there are (the Makefile's PATH_UNITS), which kernel a
render ran, and what one compilation of a unit with the Makefile's flags says about each of its kernels."""
import re
import tempfile
from collections import Counter
from pathlib import Path

import loop_stats

CSRC = "nvidia-optix-ray-tracer_amd/csrc/"
# (source stem, mangled prefix of the unit's traversal kernels, their name)
UNITS = (("kernels", "_ZN3hrt10k_traverse", "k_traverse"), ("fused", "_ZN3hrt7k_fused", "k_fused"), ("fused_blocks", "_ZN3hrt13k_path_blocks", "k_path_blocks"),
         ("fused_one", "_ZN3hrt10k_path_one", "k_path_one"), ("fused_restart", "_ZN3hrt14k_path_restart", "k_path_restart"),
         ("fused_idle", "_ZN3hrt11k_path_idle", "k_path_idle"), ("fused_direct", "_ZN3hrt13k_path_direct", "k_path_direct"),
         ("fused_capture", "_ZN3hrt14k_path_capture", "k_path_capture"), ("fused_counts", "_ZN3hrt13k_path_counts", "k_path_counts"),
         ("fused_queue", "_ZN3hrt13k_trace_queue", "k_trace_queue"))
PREFIX = {stem: prefix for stem, prefix, _ in UNITS}


def source(stem):
    """(source file, mangled prefix) of a unit: the arguments of loop_stats.loop_bodies and audit_asm_loads.audit"""
    return CSRC + f"{stem}.hip", PREFIX[stem]


def short(name):
    """k_fused<0,0,1> of _ZN3hrt7k_fusedILb0ELb0ELb1EEEvNS_12TraverseArgsE; k_path_one, which is no template, of _ZN3hrt10k_path_oneENS_12TraverseArgsE"""
    m = re.match(r"_ZN3hrt\d+(\w+?)I((?:Lb\dE)+)E", name)
    if m is None:
        return re.match(r"_ZN3hrt\d+(\w+?)ENS_", name).group(1)
    return m.group(1) + "<" + ",".join(re.findall(r"Lb(\d)E", m.group(2))) + ">"


def kernel_ran(stats):
    """the kernel the launches counted in an HrtStats went to: the highest rung of the one-group ladder that has a launch (device_types.h:
    path_ladder_rung), below it the block kernel, else k_fused"""
    for counter, name in (("direct_launches", "k_path_direct"), ("mask_idle_launches", "k_path_idle"), ("restart_launches", "k_path_restart"),
                          ("one_group_launches", "k_path_one"), ("sample_block_launches", "k_path_blocks")):
        if getattr(stats, counter):
            return name
    return "k_fused"


def one(kernels, fragment=""):
    """the one kernel of a compile_unit result whose mangled name contains `fragment`"""
    found = [k for name, k in kernels.items() if fragment in name]
    assert len(found) == 1, (fragment, sorted(kernels))
    return found[0]


def compile_unit(stem, asm=None):
    """Compiles csrc/<stem>.hip to assembly at `asm` (loop_stats.loop_bodies: with the Makefile's flags) -> {mangled name: {...}} for every kernel
    of the unit's prefix: "lines", the first copy of its traversal loop ([]: it has none); "loop" and "ops", Counters of that loop's
    instruction kinds and opcodes; "body", the kernel's lines; "meta", the ints of its amdhsa.kernels entry; "args", its (offset, size,
    value_kind) argument list."""
    src, prefix = source(stem)
    asm = Path(asm or Path(tempfile.gettempdir()) / f"hrt_unit_{stem}.s")
    loops = dict(loop_stats.loop_bodies(src, prefix, asm=asm))
    text = asm.read_text()
    entries = {re.search(r"\.name:\s+(\S+)", e).group(1): e for e in text.split("amdhsa.kernels:")[1].split("\n  - .agpr_count:")[1:]}
    out = {}
    for m in re.finditer(r"^(" + prefix + r"\w+):[^\n]*\n(.*?)s_endpgm", text, re.S | re.M):
        name, lines = m.group(1), loops.get(m.group(1), [])
        ops = Counter(op for op, _ in loop_stats.instructions(lines))
        kinds = Counter()
        for op, n in ops.items():
            kinds[loop_stats.kind(op)] += n
        out[name] = {"lines": lines, "loop": kinds, "ops": ops, "body": m.group(2).split("\n"),
                     "meta": {k: int(v) for k, v in re.findall(r"^    \.(\w+):\s+(\d+)\s*$", entries[name], re.M)},
                     "args": re.findall(r"- \.offset:\s+(\d+)\n\s+\.size:\s+(\d+)\n\s+\.value_kind:\s+(\w+)", entries[name])}
    return out
