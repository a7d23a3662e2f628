#!/usr/bin/env python3
"""Audit of the hand-issued loads of the traversal kernels (every unit of tools/path_kernels.py: k_traverse, k_fused, the k_path_* kernels,
k_trace_queue): between an asm
block that issues global_load_dwordx4 into VGPRs and the asm wait that retires them, the compiler must not read, copy or spill
those registers -- it does not know the loads are in flight, and the hardware does not interlock.  Compiles every unit to
assembly with the Makefile's own flags (`make -pn`), then prints, per kernel instantiation, the instructions that touch the
destinations of a group of loads before the wait that covers it (expected: none).  The scan follows the ORDER OF EXECUTION from
the loads -- across s_branch, down both sides of every s_cbranch -- to the first wait that retires them on each path (for the
primitives' loads the nodes' vmcnt(0) does too): the compiler lays these loops out as it likes, the header that issues the loads
may stand below the rest of the body, and what follows it in the text is then the code after the loop.
Run by tests/test_host_cpu.py; exit status 1 when anything is found.
Usage: tools/audit_asm_loads.py [-v]"""
import re, subprocess, sys, tempfile
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent


def makefile_hipflags():
    out = subprocess.run(["make", "-pn", "-C", str(ROOT)], capture_output=True, text=True).stdout
    m = re.search(r"^HIPFLAGS := (.*)$", out, re.M)
    if not m:
        raise SystemExit("HIPFLAGS not found in the Makefile")
    csrc = "nvidia-optix-ray-tracer_amd/csrc"
    return m.group(1).replace("$(ARCH)", "gfx950").replace("$(CSRC)", csrc).split()


def executed_after(body, start, stops):
    """indices of the lines that can execute after line `start`, up to (not including) a line of `stops` on every path"""
    labels = {l.split(":")[0]: i for i, l in enumerate(body) if l.startswith(".L")}
    seen, todo, out = set(), [start + 1], []
    while todo:
        k = todo.pop()
        while k < len(body) and k not in seen and k not in stops:
            seen.add(k)
            out.append(k)
            t = body[k].split()
            if t and t[0] == "s_branch":
                k = labels[t[1]]
                continue
            if t and t[0].startswith("s_cbranch"):
                todo.append(labels[t[1]])
            k += 1
    return sorted(out)


def audit(source, kernel_prefix, verbose=False):
    asm = str(Path(tempfile.gettempdir()) / f"hrt_audit_{Path(source).stem}.s")
    flags = [f for f in makefile_hipflags() if f != "-fPIC"]
    subprocess.check_call(["/opt/rocm/bin/hipcc", *flags, "-S", "--cuda-device-only", "-o", asm, source], cwd=ROOT, stderr=subprocess.DEVNULL)
    text = open(asm).read()
    bad_total = n_groups = 0
    for m in re.finditer(r"^(" + kernel_prefix + r"\w+):[^\n]*\n(.*?)s_endpgm", text, re.S | re.M):
        name, body = m.group(1), m.group(2).split("\n")
        blocks, i = [], 0
        while i < len(body):
            if "#ASMSTART" in body[i]:
                j = i
                while "#ASMEND" not in body[j]:
                    j += 1
                blocks.append((i, j, "\n".join(body[i:j + 1])))
                i = j
            i += 1
        in_asm = set()
        for b in blocks:
            in_asm.update(range(b[0], b[1] + 1))
        for what, n_loads, wait in (("node", 5, ("s_waitcnt vmcnt(0)",)), ("prim", 3, ("s_waitcnt vmcnt(5)", "s_waitcnt vmcnt(0)"))):
            loads = [b for b in blocks if b[2].count("global_load_dwordx4 v[") == n_loads]
            waits = {b[0] for b in blocks if any(w in b[2] for w in wait)}
            for lb in loads:
                regs = set()
                for r in re.finditer(r"global_load_dwordx4 v\[(\d+):(\d+)\]", lb[2]):
                    regs.update(range(int(r.group(1)), int(r.group(2)) + 1))
                if not waits:
                    continue
                n_groups += 1
                bad = []
                for k in executed_after(body, lb[1], waits):
                    l = body[k]
                    if k in in_asm or l.strip().startswith(";") or "implicit-def" in l:
                        continue
                    for r in re.finditer(r"\bv(\d+)\b|v\[(\d+):(\d+)\]", l):
                        rs = [int(r.group(1))] if r.group(1) else range(int(r.group(2)), int(r.group(3)) + 1)
                        if any(x in regs for x in rs):
                            bad.append(l.strip())
                            break
                bad_total += len(bad)
                if verbose or bad:
                    print(f"{name}: {what} loads -> {len(regs)} VGPRs, instructions touching them before the wait: {len(bad)}")
                for b in bad[:6]:
                    print("    ", b)
    return n_groups, bad_total


if __name__ == "__main__":
    v = "-v" in sys.argv
    total_groups = total_bad = 0
    sys.path.insert(0, str(ROOT / "tools"))
    import path_kernels
    for stem, _, _ in path_kernels.UNITS:
        src, prefix = path_kernels.source(stem)
        g, b = audit(src, prefix, v)
        print(f"{src}: {g} groups of in-flight loads checked, {b} hazardous instructions")
        total_groups += g; total_bad += b
    sys.exit(1 if total_bad or total_groups == 0 else 0)
