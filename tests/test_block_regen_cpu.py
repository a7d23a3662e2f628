"""What the regeneration of k_path_blocks no longer does (path_lane.h): the kBlocks instantiation takes a render in
sample blocks for granted -- no callers' rays, no cost probe, no slice order, sample_block != 0 (path_launch_admitted refuses anything
else) -- so its code neither loads PathArgs::trace_rays, slice_cost and slice_order from the kernel-argument segment nor branches on
them, and the scalar round trips of a regeneration are held to what the build shows.  Read from the assembly the Makefile's flags
produce, compiled once for the module; the fields' offsets come from a host program built against device_types.h."""
import re
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "nvidia-optix-ray-tracer_amd" / "csrc"
sys.path.insert(0, str(ROOT / "tools"))
import path_kernels          # noqa: E402
HIPCC = "/opt/rocm/bin/hipcc"
FIELDS = ("trace_rays", "slice_cost", "slice_order")

OFFSETS_CPP = r"""
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdio>
#include "device_types.h"
int main() {
    using namespace hrt;
    std::printf("trace_rays %zu\n", offsetof(TraverseArgs, path) + offsetof(PathArgs, trace_rays));
    std::printf("slice_cost %zu\n", offsetof(TraverseArgs, path) + offsetof(PathArgs, slice_cost));
    std::printf("slice_order %zu\n", offsetof(TraverseArgs, path) + offsetof(PathArgs, slice_order));
    std::printf("sizeof %zu\n", sizeof(TraverseArgs));
    return 0;
}
"""


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """{"offsets": {field: byte offset in TraverseArgs}, "bodies": {mangled kernel name: [lines]}}"""
    tmp = tmp_path_factory.mktemp("block_regen")
    bodies = {name: k["body"] for stem in ("fused", "fused_blocks") for name, k in path_kernels.compile_unit(stem, tmp / f"{stem}.s").items()}
    src, exe = tmp / "offsets.cpp", tmp / "offsets"
    src.write_text(OFFSETS_CPP)
    subprocess.check_call([HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-I" + str(ROOT / "include"), "-I" + str(CSRC), "-o", str(exe), str(src)], stderr=subprocess.DEVNULL)
    out = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    return {"offsets": {k: int(v) for k, v in out.items()}, "bodies": bodies}


def _kernel(compiled, fragment):
    found = [v for k, v in compiled["bodies"].items() if fragment in k]
    assert len(found) == 1, (fragment, sorted(compiled["bodies"]))
    return found[0]


def _scalar_loads(lines):
    """(first byte, one past the last byte) of every s_load_dword* with an immediate offset"""
    for l in lines:
        m = re.match(r"\s*s_load_dword(x\d+)?\s+[^,]+,\s*s\[\d+:\d+\],\s*(0x[0-9a-f]+|\d+)\s*(;.*)?$", l)
        if m:
            first = int(m.group(2), 0)
            yield first, first + 4 * int((m.group(1) or "x1")[1:])


def _reads(lines, offset):
    """a scalar load covers the 8 bytes of the pointer at `offset`"""
    return any(first < offset + 8 and offset < last for first, last in _scalar_loads(lines))


def _regeneration(body):
    """from the outer loop's header to the first traversal loop's node loads (tests/test_path_kernel_spills_cpu.py)"""
    outer = min(i for i, l in enumerate(body) if "Loop Header: Depth=1" in l)
    node_loads = min(i for i, l in enumerate(body) if "global_load_dwordx4" in l and "offset:64" in l)
    assert outer < node_loads
    return body[outer:node_loads]


def test_the_offsets_are_inside_the_argument(compiled):
    off = compiled["offsets"]
    assert all(0 < off[f] < off["sizeof"] for f in FIELDS) and len({off[f] for f in FIELDS}) == 3, off


@pytest.mark.parametrize("spheres", [0, 1])
@pytest.mark.parametrize("field", FIELDS)
def test_k_path_blocks_does_not_read_the_modes_it_cannot_have(compiled, spheres, field):
    body = _kernel(compiled, f"k_path_blocksILb{spheres}E")
    assert len(list(_scalar_loads(body))) > 20           # (the regeneration's constants are scalar loads: there is something to look through)
    assert not _reads(body, compiled["offsets"][field]), field


@pytest.mark.parametrize("field", FIELDS)
def test_k_fused_still_reads_them(compiled, field):
    """... so the test above can see such a load: the plain kernel has all three modes."""
    assert _reads(_kernel(compiled, "k_fusedILb0ELb0ELb0E"), compiled["offsets"][field]), field


# s_waitcnt lgkmcnt(0) in the regeneration of k_path_blocks<false>: 46 before the modes became compile-time facts (profiles/r23_block_regen.txt)
WAITS_CAP = 33


def test_scalar_round_trips_of_a_regeneration(compiled):
    region = _regeneration(_kernel(compiled, "k_path_blocksILb0E"))
    waits = sum(1 for l in region if re.search(r"^\s*s_waitcnt\b.*lgkmcnt\(0\)", l))
    assert 0 < waits <= WAITS_CAP, waits
