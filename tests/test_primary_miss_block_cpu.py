"""HRT_MISS_BLOCK on the CPU (csrc/path_lane.h: path_finish, kDirect; DESIGN.md section 2.1 "A primary miss takes the rest of its block").
  (a) k_path_direct's miss block steps through a block's samples with hold_ends (device_types.h), path_finish's own end-of-hold test written as
      a function.  hrt_sample_schedule walks every schedule it makes with that function too and fails where it and the passes disagree: a
      lane's hold must end behind sample p - 1 exactly where a pass starts or the launch's samples end -- for uniform blocks of every size the
      GPU test uses and a few more, and for tapered schedules, over 1 to 300 samples (a tapered walk of 1 to 1100: tests/test_sample_taper_cpu.py).
  (b) static, from one compilation of fused_direct.hip with the Makefile's flags through tools/path_kernels.py: nothing spilled, no scratch, no
      flat_ instruction, with the loop in the regeneration.
  (c) the knob is in knobs.def, in the table made from it, in the context, and reaches the kernel where the text says."""
import ctypes as C
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "nvidia-optix-ray-tracer_amd" / "csrc"
sys.path.insert(0, str(ROOT / "tools"))
import knob_table, loop_stats, path_kernels          # noqa: E402

UNIFORM = (1, 2, 3, 4, 7, 8, 64, 100, 127, 300, 1000, 65535)
TAPERS = ((8, 2), (64, 8), (4, 2), (16, 1))


def _schedule(lib, spp, big, small):
    first = (C.c_uint32 * (spp + 1))()
    n = C.c_uint32(0)
    rc = lib.hrt_sample_schedule(spp, big, small, first, spp + 1, C.byref(n))
    return rc, list(first[:n.value + 1])


def _hold_ends(spp, k_big, magic, k_min, taper_end, p):
    """device_types.h: hold_ends and block_ends, in Python's integers cut to 32 bits"""
    m32 = 0xffffffff
    ends = p >= spp
    if magic:
        rem = (p - ((p * magic) >> 32) * k_big) & m32
        return ends or rem == 0 or rem == k_big
    q = (taper_end - p) & m32
    if q & 0x80000000:
        q &= (k_min - 1) & m32
    below = min((q - 1) & m32, (k_big - 1) & m32)
    return ends or (q & (below | ((k_min - 1) & m32))) == 0


@pytest.mark.parametrize("k", UNIFORM)
def test_uniform_blocks_end_where_the_passes_start(hrt, k):
    lib = hrt.load_library()
    magic = min((1 << 32) // k, 0xffffffff)
    for spp in range(1, 301):
        rc, first = _schedule(lib, spp, k, 0)
        assert rc == 0, (rc, spp, k)          # (the library's own walk with hold_ends agreed with its passes)
        assert first == list(range(0, spp, k)) + [spp], (spp, k, first)
        # ... and so does the same arithmetic here, against the same passes
        for p in range(1, spp + 1):
            assert _hold_ends(spp, k, magic, 0, 0, p) == (p in first[1:]), (spp, k, p)


@pytest.mark.parametrize("big,small", TAPERS)
def test_tapered_blocks_end_where_the_passes_start(hrt, big, small):
    lib = hrt.load_library()
    for spp in range(1, 301):
        rc, first = _schedule(lib, spp, big, small)
        assert rc == 0, (rc, spp, big, small)
        k_big = big
        while k_big > 1 and k_big > spp:
            k_big >>= 1
        k_min, taper_end = min(small, k_big), spp // k_big * k_big           # (path_plan.h: sample_schedule)
        for p in range(1, spp + 1):
            assert _hold_ends(spp, k_big, 0, k_min, taper_end, p) == (p in first[1:]), (spp, big, small, p)


def test_the_library_walks_its_schedules_with_hold_ends():
    api = (CSRC / "hrt_api.cpp").read_text()
    body = api.split("int hrt_sample_schedule(")[1].split("\n}\n")[0]
    assert "hold_ends(spp, sc.k_big, magic," in body and "return HRT_ERR_STATE" in body
    lane = (CSRC / "path_lane.h").read_text()
    assert lane.count("ends = hold_ends(a.path.spp, a.path.sample_block, a.path.block_magic, a.path.block_min, a.path.block_taper_end, P.px_sample);") == 1


@pytest.fixture(scope="module")
def direct(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("primary_miss_block")
    k = path_kernels.one(path_kernels.compile_unit("fused_direct", tmp / "fused_direct.s"))
    return {"body": k["body"], "meta": k["meta"]}


def test_nothing_spilled_no_scratch_no_flat(direct):
    meta = direct["meta"]
    print("k_path_direct", meta)
    assert meta["vgpr_count"] <= 128 and meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, meta
    assert meta.get("private_segment_fixed_size", 0) == 0, meta
    assert meta["group_segment_fixed_size"] == 10240, meta
    ops = [op for op, _ in loop_stats.instructions(direct["body"])]
    assert not any(op.startswith("flat_") or op.startswith("scratch_") for op in ops)


def test_the_knob_its_row_and_its_way_to_the_kernel():
    knobs = (CSRC / "knobs.def").read_text()
    line = next(l for l in knobs.splitlines() if l.startswith('HRT_KNOB("HRT_MISS_BLOCK", "1"'))
    assert "ctx->miss_block = std::atoi(e) != 0" in line
    table = knob_table.table()
    assert "| `HRT_MISS_BLOCK` | 1 |" in table
    assert knob_table.current((ROOT / "INTEGRATION.md").read_text()) == table
    assert "bool miss_block = true;" in (CSRC / "hrt_internal.hpp").read_text()
    # it travels in a field of the kernel's arguments that a block render does not have, set for k_path_direct's launches alone, and the
    # regeneration reads it there: no argument is added, so no other kernel's argument block moves
    assert "pa.trace_any = l.kernel == PathKernel::Direct && ctx->miss_block ? 1u : 0u;" in (CSRC / "hrt_api.cpp").read_text()
    lane = (CSRC / "path_lane.h").read_text()
    block = lane.split("if constexpr (V::kDirect) {\n            // The miss block")[1].split("if (ends) {")[0]
    assert "if (miss && P.px_depth == 1u && !restartable && a.seed_primary >= 2 && a.path.trace_any != 0u) {" in block
    assert "++P.px_sample; ++P.px_rays_closest;" in block
    assert "s_seed + tx, s.binst, s.tlo > tmin, s_restart + tx);" in (CSRC / "fused_body.h").read_text()


REFILL_PROGRAM = r"""
#include <hip/hip_runtime.h>
#include <cstdio>
#include "path_plan.h"
using namespace hrt;
int main() {
    // every kernel, with the render's 20 and the two-level trees' 12, while nobody set HRT_REFILL_THRESHOLD and after somebody did
    for (int k = 0; k <= (int)PathKernel::Direct; ++k)          // (the last enumerator)
        std::printf("%d %d %d %d %d\n", k, (int)((PathKernel)k == PathKernel::Direct), launch_refill_threshold((PathKernel)k, 20, true),
                    launch_refill_threshold((PathKernel)k, 12, true), launch_refill_threshold((PathKernel)k, 27, false));
    return 0;
}
"""


def test_only_k_path_directs_launches_get_their_own_refill_threshold(tmp_path):
    """path_plan.h: launch_refill_threshold -- 26 for a launch of k_path_direct while HRT_REFILL_THRESHOLD is unset, the render's value for every
    other kernel, and an explicit HRT_REFILL_THRESHOLD for all of them"""
    import subprocess
    src, exe = tmp_path / "refill.cpp", tmp_path / "refill"
    src.write_text(REFILL_PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{ROOT / 'include'}", f"-I{CSRC}", "-o", str(exe), str(src)])
    rows = [[int(x) for x in line.split()] for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()]
    assert len(rows) == 10 and sum(r[1] for r in rows) == 1
    for k, is_direct, auto20, auto12, explicit in rows:
        assert (auto20, auto12, explicit) == ((26, 26, 27) if is_direct else (20, 12, 27)), (k, auto20, auto12, explicit)
    api = (CSRC / "hrt_api.cpp").read_text()
    assert "ta.refill_threshold = launch_refill_threshold(l.kernel, render_refill, ctx->refill_auto);" in api
