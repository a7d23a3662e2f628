"""What csrc/denoise.hip compiles to: one pass kernel, k_denoise_pass<kSquarings, kVariance>, in four
instantiations and no second copy of it; nothing in any denoise kernel spilled to scratch; and the pass's registers within the waves per
SIMD that profiles/r12_denoise_variance.txt records.  Read from the code-object metadata of the assembly the Makefile's flags produce,
compiled once for the module (in the manner of tests/test_path_kernel_spills_cpu.py)."""
import re
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SOURCE = "nvidia-optix-ray-tracer_amd/csrc/denoise.hip"
# <kSquarings, kVariance> as mangled -> waves per SIMD (profiles/r12_denoise_variance.txt: plain <3>, <-1> 7; variance <3> 5, <-1> 6)
PASS_WAVES = {"ILi3ELb0E": 7, "ILin1ELb0E": 7, "ILi3ELb1E": 5, "ILin1ELb1E": 6}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{mangled kernel name: {metadata key: int}} of every kernel of denoise.hip"""
    sys.path.insert(0, str(ROOT / "tools"))
    from audit_asm_loads import makefile_hipflags
    asm = tmp_path_factory.mktemp("denoise_kernels") / "denoise.s"
    flags = [f for f in makefile_hipflags() if f != "-fPIC"]
    subprocess.check_call(["/opt/rocm/bin/hipcc", *flags, "-S", "--cuda-device-only", "-o", str(asm), SOURCE], cwd=ROOT, stderr=subprocess.DEVNULL)
    out = {}
    for entry in asm.read_text().split("amdhsa.kernels:")[1].split("\n  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", entry).group(1)
        out[name] = {k: int(v) for k, v in re.findall(r"^    \.(\w+):\s+(\d+)\s*$", entry, re.M)}
    return out


def _waves_per_simd(vgprs):
    """512 VGPRs per lane and SIMD, allocated in blocks of 8, at most 8 waves"""
    return min(8, 512 // (-(-vgprs // 8) * 8))


def test_one_pass_kernel_in_four_instantiations(kernels):
    passes = sorted(k for k in kernels if "k_denoise_pass" in k)
    assert len(passes) == 4 and not any("k_denoise_pass_var" in k for k in kernels), sorted(kernels)
    assert all(sum("k_denoise_pass" + inst in k for k in passes) == 1 for inst in PASS_WAVES), passes
    assert len(kernels) == 9 and all("k_denoise_" in k for k in kernels), sorted(kernels)      # rays, guides, temporal x 2, variance


def test_no_denoise_kernel_uses_scratch(kernels):
    for name, meta in kernels.items():
        assert meta["private_segment_fixed_size"] == 0, (name, meta)


@pytest.mark.parametrize("instantiation", sorted(PASS_WAVES))
def test_pass_kernel_keeps_its_waves_per_simd(kernels, instantiation):
    (meta,) = [m for k, m in kernels.items() if "k_denoise_pass" + instantiation in k]
    assert _waves_per_simd(meta["vgpr_count"]) == PASS_WAVES[instantiation], meta
