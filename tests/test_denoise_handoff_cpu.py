"""The denoiser's history hand-over across TLAS handles without a GPU (include/hrt.h hrt_denoise_temporal_rebind): properties of the
numpy specification (tests/denoise_handoff_ref.py) that the GPU tests pin k_denoise_temporal_linked to, over the oracle's primary
hits; the public header; the library's argument checks; and what csrc/denoise_link.hip compiles to."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import denoise_handoff_cases as cases
import denoise_handoff_ref as href

ROOT = Path(__file__).resolve().parent.parent
NO = int(href.NO_INSTANCE)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    gn, wn = np.isnan(got), np.isnan(want)
    return np.array_equal(gn, wn) and np.array_equal(_bits(np.where(gn, 0, got)), _bits(np.where(wn, 0, want)))


def _colors(seed, n, h, w):
    rng = np.random.default_rng(seed)
    return [rng.uniform(0, 1, (h, w, 4)).astype(np.float32) for _ in range(n)]


@pytest.fixture(scope="module")
def history(hrt, oracle):
    """{variance: (scene, camera, colours, history after two frames on TLAS A)} at 61 x 37, computed once and left unchanged."""
    w, h = cases.SIZES[1]
    sc = cases.scene(hrt, w, h)
    cam = cases.camera(hrt, sc)
    out = {}
    for variance in (False, True):
        col = _colors(11, 3, h, w)
        hist = None
        for k in range(2):
            cur = href.sub_scene(sc, None, cases.poses(hrt, k))
            _, hist = cases.spec_frame(oracle, variance, hist, None, col[k], cur, cam, w, h)
        out[variance] = (sc, cam, col, hist)
    return out


@pytest.mark.parametrize("variance", [False, True])
def test_spec_identity_handover_is_the_unlinked_continuation(hrt, oracle, history, variance):
    """The identity map onto an identical instance list: every output equals the ordinary next call's, bit for bit."""
    w, h = cases.SIZES[1]
    sc, cam, col, hist = history[variance]
    nxt = href.sub_scene(sc, None, cases.poses(hrt, 2))
    want, hw = cases.spec_frame(oracle, variance, hist, None, col[2], nxt, cam, w, h)
    link = href.make_link(href.blas_ids(sc), href.blas_ids(sc))
    assert np.array_equal(link, np.arange(len(sc["instances"]), dtype=np.uint32))
    got, hg = cases.spec_frame(oracle, variance, hist, link, col[2], nxt, cam, w, h)
    for k in want:
        assert _same(got[k], want[k]), k
    for k in ("inst", "prim", "depth", "xf"):
        assert np.array_equal(hg[k], hw[k]), k
    assert (want["L"] > 1).sum() > 0.3 * (want["L"] > 0).sum()


@pytest.mark.parametrize("variance", [False, True])
def test_spec_permuted_handover_is_the_sequence_relabelled(hrt, oracle, history, variance):
    """TLAS B lists the instances in another order, with that order as the map: the images are the unpermuted continuation's and the
    history's instance ids are B's."""
    w, h = cases.SIZES[1]
    sc, cam, col, hist = history[variance]
    n = len(sc["instances"])
    order = [int(k) for k in np.random.default_rng(5).permutation(n)]
    p2 = cases.poses(hrt, 2)
    want, hw = cases.spec_frame(oracle, variance, hist, None, col[2], href.sub_scene(sc, None, p2), cam, w, h)
    link = href.make_link(href.blas_ids(sc), href.blas_ids(sc, order), order)
    assert np.array_equal(link, np.asarray(order, np.uint32))
    got, hg = cases.spec_frame(oracle, variance, hist, link, col[2], href.sub_scene(sc, order, p2[order]), cam, w, h)
    for k in want:
        assert _same(got[k], want[k]), k
    hit = hw["inst"] != href.MISS
    assert np.array_equal(hit, hg["inst"] != href.MISS)
    assert np.array_equal(np.asarray(order, np.uint32)[hg["inst"][hit]], hw["inst"][hit])


@pytest.mark.parametrize("variance", [False, True])
def test_spec_uncarried_instance_starts_afresh_and_touches_nothing_else(hrt, oracle, history, variance):
    """One visible instance mapped to HRT_NO_INSTANCE: L = 1 and NaN motion on all its pixels, A = C there; every other pixel is the
    identity hand-over's bit for bit (before the filter, which mixes neighbours)."""
    w, h = cases.SIZES[1]
    sc, cam, col, hist = history[variance]
    n = len(sc["instances"])
    nxt = href.sub_scene(sc, None, cases.poses(hrt, 2))
    ident = list(range(n))
    want, hw = cases.spec_frame(oracle, variance, hist, href.make_link(href.blas_ids(sc), href.blas_ids(sc), ident), col[2], nxt, cam, w, h)
    ids, counts = np.unique(hw["inst"][(hw["inst"] != href.MISS) & (hw["inst"] != 0)], return_counts=True)
    victim = int(ids[np.argmax(counts)])                      # the particle with the most pixels
    assert (want["L"][hw["inst"] == victim] > 1).any()
    m = list(ident)
    m[victim] = NO
    got, hg = cases.spec_frame(oracle, variance, hist, href.make_link(href.blas_ids(sc), href.blas_ids(sc), m), col[2], nxt, cam, w, h)
    on = hg["inst"] == victim
    assert on.sum() > 5
    assert np.all(got["L"][on] == 1) and np.isnan(got["motion"][on]).all()
    assert np.array_equal(_bits(got["A"][on]), _bits(col[2][on]))
    for k in ("A", "L", "motion") + (("M",) if variance else ()):
        assert _same(got[k][~on], want[k][~on]), k
    # ... and a BLAS that differs at an index does the same through make_link (a NULL map over another geometry)
    other = next(k for k in range(1, n) if href.blas_ids(sc)[k] != href.blas_ids(sc)[victim])
    swapped = ident[:victim] + [other] + ident[victim + 1:]
    assert href.make_link(href.blas_ids(sc), href.blas_ids(sc, swapped))[victim] == NO


@pytest.mark.parametrize("size", cases.SIZES)
def test_spec_sequence_reuses_history_across_the_handover(hrt, oracle, size):
    """The GPU test's sequence (cases.SEQUENCE): on frame 3, the first on TLAS B, more than 0.3 of the hit pixels have L > 1 -- the
    figure test_temporal_bit_exact asks of its frames -- so the bit-exact comparison there is of a blend, not of a fresh start."""
    w, h = size
    sc = cases.scene(hrt, w, h)
    cam = cases.camera(hrt, sc)
    col = _colors(3, len(cases.SEQUENCE), h, w)
    hist, prev_tlas = None, "A"
    for k, (tlas, pose) in enumerate(cases.SEQUENCE):
        link = href.make_link(href.blas_ids(sc), href.blas_ids(sc)) if tlas != prev_tlas else None
        r, hist = cases.spec_frame(oracle, False, hist, link, col[k], href.sub_scene(sc, None, cases.poses(hrt, pose)), cam, w, h)
        share = (r["L"] > 1).sum() / max((r["L"] > 0).sum(), 1)
        print(f"{w}x{h} frame {k} on {tlas}: hit pixels with history {share:.3f}")
        if k > 0:
            assert share > 0.3, (k, share)
        prev_tlas = tlas


def test_header_declares_the_call(hrt, tmp_path):
    """include/hrt.h compiles as C++ and as C with the new call, its constant and the new statistics field (ahead of the three counters that
    tests/test_primary_capture_cpu.py pins as the structure's last); the ctypes mirror of HrtStats has the same size and the field at
    the same offset."""
    body = ('#include <stddef.h>\n#include "hrt.h"\n'
            'int (*rebind)(HrtContext *, HrtTraversable, const uint32_t *, uint32_t, void *) = hrt_denoise_temporal_rebind;\n'
            'unsigned none = HRT_NO_INSTANCE;\n'
            'char field_at[offsetof(HrtStats, denoise_history_rebinds) + 8 == offsetof(HrtStats, primary_capture_launches) ? 1 : -1];\n'
            'char stats_size[sizeof(HrtStats) == %d ? 1 : -1];\n'
            'int main(void) { return 0; }\n' % C.sizeof(hrt.Stats))
    for name, compiler in (("check.cpp", ["g++", "-std=c++17"]), ("check.c", ["gcc", "-std=c11"])):
        src = tmp_path / name
        src.write_text(body)
        subprocess.run([*compiler, "-fsyntax-only", f"-I{ROOT / 'include'}", str(src)], check=True)
    assert hrt.Stats.denoise_history_rebinds.offset + 8 == hrt.Stats.primary_capture_launches.offset
    assert hrt.NO_INSTANCE == 0xFFFFFFFF and "hrt_denoise_temporal_rebind" in hrt.EXPORTS


def test_rebind_refuses_a_null_context(hrt):
    lib = hrt.load_library()
    assert lib.hrt_denoise_temporal_rebind(None, 0x1000, None, 0, None) == -1


@pytest.fixture(scope="module")
def link_kernels(tmp_path_factory):
    """{mangled kernel name: {metadata key: int}} of csrc/denoise_link.hip, compiled with the Makefile's flags
    (in the manner of tests/test_denoise_kernels_cpu.py)"""
    sys.path.insert(0, str(ROOT / "tools"))
    from audit_asm_loads import makefile_hipflags
    asm = tmp_path_factory.mktemp("denoise_link") / "denoise_link.s"
    flags = [f for f in makefile_hipflags() if f != "-fPIC"]
    subprocess.check_call(["/opt/rocm/bin/hipcc", *flags, "-S", "--cuda-device-only", "-o", str(asm), "nvidia-optix-ray-tracer_amd/csrc/denoise_link.hip"],
                          cwd=ROOT, stderr=subprocess.DEVNULL)
    out = {}
    for entry in asm.read_text().split("amdhsa.kernels:")[1].split("\n  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", entry).group(1)
        out[name] = {k: int(v) for k, v in re.findall(r"^    \.(\w+):\s+(\d+)\s*$", entry, re.M)}
    return out


def test_link_unit_holds_two_kernels_without_scratch(link_kernels):
    assert len(link_kernels) == 2 and all("k_denoise_temporal_linked" in k for k in link_kernels), sorted(link_kernels)
    assert sum("ILb0E" in k for k in link_kernels) == 1 and sum("ILb1E" in k for k in link_kernels) == 1
    for name, meta in link_kernels.items():
        assert meta["private_segment_fixed_size"] == 0, (name, meta)
        # its argument segment is the unlinked kernels' 200 bytes and the table's pointer behind them (device_types.h)
        assert meta["kernarg_segment_size"] >= 208, (name, meta)
