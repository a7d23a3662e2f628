"""The denoiser's history hand-over across rebuilt BLASes without a GPU (include/hrt.h hrt_denoise_temporal_rebind_geometry): properties
of the numpy specification (tests/denoise_by_primitive_ref.py) that the GPU tests pin k_denoise_temporal_by_prim to, over the oracle's
primary hits; the public header; the library's argument check; and what csrc/denoise_link_prim.hip compiles to."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import denoise_by_primitive_cases as cases
import denoise_by_primitive_ref as pref
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


def _link(prev_scene, next_scene, prev_instance=None):
    link, by_prim = pref.make_link(pref.blas_info(prev_scene), pref.blas_info(next_scene), prev_instance)
    return link, by_prim, pref.scene_verts(prev_scene)


@pytest.fixture(scope="module")
def history(hrt, oracle):
    """{variance: (scene, camera, colours, the scene of the last frame on A, history after two frames on TLAS A)} at 96 x 64 (at
    61 x 37 a particle covers a pixel or two), computed once and left unchanged."""
    w, h = cases.SIZES[0]
    sc = cases.scene(hrt, w, h)
    cam = cases.camera(hrt, sc)
    out = {}
    for variance in (False, True):
        col = _colors(11, 3, h, w)
        hist = None
        for k in range(2):
            cur = href.sub_scene(sc, None, cases.poses(hrt, k))
            _, hist = cases.spec_frame(oracle, variance, hist, None, col[k], cur, cam, w, h)
        out[variance] = (sc, cam, col, cur, hist)
    return out


@pytest.mark.parametrize("size", cases.SIZES)
def test_cases_carry_history_by_primitive(hrt, oracle, size):
    """cases.SEQUENCE with TLAS B over the deformed half of the particles: on frame 3, the first on B, more than 0.3 of the hit
    pixels linked by primitive have L > 1 in the specification alone -- the GPU test's bit-exact comparison there is of a blend
    through the previous vertices, not of a fresh start -- and every deformed particle is linked by primitive, nothing else is."""
    w, h = size
    sc = cases.scene(hrt, w, h)
    cam = cases.camera(hrt, sc)
    col = _colors(3, len(cases.SEQUENCE), h, w)
    hist, on, prev = None, "A", None
    for k, (tlas, pose) in enumerate(cases.SEQUENCE):
        cur = cases.scene_b(hrt, sc, pose) if tlas == "B" else href.sub_scene(sc, None, cases.poses(hrt, pose))
        link = _link(prev, cur) if tlas != on else None
        r, hist = cases.spec_frame(oracle, False, hist, link, col[k], cur, cam, w, h)
        if link is not None:
            assert sorted(np.nonzero(link[1])[0]) == cases.DEFORMED and np.array_equal(link[0], np.arange(len(link[0])))
            px = cases.by_primitive_pixels(hist, link[1])
            share = (r["L"][px] > 1).sum() / max(px.sum(), 1)
            print(f"{w}x{h} frame {k}: {px.sum()} by-primitive hit pixels, with history {share:.3f}")
            assert px.any() and share > 0.3, (px.sum(), share)
            rigid = (hist["inst"] != href.MISS) & ~px
            assert (r["L"][rigid] > 1).any()
        on, prev = tlas, cur


def test_spec_without_by_primitive_entries_is_the_handoff_specification(hrt, oracle, history):
    """Between TLASes that share every BLAS, the by-primitive specification is denoise_handoff_ref's bit for bit."""
    w, h = cases.SIZES[0]
    for variance in (False, True):
        sc, cam, col, last, hist = history[variance]
        nxt = href.sub_scene(sc, None, cases.poses(hrt, 2))
        link = _link(last, nxt)
        assert not link[1].any() and np.array_equal(link[0], href.make_link(href.blas_ids(sc), href.blas_ids(sc)))
        got, _ = cases.spec_frame(oracle, variance, hist, link, col[2], nxt, cam, w, h)
        import denoise_handoff_cases as hcases
        want, _ = hcases.spec_frame(oracle, variance, hist, link[0], col[2], nxt, cam, w, h)
        for k in want:
            assert _same(got[k], want[k]), k


def test_spec_rebaked_identity(hrt, oracle):
    """The same bodies baked differently: new vertices = old vertices x 2 and the instance's transform x 0.5, both exact in float32,
    under a static camera and static poses.  By primitive, every carried hit pixel's Po mapped to the world lies within 64 ulp of the
    largest coordinate among these points and the camera's centre -- the particles' part of the scene -- from o + d t (two rounded
    three-term sums against one rounded ray-point evaluation; measured: 24.6 ulp of 2.2), and the motion lands on the pixel's own
    centre to within 0.01 pixel (the rounding is about 1e-4 pixel at these sizes; measured: 4.6e-5 pixel).  Independent of the
    restatement's own arithmetic, this pins the vertex order and the roles of u and v: with u and v exchanged, or the vertices in
    another order, Po lands elsewhere on the triangle."""
    w, h = cases.SIZES[0]
    sc = cases.scene(hrt, w, h)
    cam = cases.camera(hrt, sc)
    col = _colors(5, 2, h, w)
    a = href.sub_scene(sc, None, cases.poses(hrt, 1))
    _, hist = cases.spec_frame(oracle, False, None, None, col[0], a, cam, w, h)
    subset = list(range(1, cases.N_PARTICLES + 1))
    tf = cases.poses(hrt, 1).copy()
    tf[subset] = (tf[subset].reshape(-1, 3, 4) * np.array([0.5, 0.5, 0.5, 1.0], np.float32)).reshape(-1, 12)
    verts = {j: (sc["instances"][j]["vertices"] * np.float32(2)).astype(np.float32) for j in subset}
    b = pref.with_vertices(href.sub_scene(sc, None, tf), verts, {j: sc["instances"][j]["normals"] for j in subset}, "baked")
    link = _link(a, b)
    assert sorted(np.nonzero(link[1])[0]) == subset
    diag = {}
    r, hist2 = cases.spec_frame(oracle, False, hist, link, col[1], b, cam, w, h, diag=diag)
    bp = diag["by_prim"]
    assert bp.sum() > 100, bp.sum()
    sel, po = diag["sel"][bp], diag["po"][bp]
    inst = hist2["inst"].reshape(-1)[sel].astype(np.int64)
    xf = cases.poses(hrt, 1)[inst].astype(np.float64).reshape(-1, 3, 4)
    world = np.einsum("nij,nj->ni", xf[:, :, :3], po.astype(np.float64)) + xf[:, :, 3]
    import denoise_ref as ref
    dirs = ref.primary_directions(w, h, *cam[1:])
    hp = np.asarray(cam[0], np.float64) + dirs[sel].astype(np.float64) * hist2["depth"].reshape(-1)[sel].astype(np.float64)[:, None]
    largest = max(np.abs(world).max(), np.abs(hp).max(), np.abs(np.asarray(cam[0])).max())      # (the ray's origin: what o + d t rounds at)
    ulp = float(np.spacing(np.float32(largest)))
    err = np.abs(world - hp).max() / ulp
    ys, xs = np.divmod(sel, w)
    mo = r["motion"].reshape(-1, 2)[sel].astype(np.float64)
    assert np.isfinite(mo).all()
    off = np.abs(mo - np.stack([xs, ys], axis=1)).max()
    print(f"re-baked identity: {bp.sum()} pixels, |X Po - (o + d t)| max {err:.2f} ulp of {largest:.3f}, motion off centre max {off:.3g} px")
    assert err <= 64
    assert off <= 0.01
    assert (r["L"].reshape(-1)[sel] == 2).all()           # a static scene: every such pixel finds its own history


@pytest.mark.parametrize("variance", [False, True])
def test_spec_permuted_by_primitive_handover_is_the_sequence_relabelled(hrt, oracle, history, variance):
    """TLAS B lists the instances in another order, the deformed ones among them, with that order as the map: the images are the
    unpermuted by-primitive continuation's and the history's instance ids are B's."""
    w, h = cases.SIZES[0]
    sc, cam, col, last, hist = history[variance]
    n = len(sc["instances"])
    order = [int(k) for k in np.random.default_rng(5).permutation(n)]
    b = cases.scene_b(hrt, sc, 2)
    link = _link(last, b)
    want, hw = cases.spec_frame(oracle, variance, hist, link, col[2], b, cam, w, h)
    bperm = {k: v for k, v in b.items() if k != "instances"}
    bperm["instances"] = [b["instances"][k] for k in order]
    lp = pref.make_link(pref.blas_info(last), pref.blas_info(bperm, order), order) + (pref.scene_verts(last),)
    assert np.array_equal(lp[0], np.asarray(order, np.uint32)) and np.array_equal(lp[1], link[1][order]) and lp[1].sum() == len(cases.DEFORMED)
    got, hg = cases.spec_frame(oracle, variance, hist, lp, col[2], bperm, cam, w, h)
    for k in want:
        assert _same(got[k], want[k]), k
    hit = hw["inst"] != href.MISS
    assert np.array_equal(hit, hg["inst"] != href.MISS)
    assert np.array_equal(np.asarray(order, np.uint32)[hg["inst"][hit]], hw["inst"][hit])


def _swap_cases(sc, victim):
    """name -> (the instance dict that replaces scene instance `victim`, a deformed particle, on B, or None; the predecessor it
    claims): a sphere BLAS where a triangle BLAS was, a triangle BLAS of another count, and the deformed triangles claiming the ground
    sphere as their predecessor."""
    inst = sc["instances"]
    small = next(k for k in cases.DEFORMED if len(inst[k]["vertices"]) != len(inst[victim]["vertices"]))
    sphere = dict(inst[0], centers=np.zeros((1, 3), np.float32), radii=np.array([0.06], np.float32), own=("sphere", victim))
    other = dict(inst[small], own=("other-count", victim))
    return {"sphere_for_triangles": (sphere, victim), "other_count": (other, victim), "triangles_for_sphere": (None, 0)}


@pytest.mark.parametrize("case", ["sphere_for_triangles", "other_count", "triangles_for_sphere"])
def test_spec_ineligible_entry_starts_afresh_and_touches_nothing_else(hrt, oracle, history, case):
    """A predecessor that cannot be linked by primitive -- a sphere BLAS on either side, another primitive count -- makes its entry
    HRT_NO_INSTANCE: L = 1, NaN motion and A = C on the instance's pixels, and every other pixel holds the bits it has when the same
    B is linked with that entry HRT_NO_INSTANCE by the caller (before the filter, which mixes neighbours).  The instance is the
    deformed particle with the most pixels on A."""
    w, h = cases.SIZES[0]
    sc, cam, col, last, hist = history[False]
    counts = [(hist["inst"] == j).sum() for j in cases.DEFORMED]
    victim = cases.DEFORMED[int(np.argmax(counts))]
    repl, pred = _swap_cases(sc, victim)[case]
    b = cases.scene_b(hrt, sc, 2)
    if repl is not None:
        b["instances"][victim] = dict(repl, transform=b["instances"][victim]["transform"])
    m = list(range(len(b["instances"])))
    m[victim] = pred
    link = _link(last, b, m)
    assert link[0][victim] == NO and not link[1][victim] and link[1].sum() == len(cases.DEFORMED) - 1
    got, hg = cases.spec_frame(oracle, False, hist, link, col[2], b, cam, w, h)
    on = hg["inst"] == victim
    assert on.any()
    assert np.all(got["L"][on] == 1) and np.isnan(got["motion"][on]).all()
    assert np.array_equal(_bits(got["A"][on]), _bits(col[2][on]))
    m[victim] = NO
    want, _ = cases.spec_frame(oracle, False, hist, _link(last, b, m), col[2], b, cam, w, h)
    for k in ("A", "L", "motion"):
        assert _same(got[k], want[k]), k
    px = cases.by_primitive_pixels(hg, link[1])
    assert (got["L"][px] > 1).any() and (got["L"][~on & ~px] > 1).any()


def test_header_declares_the_call(hrt, tmp_path):
    """include/hrt.h compiles as C++ and as C with the new call and the new statistics field, directly ahead of
    denoise_history_rebinds; the ctypes mirror of HrtStats has the same size and the field at the same offset."""
    body = ('#include <stddef.h>\n#include "hrt.h"\n'
            'int (*rebind)(HrtContext *, HrtTraversable, const uint32_t *, uint32_t, void *) = hrt_denoise_temporal_rebind_geometry;\n'
            'char field_at[offsetof(HrtStats, denoise_by_primitive_links) + 8 == offsetof(HrtStats, denoise_history_rebinds) ? 1 : -1];\n'
            'char after[offsetof(HrtStats, one_group_launches) + 8 == offsetof(HrtStats, denoise_by_primitive_links) ? 1 : -1];\n'
            'char stats_size[sizeof(HrtStats) == %d ? 1 : -1];\n'
            'int main(void) { return 0; }\n' % C.sizeof(hrt.Stats))
    for name, compiler in (("check.cpp", ["g++", "-std=c++17"]), ("check.c", ["gcc", "-std=c11"])):
        src = tmp_path / name
        src.write_text(body)
        subprocess.run([*compiler, "-fsyntax-only", f"-I{ROOT / 'include'}", str(src)], check=True)
    assert hrt.Stats.denoise_by_primitive_links.offset + 8 == hrt.Stats.denoise_history_rebinds.offset
    assert hrt.Stats.denoise_history_rebinds.offset + 8 == hrt.Stats.primary_capture_launches.offset
    assert "hrt_denoise_temporal_rebind_geometry" in hrt.EXPORTS


def test_rebind_geometry_refuses_a_null_context(hrt):
    lib = hrt.load_library()
    assert lib.hrt_denoise_temporal_rebind_geometry(None, 0x1000, None, 0, None) == -1


@pytest.fixture(scope="module")
def prim_kernels(tmp_path_factory):
    """{mangled kernel name: {metadata key: int}} of csrc/denoise_link_prim.hip, compiled with the Makefile's flags"""
    sys.path.insert(0, str(ROOT / "tools"))
    from audit_asm_loads import makefile_hipflags
    asm = tmp_path_factory.mktemp("denoise_link_prim") / "denoise_link_prim.s"
    flags = [f for f in makefile_hipflags() if f != "-fPIC"]
    subprocess.check_call(["/opt/rocm/bin/hipcc", *flags, "-S", "--cuda-device-only", "-o", str(asm),
                           "nvidia-optix-ray-tracer_amd/csrc/denoise_link_prim.hip"], cwd=ROOT, stderr=subprocess.DEVNULL)
    out = {}
    for entry in asm.read_text().split("amdhsa.kernels:")[1].split("\n  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", entry).group(1)
        out[name] = {k: int(v) for k, v in re.findall(r"^    \.(\w+):\s+(\d+)\s*$", entry, re.M)}
    return out


def test_by_primitive_unit_holds_two_kernels_without_scratch(prim_kernels):
    assert len(prim_kernels) == 2 and all("k_denoise_temporal_by_prim" in k for k in prim_kernels), sorted(prim_kernels)
    assert sum("ILb0E" in k for k in prim_kernels) == 1 and sum("ILb1E" in k for k in prim_kernels) == 1
    for name, meta in prim_kernels.items():
        assert meta["private_segment_fixed_size"] == 0, (name, meta)
        # its argument segment is the unlinked kernels' 200 bytes and the two tables' pointers behind them (device_types.h)
        assert meta["kernarg_segment_size"] >= 216, (name, meta)
