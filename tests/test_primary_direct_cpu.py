"""The argument behind HRT_PRIMARY_DIRECT (DESIGN.md sections 2.1 "The record tested where the ray is made" and 4.1; csrc/fused_direct.hip), on
the CPU.  A pixel's repeat primary ray is the ray whose complete walk accepted its hit from record R of primitive W at t.  k_path_direct does not
walk again: the regeneration that makes the ray fetches R and runs the canonical primitive test on it with the culling bound at t.  Three parts,
none needs a GPU:
  (a) with the numpy walker and the canonical test of tests/test_primary_restart_cpu.py, on the 3000-triangle soup with and without spatial splits
      and with every triangle stored twice: for EVERY hit ray of 1500, the test of the one record the complete walk accepted, with bt = t, is
      accepted by the canonical order (a hit AT the bound against "no hit yet") and gives the same primitive and the same t, u, v bits -- for
      the record of the pixel's first, unwindowed walk as for the record of a windowed walk.  On the split tree the first walk's record is the
      case that k_path_restart had to leave to the root: started at that record's node, inside the window, some rays miss (the node step's
      slot test fails).  Here nothing but the record is tested, so they all reproduce; the test counts them and wants the count non-zero;
  (b) static, from one compilation of fused_direct.hip and one of fused_idle.hip with the Makefile's flags: k_path_direct's first loop copy is
      k_path_idle's, instruction for instruction (opcodes and their split into dual-pipe, single-pipe, scalar and memory), 10240 B of LDS, at
      most 128 VGPRs, nothing spilled, no scratch, no flat_ instruction, no load hazard, and the record's three loads stand in the regeneration in
      front of the path-end code;
  (c) the flag, the variant, the knob and the counter are where the text says, and the kernel has its enumerator and its case of the launch entry.
(That the other translation units' assembly equals the parent commit's cannot be read from one tree: profiles/r30_primary_direct.txt says how it
was checked.)"""
import re
import sys
from pathlib import Path

import numpy as np
import pytest

import test_primary_restart_cpu as pr
from test_host_cpu import _build
from test_primary_window_cpu import _delta

ROOT = Path(__file__).resolve().parent.parent
CSRC = "nvidia-optix-ray-tracer_amd/csrc/"
sys.path.insert(0, str(ROOT / "tools"))
import audit_asm_loads, loop_stats, path_kernels          # noqa: E402
f32 = np.float32
MISS = pr.MISS


# ---------------------------------------------------------------- (a) the record's test ----------------------------------------------------------------
def _record_test_accepts(T, rec, o, d, bt):
    """the regeneration's test of record `rec` against a best hit of (bt, no primitive) -> (accepted, t, u, v, prim)"""
    ok, t, u, v, prim = pr.prim_test(T, rec, o, d)
    accepted = ok and (t < bt or (t == bt and prim < MISS))
    return accepted, t, u, v, prim


def _check_records(hrt, oracle, verts, label):
    """-> (hit rays, rays whose first walk's record misses when the walk is started at its node inside the window)"""
    import ctypes as C
    delta = f32(_delta())
    lib, blob = _build(hrt, verts)
    try:
        T = pr.Tree(blob)
        table = pr.host_table(lib, blob)
        o, d = oracle.random_rays(pr.N_RAYS, 5)
        t, u, v, prim, inst, _, _ = oracle.bvh8_trace(blob.nodes, blob.triangles, o, d)
        hit = np.flatnonzero(prim != MISS)
        assert 0.3 * pr.N_RAYS < len(hit) < pr.N_RAYS
        checked = node_start_misses = 0
        for i in hit:
            oi, di = o[i], d[i]
            # the complete walk from the root, unwindowed: a pixel's first sample.  Its record is what the lane keeps
            ft, fu, fv, fprim, frec, _, _ = pr.walk(T, oi, di)
            assert fprim == prim[i] and pr._bits(ft) == pr._bits(t[i]), (label, i)
            lower = max(pr.TMIN, f32(t[i] * (f32(1.0) - delta)))
            # ... and the windowed root walk: a block's first primary ray, a ray whose test did not accept
            wt, wu, wv, wprim, wrec, _, _ = pr.walk(T, oi, di, 0, t[i], lower)
            assert wprim == prim[i], (label, i)
            for which, rec in (("first walk", frec), ("windowed walk", wrec)):
                assert rec != MISS and int(T.rec_u[rec, 3]) == prim[i], (label, i, which)
                accepted, rt, ru, rv, rprim = _record_test_accepts(T, rec, oi, di, t[i])
                assert accepted, (label, i, which)
                assert rprim == prim[i], (label, i, which, rprim, prim[i])
                assert pr._bits(rt) == pr._bits(t[i]) and pr._bits(ru) == pr._bits(u[i]) and pr._bits(rv) == pr._bits(v[i]), (label, i, which)
            # what k_path_restart could not use: the first walk's record, started at its node inside the window
            node_start_misses += pr.walk(T, oi, di, int(table[frec]), t[i], lower)[3] != prim[i]
            checked += 1
        assert checked == len(hit)          # no ray left out
        print(f"{label}: {checked} hit rays, every accepted record reproduces its hit; {node_start_misses} of them have a first-walk record that misses when started at its node")
        return checked, node_start_misses
    finally:
        lib.hrt_host_free(C.byref(blob))


def test_the_accepted_record_reproduces_the_hit_without_splits(hrt, oracle, monkeypatch):
    monkeypatch.setenv("HRT_SBVH", "0")
    _check_records(hrt, oracle, pr.soup(hrt), "HRT_SBVH=0")


def test_the_first_unwindowed_walks_record_reproduces_the_hit_on_the_split_tree(hrt, oracle, monkeypatch):
    monkeypatch.setenv("HRT_SBVH", "1")
    checked, node_start_misses = _check_records(hrt, oracle, pr.soup(hrt), "HRT_SBVH=1")
    assert node_start_misses > 0, "the split tree no longer has a first-walk record whose node start misses: the case is not exercised"


def test_a_tie_in_t_is_decided_by_the_record_that_won_it(hrt, oracle, monkeypatch):
    """every triangle twice (ids i and i + N): every hit is a tie, the walk accepted it from the lower id's record, and that record's test says so again"""
    monkeypatch.setenv("HRT_SBVH", "0")
    _check_records(hrt, oracle, pr.soup(hrt, twice=True), "every triangle twice")


# ---------------------------------------------------------------- (b) static ----------------------------------------------------------------
@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("primary_direct")
    out = {}
    for key, stem in (("direct", "fused_direct"), ("idle", "fused_idle")):
        k = path_kernels.one(path_kernels.compile_unit(stem, tmp / f"{stem}.s"))
        out[key] = {"text": (tmp / f"{stem}.s").read_text(), "loop": [op for op, _ in loop_stats.instructions(k["lines"])], "body": k["body"], "meta": k["meta"]}
    return out


def test_the_loop_is_k_path_idles(compiled):
    from collections import Counter
    direct, idle = compiled["direct"]["loop"], compiled["idle"]["loop"]
    split = lambda ops: Counter(loop_stats.kind(op) for op in ops)
    print("loop: k_path_direct", len(direct), dict(split(direct)), "k_path_idle", len(idle), dict(split(idle)))
    assert len(direct) == len(idle) == 402, (len(direct), len(idle))
    assert split(direct) == split(idle)
    assert direct == idle           # the same opcodes in the same layout order


def test_one_kernel_its_lds_registers_and_no_spill(compiled):
    k = compiled["direct"]
    assert len(re.findall(r"^\s*\.amdhsa_kernel\s", k["text"], re.M)) == 1
    meta = k["meta"]
    print("k_path_direct", meta)
    assert meta["group_segment_fixed_size"] == 10240, meta
    assert meta["vgpr_count"] <= 128 and meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, meta
    assert meta.get("private_segment_fixed_size", 0) == 0, meta
    ops = [op for op, _ in loop_stats.instructions(k["body"])]
    assert not any(op.startswith("flat_") or op.startswith("scratch_") for op in ops)


def test_the_records_loads_stand_at_the_top_of_the_regeneration(compiled):
    """in layout order: the regeneration's priority, then the record's loads (A whole, three words each of B and C), and only then the first
    store of a path's end -- and k_path_idle has no such loads"""
    ins = [(op, l.strip()) for op, l in loop_stats.instructions(compiled["direct"]["body"])]
    prio = next(i for i, (op, l) in enumerate(ins) if l == "s_setprio 2")
    rec = [i for i, (op, _) in enumerate(ins) if op == "global_load_dwordx3"]
    assert len(rec) == 2 and prio < rec[0], (prio, rec)
    whole = [i for i, (op, l) in enumerate(ins[rec[0] - 3:rec[1] + 3], rec[0] - 3) if op == "global_load_dwordx4"]
    assert len(whole) == 1, whole
    first_store = next(i for i, (op, _) in enumerate(ins) if i > prio and (op.startswith("global_store") or op.startswith("global_atomic")))
    assert max(rec + whole) < first_store, (rec, whole, first_store)
    assert not any(op == "global_load_dwordx3" for op, _ in loop_stats.instructions(compiled["idle"]["body"]))


def test_hand_issued_loads_are_not_touched_before_their_wait():
    groups, bad = audit_asm_loads.audit(*path_kernels.source("fused_direct"))
    assert groups > 0 and bad == 0, (groups, bad)


# ---------------------------------------------------------------- (c) the flag, the variant, the knob, the counter ----------------------------------------------------------------
def test_the_flag_the_variant_the_knob_and_the_counter(hrt):
    for path in sorted((ROOT / CSRC).glob("*.hip")):
        assert "kDirect" not in path.read_text() or path.name == "fused_direct.hip", path.name       # (which points at the headers that read it)
    body = (ROOT / CSRC / "fused_direct.hip").read_text()
    assert re.findall(r"fused_body<([^;]*)>\(", body) == ["DirectVariant"]
    common = (ROOT / CSRC / "trav_common.h").read_text()
    assert "static constexpr bool kDirect = false;" in common
    flags = lambda text, name: (re.search(r"struct " + name + r" : (\S+) \{(.*?)\};", text, re.S).group(1),
                                re.sub(r"\s+", " ", re.search(r"struct " + name + r" : (\S+) \{(.*?)\};", text, re.S).group(2)).strip())
    base_i, flags_i = flags((ROOT / CSRC / "fused_idle.hip").read_text(), "MaskIdleVariant")
    base_d, flags_d = flags(body, "DirectVariant")
    assert "DirectVariant" not in common          # (a kernel's variant lives in the kernel's own unit)
    assert base_d == base_i and flags_d == flags_i.rstrip(";") + ", kDirect = true;", (flags_i, flags_d)
    # an enumerator and a case of the one launch entry like every other kernel: k_path_idle's launcher launches k_path_idle, and no value of
    # seed_primary stands for a kernel
    enum = (ROOT / CSRC / "device_types.h").read_text().split("enum class PathKernel {")[1].split("};")[0]
    assert re.search(r"\bDirect\b", re.sub(r"//.*", "", enum))
    assert "case PathKernel::Direct: launch_path_direct(a, scene, grid_blocks, s); break;" in (ROOT / CSRC / "fused.hip").read_text()
    idle = (ROOT / CSRC / "fused_idle.hip").read_text()
    assert "launch_path_direct" not in idle and "seed_primary" not in idle
    for path in sorted((ROOT / CSRC).rglob("*")):
        if path.is_file():
            assert not re.search(r"seed_primary\s*==?\s*3", path.read_text(errors="replace")), path.name
    knobs = (ROOT / CSRC / "knobs.def").read_text()
    line = next(l for l in knobs.splitlines() if l.startswith('HRT_KNOB("HRT_PRIMARY_DIRECT"'))
    assert "ctx->primary_direct = std::atoi(e) != 0" in line
    seed = next(l for l in knobs.splitlines() if l.startswith('HRT_KNOB("HRT_SEED_PRIMARY"'))
    assert "v >= 0 && v <= 2" in seed                                   # the environment's stays 0..2
    names = [f[0] for f in hrt.Stats._fields_]
    assert names.index("direct_launches") + 1 == names.index("mask_idle_launches")
    assert ("fused_direct", "_ZN3hrt13k_path_direct", "k_path_direct") in path_kernels.UNITS
