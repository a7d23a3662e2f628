"""The argument behind HRT_PRIMARY_RESTART (DESIGN.md section 4.1 "The start under the known hit"; csrc/fused_restart.hip), on the CPU.  A pixel's
repeat primary ray is the ray that found record R of primitive W at t before; with HRT_SEED_PRIMARY=2 it walks inside the window
[t (1 - delta), t] and ends in W again.  k_path_restart starts that walk at leaf_parent[R], the node whose leaf slot holds R, instead of at
the root.  Four parts, none needs a GPU:
  (a) the host's leaf_parent table: every record is covered by exactly one leaf slot, of the node the table names; inner slots cover none;
  (b) a numpy walker over the blob's bytes -- the node step in its window form (tests/test_slab_interval_cpu.py's float32 emulation, all eight
      slots at once) and the canonical primitive test, operation for operation -- that can start at any node (the oracle's walker cannot, and
      oracle/ does not change): the root walk gives the oracle's record, and the walk restarted at leaf_parent[R] gives the same primitive and
      the same t, u, v bits, in no more node visits than the windowed root walk, for EVERY hit ray;
  (c) the same on the soup with every triangle stored twice, where every hit is a tie in t: the lower id wins from the restart as from the root;
  (d) static, from one compilation of fused_restart.hip with the Makefile's flags: one kernel, LDS 10240 B, at most 128 VGPRs, no spill, no
      flat_ or scratch_ instruction, 16 clamped FMAs per loop copy, the loop at most k_path_one's plus the one select.

WHICH record.  R is the record the hit was accepted from in a walk that had the window -- the windowed root walk, which is what a block's first
primary ray and a pixel's second sample are.  The node step depends on the node's bytes, the ray, bt and tlo only, and bt = t from the first
step of a windowed walk to its last, so the node step of leaf_parent[R] passes R's slot again, bit for bit, whatever the tree: R is tested and
W found.  The record of the pixel's FIRST walk, which began at the launch's tmin, is not used: with spatial splits (HRT_SBVH=1) a record's box
is the part of the triangle inside its leaf, the first walk may accept W through a record whose box the ray crosses well before t, and that
slot fails the window.  The test counts such records (printed; the kernel leaves the root for them: path_lane.h, `restartable`).
Both forms of the bound are walked: tmax = nextafter(t), and the kernel's bt = t (a hit at the bound is accepted against "no hit yet")."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest

import test_slab_interval_cpu as si
from test_host_cpu import _build
from test_primary_window_cpu import _delta

ROOT = Path(__file__).resolve().parent.parent
CSRC = "nvidia-optix-ray-tracer_amd/csrc/"
sys.path.insert(0, str(ROOT / "tools"))
import audit_asm_loads, loop_stats, path_kernels          # noqa: E402
f32, f64 = np.float32, np.float64
MISS = 0xFFFFFFFF
TMIN, TMAX = f32(1e-6), f32(1e16)
N_TRIANGLES, N_RAYS = 3000, 1500


# ---------------------------------------------------------------- the blob ----------------------------------------------------------------
class Tree:
    """the blob's bytes as arrays (bvh8.h: Bvh8Node 80 B, PrimRecord 48 B)"""

    def __init__(self, blob):
        n, m = int(blob.n_nodes), int(blob.n_triangles)
        raw = np.frombuffer((C.c_uint8 * (80 * n)).from_address(blob.nodes), np.uint8).reshape(n, 80).copy()
        self.n_nodes, self.n_records = n, m
        self.p = raw[:, 0:12].copy().view(f32).reshape(n, 3)
        self.e = raw[:, 12:15]
        self.imask = raw[:, 15]
        self.child_base = raw[:, 16:20].copy().view(np.uint32).reshape(n)
        self.prim_base = raw[:, 20:24].copy().view(np.uint32).reshape(n)
        self.meta = raw[:, 24:32]
        self.qlo = raw[:, 32:56].reshape(n, 3, 8)
        self.qhi = raw[:, 56:80].reshape(n, 3, 8)
        rec = np.frombuffer((C.c_uint8 * (48 * m)).from_address(blob.triangles), np.uint8).reshape(m, 48).copy()
        self.rec_f = rec.view(f32).reshape(m, 12)
        self.rec_u = rec.view(np.uint32).reshape(m, 12)


def host_table(lib, blob):
    lib.hrt_host_leaf_parent.restype = C.c_int
    lib.hrt_host_leaf_parent.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_uint64]
    out = np.zeros(int(blob.n_triangles), np.uint32)
    rc = lib.hrt_host_leaf_parent(C.byref(blob), out.ctypes.data_as(C.POINTER(C.c_uint32)), len(out))
    assert rc == 0, lib.hrt_last_error(None)
    return out


def soup(hrt, twice=False):
    v = np.asarray(hrt.scenes.random_soup(N_TRIANGLES, 0.12, 17)["instances"][0]["vertices"], f32).reshape(-1, 3, 3)
    return np.concatenate([v, v]) if twice else v


# ---------------------------------------------------------------- (a) the table ----------------------------------------------------------------
@pytest.mark.parametrize("sbvh", ["0", "1"])
def test_every_record_has_exactly_one_leaf_slot_and_the_table_names_its_node(hrt, monkeypatch, sbvh):
    monkeypatch.setenv("HRT_SBVH", sbvh)
    lib, blob = _build(hrt, soup(hrt))
    try:
        assert blob.n_triangles > N_TRIANGLES if sbvh == "1" else blob.n_triangles == N_TRIANGLES
        T = Tree(blob)
        table = host_table(lib, blob)
        covered = np.zeros(T.n_records, np.int64)
        owner = np.full(T.n_records, -1, np.int64)
        inner_slots = leaf_slots = 0
        for n in range(T.n_nodes):
            for s in range(8):
                meta = int(T.meta[n, s])
                inner = (meta & 0x18) == 0x18
                assert inner == bool((int(T.imask[n]) >> s) & 1), (n, s, meta)          # the meta byte and the inner mask agree
                if inner or meta == 0:
                    inner_slots += inner
                    continue
                count = bin(meta >> 5).count("1")
                assert (meta >> 5) in (1, 3, 7) and (meta & 0x1f) < 24, (n, s, meta)
                first = int(T.prim_base[n]) + (meta & 0x1f)
                assert first + count <= T.n_records
                covered[first:first + count] += 1
                owner[first:first + count] = n
                leaf_slots += 1
        assert (covered == 1).all(), np.flatnonzero(covered != 1)[:8]                      # every record once; inner slots contributed nothing
        assert np.array_equal(owner, table.astype(np.int64))
        assert inner_slots == T.n_nodes - 1 and leaf_slots > 0                             # every node but the root is some inner slot's child
        # ... and the entry point refuses a table that is too small
        assert lib.hrt_host_leaf_parent(C.byref(blob), table.ctypes.data_as(C.POINTER(C.c_uint32)), len(table) - 1) != 0
    finally:
        lib.hrt_host_free(C.byref(blob))


# ---------------------------------------------------------------- (b), (c) the walker ----------------------------------------------------------------
def ray_consts(o, d):
    """lean_start: guarded reciprocals, capped, the slack folded in (test_slab_interval_cpu.ray_start with the exact reciprocal)"""
    idx, bt0 = si.ray_start(d[None, :], TMAX, np.zeros((1, 3), np.int64), True)
    return idx[0], bt0[0]


def node_step(T, n, o, d, idx, bt, tlo):
    """node_slab_test<true> (trav_common.h) for the eight slots of node n: the interval [tlo, bt] mapped onto [0, 1], the clamp on the z axis.
    -> bool[8]"""
    with np.errstate(all="ignore"):
        neg = d < 0
        qn = np.where(neg[:, None], T.qhi[n], T.qlo[n]).astype(f32)
        qf = np.where(neg[:, None], T.qlo[n], T.qhi[n]).astype(f32)                        # (3, 8)
        es = (T.e[n].astype(np.uint32) << 23).view(f32)
        k = si.rcp(np.asarray([(f32(bt) - f32(tlo)) + si.FLOOR], f32), np.zeros(1, np.int64))[0]
        kk = (idx * k).astype(f32)
        c0 = f32(-(f32(tlo) * k))
        ai = (es * kk).astype(f32)
        ao = si.fma((T.p[n] - o).astype(f32), kk, np.full(3, c0, f32))
        tn = si.fma(qn, np.broadcast_to(ai[:, None], qn.shape), np.broadcast_to(ao[:, None], qn.shape))
        tf = si.fma(qf, np.broadcast_to(ai[:, None], qf.shape), np.broadcast_to(ao[:, None], qf.shape))
        clamp = lambda x: np.where(np.isnan(x), f32(0), np.minimum(np.maximum(x, f32(0)), f32(1))).astype(f32)
        lo = np.fmax(np.fmax(tn[0], tn[1]), clamp(tn[2]))
        hi = np.fmin(np.fmin(tf[0], tf[1]), clamp(tf[2]))
        return lo < hi


def _dot(a, b):
    return f32(f32(f32(a[0] * b[0]) + f32(a[1] * b[1])) + f32(a[2] * b[2]))


def _cross(a, b):
    return (f32(f32(a[1] * b[2]) - f32(a[2] * b[1])), f32(f32(a[2] * b[0]) - f32(a[0] * b[2])), f32(f32(a[0] * b[1]) - f32(a[1] * b[0])))


def prim_test(T, r, o, d):
    """the canonical test (trav_common.h: test_prim_ray, the straight-line form) of record r -> (ok, t, u, v, prim)"""
    A, B, Cc = T.rec_f[r, 0:3], T.rec_f[r, 4:7], T.rec_f[r, 8:11]
    with np.errstate(all="ignore"):
        pvec = _cross(d, Cc)
        det = _dot(B, pvec)
        inv = f32(1.0) / det
        tvec = (f32(o[0] - A[0]), f32(o[1] - A[1]), f32(o[2] - A[2]))
        u = f32(_dot(tvec, pvec) * inv)
        qvec = _cross(tvec, B)
        v = f32(_dot(d, qvec) * inv)
        t = f32(_dot(Cc, qvec) * inv)
        ok = det != 0 and u >= 0 and v >= 0 and f32(u + v) <= 1 and t > TMIN and t < TMAX
    return bool(ok), t, u, v, int(T.rec_u[r, 3])


def walk(T, o, d, start=0, bt0=None, tlo=TMIN):
    """A closest-hit walk from node `start` with an empty stack.  bt0: the first culling bound (None: the ray's own); tlo: where the node step's
    interval begins.  The canonical order decides: the smaller t, a tie in t to the lower primitive id, "no hit yet" above every id -- so a
    hit AT the bound is accepted once (the kernel's bt = t), like one below it (tmax = nextafter(t)).
    -> (t, u, v, prim, record, node visits, primitive tests)"""
    idx, reach = ray_consts(o, d)
    bt = reach if bt0 is None else min(f32(bt0), reach)
    best = (f32(bt), f32(0), f32(0), MISS, MISS)
    stack, visits, tests = [start], 0, 0
    while stack:
        n = stack.pop()
        visits += 1
        hit = node_step(T, n, o, d, idx, best[0], tlo)
        kids = []
        for s in np.flatnonzero(hit):
            meta = int(T.meta[n, s])
            if meta == 0:
                continue
            if (meta & 0x18) == 0x18:
                kids.append(int(T.child_base[n]) + bin(int(T.imask[n]) & ((1 << int(s)) - 1)).count("1"))
                continue
            first = int(T.prim_base[n]) + (meta & 0x1f)
            for r in range(first, first + bin(meta >> 5).count("1")):
                tests += 1
                ok, t, u, v, prim = prim_test(T, r, o, d)
                if ok and (t < best[0] or (t == best[0] and prim < best[3])):
                    best = (t, u, v, prim, r)
        stack += kids
    return best + (visits, tests)


def _bits(x):
    return np.asarray(x, f32).view(np.uint32)


def _check_restarts(hrt, oracle, verts, label):
    """parts (b) and (c) on one tree -> (windowed root visits, restarted visits, windowed root tests, restarted tests)"""
    delta = f32(_delta())
    lib, blob = _build(hrt, verts)
    try:
        T = Tree(blob)
        table = host_table(lib, blob)
        o, d = oracle.random_rays(N_RAYS, 5)
        t, u, v, prim, inst, _, _ = oracle.bvh8_trace(blob.nodes, blob.triangles, o, d)
        hit = np.flatnonzero(prim != MISS)
        assert 0.3 * N_RAYS < len(hit) < N_RAYS
        root_v = rest_v = root_t = rest_t = checked = depth_sum = first_walk_fails = 0
        for i in hit:
            oi, di = o[i], d[i]
            # the root walk: the oracle's record
            ft, fu, fv, fprim, frec, _, _ = walk(T, oi, di)
            assert fprim == prim[i] and _bits(ft) == _bits(t[i]) and _bits(fu) == _bits(u[i]) and _bits(fv) == _bits(v[i]), (label, i)
            assert int(T.rec_u[frec, 3]) == prim[i]
            lower = max(TMIN, f32(t[i] * (f32(1.0) - delta)))
            for strict, bound in ((True, np.nextafter(t[i], f32(np.inf))), (False, t[i])):      # tmax = nextafter(t); the kernel's bt = t
                # the windowed root walk (a block's first primary ray, a pixel's second sample) notes the record ...
                wt, wu, wv, wprim, wrec, wn, wtests = walk(T, oi, di, 0, bound, lower)
                assert wprim == prim[i] and _bits(wt) == _bits(t[i]) and _bits(wu) == _bits(u[i]) and _bits(wv) == _bits(v[i]), (label, i, strict)
                # ... and the walk restarted at that record's node ends in the same primitive with the same bits, in no more visits
                rt, ru, rv, rprim, rrec, rn, rtests = walk(T, oi, di, int(table[wrec]), bound, lower)
                assert rprim == prim[i], (label, i, strict, rprim, prim[i])               # never a miss, never the tie's other triangle
                assert _bits(rt) == _bits(t[i]) and _bits(ru) == _bits(u[i]) and _bits(rv) == _bits(v[i]), (label, i, strict)
                assert rrec == wrec and rn <= wn, (label, i, strict, rn, wn)
                if not strict:
                    root_v += wn; rest_v += rn; root_t += wtests; rest_t += rtests
            # (for the record: would the FIRST walk's record have done?  Not asserted -- see the module's docstring)
            first_walk_fails += walk(T, oi, di, int(table[frec]), t[i], lower)[3] != prim[i]
            checked += 1
        assert checked == len(hit)                                                         # no ray left out
        assert rest_v < root_v
        print(f"{label}: {checked} hits, node visits per ray {root_v / checked:.3f} (windowed root walk) -> {rest_v / checked:.3f} (restarted), "
              f"primitive tests per ray {root_t / checked:.3f} -> {rest_t / checked:.3f}; totals {root_v} -> {rest_v}, {root_t} -> {rest_t}; "
              f"{first_walk_fails} rays whose first (unwindowed) walk's record would not restart")
        return root_v, rest_v, root_t, rest_t
    finally:
        lib.hrt_host_free(C.byref(blob))


@pytest.mark.parametrize("sbvh", ["0", "1"])
def test_a_walk_restarted_at_the_known_hits_node_finds_it_again_in_fewer_visits(hrt, oracle, monkeypatch, sbvh):
    monkeypatch.setenv("HRT_SBVH", sbvh)
    _check_restarts(hrt, oracle, soup(hrt), f"HRT_SBVH={sbvh}")


def test_a_tie_in_t_goes_to_the_lower_id_from_the_restart_as_from_the_root(hrt, oracle, monkeypatch):
    """every triangle twice (ids i and i + N): every hit is a tie, and the oracle's record is the lower id's"""
    monkeypatch.setenv("HRT_SBVH", "0")
    _check_restarts(hrt, oracle, soup(hrt, twice=True), "every triangle twice")


# ---------------------------------------------------------------- (d) static ----------------------------------------------------------------
@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("primary_restart")
    out = {}
    for key, stem in (("restart", "fused_restart"), ("one", "fused_one")):
        k = path_kernels.one(path_kernels.compile_unit(stem, tmp / f"{stem}.s"))
        out[key] = {"text": (tmp / f"{stem}.s").read_text(), "loop": k["lines"], "body": k["body"], "meta": k["meta"]}
    return out


def test_one_kernel_its_lds_registers_and_no_spill(compiled):
    k = compiled["restart"]
    assert len(re.findall(r"^\s*\.amdhsa_kernel\s", k["text"], re.M)) == 1
    meta = k["meta"]
    print("k_path_restart", meta)
    assert meta["group_segment_fixed_size"] == 10240, meta
    assert meta["vgpr_count"] <= 128 and meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, meta
    assert meta.get("private_segment_fixed_size", 0) == 0, meta
    ops = loop_stats.opcodes(k["body"])
    assert not any(op.startswith("flat_") or op.startswith("scratch_") for op in ops)


def test_the_loop_is_k_path_ones_plus_the_select(compiled):
    restart, one = loop_stats.opcodes(compiled["restart"]["loop"]), loop_stats.opcodes(compiled["one"]["loop"])
    print("loop: k_path_restart", len(restart), "k_path_one", len(one))
    assert len(restart) <= len(one) + 1, (len(restart), len(one))
    assert restart.count("v_cndmask_b32") <= one.count("v_cndmask_b32") + 1
    assert sum(op.startswith("s_waitcnt") for op in restart) <= sum(op.startswith("s_waitcnt") for op in one)
    clamped = [l for op, l in loop_stats.instructions(compiled["restart"]["loop"]) if op == "v_fma_f32" and re.search(r"\bclamp\b", l)]
    assert len(clamped) == 16, len(clamped)


def test_hand_issued_loads_are_not_touched_before_their_wait():
    groups, bad = audit_asm_loads.audit(*path_kernels.source("fused_restart"))
    assert groups > 0 and bad == 0, (groups, bad)


def test_the_other_translation_units_do_not_name_the_flag():
    for stem in ("fused", "fused_blocks", "fused_one", "fused_capture", "fused_queue", "kernels"):
        text = (ROOT / CSRC / f"{stem}.hip").read_text()
        assert "RESTART" not in text and "kRestart" not in text, stem
    # ... and the file instantiates exactly the restart variant (trav_common.h: PathVariant), with exactly the flags it had: one group, in blocks, restart
    # -- no spheres, one level, no capture, no primary-hit cache (hence the seed)
    body = (ROOT / CSRC / "fused_restart.hip").read_text()
    assert re.findall(r"fused_body<([^;]*)>\(", body) == ["RestartVariant"]
    variant = re.search(r"struct RestartVariant : (\S+) \{(.*?)\};", body, re.S)
    assert variant.group(1) == "FusedBodyVariant<false>"
    assert re.sub(r"\s+", " ", variant.group(2)).strip() == "static constexpr bool kBlocks = true, kOneGroup = true, kRestart = true;"


def test_the_knob_and_the_counter(hrt):
    knobs = (ROOT / CSRC / "knobs.def").read_text()
    line = next(l for l in knobs.splitlines() if l.startswith('HRT_KNOB("HRT_PRIMARY_RESTART"'))
    assert "ctx->primary_restart = std::atoi(e) != 0" in line
    names = [f[0] for f in hrt.Stats._fields_]
    assert names.index("restart_launches") + 1 == names.index("one_group_launches")
    assert "hrt_host_leaf_parent" in hrt.EXPORTS and "hrt_tlas_leaf_parent" in hrt.EXPORTS
