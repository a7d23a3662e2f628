"""hrt_render_accumulate on the MI355X (include/hrt.h; csrc/fused_counts.hip k_path_counts, csrc/kernels.hip k_finalize_counts): per-pixel
sample counts over sums the caller keeps.  Bit for bit everywhere: a pixel that took n samples in total, over any number of launches, holds
what hrt_render_launch(spp = n) gives it from the same initial RNG states -- colour, linear output, state -- and its sums are the
reference's over the CPU oracle (tests/sample_counts_ref.py).  Scenes: triangles and spheres over one and two levels, so that all four
instantiations of the kernel run."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import sample_counts_ref as ref

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
MODES = ["mixed-flat", "particles-two-level", "c1-flat", "mixed-two-level"]       # k_path_counts<1, 0>, <0, 1>, <0, 0>, <1, 1>
MAIN = MODES[:2]


@pytest.fixture(scope="module")
def hrt_gpu(hrt):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return hrt


def _scene(hrt, mode, w, h):
    s = hrt.scenes
    scene = {"mixed": lambda: s.mixed_test_scene(width=w, height=h, transforms=True), "particles": lambda: s.particle_scene(12, w, h, 1, frame=2),
             "c1": lambda: s.cornell_box(w, h, 1)}[mode.split("-")[0]]()
    two = mode.endswith("two-level")
    return scene, (hrt.CTX_TWO_LEVEL if two else 0), two


def _renderer(hrt, scene, flags, w, h):
    r = hrt.Renderer(0, flags)
    r.load_scene(scene)
    r.set_frame(w, h, hrt.scenes.SEED_SALT, linear=True)
    return r


def _fresh(hrt, r):
    """the frame as new: initial RNG states, no sample taken, stats at zero"""
    r.set_frame(r.width, r.height, hrt.scenes.SEED_SALT, linear=True)
    r.reset_stats()


def _bits(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint32)


def _frame(r):
    """(colour, linear, states) as bits, per pixel"""
    n = r.width * r.height
    return _bits(r.color).reshape(n, 4), _bits(r.linear).reshape(n, 4), r.rng_states_numpy()


def _sums(r):
    n = r.width * r.height
    return _bits(r.sum).reshape(n, 4), r.taken.cpu().numpy().reshape(n).view(np.uint32)


def _same(got, want, sel=slice(None)):
    for g, w_, what in zip(got, want, ("colour", "linear", "states")):
        assert np.array_equal(g[sel], w_[sel]), (what, np.argwhere((g[sel] != w_[sel]).any(axis=-1))[:8].ravel())


def _counts_tensor(r, counts):
    import torch
    return torch.from_numpy(np.ascontiguousarray(counts.reshape(r.height, r.width)).view(np.int32)).to(r.device)


SENTINEL = 0.3125


def _sentinels(r):
    r.color.fill_(SENTINEL); r.linear.fill_(SENTINEL); r.sum.fill_(SENTINEL)


@pytest.mark.parametrize("size", [(61, 37), (8, 6), (1, 1)])
@pytest.mark.parametrize("mode", MODES)
def test_uniform_equals_the_launch(hrt_gpu, oracle, mode, size):
    """accumulate(spp) from zeroed totals is render(spp) of a second context -- colour, linear output, RNG states, ray counts --, its sums are
    the reference's over the oracle, taken == spp everywhere and paths == W H spp."""
    hrt = hrt_gpu
    w, h = size
    scene, flags, two = _scene(hrt, mode, w, h)
    ra, rr = _renderer(hrt, scene, flags, w, h), _renderer(hrt, scene, flags, w, h)
    osc = oracle.OracleScene(scene, instanced=two)
    try:
        states = oracle.rng_init(w, h, hrt.scenes.SEED_SALT)
        sum4 = np.zeros((w * h, 4), np.float32); taken = np.zeros(w * h, np.uint32)
        for spp in (1, 3, 5):
            ref.accumulate(osc, w, h, states, spp - int(taken[0]), sum4, taken)         # (the oracle goes on where it was: 1, then 3, then 5 in total)
            _fresh(hrt, ra); _fresh(hrt, rr)
            ra.sum.fill_(float("nan"))                                                   # d_sum need not be zeroed
            ra.accumulate(spp)
            rr.render(spp)
            _same(_frame(ra), _frame(rr))
            got_sum, got_taken = _sums(ra)
            assert np.all(got_taken == spp)
            assert np.array_equal(got_sum, sum4.view(np.uint32)), (spp, np.argwhere((got_sum != sum4.view(np.uint32)).any(axis=-1))[:8].ravel())
            sa, sr = ra.stats(), rr.stats()
            assert (sa.rays, sa.rays_closest, sa.rays_any) == (sr.rays, sr.rays_closest, sr.rays_any)
            assert sa.paths == w * h * spp == sr.paths
            assert np.all(_bits(ra.albedo) == 0) and np.all(_bits(ra.normal) == 0)
    finally:
        osc.close(); ra.close(); rr.close()


@pytest.mark.parametrize("mode", MAIN)
def test_split_equals_whole(hrt_gpu, oracle, mode):
    """accumulate(2) then accumulate(3) is render(5): states, colour, linear output; the sums are the oracle's of five samples."""
    hrt = hrt_gpu
    w, h = 61, 37
    scene, flags, two = _scene(hrt, mode, w, h)
    ra, rr = _renderer(hrt, scene, flags, w, h), _renderer(hrt, scene, flags, w, h)
    osc = oracle.OracleScene(scene, instanced=two)
    try:
        ra.accumulate(2); ra.accumulate(3)
        rr.render(5)
        _same(_frame(ra), _frame(rr))
        states = oracle.rng_init(w, h, hrt.scenes.SEED_SALT)
        sum4 = np.zeros((w * h, 4), np.float32); taken = np.zeros(w * h, np.uint32)
        ref.accumulate(osc, w, h, states, 5, sum4, taken)
        got_sum, got_taken = _sums(ra)
        assert np.all(got_taken == 5) and np.array_equal(got_sum, sum4.view(np.uint32))
        assert ra.stats().paths == w * h * 5
    finally:
        osc.close(); ra.close(); rr.close()


def _hand_made_map(w, h):
    """values from {0, 1, 2, 3, 7, 19} (19 is clamped by spp = 7); row 5 all zeros; a run of 100 zeros from the middle of row 10 across its end; of
    the last 80 pixels only the very last takes samples"""
    n = w * h
    values = np.array([0, 1, 2, 3, 7, 19], np.uint32)
    counts = values[(np.arange(n, dtype=np.uint64) * 2654435761 >> 7) % 6].astype(np.uint32)
    counts.reshape(h, w)[5, :] = 0
    counts[10 * w + 30:10 * w + 130] = 0
    counts[n - 80:] = 0
    counts[n - 1] = 3
    return counts


@pytest.mark.parametrize("mode", MAIN)
def test_a_hand_made_map(hrt_gpu, mode):
    """For each distinct effective count s the pixels with that count are render(s) from freshly initialised states; pixels of count 0 keep
    their initial state, their sentinel colour and sum, and no total; paths is the sum of the effective counts."""
    hrt = hrt_gpu
    w, h, spp = 61, 37, 7
    counts = _hand_made_map(w, h)
    c = ref.effective_counts(w * h, spp, counts)
    assert set(np.unique(counts)) == {0, 1, 2, 3, 7, 19} and set(np.unique(c)) == {0, 1, 2, 3, 7}
    scene, flags, _ = _scene(hrt, mode, w, h)
    ra, rr = _renderer(hrt, scene, flags, w, h), _renderer(hrt, scene, flags, w, h)
    try:
        initial = ra.rng_states_numpy()
        _sentinels(ra)
        ra.reset_stats()
        ra.accumulate(spp, counts=_counts_tensor(ra, counts))
        got = _frame(ra)
        got_sum, got_taken = _sums(ra)
        assert np.array_equal(got_taken, c)
        for s in (1, 2, 3, 7):
            _fresh(hrt, rr)
            rr.render(s)
            _same(got, _frame(rr), c == s)
        zero = c == 0
        sentinel = np.float32(SENTINEL).view(np.uint32)
        assert np.array_equal(got[2][zero], initial[zero])
        assert np.all(got[0][zero] == sentinel) and np.all(got[1][zero] == sentinel) and np.all(got_sum[zero] == sentinel)
        assert ra.stats().paths == int(c.sum())
    finally:
        ra.close(); rr.close()


ZERO_MAP_CHILD = r"""
import importlib, sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import torch
hrt = importlib.import_module("nvidia-optix-ray-tracer_amd")
mode, w, h = sys.argv[2], 61, 37
scene = hrt.scenes.mixed_test_scene(width=w, height=h, transforms=True) if mode == "mixed-flat" else hrt.scenes.particle_scene(12, w, h, 1, frame=2)
r = hrt.Renderer(0, 0 if mode == "mixed-flat" else hrt.CTX_TWO_LEVEL)
r.load_scene(scene)
r.set_frame(w, h, hrt.scenes.SEED_SALT, linear=True)
bits = lambda t: np.ascontiguousarray(t.cpu().numpy()).view(np.uint32)
r.color.fill_(0.3125); r.linear.fill_(0.3125); r.sum.fill_(0.3125)
before = (r.rng_states_numpy(), bits(r.sum), bits(r.taken), bits(r.color), bits(r.linear))
r.accumulate(7, counts=torch.zeros((h, w), dtype=torch.int32, device=r.device), sync=False)
print("returned", flush=True)
r._check(r.lib.hrt_sync(r.ctx, r._stream()), "hrt_sync")
print("synchronised", flush=True)
after = (r.rng_states_numpy(), bits(r.sum), bits(r.taken), bits(r.color), bits(r.linear))
assert all(np.array_equal(a, b) for a, b in zip(before, after)), "something changed"
assert r.stats().paths == 0 and r.stats().rays == 0
r.render(1)          # ... and the context renders on
print("unchanged", flush=True)
r.close()
"""


@pytest.mark.parametrize("mode", MAIN)
def test_an_all_zero_map_returns_and_changes_nothing(hrt_gpu, mode):
    """The call returns, the following hrt_sync returns, and states, sums, totals and the sentinel colour are what they were: in a process of
    its own under a time limit that is generous for a kernel with nothing to do (what it costs is the process's start) -- a kill there is a
    hang of k_path_counts."""
    done = subprocess.run([sys.executable, *(["-s"] if sys.flags.no_user_site else []), "-c", ZERO_MAP_CHILD, str(ROOT), mode], capture_output=True, text=True, timeout=240)
    assert done.returncode == 0 and done.stdout.split() == ["returned", "synchronised", "unchanged"], (done.returncode, done.stdout, done.stderr[-2000:])


@pytest.mark.parametrize("mode", MAIN)
def test_a_tile_leaves_the_rest_alone(hrt_gpu, oracle, mode):
    """Rows 3, 4 and 10 of 16: inside as the uniform launch, everything outside -- colour, linear output, sums, totals, states -- untouched."""
    hrt = hrt_gpu
    w, h, spp = 37, 16, 3
    rows = [3, 4, 10]
    tile = hrt.Tile(3, 11, 5, 2, 0)                 # rows y of [3, 11) with (y / 5) % 2 == 0
    scene, flags, two = _scene(hrt, mode, w, h)
    ra, rr = _renderer(hrt, scene, flags, w, h), _renderer(hrt, scene, flags, w, h)
    osc = oracle.OracleScene(scene, instanced=two)
    try:
        inside = np.zeros((h, w), bool); inside[rows] = True; inside = inside.reshape(-1)
        initial = ra.rng_states_numpy()
        _sentinels(ra)
        ra.reset_stats()
        ra.accumulate(spp, tile=tile)
        rr.render(spp)
        got = _frame(ra)
        _same(got, _frame(rr), inside)
        states = oracle.rng_init(w, h, hrt.scenes.SEED_SALT)
        sum4 = np.full((w * h, 4), SENTINEL, np.float32); taken = np.zeros(w * h, np.uint32)
        ref.accumulate(osc, w, h, states, spp, sum4, taken, rows=rows)
        got_sum, got_taken = _sums(ra)
        assert np.array_equal(got_sum, sum4.view(np.uint32)) and np.array_equal(got_taken, taken) and np.array_equal(got[2], states)
        sentinel = np.float32(SENTINEL).view(np.uint32)
        assert np.all(got[0][~inside] == sentinel) and np.all(got[1][~inside] == sentinel) and np.array_equal(got[2][~inside], initial[~inside])
        assert ra.stats().paths == len(rows) * w * spp
    finally:
        osc.close(); ra.close(); rr.close()


@pytest.mark.parametrize("second_stream", [False, True])
@pytest.mark.parametrize("mode", MAIN)
def test_neighbouring_launches_are_undisturbed(hrt_gpu, mode, second_stream):
    """render(3), accumulate(2), render(3) on one context against the same without the accumulate on another: the plain renders' frames and
    states agree (the slice counters' protocol holds in both directions) -- also with the accumulate on a second stream, then a sync.  The
    61 x 37 frame has more pixels than the counters have words, so both finalize kernels zero them; 8 x 6 has fewer, so the launches do."""
    import torch
    hrt = hrt_gpu
    for w, h in ((61, 37), (8, 6)):
        scene, flags, _ = _scene(hrt, mode, w, h)
        ra, rr = _renderer(hrt, scene, flags, w, h), _renderer(hrt, scene, flags, w, h)
        try:
            ra.render(3); rr.render(3)
            _same(_frame(ra), _frame(rr))
            if second_stream:
                side = torch.cuda.Stream(device=ra.device)
                with torch.cuda.stream(side):
                    ra.accumulate(2)
                torch.cuda.synchronize(ra.device)
            else:
                ra.accumulate(2)
            states = ra.rng_states_numpy()
            assert np.all(ra.taken.cpu().numpy() == 2)
            ra.render(3)
            # the accumulate drew two samples' random numbers: the other context draws them with a render of its own, whose image is not looked at
            rr.render(2)
            assert np.array_equal(states, rr.rng_states_numpy())
            rr.render(3)
            _same(_frame(ra), _frame(rr))
            ra.accumulate(1)                            # ... and the reverse: an accumulate behind a plain launch renders every pixel
            assert np.all(ra.taken.cpu().numpy() == 3)
            rr.render(1)
            assert np.array_equal(ra.rng_states_numpy(), rr.rng_states_numpy())
        finally:
            ra.close(); rr.close()


@pytest.mark.parametrize("mode,size", [("c1-flat", (32, 24)), ("particles-two-level", (48, 32))])
def test_end_to_end(hrt_gpu, oracle, mode, size):
    """render_adaptive(pilot 8, max_total 64): the counts are the reference's from the oracle's pilot, the totals pilot + counts, and every
    pixel's colour, linear output and RNG state are the oracle's at that pixel's total.  The map is worth the test: on C1 between 0.3 and 0.9
    of the pixels take no more samples and the others take at least 10 distinct counts; the particle scene's map (little of its frame is
    quiet after 8 samples) has pixels of both kinds and as many distinct counts."""
    hrt = hrt_gpu
    w, h = size
    pilot, params = 8, dict(ref.DEFAULTS, max_total=64)
    scene, flags, two = _scene(hrt, mode, w, h)
    r = _renderer(hrt, scene, flags, w, h)
    osc = oracle.OracleScene(scene, instanced=two)
    try:
        got_counts = r.render_adaptive(pilot, dict(max_total=64)).cpu().numpy().view(np.uint32)
        first = oracle.rng_init(w, h, hrt.scenes.SEED_SALT)
        states = first.copy()
        sum4 = np.zeros((w * h, 4), np.float32); taken = np.zeros(w * h, np.uint32)
        ref.accumulate(osc, w, h, states, pilot, sum4, taken)
        counts = ref.sample_counts(sum4.reshape(h, w, 4), taken.reshape(h, w), **params)
        assert np.array_equal(got_counts, counts), np.argwhere(got_counts != counts)[:8]
        zero = float(np.mean(counts == 0))
        print(f"{mode}: zero share {zero:.2f}, {len(np.unique(counts))} distinct counts, largest {counts.max()}")
        assert len(np.unique(counts)) >= 10 and (0.3 <= zero <= 0.9 if mode == "c1-flat" else 0.0 < zero < 1.0)
        ref.accumulate(osc, w, h, states, params["max_total"], sum4, taken, counts)
        got_sum, got_taken = _sums(r)
        assert np.array_equal(got_taken, pilot + counts.reshape(-1)) and np.array_equal(got_taken, taken)
        assert np.array_equal(got_sum, sum4.view(np.uint32))
        colour, linear, got_states = _frame(r)
        assert np.array_equal(got_states, states)
        assert np.array_equal(linear[:, :3], ref.mean(sum4, taken).view(np.uint32))
        for total in np.unique(taken):                  # the oracle's render of every distinct total, from the initial states
            st = first.copy()
            want = osc.render(w, h, st, int(total))
            sel = taken == total
            assert np.array_equal(colour[sel], want["color"].reshape(-1, 4).view(np.uint32)[sel]), total
            assert np.array_equal(linear[sel], want["linear"].reshape(-1, 4).view(np.uint32)[sel]), total
            assert np.array_equal(got_states[sel], st[sel]), total
        assert r.stats().paths == int(taken.sum())
    finally:
        osc.close(); r.close()


def _refused(hrt, r, status, **kw):
    with pytest.raises(hrt.HrtError, match=f"status {status}"):
        r.accumulate(**kw)


def _still_renders(hrt, r, scene, oracle_mod, two=False):
    """after a refused call: a render(1) on the same context is bit-exact against the oracle and nothing of the caller's was touched"""
    assert np.all(_bits(r.sum) == np.float32(SENTINEL).view(np.uint32)) and np.all(r.taken.cpu().numpy() == 0)
    r.set_frame(r.width, r.height, hrt.scenes.SEED_SALT, linear=True)
    r.render(1)
    osc = oracle_mod.OracleScene(scene, instanced=two)
    want = osc.render(r.width, r.height, oracle_mod.rng_init(r.width, r.height, hrt.scenes.SEED_SALT), 1)
    osc.close()
    assert np.array_equal(_bits(r.linear), want["linear"].view(np.uint32)) and np.array_equal(_bits(r.color), want["color"].view(np.uint32))


def test_refusals(hrt_gpu, oracle, monkeypatch):
    """A counting context and a tree forced out of k_fused: -5.  NULL d_sum, spp 0 and 65537: -1.  Every refused call touches nothing, and
    the context renders on, bit-exact."""
    import ctypes as C
    hrt = hrt_gpu
    w, h = 24, 16
    scene, _, _ = _scene(hrt, "mixed-flat", w, h)
    r = _renderer(hrt, scene, hrt.CTX_COUNT, w, h)
    try:
        r.sum.fill_(SENTINEL)
        _refused(hrt, r, -5, spp=1)
        _still_renders(hrt, r, scene, oracle)
    finally:
        r.close()
    monkeypatch.setenv("HRT_FUSED_MAX_DEPTH", "0")
    r = _renderer(hrt, scene, 0, w, h)
    monkeypatch.delenv("HRT_FUSED_MAX_DEPTH")
    try:
        r.sum.fill_(SENTINEL)
        _refused(hrt, r, -5, spp=1)
        _still_renders(hrt, r, scene, oracle)
        assert r.stats().fused_fallback_launches >= 1          # (that render went to round 1's kernel: the tree is outside k_fused's limits)
    finally:
        r.close()
    r = _renderer(hrt, scene, 0, w, h)
    try:
        r.sum.fill_(SENTINEL)
        _refused(hrt, r, -1, spp=0)
        _refused(hrt, r, -1, spp=65537)
        params, rg = r._launch_blocks()
        rc = r.lib.hrt_render_accumulate(r.ctx, C.byref(params), C.byref(rg), 1, None, None, r.taken.data_ptr(), None, r._stream())
        assert rc == -1
        rc = r.lib.hrt_render_accumulate(r.ctx, C.byref(params), C.byref(rg), 1, None, r.sum.data_ptr(), None, None, r._stream())
        assert rc == -1
        rg.colorBuffer = None
        assert r.lib.hrt_render_accumulate(r.ctx, C.byref(params), C.byref(rg), 1, None, r.sum.data_ptr(), r.taken.data_ptr(), None, r._stream()) == -1
        _still_renders(hrt, r, scene, oracle)
        r.accumulate(65536, counts=_counts_tensor(r, np.ones(w * h, np.uint32)))        # the largest spp is taken; every pixel draws one sample
        assert np.all(r.taken.cpu().numpy() == 1)
    finally:
        r.close()
