"""The argument behind HRT_SEED_PRIMARY, on the CPU: a closest-hit walk that starts with its culling bound at the
distance the same ray found before ends in the same primitive with the same t, bit for bit, and visits no more nodes.  The oracle's
canonical walker (oracle_py.bvh8_trace) over trees of the host builder, with and without spatial splits (a primitive referenced from
several leaves).

The walker takes one tmax per call and uses it for two things: the culling bound starts there, and its primitive test accepts t < tmax
only.  The kernels start the culling bound at the found t and keep the launch's tmax in the primitive test, where t == bound is accepted
for a lower id than the best so far.  So each ray is walked again, in a call of its own, with tmax = the next float above its t: the
culling bound is within one ulp of the kernels' and the old hit is the only t the primitive test can still accept at or beyond it.  (The
bound is NOT emulated by scaling directions: that changes the rounding of every t.)"""
import ctypes as C

import numpy as np
import pytest

from test_host_cpu import _build

N_TRIANGLES, N_RAYS = 3000, 1500


@pytest.mark.parametrize("sbvh", ["0", "1"])
def test_a_walk_bounded_at_its_known_hit_finds_it_again_in_fewer_visits(hrt, oracle, monkeypatch, sbvh):
    monkeypatch.setenv("HRT_SBVH", sbvh)
    scene = hrt.scenes.random_soup(N_TRIANGLES, 0.12, 17)
    lib, blob = _build(hrt, scene["instances"][0]["vertices"])
    try:
        assert blob.n_triangles > N_TRIANGLES if sbvh == "1" else blob.n_triangles == N_TRIANGLES
        o, d = oracle.random_rays(N_RAYS, 5)
        per_ray = np.zeros(N_RAYS, np.uint32)
        t, u, v, prim, inst, visits, tests = oracle.bvh8_trace(blob.nodes, blob.triangles, o, d, per_ray_nodes=per_ray)
        hit = prim != 0xFFFFFFFF
        assert 0.3 * N_RAYS < hit.sum() < N_RAYS and int(per_ray.sum()) == visits
        seeded_visits = seeded_tests = 0
        for i in np.flatnonzero(hit):
            bound = float(np.nextafter(t[i], np.float32(np.inf)))
            st, su, sv, sprim, sinst, nv, nt = oracle.bvh8_trace(blob.nodes, blob.triangles, o[i], d[i], tmax=bound)
            assert sprim[0] == prim[i] and sinst[0] == inst[i], (i, prim[i], sprim[0])      # never a miss, never a neighbour
            assert st.view(np.uint32)[0] == t.view(np.uint32)[i] and su.view(np.uint32)[0] == u.view(np.uint32)[i] and sv.view(np.uint32)[0] == v.view(np.uint32)[i]
            assert nv <= per_ray[i], (i, nv, per_ray[i])
            seeded_visits += nv
            seeded_tests += nt
        # the rays that hit walk fewer nodes in all (C4's tree: -22 % of their node visits, profiles/r18_primary_seed.txt section 2)
        assert seeded_visits < int(per_ray[hit].sum())
        print(f"HRT_SBVH={sbvh}: {int(hit.sum())} hits, node visits {int(per_ray[hit].sum())} -> {seeded_visits}, primitive tests (all rays) {tests}, seeded hits' {seeded_tests}")
    finally:
        lib.hrt_host_free(C.byref(blob))
