"""Hostile normals, materials, radiance values and cameras (tests/shading_cases.py) through every copy of the shading code on the device.

The shading half of a path -- csrc/trav_common.h: normalize3, hit_normal, scatter_at / scatter<> (the wavefront k_shade), scatter_programs<>
(k_fused, k_path_blocks and their instanced form, through path_lane.h), the path form of k_traverse, program_draws, fold_chain,
primary_direction -- is mostly guards, and the scenes of the rest of the suite (unit normals, albedo in (0, 1), fuzz 0 .. 0.5, a finite
background, a healthy camera) reach none of them.  These do: zero, tiny, huge and non-finite normals, fuzz that is negative, denormal, huge
or NaN, albedos and backgrounds that overflow or are not finite, camera bases normalize3 gives up on, and the one pinned sample whose
rough scatter is degenerate.  That every case takes the branches it is there for is shown on the oracle in test_shading_cases_cpu.py.

Every configuration that has its own copy of that code, or its own way of calling it, renders every case at 61 x 37 with 4 samples and
then 1 more on the same RNG streams, and after either launch the linear radiance and the sRGB colour buffer are the oracle's bit for bit
-- except that a NaN equals a NaN (shading_cases.components_differ says why; the only relaxation) --, the final RNG states are its bits
(one draw too many or too few, e.g. from a `fuzz > 0` that sees a denormal differently, puts a pixel's stream out of step for good) and
HrtStats.rays is its count.  No pixel is left out, nothing carries a tolerance."""
import numpy as np
import pytest

import shading_cases as sh

pytestmark = pytest.mark.gpu

CONFIGURATIONS = {
    "production": (0, {}),                                                                # k_fused
    "sample-blocks": (0, {"HRT_SAMPLE_BLOCK": "2"}),                                      # k_path_blocks: 61 x 37 is more than 448 pixels
    "wavefront": (0, {"HRT_FUSED": "0"}),                                                 # k_generate / k_shade / k_accumulate
    "wavefront-graph": (0, {"HRT_FUSED": "0", "HRT_WAVEFRONT_GRAPH": "1"}),
    "round-1-path-kernel": (0, {"HRT_FUSED_MAX_DEPTH": "1"}),
    "round-1-traverse-kernel": (0, {"HRT_FUSED": "0", "HRT_FUSED_MAX_DEPTH": "1"}),
    "counting": ("CTX_COUNT", {}),
    "two-level": ("CTX_TWO_LEVEL", {}),                                                   # against the oracle's instanced mode
    "reuse-primary": ("CTX_REUSE_PRIMARY", {}),
    "no-primary-seed": (0, {"HRT_SEED_PRIMARY": "0"}),
    "three-launches": (0, {"HRT_FUSED_MAX_SPP": "2"}),                                    # 4 samples = 2 + 2, then 1
}


def _describe(name, launch, what, diff, scene, oracle, instanced, w, h, start_states):
    """What failed, with the oracle's rays of the first differing pixel's first sample in that launch: the diverging bounce is in there."""
    flat = diff.reshape(w * h, -1).any(1)
    j = int(np.argmax(flat))
    x, y = j % w, j // w
    o = oracle.OracleScene(scene, instanced=instanced)
    rays, result = o.pixel_path(w, h, start_states.copy(), x, y)
    o.close()
    lines = ["%s, launch %d, %s: %d differing pixels, the first (%d, %d); the oracle's path there (origin, direction, any-hit, t, primitive, instance):"
             % (name, launch, what, int(flat.sum()), x, y)]
    lines += ["    %s %s %d %r %d %d" % (r[0:3].tolist(), r[3:6].tolist(), int(r[6]), float(r[7]), int(r[8:9].view(np.uint32)[0]), int(r[9:10].view(np.uint32)[0])) for r in rays]
    return "\n".join(lines + ["    its radiance %s" % result.tolist()])


@pytest.mark.parametrize("configuration", sorted(CONFIGURATIONS))
def test_shading_cases_in_every_configuration(hrt, oracle, gpu_available, monkeypatch, configuration):
    if not gpu_available:
        pytest.skip("no GPU in this container")
    flags, env = CONFIGURATIONS[configuration]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    instanced = configuration == "two-level"
    reuse = configuration == "reuse-primary"
    r = hrt.Renderer(0, getattr(hrt, flags) if flags else 0)
    fallback_launches = block_launches = 0
    failures = []                                                       # every case runs, whatever became of the ones before it
    try:
        for name in sh.CASES:
            scene, launches, _ = sh.reference(hrt.scenes, oracle, name, instanced)
            w, h, spps, salt = sh.frame(name, hrt.scenes.SEED_SALT)
            r.load_scene(scene)
            basis = sh.camera_basis(scene)
            if basis is not None:
                r.cam = basis                                           # a basis configure_camera never returns
            r.set_frame(w, h, salt, linear=True)
            r.reset_stats()
            start, saved = oracle.rng_init(w, h, salt), 0
            for k, (spp, want) in enumerate(zip(spps, launches)):
                r.render(spp)
                got = {"linear": r.linear.cpu().numpy(), "color": r.color.cpu().numpy()}
                for what in ("linear", "color"):
                    diff = sh.components_differ(got[what], want[what])
                    if diff.any():
                        failures.append(_describe(name, k, what, diff, scene, oracle, instanced, w, h, start))
                diff = r.rng_states_numpy() != want["states"]
                if diff.any():
                    failures.append(_describe(name, k, "RNG states", diff, scene, oracle, instanced, w, h, start))
                # HRT_CTX_REUSE_PRIMARY traverses a pixel's primary ray once per launch (test_primary_reuse_gpu.py): that many rays fewer
                saved += w * h * (spp - 1) if reuse else 0
                if int(r.stats().rays) != want["rays"] - saved:
                    failures.append("%s, launch %d: %d rays, the oracle's %d less %d reused" % (name, k, int(r.stats().rays), want["rays"], saved))
                start = want["states"]
            st = r.stats()
            fallback_launches += int(st.fused_fallback_launches)
            block_launches += int(st.sample_block_launches)
        assert not failures, "\n".join(failures)
        if configuration == "round-1-path-kernel":
            assert fallback_launches > 0                                # round 1's path kernel did run
        if configuration == "sample-blocks":
            assert block_launches > 0                                   # k_path_blocks did run
    finally:
        r.close()
