"""The denoiser on the MI355X (include/hrt.h "denoiser", csrc/denoise.hip): guides and filter bit for bit against the numpy specification
(tests/denoise_ref.py) over the oracle's primary hits, the convenience call against its two halves, the image quality it buys, and the
C++ driver's --denoise switch."""
import importlib
import subprocess
from pathlib import Path

import numpy as np
import pytest

import denoise_ref as ref

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
SAMPLE = ROOT / "tests" / "golden" / "files" / "config.json"


@pytest.fixture(scope="module")
def hrt_gpu(hrt):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return hrt


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _scene(hrt, name, w, h):
    s = hrt.scenes
    return {"c1": lambda: s.cornell_box(w, h, 1), "sphere_in_box": lambda: s.sphere_in_box(w, h, 1),
            "mixed": lambda: s.mixed_test_scene(width=w, height=h, transforms=True)}[name]()


@pytest.mark.parametrize("mode", ["production", "counting", "two_level"])
@pytest.mark.parametrize("name", ["c1", "sphere_in_box", "mixed"])
def test_guides_bit_exact(hrt_gpu, oracle, name, mode):
    """hrt_denoise_guides: normal and albedo of every primary hit (quirks Q1 / Q2 and the front-face flip included), rounded to halves,
    and the hit distance -- the oracle's primary hits (its instanced mode for two-level trees) shaded by the specification.  The AOV
    buffers of the reference stay zero (Q3) through a launch and a denoise."""
    hrt = hrt_gpu
    w, h = 96, 64
    flags = {"production": 0, "counting": hrt.CTX_COUNT, "two_level": hrt.CTX_TWO_LEVEL}[mode]
    scene = _scene(hrt, name, w, h)
    r = hrt.Renderer(0, flags)
    try:
        r.load_scene(scene)
        r.set_frame(w, h, hrt.scenes.SEED_SALT)
        got = r.denoise_guides().cpu().numpy().view(np.uint16)
        want = ref.primary_guides(oracle.OracleScene(scene, instanced=(mode == "two_level")), scene, r.cam, w, h)
        assert np.array_equal(got, want), np.argwhere((got != want).any(axis=-1))[:8]
        z = ref.unpack_guides(got)[2]
        assert 0 < np.isinf(z).sum() < w * h                      # some background, some geometry
        r.render(1)
        r.denoise()
        assert not r.albedo.any().item() and not r.normal.any().item()
    finally:
        r.close()


def test_guides_of_a_two_level_tree_in_a_counting_context_are_refused(hrt_gpu):
    hrt = hrt_gpu
    r = hrt.Renderer(0, hrt.CTX_TWO_LEVEL)
    try:
        r.load_scene(hrt.scenes.particle_scene(12, 32, 24, 1, frame=2))
        r.set_frame(32, 24, hrt.scenes.SEED_SALT)
        r.set_flags(hrt.CTX_TWO_LEVEL | hrt.CTX_COUNT)
        with pytest.raises(hrt.HrtError, match="status -5"):
            r.denoise_guides()
    finally:
        r.close()


def _random_guides(rng, h, w):
    """Guides with structure: blocks of a few normals and albedos, smooth depth with steps, a sprinkling of background."""
    by, bx = np.meshgrid(np.arange(h) // 7, np.arange(w) // 5, indexing="ij")
    dirs = np.array([[0, 0, 1], [0, 1, 0], [0.6, 0, 0.8], [-0.8, 0.6, 0], [0, -0.6, -0.8]], np.float32)
    n = dirs[(by * 3 + bx) % 5] + rng.normal(0, 0.05, (h, w, 3)).astype(np.float32)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    a = np.array([[0.73, 0.73, 0.73], [0.65, 0.05, 0.05], [0.12, 0.45, 0.15]], np.float32)[(by + bx) % 3]
    z = (1.0 + 0.01 * np.arange(w)[None, :] + 0.3 * ((by + 2 * bx) % 4)).astype(np.float32) + rng.uniform(0, 0.01, (h, w)).astype(np.float32)
    z[rng.uniform(size=(h, w)) < 0.08] = np.inf
    return ref.pack_guides(n, a, z)


@pytest.mark.parametrize("size,params", [
    ((1, 1), {"iterations": 1}),
    ((17, 5), {"iterations": 3}),
    ((5, 17), {"iterations": 8, "sigma_color": 2.0, "sigma_albedo": 0.3, "sigma_depth": 0.1, "normal_power_log2": 2}),
    ((64, 48), {"iterations": 6, "normal_power_log2": 0}),
    ((203, 97), {"iterations": 7, "sigma_color": 0.125, "sigma_depth": 0.005, "normal_power_log2": 8}),
    ((1920, 1080), None),
])
def test_filter_bit_exact(hrt_gpu, size, params):
    hrt = hrt_gpu
    import torch
    w, h = size
    rng = np.random.default_rng(w * 1000 + h)
    g = _random_guides(rng, h, w)
    c = (rng.uniform(0, 1, (h, w, 4)) ** 2).astype(np.float32)
    want = ref.atrous(c, g, params)
    r = hrt.Renderer(0, 0)
    try:
        dc, dg = torch.from_numpy(c).cuda(), torch.from_numpy(g.view(np.int16)).cuda()
        got = r.denoise_filter(dc, dg, params).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(want)), np.argwhere(_bits(got) != _bits(want))[:8]
        r.denoise_filter(dc, dg, params, out=dc)                  # in place
        assert np.array_equal(_bits(dc.cpu().numpy()), _bits(want))
    finally:
        r.close()


def test_filter_rejects_bad_parameters(hrt_gpu):
    hrt = hrt_gpu
    import torch
    r = hrt.Renderer(0, 0)
    try:
        c = torch.zeros((4, 4, 4), dtype=torch.float32, device="cuda")
        g = torch.zeros((4, 4, 8), dtype=torch.int16, device="cuda")
        for bad in ({"iterations": 0}, {"iterations": 17}, {"sigma_color": 0.0}, {"sigma_depth": float("inf")},
                    {"sigma_albedo": -1.0}, {"normal_power_log2": 9}, {"reserved": 1}):
            with pytest.raises(hrt.HrtError, match="status -1"):
                r.denoise_filter(c, g, bad)
    finally:
        r.close()


def test_real_frame_filter_and_launch(hrt_gpu, oracle):
    """A 1-spp C1 frame with its real guides: the filter against the specification, hrt_denoise_launch against guides + filter
    (twice, the same bits), in place into the colour buffer; the AOV buffers are not written."""
    hrt = hrt_gpu
    w, h = 128, 96
    scene = hrt.scenes.cornell_box(w, h, 1)
    r = hrt.Renderer(0, 0)
    try:
        r.load_scene(scene)
        r.set_frame(w, h, hrt.scenes.SEED_SALT)
        r.render(1)
        color = r.color.cpu().numpy()
        guides = r.denoise_guides()
        want = ref.atrous(color, guides.cpu().numpy().view(np.uint16))
        assert np.array_equal(_bits(r.denoise_filter(r.color, guides).cpu().numpy()), _bits(want))
        r.albedo.fill_(7.0)
        r.normal.fill_(7.0)
        a = r.denoise().cpu().numpy()
        b = r.denoise().cpu().numpy()
        assert np.array_equal(_bits(a), _bits(want)) and np.array_equal(_bits(b), _bits(want))
        assert np.array_equal(_bits(r.color.cpu().numpy()), _bits(color))          # the input is left alone
        assert (r.albedo == 7.0).all().item() and (r.normal == 7.0).all().item()
        r.denoise(out=r.color)
        assert np.array_equal(_bits(r.color.cpu().numpy()), _bits(want))
        assert not np.array_equal(want, color)
    finally:
        r.close()


def _edge_pixels(guides):
    """Pixels with a guide discontinuity in their 3x3 neighbourhood: a hit next to a miss, or n . n' < 0.9."""
    n, _, z = ref.unpack_guides(guides)
    hit = (z > 0) & np.isfinite(z)
    h, w = hit.shape
    edge = np.zeros((h, w), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
            P, Q = (slice(y0, y1), slice(x0, x1)), (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
            d = (n[P] * n[Q]).sum(-1)
            edge[P] |= (hit[P] != hit[Q]) | (hit[P] & hit[Q] & (d < 0.9))
    return edge


def _time_mode_frame(hrt, r, w, h):
    io = importlib.import_module("nvidia-optix-ray-tracer_amd.io")
    tm = io.time_mode_scene(SAMPLE, width=w, height=h)
    cfg = tm["config"]
    r.load_scene(tm["scene"])
    r.set_frame(w, h, hrt.scenes.SEED_SALT)
    return tm, cfg


def _pose_first_frame(r, tm, cfg):
    nxt = tm["states"][min(1, len(tm["states"]) - 1)]
    r.pose_instances(tm["states"][0], nxt, float(tm["durations"][0]), 0, tm["frame_counts"][0], first_instance=tm["n_extra"],
                     offset=cfg["particle-shift"], scale=cfg["particle-scale"])


@pytest.mark.parametrize("name,bound", [("c1", 0.15), ("sample", 0.45)])
def test_denoised_frame_is_closer_to_the_converged_one(hrt_gpu, name, bound):
    """4 spp denoised against 4096 spp of the same scene and seed: the MSE falls to at most `bound` times the raw frame's, and next to
    guide discontinuities the denoised frame is no worse than the raw one (no bleeding across edges).  The bounds leave room above
    the measured ratios, C1 0.061 and the shipped sample 0.315 (its particles are a few pixels wide, bounded by normal and albedo
    edges: little to average over at 300x200): profiles/r05_denoise.txt."""
    hrt = hrt_gpu
    w, h = (256, 256) if name == "c1" else (300, 200)
    frames = {}
    for spp in (4, 4096):
        r = hrt.Renderer(0, 0)
        try:
            if name == "c1":
                r.load_scene(hrt.scenes.cornell_box(w, h, spp))
                r.set_frame(w, h, hrt.scenes.SEED_SALT)
            else:
                tm, cfg = _time_mode_frame(hrt, r, w, h)
                _pose_first_frame(r, tm, cfg)
            r.render(spp)
            frames[spp] = r.color.cpu().numpy()[..., :3].astype(np.float64)
            if spp == 4:
                den = r.denoise().cpu().numpy()[..., :3].astype(np.float64)
                edge = _edge_pixels(r.denoise_guides().cpu().numpy().view(np.uint16))
        finally:
            r.close()
    conv = frames[4096]
    mse_raw = ((frames[4] - conv) ** 2).mean()
    mse_den = ((den - conv) ** 2).mean()
    e_raw = ((frames[4] - conv) ** 2)[edge].mean()
    e_den = ((den - conv) ** 2)[edge].mean()
    print(f"{name}: mse raw {mse_raw:.6g} denoised {mse_den:.6g} ratio {mse_den / mse_raw:.4f}; "
          f"edges ({edge.sum()} px) raw {e_raw:.6g} denoised {e_den:.6g} ratio {e_den / e_raw:.4f}")
    assert mse_den <= bound * mse_raw
    assert e_den <= e_raw


def test_time_driver_denoise_switch(hrt_gpu, tmp_path):
    """hrt_time_render --denoise on the shipped sample: its image is hrt_to_rgba8 of hrt_denoise_launch of the same frame, rendered here
    through the Python host (the driver's untimed first launch included: it advances the RNG streams)."""
    hrt = hrt_gpu
    w, h = 120, 80
    exe = ROOT / "nvidia-optix-ray-tracer_amd" / "lib" / "hrt_time_render"
    assert exe.exists(), "run `make tools`"
    out = tmp_path / "frame.ppm"
    subprocess.run([str(exe), str(SAMPLE), str(SAMPLE.parent), "1", str(out), str(w), str(h), "--denoise"], check=True, timeout=300)
    raw = out.read_bytes()
    header = f"P6\n{w} {h}\n255\n".encode()
    assert raw.startswith(header)
    got = np.frombuffer(raw[len(header):], np.uint8).reshape(h, w, 3)
    r = hrt.Renderer(0, 0)
    try:
        tm, cfg = _time_mode_frame(hrt, r, w, h)
        r.render(1)                                               # the driver's untimed launch, identity poses
        _pose_first_frame(r, tm, cfg)
        r.render(1)
        raw_rgba = r.to_rgba8().cpu().numpy()[..., :3]
        want = r.to_rgba8_of(r.denoise()).cpu().numpy()[..., :3]
    finally:
        r.close()
    assert np.array_equal(got, want)
    assert not np.array_equal(got, raw_rgba)
