"""bench.py on the GPU: a plain run prints the headline line only, and --dump-outputs writes the same colour buffer in every run
of the same arguments -- with or without --full, whose extra passes come after the timed steps."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


def _bench(*args):
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), *args], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = [line for line in p.stdout.splitlines() if line.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_and_dumped_outputs(gpu_available, tmp_path):
    if not gpu_available:
        pytest.skip("no GPU in this container")
    common = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--spp", "2"]
    plain = _bench(*common, "--dump-outputs", str(tmp_path / "plain"))
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in plain, key
    assert plain["steps"] == 2 and plain["warmup"] == 1 and plain["value"] > 0 and plain["ms_per_step"] > 0
    assert plain["unit"] == "Mrays/s" and plain["higher_is_better"] is True and plain["dtype"] == "f32"
    assert not {"roofline", "cpu_baseline", "parity"} & set(plain) and "alt_builders" not in plain["config"]
    full = _bench(*common, "--full", "--no-cpu-baseline", "--no-alt-builder", "--dump-outputs", str(tmp_path / "full"))
    assert full["roofline"]["nodes_per_ray"] > 0 and full["steps"] == 2
    a = np.load(tmp_path / "plain" / "color.npy")
    b = np.load(tmp_path / "full" / "color.npy")
    assert a.dtype == np.float32 and a.shape == (1080, 1920, 4) and np.isfinite(a).all() and a[..., :3].max() > 0
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
