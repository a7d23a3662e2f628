"""hrt_sample_counts on the MI355X (include/hrt.h; csrc/kernels.hip k_sample_counts) against tests/sample_counts_ref.py, bit for bit, over
synthetic sums and totals: hostile values (+-inf, NaN, subnormals, a second moment smaller than the first one's square), totals of 0, 1, 2 and
2^20, every window radius, non-default target and limits, frames of one pixel, of fewer pixels than a window, of odd sizes and of more than
one workgroup.  tests/test_sample_counts_cpu.py holds these inputs to reaching every branch of the definition."""
import ctypes as C

import numpy as np
import pytest

import sample_counts_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(hrt):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    r = hrt.Renderer(0, 0)
    yield hrt, r
    r.close()


def _run(hrt, r, sum4, taken, params, fill=0xDEADBEEF):
    """(status, counts as (H, W) uint32) of one call; `counts` starts as `fill` everywhere"""
    import torch
    h, w = taken.shape
    d_sum = torch.from_numpy(np.ascontiguousarray(sum4)).to(r.device)
    d_taken = torch.from_numpy(np.ascontiguousarray(taken).view(np.int32)).to(r.device)
    d_counts = torch.from_numpy(np.full((h, w), fill, np.uint32).view(np.int32)).to(r.device)
    p = None
    if params is not None:
        p = hrt.SampleCountParams()
        assert r.lib.hrt_sample_counts_default_params(C.byref(p)) == 0
        for k, v in params.items():
            if k == "reserved":
                p.reserved[0], p.reserved[1] = v
            else:
                setattr(p, k, v)
    rc = r.lib.hrt_sample_counts(r.ctx, d_sum.data_ptr(), d_taken.data_ptr(), w, h, C.byref(p) if p is not None else None, d_counts.data_ptr(), r._stream())
    torch.cuda.synchronize(r.device)
    return rc, d_counts.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("size", ref.SIZES)
def test_the_counts_are_the_references(ctx, size):
    hrt, r = ctx
    w, h = size
    for seed in range(ref.N_KINDS if w * h < 3 * ref.N_KINDS else 2):
        sum4, taken = ref.synthetic_frame(w, h, seed)
        for base in ref.PARAM_SETS:
            for radius in (0, 1, 2):
                params = dict(base, radius=radius)
                rc, got = _run(hrt, r, sum4, taken, params)
                want = ref.sample_counts(sum4, taken, **params)
                assert rc == 0 and np.array_equal(got, want), (seed, params, np.argwhere(got != want)[:8], got[got != want][:8], want[got != want][:8])


def test_null_parameters_are_the_defaults(ctx):
    hrt, r = ctx
    p = hrt.SampleCountParams()
    assert r.lib.hrt_sample_counts_default_params(C.byref(p)) == 0
    assert (np.float32(p.target_sigma), p.min_total, p.max_total, p.radius, tuple(p.reserved)) == (np.float32(0.05), 1, 64, 1, (0, 0))
    sum4, taken = ref.synthetic_frame(37, 29, 3)
    rc, got = _run(hrt, r, sum4, taken, None)
    assert rc == 0 and np.array_equal(got, ref.sample_counts(sum4, taken, **ref.DEFAULTS))


@pytest.mark.parametrize("bad", [dict(target_sigma=0.0), dict(target_sigma=-1.0), dict(target_sigma=float("inf")), dict(target_sigma=float("nan")),
                                 dict(min_total=0), dict(min_total=65537, max_total=65537), dict(min_total=9, max_total=8), dict(max_total=65537),
                                 dict(radius=3), dict(reserved=(1, 0)), dict(reserved=(0, 7))])
def test_bad_parameters_are_refused_and_nothing_is_written(ctx, bad):
    hrt, r = ctx
    sum4, taken = ref.synthetic_frame(5, 3, 0)
    rc, got = _run(hrt, r, sum4, taken, bad)
    assert rc == -1 and np.all(got == 0xDEADBEEF)
    assert r.lib.hrt_sample_counts(r.ctx, None, None, 5, 3, None, None, r._stream()) == -1
