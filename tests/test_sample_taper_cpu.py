"""The host's block schedule (hrt_sample_schedule: what render_fused cuts a path-kernel launch into, HRT_SAMPLE_TAPER / HRT_SAMPLE_BLOCK),
for every sample count from 1 to 1100.  A tapered schedule's blocks are powers of two that never grow from one pass to the next, so
every boundary is a multiple of the block that ends there; they add up to the launch's samples, the last one cut short where the samples
end when the count is no multiple of it (the only block that may be: 13 samples at 8:2 are 4, 2, 2, 2, 2 and 1 of a block of 2).  The
function itself also walks the samples with the kernel's end-of-block test (device_types.h: block_ends) and fails where that test and
the pass starts disagree."""
import ctypes as C

import pytest

SPP = range(1, 1101)
TAPERS = [(64, 8), (8, 2), (32, 4), (128, 16), (64, 64), (16, 1), (1, 1)]


def _schedule(lib, spp, big, small):
    first = (C.c_uint32 * (spp + 1))()
    n = C.c_uint32(0)
    rc = lib.hrt_sample_schedule(spp, big, small, first, spp + 1, C.byref(n))
    assert rc == 0, (rc, spp, big, small)
    return list(first[:n.value + 1])


def _is_pow2(x):
    return x >= 1 and x & (x - 1) == 0


@pytest.mark.parametrize("big,small", TAPERS)
def test_tapered_schedules_of_1_to_1100_samples(hrt, big, small):
    lib = hrt.load_library()
    for spp in SPP:
        first = _schedule(lib, spp, big, small)
        assert first[0] == 0 and first[-1] == spp and len(first) >= 2, (spp, first)
        sizes = [b - a for a, b in zip(first, first[1:])]
        assert sum(sizes) == spp
        # the nominal size of the last block: the power of two it would have had, had the samples not ended -- no larger than its
        # predecessor (nor than the largest block), no smaller than what is left
        nominal = list(sizes)
        if not _is_pow2(sizes[-1]) or first[-2] % sizes[-1] != 0:
            cap = sizes[-2] if len(sizes) > 1 else big
            nominal[-1] = min(cap, 1 << (sizes[-1] - 1).bit_length())
            assert sizes[-1] < nominal[-1], (spp, sizes)
        assert all(_is_pow2(k) for k in nominal), (spp, sizes)
        assert all(a >= b for a, b in zip(nominal, nominal[1:])), (spp, sizes)
        assert all(k <= big for k in nominal) and (spp < small or nominal[-1] <= small), (spp, sizes)
        assert all((f + k) % k == 0 for f, k in zip(first, nominal)), (spp, sizes)      # a boundary is a multiple of the block that ends there
        if spp % small == 0:                                                             # nothing is cut: the sizes themselves are the powers of two
            assert nominal == sizes, (spp, sizes)


def test_the_schedules_the_design_names(hrt):
    lib = hrt.load_library()
    sizes = lambda spp, big, small: [b - a for a, b in zip(*(lambda f: (f, f[1:]))(_schedule(lib, spp, big, small)))]
    assert sizes(256, 64, 8) == [64, 64, 64, 32, 16, 8, 8]
    assert sizes(16, 8, 2) == [8, 4, 2, 2]
    assert sizes(512, 64, 8) == [64] * 7 + [32, 16, 8, 8]
    assert sizes(200, 64, 8) == [64, 64, 32, 16, 8, 8, 8]           # the halvings are the last whole 64, the rest goes in eights
    assert sizes(24, 64, 8) == [8, 8, 8]                             # fewer samples than the largest block: it starts at 16, the window's first is 8
    assert sizes(13, 8, 2) == [4, 2, 2, 2, 2, 1] and sizes(7, 8, 2) == [2, 2, 2, 1]


@pytest.mark.parametrize("k", [1, 2, 5, 7, 32, 33])
def test_uniform_schedules(hrt, k):
    """block_min = 0: HRT_SAMPLE_BLOCK=N, blocks of N and a short last one, as before"""
    lib = hrt.load_library()
    for spp in SPP:
        first = _schedule(lib, spp, k, 0)
        assert first == list(range(0, spp, k)) + [spp]


def test_what_is_refused(hrt):
    lib = hrt.load_library()
    first = (C.c_uint32 * 8)()
    n = C.c_uint32(0)
    assert lib.hrt_sample_schedule(256, 64, 8, first, 8, C.byref(n)) == 0 and n.value == 7
    assert lib.hrt_sample_schedule(256, 64, 8, first, 7, C.byref(n)) != 0           # no room for the closing entry
    assert lib.hrt_sample_schedule(256, 48, 8, first, 8, C.byref(n)) != 0           # not a power of two
    assert lib.hrt_sample_schedule(256, 8, 64, first, 8, C.byref(n)) != 0           # grows
    assert lib.hrt_sample_schedule(0, 64, 8, first, 8, C.byref(n)) != 0
    assert lib.hrt_sample_schedule(256, 0, 0, first, 8, C.byref(n)) != 0
