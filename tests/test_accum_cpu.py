"""The accumulator's host pass (host/frt_accum.c, the definition the device pass repeats) against the numpy Welford of
tests/accum_ref.py, its edge cases and its refusals. No GPU."""
import ctypes

import numpy as np
import pytest

import accum_ref


@pytest.fixture(scope="module")
def rt(built):
    from fast_ray_tracer_amd import runtime
    runtime.host_lib()
    return runtime


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("count", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("npixels", [1, 63, 257 * 3])
def test_host_accumulator_is_the_reference(rt, npixels, count):
    xs = accum_ref.samples(npixels, count, seed=10 * npixels + count)
    ref = accum_ref.Welford(npixels)
    acc = rt.Accumulator(npixels, device=None)
    try:
        for x in xs:
            ref.add(x)
            acc.add(x)
        mean, var, st = acc.resolve(stats=True)
    finally:
        acc.close()
    want_mean, want_var = ref.resolve()
    assert _same_bits(mean, want_mean) and _same_bits(var, want_var)
    assert (st.pixels, st.frames, st.skipped, st.device) == (npixels, count, ref.skipped, -1)
    assert np.array_equal(var[:, 3], ref.n)
    if npixels >= 8:
        assert ref.skipped >= 2 * count and ref.n[0] == 0 and ref.n[1] == 1 and ref.n.max() == count
        # n == 0: zeros; n == 1: the sample itself; no variance under two samples
        assert not mean[0].any() and not var[0].any()
        assert _same_bits(mean[1], xs[0, 1]) and not var[1, :3].any() and var[1, 3] == 1.0
        assert not var[ref.n < 2, :3].any()
        if count >= 2:
            assert (var[ref.n >= 2, :3] > 0).all()
    assert np.isfinite(mean).all() and np.isfinite(var).all()


def test_identical_samples_have_no_variance(rt):
    rng = np.random.default_rng(5)
    x = rng.uniform(-3.0, 3.0, (63, 4))
    acc = rt.Accumulator(63, device=None)
    try:
        for _ in range(5):
            acc.add(x)
        mean, var = acc.resolve()
        assert _same_bits(mean, x) and not var[:, :3].any() and (var[:, 3] == 5.0).all()
        # reset: back to nothing, and the same again
        acc.reset()
        mean0, var0, st = acc.resolve(stats=True)
        assert not mean0.any() and not var0.any() and (st.frames, st.skipped) == (0, 0)
        acc.add(x)
        assert _same_bits(acc.resolve()[0], x)
    finally:
        acc.close()


def test_shape_and_mean_of_two(rt):
    acc = rt.Accumulator((3, 5), device=None)
    try:
        a = np.full((3, 5, 4), 1.0)
        b = np.full((3, 5, 4), 3.0)
        acc.add(a)
        acc.add(b)
        mean, var = acc.resolve()
        assert mean.shape == var.shape == (3, 5, 4)
        # m2 = 2, / (n - 1) = 2, / n = 1
        assert (mean == 2.0).all() and (var[..., :3] == 1.0).all() and (var[..., 3] == 2.0).all()
        with pytest.raises(ValueError):
            acc.add(np.zeros((3, 5, 3)))
    finally:
        acc.close()


def test_refusals(rt):
    """Every refusal returns -1 with a message and leaves the outputs as they were; no device is looked for."""
    lib = rt.host_lib()
    vp = ctypes.c_void_p
    for bad in (0, -1, 1 << 31, 1 << 40):
        acc = vp(0xDEAD)
        assert lib.frt_accum_create(-1, bad, ctypes.byref(acc)) == -1 and acc.value == 0xDEAD, bad
        assert lib.frt_accum_error().decode().startswith("frt_accum"), bad
        with pytest.raises(RuntimeError, match="npixels"):
            rt.Accumulator(bad, device=None)
    assert lib.frt_accum_create(-1, 4, None) == -1
    acc = vp()
    assert lib.frt_accum_create(-1, 4, ctypes.byref(acc)) == 0
    try:
        x = np.ones((4, 4))
        mean, var = np.full((4, 4), 7.25), np.full((4, 4), 7.25)
        calls = [lambda: lib.frt_accum_add(None, x.ctypes.data, 0), lambda: lib.frt_accum_add(acc, None, 0),
                 lambda: lib.frt_accum_add(acc, x.ctypes.data, 1),  # device memory, host accumulator
                 lambda: lib.frt_accum_reset(None),
                 lambda: lib.frt_accum_resolve(None, mean.ctypes.data, var.ctypes.data, 0, None),
                 lambda: lib.frt_accum_resolve(acc, None, None, 0, None),
                 lambda: lib.frt_accum_resolve(acc, mean.ctypes.data, var.ctypes.data, 1, None)]
        for k, call in enumerate(calls):
            lib.frt_accum_set_error.argtypes = [ctypes.c_char_p]
            lib.frt_accum_set_error(b"")
            assert call() == -1, k
            assert lib.frt_accum_error().decode().startswith("frt_accum"), k
            assert (mean == 7.25).all() and (var == 7.25).all(), k
        # nothing was added by the refused calls; one output alone is fine
        assert lib.frt_accum_resolve(acc, None, var.ctypes.data, 0, None) == 0
        assert not var.any() and (mean == 7.25).all()
    finally:
        lib.frt_accum_release(acc)
    lib.frt_accum_release(None)
    assert lib.frt_accum_stats_size() == ctypes.sizeof(rt.AccumStats)
