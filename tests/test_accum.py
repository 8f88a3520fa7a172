"""The accumulator's device pass (csrc/frt_accum.hip: k_accum_add, k_accum_resolve) against the host pass, which is its
definition (host/frt_accum.c; pinned against a numpy reference in test_accum_cpu.py): bit for bit, on random samples
at the kernels' edges, and through GpuRenderer.render_accumulated."""
import numpy as np
import pytest

from conftest import load_scene

import accum_ref

pytestmark = pytest.mark.gpu

SEED = 0x5EED


@pytest.fixture(scope="module")
def rt(built):
    from fast_ray_tracer_amd import runtime
    runtime.host_lib()
    return runtime


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _host(rt, xs):
    acc = rt.Accumulator(xs.shape[1], device=None)
    try:
        for x in xs:
            acc.add(x)
        return acc.resolve(stats=True)
    finally:
        acc.close()


@pytest.mark.parametrize("npixels", [1, 63, 64, 65, 67 * 130])
def test_device_accumulator_is_the_host_accumulator(rt, npixels):
    """One wave's width and its neighbours, and 35 blocks with a ragged tail; from host arrays and from device
    tensors; the skipped samples counted alike; a reset starts over."""
    import torch
    xs = accum_ref.samples(npixels, 4, seed=npixels)
    want_mean, want_var, hst = _host(rt, xs)
    if npixels >= 8:
        assert hst.skipped >= 8 and want_var[0, 3] == 0 and want_var[1, 3] == 1
    acc = rt.Accumulator(npixels, device=0)
    try:
        for x in xs:
            acc.add(x)
        mean, var, st = acc.resolve(stats=True)
        assert _same_bits(mean, want_mean) and _same_bits(var, want_var)
        assert (st.pixels, st.frames, st.skipped, st.device) == (npixels, 4, hst.skipped, 0)
        assert st.add_ms > 0 and st.resolve_ms > 0
        # from device tensors, into device tensors
        acc.reset()
        tensors = [torch.from_numpy(x).cuda() for x in xs]
        torch.cuda.synchronize()
        for t in tensors:
            acc.add(t.data_ptr())
        d_mean = torch.full((npixels, 4), -3.0, dtype=torch.float64, device="cuda")
        d_var = torch.full((npixels, 4), -3.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        st = acc.resolve_into(d_mean.data_ptr(), d_var.data_ptr())
        assert _same_bits(d_mean.cpu().numpy(), want_mean) and _same_bits(d_var.cpu().numpy(), want_var)
        assert (st.frames, st.skipped) == (4, hst.skipped)
        assert all(_same_bits(t.cpu().numpy(), x) for t, x in zip(tensors, xs))  # (the samples are left alone)
        # a reset, then fewer samples: nothing of the earlier ones is left
        acc.reset()
        mean0, var0, st0 = acc.resolve(stats=True)
        assert not mean0.any() and not var0.any() and (st0.frames, st0.skipped) == (0, 0)
        for x in xs[:2]:
            acc.add(x)
        mean2, var2 = acc.resolve()
        want2 = _host(rt, xs[:2])
        assert _same_bits(mean2, want2[0]) and _same_bits(var2, want2[1])
    finally:
        acc.close()


def test_refusals_on_the_device(rt):
    acc = rt.Accumulator(16, device=0)
    try:
        with pytest.raises(ValueError):
            acc.add(np.zeros((15, 4)))
    finally:
        acc.close()
        acc.close()
    with pytest.raises(RuntimeError, match="no such HIP device"):
        rt.Accumulator(16, device=63)


def _host_accumulation(rt, r, frames, **args):
    h, w = r.frame.height, r.frame.width
    acc = rt.Accumulator((h, w), device=None)
    try:
        for k in range(frames):
            acc.add(r.render(seed=SEED + k, **args))
        return acc.resolve()
    finally:
        acc.close()


def test_render_accumulated_stochastic(rt):
    """cornell_shipped_48_4x4 (a multi-row area light: every seed draws other cache rows): three frames accumulated on
    the device are the host accumulation of render(seed + k), whatever the batch size."""
    r = rt.GpuRenderer(load_scene("cornell_shipped_48_4x4"))
    try:
        want_mean, want_var = _host_accumulation(rt, r, 3)
        mean, var, st = r.render_accumulated(3, seed=SEED, stats=True)
        assert mean.shape == var.shape == (r.frame.height, r.frame.width, 4)
        assert _same_bits(mean, want_mean) and _same_bits(var, want_var)
        assert (var[..., 3] == 3.0).all() and (var[..., :3] > 0).any()
        one = r.render(seed=SEED, stats=True)[1]
        assert st.primary_rays == 3 * one.primary_rays and st.errors == 0
        small, small_var = r.render_accumulated(3, seed=SEED, batch_samples=4096)
        assert _same_bits(small, want_mean) and _same_bits(small_var, want_var)
        with pytest.raises(ValueError):
            r.render_accumulated(0)
    finally:
        r.close()


def test_render_accumulated_deterministic(rt):
    """checkered_sphere_200 has nothing stochastic: the mean of two frames is the frame, and the variance is 0. The
    variance-guided denoise then leaves it alone (the bound of test_denoise_var_cpu.test_zero_variance_is_left_alone),
    and one frame alone is refused."""
    import denoise_var_ref
    r = rt.GpuRenderer(load_scene("checkered_sphere_200"))
    try:
        frame = r.render(seed=SEED)
        mean, var = r.render_accumulated(2, seed=SEED)
        assert _same_bits(mean, frame)
        assert not var[..., :3].any() and (var[..., 3] == 2.0).all()
        out, out_var, st = r.render_accumulated_denoised(2, seed=SEED)
        albedo = r.render_features(seed=SEED)["albedo"]
        bound = 4e-6 * float((albedo + denoise_var_ref.DEFAULTS["albedo_eps"]).max())
        moved = float(np.abs(out - frame).max())
        print("checkered_sphere_200: the variance-guided denoise moves the frame by %.3e (bound %.3e)" % (moved, bound))
        assert moved <= bound
        assert not out_var[..., :3].any() and st["valid_pixels"] > 0
        with pytest.raises(ValueError, match="frames >= 2"):
            r.render_accumulated_denoised(1, seed=SEED)
    finally:
        r.close()
