"""The variance-guided denoise's device pass (csrc/frt_denoise_var.hip: k_denoise_var_pack, k_denoise_var_atrous)
against the host pass, which is its definition (host/frt_denoise_var.c; pinned against a numpy reference in
test_denoise_var_cpu.py): bit for bit, on random inputs at the kernels' edges and through
GpuRenderer.render_accumulated_denoised."""
import numpy as np
import pytest

from conftest import load_scene

import denoise_ref
import denoise_var_ref as ref

pytestmark = pytest.mark.gpu

FLAGS = [{"demodulate": 1, "match_material": 1}, {"demodulate": 0, "match_material": 0}]

# tests/test_denoise.py's list: a 64 x 4 tile's edges, a stack, and images with nothing or one pixel to filter
CASES = [(1, 1), (1, 63), (1, 64), (1, 65), (3, 1), (5, 130), (67, 130), (3, 6, 70), "all_invalid", "one_valid"]


@pytest.fixture(scope="module")
def rt(built):
    from fast_ray_tracer_amd import runtime
    runtime.host_lib()
    return runtime


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _inputs(case):
    if case == "all_invalid":
        rgba, geom, ids = denoise_ref.random_inputs((7, 70), seed=21)
        ids[...] = -1
        var = ref.random_var((7, 70), 21)
    elif case == "one_valid":
        rgba, geom, ids = denoise_ref.random_inputs((7, 70), seed=22)
        ids[...] = -1
        ids[3, 65] = (5, 1)
        rgba[3, 65], geom[3, 65, 0] = (0.25, 0.5, 0.75, 1.0), 2.0
        var = ref.random_var((7, 70), 22)
        var[3, 65] = (0.01, 0.0, 0.02, 4.0)
    else:
        rgba, geom, ids = denoise_ref.random_inputs(case, seed=30 + case[-1])
        var = ref.random_var(case, 30 + case[-1], among=denoise_ref.valid_mask(rgba, geom, ids))
    return rgba, var, geom, ids


def _on_device(rt, rgba, var, geom, ids, params, alias, backend="device"):
    """The pass on device-resident buffers (torch tensors); alias: out is rgba and out_var is var, or both are
    buffers of their own."""
    import torch
    d_rgba, d_var, d_geom, d_ids = (torch.from_numpy(a).cuda() for a in (rgba, var, geom, ids))
    d_out = d_rgba if alias else torch.full_like(d_rgba, -3.0)
    d_out_var = d_var if alias else torch.full_like(d_var, -3.0)
    torch.cuda.synchronize()
    k = rgba.shape[0] if rgba.ndim == 4 else 1
    st = rt._denoise_var(d_rgba.data_ptr(), d_var.data_ptr(), d_geom.data_ptr(), d_ids.data_ptr(), True,
                         rgba.shape[-2], rgba.shape[-3], k, params, backend, 0, d_out.data_ptr(), d_out_var.data_ptr())
    if not alias:  # (the inputs are left alone)
        assert _same_bits(d_rgba.cpu().numpy(), rgba) and _same_bits(d_var.cpu().numpy(), var)
    return d_out.cpu().numpy(), d_out_var.cpu().numpy(), st


@pytest.mark.parametrize("flags", FLAGS, ids=["flags_on", "flags_off"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: c if isinstance(c, str) else "x".join(map(str, c)))
def test_device_pass_is_the_host_pass(rt, case, flags):
    rgba, var, geom, ids = _inputs(case)
    params = dict(flags, iterations=5)
    want, want_var, hst = rt.denoise_var(rgba, var, (geom, ids), params=params, backend="host", stats=True)
    valid = ref.valid_mask(rgba, var, geom, ids)
    assert hst.valid_pixels == valid.sum()
    got, got_var, st = rt.denoise_var(rgba, var, (geom, ids), params=params, backend="device", stats=True)
    assert _same_bits(got, want) and _same_bits(got_var, want_var)
    d = st.as_dict()
    assert d["backend"] == "device" and d["device"] == 0 and d["iterations"] == 5 and len(d["atrous_iter_ms"]) == 5
    assert (st.pixels, st.valid_pixels) == (valid.size, valid.sum())
    assert st.pack_ms > 0 and st.atrous_ms > 0 and st.host_ms == 0
    for alias in (False, True):
        out, out_var, st = _on_device(rt, rgba, var, geom, ids, params, alias)
        assert _same_bits(out, want) and _same_bits(out_var, want_var), alias
        assert st.upload_ms == 0 and st.valid_pixels == valid.sum()


@pytest.mark.parametrize("iterations", [1, 2, 8])
def test_iteration_counts(rt, iterations):
    """One iteration: the first launch is the writing one. Eight: steps up to 128, wider than the image's height."""
    rgba, var, geom, ids = _inputs((67, 130))
    params = {"iterations": iterations, "normal_squarings": 0}
    want, want_var = rt.denoise_var(rgba, var, (geom, ids), params=params, backend="host")
    got, got_var = rt.denoise_var(rgba, var, (geom, ids), params=params, backend="device")
    assert _same_bits(got, want) and _same_bits(got_var, want_var)
    out, out_var, _ = _on_device(rt, rgba, var, geom, ids, params, True)
    assert _same_bits(out, want) and _same_bits(out_var, want_var)


def test_no_out_var_and_host_backend_on_device_buffers(rt):
    """out_var may be NULL; frt_denoise_var with the host backend fetches device-resident buffers and puts both
    outputs back."""
    import ctypes

    import torch
    rgba, var, geom, ids = _inputs((5, 130))
    want, want_var = rt.denoise_var(rgba, var, (geom, ids), backend="host")
    out = np.empty_like(rgba)
    p = rt.DenoiseVarParams()
    rc = rt.host_lib().frt_denoise_var_device(rgba.ctypes.data, var.ctypes.data, geom.ctypes.data, ids.ctypes.data, 0,
                                              130, 5, 1, ctypes.byref(p), 0, out.ctypes.data, None, None)
    assert rc == 0 and _same_bits(out, want)
    d_rgba, d_var, d_geom, d_ids = (torch.from_numpy(a).cuda() for a in (rgba, var, geom, ids))
    d_out = torch.zeros_like(d_rgba)
    torch.cuda.synchronize()
    st = rt._denoise_var(d_rgba.data_ptr(), d_var.data_ptr(), d_geom.data_ptr(), d_ids.data_ptr(), True, 130, 5, 1,
                         None, "device", 0, d_out.data_ptr(), None)
    assert _same_bits(d_out.cpu().numpy(), want) and _same_bits(d_var.cpu().numpy(), var)
    for backend in ("host", "auto"):
        got, got_var, st = _on_device(rt, rgba, var, geom, ids, None, False, backend=backend)
        assert st.as_dict()["backend"] == ("host" if backend == "host" else "device")
        assert _same_bits(got, want) and _same_bits(got_var, want_var)
    # the device buffers are freed and come back
    rt.denoise_var_release()
    got, got_var = rt.denoise_var(rgba, var, (geom, ids), backend="device")
    assert _same_bits(got, want) and _same_bits(got_var, want_var)
    rt.denoise_var_release()
    rt.denoise_var_release()


def test_render_accumulated_denoised(rt):
    """cornell_shipped_48_4x4, three frames: the accumulation, the features and the filter on device buffers are the
    three separate calls."""
    r = rt.GpuRenderer(load_scene("cornell_shipped_48_4x4"))
    try:
        got, got_var, st = r.render_accumulated_denoised(3, seed=11)
        mean, var = r.render_accumulated(3, seed=11)
        want, want_var = rt.denoise_var(mean, var, r.render_features(seed=11), backend="device")
        assert got.shape == (r.frame.height, r.frame.width, 4)
        assert _same_bits(got, want) and _same_bits(got_var, want_var)
        assert st["backend"] == "device" and st["upload_ms"] == 0 and st["iterations"] == 5
        assert st["valid_pixels"] > 0 and not np.array_equal(got, mean)
        host, host_var = rt.denoise_var(mean, var, r.render_features(seed=11), backend="host")
        assert _same_bits(host, want) and _same_bits(host_var, want_var)
        with pytest.raises(ValueError, match="frames >= 2"):
            r.render_accumulated_denoised(1)
        with pytest.raises(TypeError):
            r.render_accumulated_denoised(2, row_begin=2)
    finally:
        r.close()
