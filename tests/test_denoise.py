"""The denoise's device pass (csrc/frt_denoise.hip: k_denoise_pack, k_denoise_atrous) against the host pass, which is
its definition (host/frt_denoise.c; pinned against a numpy reference in test_denoise_cpu.py): bit for bit, on random
inputs at the kernels' edges, on rendered frames, and through GpuRenderer.render_denoised / render_denoised_views."""
import numpy as np
import pytest

from conftest import load_scene

import denoise_ref

pytestmark = pytest.mark.gpu

FLAGS = [{"demodulate": 1, "match_material": 1}, {"demodulate": 0, "match_material": 0}]


@pytest.fixture(scope="module")
def rt(built):
    from fast_ray_tracer_amd import runtime
    runtime.host_lib()
    return runtime


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _inputs(case):
    """A 64 x 4 tile's edges: one wave's width and its neighbours, one column, ragged tails on both axes, more than
    one block each way, a stack (taps must not cross images), and images with nothing or one pixel to filter."""
    if case == "all_invalid":
        rgba, geom, ids = denoise_ref.random_inputs((7, 70), seed=21)
        ids[...] = -1
    elif case == "one_valid":
        rgba, geom, ids = denoise_ref.random_inputs((7, 70), seed=22)
        ids[...] = -1
        ids[3, 65] = (5, 1)
        rgba[3, 65], geom[3, 65, 0] = (0.25, 0.5, 0.75, 1.0), 2.0
    else:
        rgba, geom, ids = denoise_ref.random_inputs(case, seed=30 + case[-1])
    return rgba, geom, ids


CASES = [(1, 1), (1, 63), (1, 64), (1, 65), (3, 1), (5, 130), (67, 130), (3, 6, 70), "all_invalid", "one_valid"]


def _on_device(rt, rgba, geom, ids, params, alias):
    """The device pass on device-resident buffers (torch tensors), out a buffer of its own or rgba itself."""
    import torch
    d_rgba, d_geom, d_ids = (torch.from_numpy(a).cuda() for a in (rgba, geom, ids))
    d_out = d_rgba if alias else torch.full_like(d_rgba, -3.0)
    torch.cuda.synchronize()
    k = rgba.shape[0] if rgba.ndim == 4 else 1
    st = rt._denoise(d_rgba.data_ptr(), d_geom.data_ptr(), d_ids.data_ptr(), True, rgba.shape[-2], rgba.shape[-3], k,
                     params, "device", 0, d_out.data_ptr())
    if not alias:
        assert _same_bits(d_rgba.cpu().numpy(), rgba)  # (the input is left alone)
    return d_out.cpu().numpy(), st


@pytest.mark.parametrize("flags", FLAGS, ids=["flags_on", "flags_off"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: c if isinstance(c, str) else "x".join(map(str, c)))
def test_device_pass_is_the_host_pass(rt, case, flags):
    rgba, geom, ids = _inputs(case)
    params = dict(flags, iterations=5)
    want, hst = rt.denoise(rgba, (geom, ids), params=params, backend="host", stats=True)
    valid = denoise_ref.valid_mask(rgba, geom, ids)
    assert hst.valid_pixels == valid.sum()
    got, st = rt.denoise(rgba, (geom, ids), params=params, backend="device", stats=True)
    assert _same_bits(got, want)
    d = st.as_dict()
    assert d["backend"] == "device" and d["device"] == 0 and d["iterations"] == 5 and len(d["atrous_iter_ms"]) == 5
    assert (st.pixels, st.valid_pixels) == (valid.size, valid.sum())
    assert st.pack_ms > 0 and st.atrous_ms > 0 and st.host_ms == 0
    for alias in (False, True):
        out, st = _on_device(rt, rgba, geom, ids, params, alias)
        assert _same_bits(out, want), alias
        assert st.upload_ms == 0 and st.valid_pixels == valid.sum()


@pytest.mark.parametrize("iterations", [1, 2, 8])
def test_iteration_counts(rt, iterations):
    """One iteration: the first launch is the writing one. Eight: steps up to 128, wider than the image's height."""
    rgba, geom, ids = _inputs((67, 130))
    params = {"iterations": iterations, "normal_squarings": 0}
    want = rt.denoise(rgba, (geom, ids), params=params, backend="host")
    assert _same_bits(rt.denoise(rgba, (geom, ids), params=params, backend="device"), want)
    assert _same_bits(_on_device(rt, rgba, geom, ids, params, True)[0], want)


def test_host_backend_on_device_buffers(rt):
    """frt_denoise with the host backend fetches device-resident buffers and puts out back."""
    import torch
    rgba, geom, ids = _inputs((5, 130))
    want = rt.denoise(rgba, (geom, ids), backend="host")
    d_rgba, d_geom, d_ids = (torch.from_numpy(a).cuda() for a in (rgba, geom, ids))
    d_out = torch.zeros_like(d_rgba)
    torch.cuda.synchronize()
    for backend in ("host", "auto"):
        st = rt._denoise(d_rgba.data_ptr(), d_geom.data_ptr(), d_ids.data_ptr(), True, 130, 5, 1, None, backend, 0,
                         d_out.data_ptr())
        assert st.as_dict()["backend"] == ("host" if backend == "host" else "device")
        assert _same_bits(d_out.cpu().numpy(), want)
        d_out.zero_()


# ---------------------------------------------------------------------------------------------------------------
# rendered frames

@pytest.mark.parametrize("name", ["cornell_gi_24", "checkered_sphere_200"])
def test_rendered_frames(rt, name):
    """A final-gather frame, and a frame with misses: the device's result is the host's."""
    r = rt.GpuRenderer(load_scene(name))
    try:
        frame = r.render(seed=3)
        f = r.render_features(seed=3)
    finally:
        r.close()
    hit = f["node"] >= 0
    assert hit.any()
    if name == "checkered_sphere_200":
        assert (~hit).any()
    want = rt.denoise(frame, f, backend="host")
    got, st = rt.denoise(frame, f, backend="device", stats=True)
    assert _same_bits(got, want)
    assert st.valid_pixels == (hit & np.isfinite(frame[..., :3]).all(axis=2)).sum()
    assert _same_bits(want[~hit], frame[~hit])
    assert not np.array_equal(want[hit], frame[hit])


# ---------------------------------------------------------------------------------------------------------------
# end to end

EYES = [((0.3, 0.2, -2.0), (0, 0, 0)), ((-0.4, 0.3, -1.6), (0.2, -0.2, 0.5))]


def test_render_denoised(rt):
    base = load_scene("cornell_direct_64_4x4")
    r = rt.GpuRenderer(base)
    try:
        params = rt.DenoiseParams(iterations=3)
        got, st = r.render_denoised(params=params, seed=9)
        want = rt.denoise(r.render(seed=9), r.render_features(seed=9), params=params, backend="device")
        assert got.shape == (base.height, base.width, 4) and _same_bits(got, want)
        assert st["backend"] == "device" and st["upload_ms"] == 0 and st["iterations"] == 3
        assert st["valid_pixels"] > 0
        # a strip of two views is the two single calls
        views = [base.view(f, t, hsize=40, vsize=30) for f, t in EYES]
        strip, sst = r.render_denoised_views(views, seed=9)
        assert r.frame is base and strip.shape == (2, 30, 40, 4) and sst["pixels"] == 2 * 30 * 40
        for k, v in enumerate(views):
            r.set_camera(v)
            one, _ = r.render_denoised(seed=9)
            assert _same_bits(strip[k], one), k
        r.set_camera(base)
        assert not np.array_equal(strip[0], strip[1])
        # the device buffers are freed and come back
        rt.denoise_release()
        again, _ = r.render_denoised(params=params, seed=9)
        assert _same_bits(again, want)
        rt.denoise_release()
        rt.denoise_release()
        with pytest.raises(TypeError):
            r.render_denoised_views(views, row_begin=2)
    finally:
        r.close()
