"""The variance-guided denoise's host pass (host/frt_denoise_var.c, the definition the device pass repeats) against the
numpy reference of tests/denoise_var_ref.py, its behaviour on a synthetic image with and without noise, and the
refusals. No GPU."""
import ctypes

import numpy as np
import pytest

import denoise_ref
import denoise_var_ref as ref

# the tuple shapes of tests/test_denoise.py's CASES: a 64 x 4 tile's edges, and images wide enough (70, 130) that the
# taps of the steps 32 and 64 stay inside them
SHAPES = [(1, 1), (1, 63), (1, 64), (1, 65), (3, 1), (5, 130), (67, 130), (3, 6, 70)]
FLAGS = [{"demodulate": 1, "match_material": 1}, {"demodulate": 0, "match_material": 0}]


@pytest.fixture(scope="module")
def rt(built):
    from fast_ray_tracer_amd import runtime
    runtime.host_lib()
    return runtime


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _host(rt, rgba, var, geom, ids, **params):
    return rt.denoise_var(rgba, var, (geom, ids), params=params or None, backend="host")


def _inputs(shape):
    seed = 7 + len(shape) * 100 + shape[-1]
    rgba, geom, ids = denoise_ref.random_inputs(shape, seed=seed)
    return rgba, ref.random_var(shape, seed, among=denoise_ref.valid_mask(rgba, geom, ids)), geom, ids


# ---------------------------------------------------------------------------------------------------------------
# 1. against the numpy reference

@pytest.mark.parametrize("iterations", [1, 2, 8])
@pytest.mark.parametrize("flags", FLAGS, ids=["flags_on", "flags_off"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_host_pass_is_the_reference(rt, shape, flags, iterations):
    rgba, var, geom, ids = _inputs(shape)
    params = dict(flags, iterations=iterations)
    want, want_var = ref.denoise_var(rgba, var, geom, ids, **params)
    got, got_var = _host(rt, rgba, var, geom, ids, **params)
    valid = ref.valid_mask(rgba, var, geom, ids)
    if valid.size >= 8:  # (the negative and the NaN variance: valid by colour and ids, passed through)
        assert (denoise_ref.valid_mask(rgba, geom, ids) & ~valid).sum() == 2
    if valid.sum() > 1:
        assert not np.array_equal(got[valid], rgba[valid])  # (it filtered something)
    assert _same_bits(got[valid], want[valid]) and _same_bits(got_var[valid], want_var[valid])
    assert _same_bits(got[~valid], rgba[~valid]) and _same_bits(got_var[~valid], var[~valid])
    assert _same_bits(got[..., 3], rgba[..., 3]) and _same_bits(got_var[..., 3], var[..., 3])


@pytest.mark.parametrize("alias", ["out", "out_var", "both", "no_out_var"])
def test_in_place(rt, alias):
    rgba, var, geom, ids = _inputs((3, 6, 11))
    want, want_var = _host(rt, rgba, var, geom, ids)
    b_rgba, b_var = rgba.copy(), var.copy()
    out = b_rgba if alias in ("out", "both") else np.empty_like(rgba)
    out_var = b_var if alias in ("out_var", "both") else np.empty_like(var)
    p = rt.DenoiseVarParams()
    rc = rt.host_lib().frt_denoise_var_host(b_rgba.ctypes.data, b_var.ctypes.data, geom.ctypes.data, ids.ctypes.data,
                                            11, 6, 3, ctypes.byref(p), out.ctypes.data,
                                            None if alias == "no_out_var" else out_var.ctypes.data, None)
    assert rc == 0 and _same_bits(out, want)
    if alias != "no_out_var":
        assert _same_bits(out_var, want_var)


def test_a_stack_is_its_images(rt):
    rgba, var, geom, ids = _inputs((3, 6, 11))
    whole, whole_var = _host(rt, rgba, var, geom, ids)
    for k in range(3):
        one, one_var = _host(rt, rgba[k], var[k], geom[k], ids[k])
        assert _same_bits(whole[k], one) and _same_bits(whole_var[k], one_var), k


# ---------------------------------------------------------------------------------------------------------------
# 2. behaviour: variance 0 is left alone, noise goes down

ROWS = [(4, 0.2, (48, 96)), (2, 0.2, (48, 96)), (8, 0.05, (48, 96)), (4, 0.5, (40, 70))]


def _rmse(a, b, cols):
    return float(np.sqrt(np.mean((a[:, cols:, :3] - b[:, cols:, :3]) ** 2)))


@pytest.mark.parametrize("shape", [(48, 96), (40, 70)], ids=["48x96", "40x70"])
def test_zero_variance_is_left_alone(rt, shape):
    """A stack of two: image 0 noise-free with variance 0, image 1 noisy in its right half. A tap whose colour differs
    by delta pulls the centre by at most hk * delta / (1 + delta^2 kc / var_eps)^2 <= 0.325 sigma_color sqrt(var_eps)
    hk, and the non-centre hk sum to 6.1 times the centre's: with the defaults under 4e-6 in demodulated units, so
    under 4e-6 x max(albedo + albedo_eps) in the image. The fixed-width filter at its defaults moves the same image
    by more than 1e-2."""
    h, w = shape
    truth, geom, ids = ref.synthetic(h, w)
    var0 = np.zeros((h, w, 4))
    var0[..., 3] = 4.0
    mean1, var1 = ref.accumulate_noisy(truth, geom, 4, 0.2, seed=1, noisy_from=w // 2)
    rgba = np.stack([truth, mean1])
    var = np.stack([var0, var1])
    g2, i2 = np.stack([geom, geom]), np.stack([ids, ids])
    out, out_var = _host(rt, rgba, var, g2, i2)
    moved = float(np.abs(out[0] - truth).max())
    bound = 4e-6 * float((geom[..., 4:7] + ref.DEFAULTS["albedo_eps"]).max())
    plain = rt.denoise(truth, (geom, ids), backend="host")
    plain_moved = float(np.abs(plain - truth).max())
    print("%dx%d noise-free image: variance-guided moves it by %.3e (bound %.3e), the fixed-width filter by %.3e"
          % (h, w, moved, bound, plain_moved))
    assert moved <= bound
    assert not out_var[0, ..., :3].any()
    assert plain_moved > 1e-2
    # image 1 was filtered, and image 0 did not see it
    assert not np.array_equal(out[1], mean1)
    assert _same_bits(out[0], _host(rt, truth, var0, geom, ids)[0])


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("n,sigma,shape", ROWS, ids=["n4_s0.2", "n2_s0.2", "n8_s0.05", "n4_s0.5_40x70"])
def test_noise_goes_down(rt, n, sigma, shape, seed):
    """The noisy (right) half of the synthetic image: the error to the truth and the mean variance both shrink. At
    n = 8, sigma = 0.05 the fixed-width filter at its defaults makes the same half worse."""
    h, w = shape
    truth, geom, ids = ref.synthetic(h, w)
    mean, var = ref.accumulate_noisy(truth, geom, n, sigma, seed=seed, noisy_from=w // 2)
    out, out_var = _host(rt, mean, var, geom, ids)
    before = _rmse(mean, truth, w // 2)
    ratio = _rmse(out, truth, w // 2) / before
    vratio = float(out_var[:, w // 2:, :3].mean() / var[:, w // 2:, :3].mean())
    plain = _rmse(rt.denoise(mean, (geom, ids), backend="host"), truth, w // 2) / before
    print("n %d sigma %.2f %dx%d seed %d: RMSE after / before %.4f (fixed-width filter %.4f), variance after / before "
          "%.4f" % (n, sigma, h, w, seed, ratio, plain, vratio))
    assert ratio < 1
    assert vratio < 1
    if (n, sigma) == (8, 0.05):
        assert plain > 1


# ---------------------------------------------------------------------------------------------------------------
# 3. refusals, sizes, defaults

def test_defaults_and_sizes(rt):
    lib = rt.host_lib()
    assert lib.frt_denoise_var_params_size() == ctypes.sizeof(rt.DenoiseVarParams)
    assert ctypes.sizeof(rt.DenoiseVarStats) == lib.frt_denoise_stats_size()
    assert rt.DenoiseVarParams().as_dict() == ref.DEFAULTS
    assert rt.DenoiseVarParams(var_eps=1e-6).var_eps == 1e-6
    with pytest.raises(TypeError):
        rt.DenoiseVarParams(sigma=1.0)
    # the fixed-width filter's parameters are what they were
    assert ctypes.sizeof(rt.DenoiseParams) == 40 and rt.DenoiseParams().sigma_color == 1.0


BAD_PARAMS = [{"iterations": 0}, {"iterations": 9}, {"normal_squarings": -1}, {"normal_squarings": 9},
              {"demodulate": 2}, {"match_material": -1}, {"sigma_color": 0.0}, {"sigma_color": float("nan")},
              {"sigma_depth": 0.0}, {"sigma_depth": float("inf")}, {"albedo_eps": 0.0}, {"var_eps": 0.0},
              {"var_eps": -1.0}, {"var_eps": float("nan")}, {"var_eps": float("inf")}]
BAD_SIZES = [(0, 4, 1), (4, 0, 1), (4, 4, 0), (-1, 4, 1), (4, 4, -1), (65536, 32768, 1), (1 << 20, 1 << 10, 2),
             (1 << 31, 1, 1), (1 << 40, 1 << 40, 1)]


@pytest.mark.parametrize("entry", ["host", "device", "front_host", "front_device", "front_auto"])
def test_refusals(rt, entry):
    """Every refusal returns -1 with a message, before any device is looked for, and leaves out and out_var as they
    were."""
    lib = rt.host_lib()
    rgba, geom, ids = denoise_ref.random_inputs((4, 4), seed=1)
    var = ref.random_var((4, 4), 1)
    out, out_var = np.full_like(rgba, 7.25), np.full_like(var, 7.25)
    good = rt.DenoiseVarParams()

    def call(r, v, g, i, w, h, n, p, o):
        lib.frt_denoise_set_error.argtypes = [ctypes.c_char_p]
        lib.frt_denoise_set_error(b"")
        pp = ctypes.byref(p) if p is not None else None
        if entry == "host":
            return lib.frt_denoise_var_host(r, v, g, i, w, h, n, pp, o, out_var.ctypes.data, None)
        if entry == "device":
            return lib.frt_denoise_var_device(r, v, g, i, 0, w, h, n, pp, 0, o, out_var.ctypes.data, None)
        return lib.frt_denoise_var(r, v, g, i, 0, w, h, n, pp, ("front_host", "front_device", "front_auto").index(entry),
                                   0, o, out_var.ctypes.data, None)

    ptrs = [rgba.ctypes.data, var.ctypes.data, geom.ctypes.data, ids.ctypes.data]
    cases = []
    for k in range(4):
        cases.append(("null %d" % k, ptrs[:k] + [None] + ptrs[k + 1:], (4, 4, 1), good, out.ctypes.data))
    cases.append(("null params", ptrs, (4, 4, 1), None, out.ctypes.data))
    cases.append(("null out", ptrs, (4, 4, 1), good, None))
    cases += [("size %r" % (s,), ptrs, s, good, out.ctypes.data) for s in BAD_SIZES]
    cases += [("param %r" % (b,), ptrs, (4, 4, 1), rt.DenoiseVarParams(**b), out.ctypes.data) for b in BAD_PARAMS]
    for what, (r, v, g, i), (w, h, n), p, o in cases:
        assert call(r, v, g, i, w, h, n, p, o) == -1, what
        assert lib.frt_denoise_error().decode().startswith("frt_denoise_var"), what
        assert (out == 7.25).all() and (out_var == 7.25).all(), what
    if entry.startswith("front"):
        assert lib.frt_denoise_var(*ptrs, 0, 4, 4, 1, ctypes.byref(good), 3, 0, out.ctypes.data, None, None) == -1
        assert "backend" in lib.frt_denoise_error().decode() and (out == 7.25).all()
    with pytest.raises(RuntimeError, match="iterations must be 1..8"):
        rt.denoise_var(rgba, var, (geom, ids), params={"iterations": 9}, backend="host")
    with pytest.raises(ValueError):
        rt.denoise_var(rgba, var[:3], (geom, ids), backend="host")
    with pytest.raises(ValueError):
        rt.denoise_var(rgba, var, (geom, ids), backend="cpu")
