"""The 16-bit image encode (write_ppm_file / write_png values) on the device, byte-identical to the host pass.

The reference for every comparison is the host pass (``encode_ppm`` / ``encode16(backend="host")``, the reference's
three passes with libm's pow) and, for the goldens, the reference's own ``ppm_sha256``.

The adversarial set: the per-code boundary values (256 codes x 5 neighbours = 1280 values) are undecided by
construction, and the device declines an image with more than 1/64 of its values undecided, so the full set sits in a
67 x 449 canvas (90 249 values, cap 1410). The 67 x 3 canvas (603 values, cap 9) carries every other class and the
neighbours of one code; the 1 x 1 canvas (cap 0) a single ordinary pixel. The widths stay odd.
"""
import ctypes
import hashlib
import os

import numpy as np
import pytest

from conftest import canvas_goldens, golden_index, load_golden_canvas, load_scene

MODES = ("ppm_scaled", "ppm_clamped", "png")
SQRT3 = 1.7320508075688772


def srgb_one():
    from fast_ray_tracer_amd.runtime import host_lib
    lib = host_lib()
    a = (ctypes.c_double * 4)(1.0, 1.0, 1.0, 0.0)
    b = (ctypes.c_double * 4)()
    lib.rgb_to_srgb.restype = None
    lib.rgb_to_srgb.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.rgb_to_srgb(a, b)
    return b[0]


def payload(rgba, use_scaling):
    from fast_ray_tracer_amd.runtime import encode_ppm
    h, w = rgba.shape[:2]
    data = encode_ppm(rgba, use_scaling)
    return np.frombuffer(data[len(data) - 1 - 6 * h * w:len(data) - 1], dtype=">u2").reshape(h, w, 3).astype(np.uint16)


def ppm_bytes(values):
    h, w = values.shape[:2]
    return b"P6\n%d %d\n65535\n" % (w, h) + values.astype(">u2").tobytes() + b"\n"


def ulps(x, n):
    x = np.float64(x)
    for _ in range(abs(n)):
        x = np.nextafter(x, np.float64(np.inf if n > 0 else -np.inf))
    return float(x)


def code_boundary(k, inverse):
    """The double nearest the linear value whose sRGB value times inverse is the integer k."""
    s = k / inverse
    return float(((s + 0.055) / 1.055) ** 2.4)


def sum_to(target):
    """Three channels whose left-to-right sum is exactly target."""
    a, b = 0.5, 0.625
    c = target - (a + b)
    for step in range(-8, 9):
        cc = ulps(c, step)
        if (a + b) + cc == target:
            return [a, b, cc]
    raise AssertionError("no third channel sums to %r" % target)


def special_pixels(codes):
    inverse = 65535.0 / srgb_one()
    px = []
    for n in (-2, -1, 0, 1, 2):  # both sides of the linear / pow threshold
        px.append([ulps(0.0031308, n), 0.25, 0.0031308 * 0.5])
    for n in (-1, 0, 1):  # sums straddling sqrt(3) by one ulp
        px.append(sum_to(ulps(SQRT3, n)))
    px.append([1.0, 1.0, 1.0])  # exact 1.0 (clamped modes) and a sum over sqrt(3) (scaled mode)
    px.append([1.0, 0.25, 0.125])  # exact 1.0, not scaled
    px.append([ulps(1.0, -1), ulps(1.0, 1), 0.5])  # just below and above 1.0
    px.append([ulps(1.0, -2), 0.125, ulps(1.0, 2)])
    px.append([-0.25, -1e-300, -0.0])  # negatives
    px.append([1.5, 7.0, 1e300])  # above the maximum code
    px.append([5e-324, 2.2250738585072009e-308, 1e-310])  # subnormals
    px.append([3.0, 2.0, -4.5])
    for j, k in enumerate(codes):  # a code boundary and its +-1, +-2 ulp neighbours, one per pixel
        t = code_boundary(k, inverse)
        for n in (0, -1, 1, -2, 2):
            p = [0.03125, 0.0625, 0.015625]
            p[(j + n) % 3] = ulps(t, n)
            px.append(p)
    return px


def adversarial(width, height, codes, seed):
    rng = np.random.default_rng(seed)
    img = np.zeros((height, width, 4))
    img[:, :, :3] = rng.random((height, width, 3)) * 1.25  # ordinary values, some over 1 and some sums over sqrt(3)
    img[:, :, 3] = rng.random((height, width))
    px = special_pixels(codes)
    assert len(px) <= width * height
    at = rng.permutation(width * height)[:len(px)]
    flat = img.reshape(-1, 4)
    for i, p in zip(at, px):
        flat[i, :3] = p
    return img


_cache = {}


def canvas(name):
    if name not in _cache:
        if name == "adv_67x449":
            c = adversarial(67, 449, [1 + (65533 * j) // 255 for j in range(256)], 1)
        elif name == "adv_67x3":
            c = adversarial(67, 3, [40000], 2)
        elif name == "adv_1x1":
            c = np.array([[[0.4, 0.7, 0.2, 0.0]]])
        elif name == "over_cap":  # one value on a code boundary, below sqrt(3)/3 so that no mode moves it
            c = np.zeros((64, 64, 4))
            c[:, :, :3] = code_boundary(40000, 65535.0 / srgb_one())
        else:
            c = load_golden_canvas(name)
        c.setflags(write=False)
        _cache[name] = c
    return _cache[name]


_host = {}


def host_values(name, mode):
    """The host pass's values of a canvas (computed once per session)."""
    if (name, mode) not in _host:
        from fast_ray_tracer_amd.runtime import encode16
        v, st = encode16(canvas(name), mode, backend="host")
        assert st["backend"] == "host" and st["decline"] is None
        _host[(name, mode)] = v
    return _host[(name, mode)]


ADVERSARIAL = ("adv_67x449", "adv_67x3", "adv_1x1", "over_cap")


# ---------------------------------------------------------------------------------------------------------------
# CPU tests

def test_host_backend_equals_encode_ppm(built):
    """The refactored host pass (one per-pixel helper) is encode_ppm's payload, and the goldens' is the reference's."""
    index = golden_index()
    for name in list(canvas_goldens()) + list(ADVERSARIAL):
        c = canvas(name)
        for mode, scaling in (("ppm_scaled", True), ("ppm_clamped", False)):
            want = payload(c, scaling)
            assert np.array_equal(host_values(name, mode), want), (name, mode)
        if name in index and "ppm_sha256" in index[name]:
            assert hashlib.sha256(ppm_bytes(host_values(name, "ppm_scaled"))).hexdigest() == index[name]["ppm_sha256"]


def test_srgb_max_shortcut(built):
    """srgb_max is rgb_to_srgb(1.0) whenever every channel maximum is positive: the full second pass agrees on
    canvases whose maxima have 1-to-4-ulp-smaller neighbours (the quotients nearest below 1.0)."""
    from fast_ray_tracer_amd.runtime import srgb_max_full
    one = srgb_one()
    assert one <= 1.0
    rng = np.random.default_rng(7)
    for top in (1.0, 0.7, 3.3, 1e-3, 123.456, 1e-300, 0.0031308, 65535.0):
        img = np.zeros((16, 16, 4))
        img[:, :, :3] = rng.random((16, 16, 3)) * top
        flat = img.reshape(-1, 4)
        for k in range(3):
            for n in range(5):
                flat[7 * k + n, k] = ulps(top * (1.0 + 0.125 * k), -n)
        assert srgb_max_full(img) == [one, one, one], top
    for name in canvas_goldens():
        c = canvas(name)
        if (c.reshape(-1, c.shape[2])[:, :3].max(axis=0) > 0).all():
            assert srgb_max_full(c) == [one, one, one], name


def declined_canvases():
    rng = np.random.default_rng(3)
    base = np.zeros((9, 13, 4))
    base[:, :, :3] = rng.random((9, 13, 3)) * 1.5
    out = {}
    c = base.copy()
    c[:, :, 1] = 0.0
    out["zero_channel"] = (c, "zero_max")
    c = base.copy()
    c[4, 5, 2] = np.nan
    out["nan_pixel"] = (c, "non_finite")
    c = base.copy()
    c[8, 12, 0] = np.inf
    out["inf_pixel"] = (c, "non_finite")
    c = base.copy()
    c[:, :, 2] = -c[:, :, 2] - 0.125
    out["negative_channel"] = (c, "zero_max")
    return out


@pytest.mark.parametrize("case", ["zero_channel", "nan_pixel", "inf_pixel", "negative_channel"])
def test_declined_canvases_take_the_host_path(built, case):
    from fast_ray_tracer_amd.runtime import encode16
    c, reason = declined_canvases()[case]
    for mode, scaling in (("ppm_scaled", True), ("ppm_clamped", False)):
        with np.errstate(all="ignore"):
            v, st = encode16(c, mode, backend="device")
        assert st["backend"] == "host" and st["decline"] == reason, st
        assert np.array_equal(v, payload(c, scaling))


def test_encode_device_without_gpu_still_writes_the_files(built, tmp_path, monkeypatch):
    """FRT_ENCODE=device writes the PPM and the PNG FRT_ENCODE=host writes (on a machine without a GPU through the
    fall-back to the host pass)."""
    from fast_ray_tracer_amd.runtime import write_png, write_ppm
    c = np.zeros((48, 48, 4))
    c[:, :, :3] = np.random.default_rng(11).random((48, 48, 3)) * 1.4
    sha = {}
    for backend in ("host", "device"):
        monkeypatch.setenv("FRT_ENCODE", backend)
        base = str(tmp_path / backend)
        st = write_ppm(base, c)
        assert st["backend"] in ("host", "device") and (backend != "host" or st["backend"] == "host")
        write_png(base, c)
        sha[backend] = [hashlib.sha256(open(base + ext, "rb").read()).hexdigest() for ext in (".ppm", ".png")]
    assert sha["host"] == sha["device"]
    assert hashlib.sha256(open(str(tmp_path / "host") + ".ppm", "rb").read()).digest() == hashlib.sha256(
        ppm_bytes(payload(c, True))).digest()


# ---------------------------------------------------------------------------------------------------------------
# GPU tests

def device_values(name, mode):
    from fast_ray_tracer_amd.runtime import encode16
    v, st = encode16(canvas(name), mode, backend="device")
    print(name, mode, {k: st[k] for k in ("backend", "decline", "undecided", "values")})
    return v, st


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in canvas_goldens() if "ppm_sha256" in golden_index()[n]])
def test_goldens_on_the_device(built, name):
    for mode in MODES:
        v, st = device_values(name, mode)
        assert st["backend"] == "device" and st["decline"] is None, st
        assert st["undecided"] <= 1e-4 * st["values"], st
        if mode == "ppm_scaled":
            assert hashlib.sha256(ppm_bytes(v)).hexdigest() == golden_index()[name]["ppm_sha256"]
        assert np.array_equal(v, host_values(name, mode)), mode


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["adv_67x449", "adv_67x3", "adv_1x1"])
def test_adversarial_canvas_on_the_device(built, name):
    for mode in MODES:
        v, st = device_values(name, mode)
        assert st["backend"] == "device" and st["decline"] is None, st
        bad = np.argwhere(v != host_values(name, mode))
        assert len(bad) == 0, (mode, bad[:8], canvas(name)[tuple(bad[0][:2])] if len(bad) else None)
        if name != "adv_1x1":
            assert st["undecided"] >= 1, st  # (the patch path ran)


@pytest.mark.gpu
def test_over_the_cap_is_declined(built):
    for mode in MODES:
        v, st = device_values("over_cap", mode)
        assert st["backend"] == "host" and st["decline"] == "over_cap", st
        assert np.array_equal(v, host_values("over_cap", mode))


@pytest.mark.gpu
def test_encode_selftest(built):
    from fast_ray_tracer_amd.runtime import encode_selftest
    bad, out = encode_selftest(1 << 20, 0x5EED)
    print("encode selftest: failed %d, worst sRGB deviation %.3e (2^%.1f), pow %.3e, differing %d"
          % (bad, out[0], np.log2(out[0]) if out[0] > 0 else -np.inf, out[1], out[2]))
    assert bad == 0
    assert out[0] < 2.0 ** -44


@pytest.mark.gpu
def test_render_encoded_from_device_memory(built):
    from fast_ray_tracer_amd.runtime import GpuRenderer, encode16
    name = "cornell_direct_64_4x4"
    r = GpuRenderer(load_scene(name))
    try:
        v, st = r.render_encoded("ppm_scaled")
        assert st["backend"] == "device" and st["upload_ms"] == 0.0, st
        want, _ = encode16(r.render(), "ppm_scaled", backend="host")
        assert np.array_equal(v, want)
        assert hashlib.sha256(ppm_bytes(v)).hexdigest() == golden_index()[name]["ppm_sha256"]
        for mode in ("ppm_clamped", "png"):
            v, st = r.render_encoded(mode)
            assert st["backend"] == "device"
            assert np.array_equal(v, encode16(r.render(), mode, backend="host")[0])
    finally:
        r.close()


@pytest.mark.gpu
def test_drop_in_writes_through_the_device(built, tmp_path, monkeypatch):
    """After render_multi the default (auto) encodes write_ppm_file / write_png on the device; the files are the
    host pass's."""
    from fast_ray_tracer_amd.runtime import release_render_multi, render_multi, write_png, write_ppm
    monkeypatch.delenv("FRT_ENCODE", raising=False)
    c = render_multi(load_scene("cornell_direct_64_4x4"), devices="0")
    try:
        sha = {}
        for backend in ("auto", "host"):
            if backend == "host":
                monkeypatch.setenv("FRT_ENCODE", "host")
            base = str(tmp_path / backend)
            st_ppm = write_ppm(base, c)
            st_png = write_png(base, c)
            assert st_ppm["backend"] == st_png["backend"] == ("device" if backend == "auto" else "host"), (st_ppm, st_png)
            sha[backend] = [hashlib.sha256(open(base + ext, "rb").read()).hexdigest() for ext in (".ppm", ".png")]
        assert sha["auto"] == sha["host"]
        assert sha["host"][0] == golden_index()["cornell_direct_64_4x4"]["ppm_sha256"]
    finally:
        del c
        release_render_multi()
