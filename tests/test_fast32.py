"""The fast shading mode (frt_frame_params.precision = FRT_PRECISION_FAST32, FRT_PRECISION=fast32): the light-point
loop of lighting_microfacet in binary32 (k_shade_lit32, csrc/frt_shade32.hpp), everything else binary64. Opt-in: the
default and "parity" stay the reference's arithmetic bit for bit; a fast frame stays within TOL_FAST of the
reference's golden canvases and keeps the engine's invariants (bit-reproducible; independent of row split, batch
size and the lit list's order)."""
import ctypes
import os

import numpy as np
import pytest

from conftest import canvas_goldens, golden_index, load_golden_canvas, load_scene

# 4 x the largest max_abs_vs_reference of a deterministic canvas golden in profiles/fast32_mismatch.json (4.47e-4,
# area_light_test_100: measured against the reference's golden canvases on an MI355X with the build of the commit
# that adds this file, on top of d300050), rounded up to one significant digit. The 4 covers another compiler's
# ordering of the binary32 operations and the device library's log2 / exp2; on one build the mode is
# bit-reproducible (the tests below). A measured maximum above 1e-3 is a bug to find, not a reason to raise this.
TOL_FAST = 2e-3

DETERMINISTIC = [n for n in canvas_goldens() if not golden_index()[n].get("stochastic")]


def test_frame_params_mirror_matches_the_library(built):
    from fast_ray_tracer_amd.runtime import FrameParams, host_lib
    lib = host_lib()
    lib.frt_frame_params_size.restype = ctypes.c_size_t
    assert lib.frt_frame_params_size() == ctypes.sizeof(FrameParams) == 48
    assert FrameParams.precision.offset == 44 and FrameParams.precision.size == 4  # (the former padding word)
    assert not hasattr(FrameParams, "pad")


_renderers = {}
_frames = {}


def renderer(name):
    from fast_ray_tracer_amd.runtime import GpuRenderer
    if name not in _renderers:
        _renderers[name] = GpuRenderer(load_scene(name))
    return _renderers[name]


def frame(name, precision):
    """The full frame of a golden scene in one mode (rendered once, shared by the tests, never written to)."""
    if (name, precision) not in _frames:
        img = renderer(name).render(precision=precision)
        img.setflags(write=False)
        _frames[(name, precision)] = img
    return _frames[(name, precision)]


class _env:
    def __init__(self, **env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _render_env(name, env, **kw):
    """Render with environment switches that the engine reads at upload."""
    from fast_ray_tracer_amd.runtime import GpuRenderer
    with _env(**env):
        r = GpuRenderer(load_scene(name))
    try:
        return r.render(**kw)
    finally:
        r.close()


@pytest.mark.gpu
def test_default_is_parity_and_precision_is_per_frame(built):
    name = "cornell_direct_64_4x4"
    r = renderer(name)
    default, st_default = r.render(stats=True)
    parity, st_parity = r.render(stats=True, precision="parity")
    with _env(FRT_PRECISION="parity"):
        env_parity = r.render()
    assert np.array_equal(default, parity) and np.array_equal(default, env_parity)
    for st in (st_default, st_parity):
        launches = st.as_dict()["sub_launches"]
        assert "k_shade_lit" in launches and "k_shade_lit32" not in launches
    fast, st_fast = r.render(stats=True, precision="fast32")
    launches = st_fast.as_dict()["sub_launches"]
    assert "k_shade_lit32" in launches and "k_shade_lit" not in launches
    with _env(FRT_PRECISION="fast32"):  # (read at every frame: the same handle, no new upload)
        env_fast, st_env = r.render(stats=True)
        explicit = r.render(precision="parity")
    assert "k_shade_lit32" in st_env.as_dict()["sub_launches"]
    assert np.array_equal(env_fast, fast)
    assert np.array_equal(explicit, default)  # (the params win over the environment)
    with pytest.raises(RuntimeError, match="precision 7 is not supported"):
        r.render(precision=7)
    with _env(FRT_PRECISION="half"):
        with pytest.raises(RuntimeError, match="not supported"):
            r.render()
    with _env(FRT_SHADE_SPLIT="0"):  # (k_shade alone shades every node in binary64: refused, not rendered as parity)
        with pytest.raises(RuntimeError, match="not supported"):
            r.render(precision="fast32")
    assert np.array_equal(r.render(), default)


@pytest.mark.gpu
@pytest.mark.parametrize("name", DETERMINISTIC)
def test_fast32_close_to_reference_canvas(built, name):
    from fast_ray_tracer_amd.runtime import ppm_values
    img = frame(name, "fast32")[:, :, :3]
    ref = load_golden_canvas(name)
    assert np.isfinite(frame(name, "fast32")).all()
    diff = np.abs(img - ref)
    got, want = ppm_values(img), ppm_values(ref)
    print(f"{name}: max|fast32 - reference|={diff.max():.3e} ppm mismatch fraction={(got != want).mean():.4%} "
          f"max step={np.abs(got - want).max()}")
    assert diff.max() <= TOL_FAST


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["shadow_glamour_150x60", "cornell_direct_64_4x4"])
def test_fast32_is_a_different_mode(built, name):
    assert not np.array_equal(frame(name, "fast32"), frame(name, "parity"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell_direct_64_4x4", "csg_nested_96x64"])
def test_fast32_reproducible_and_split_and_batch_invariant(built, name):
    r = renderer(name)
    full = frame(name, "fast32")
    assert np.array_equal(full, r.render(precision="fast32"))
    for n in (2, 3):
        for k in range(n):
            assert np.array_equal(full[k::n], r.render(k, None, n, precision="fast32")), (n, k)
    assert np.array_equal(full, r.render(batch_samples=1 << 12, precision="fast32"))
    row = full.shape[0] // 2 + 1  # (one row: fewer lit nodes than a wave's worth of list segments)
    assert np.array_equal(full[row:row + 1], r.render(row, row + 1, precision="fast32"))


@pytest.mark.gpu
def test_fast32_multi_row_light(built):
    """The shipped area light's cache (a row per shading draw): fast32 against parity at the same seed (the one
    deterministic yardstick of a stochastic scene), and the row-ordered shading's modes against list order."""
    name = "cornell_shipped_48_4x4"
    parity = _render_env(name, {"FRT_SHADE_SORT": "0"}, precision="parity")
    plain = _render_env(name, {"FRT_SHADE_SORT": "0"}, precision="fast32")
    assert np.isfinite(plain).all() and plain[:, :, :3].max() > 0
    d = np.abs(plain - parity).max()
    print(f"{name}: max|fast32 - parity|={d:.3e}")
    assert d <= TOL_FAST
    assert not np.array_equal(plain, parity)
    for mode in ("0", "1", "2"):
        other = _render_env(name, {"FRT_SHADE_SORT": "1", "FRT_SHADE_STAGE": mode}, precision="fast32")
        assert np.array_equal(other, plain), mode


@pytest.mark.gpu
def test_shade32_selftest(built):
    from fast_ray_tracer_amd.runtime import host_lib
    lib = host_lib()
    lib.frt_shade32_selftest.restype = ctypes.c_int64
    lib.frt_shade32_selftest.argtypes = [ctypes.c_int64, ctypes.c_uint64, ctypes.POINTER(ctypes.c_double),
                                         ctypes.c_int]
    for seed in (1, 0x5eed):
        out = (ctypes.c_double * 4)()
        bad = lib.frt_shade32_selftest(1 << 20, seed, out, 4)
        print(f"seed {seed:#x}: bad={bad} worst specular deviation={out[0]:.3e} (Ns <= 200: {out[1]:.3e}) "
              f"worst |l.n| deviation={out[2]:.3e} over {int(out[3])} lanes")
        assert bad == 0
        assert out[3] > (1 << 20) / 8  # (the record is of real lanes)
