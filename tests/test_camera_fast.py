"""FRT_CAM_FAST (csrc/frt_knobs.hpp, a frame knob): level 0's camera arithmetic in its cheap form — the two index
divisions of frt_camera.hpp camera_sample by multiply-shift in 32 bits (csrc/frt_cam_index.hpp), column and row
converted from 32-bit integers, and the one ray origin of a camera without an aperture taken from the host — against
FRT_CAM_FAST=0, the 64-bit divisions and the origin computed per ray. The integers are the same integers and the
doubles the same doubles, so every comparison here is np.array_equal: rays (through the closest hits and the
canvases), keys (through the rows a multi-row light draws and the children's keys) and feature planes.

The knob is read at the top of each frame, so one renderer renders both sides. The shapes are small: waves that
straddle pixels (spp 9), divisors that are no powers of two (7, 9, 30), batches that begin inside a row, strided
rows, and a strip of views (which keeps the 64-bit arithmetic by design: both sides must still agree).
"""
import os

import numpy as np
import pytest

from conftest import load_scene

pytestmark = pytest.mark.gpu

EYE = ((0.3, 0.2, -2.0), (0, 0, 0))


def _both(call):
    """call() under the default (FRT_CAM_FAST unset: on) and under FRT_CAM_FAST=0."""
    saved = os.environ.pop("FRT_CAM_FAST", None)
    try:
        fast = call()
        os.environ["FRT_CAM_FAST"] = "0"
        slow = call()
    finally:
        os.environ.pop("FRT_CAM_FAST", None)
        if saved is not None:
            os.environ["FRT_CAM_FAST"] = saved
    return fast, slow


def _same_canvas(fast, slow, what):
    assert fast.shape == slow.shape and np.isfinite(fast).all() and fast[..., :3].max() > 0, what
    assert np.array_equal(fast, slow), what


def test_small_views_batches_and_row_splits(built):
    """One resident cornell box under three cameras: 7x5 at 3x3 (spp 9: a wave holds seven pixels and a bit, neither
    divisor is a power of two), 16x9 at 8x8 in batches of 320 samples (five pixels: every batch but the first begins
    inside a row), and 30x17 at 3x3 as rows 1, 4, 7, ... (row_begin 1, row_stride 3), whole and in batches."""
    from fast_ray_tracer_amd.runtime import GpuRenderer
    base = load_scene("cornell_direct_64_4x4")
    r = GpuRenderer(base)
    try:
        r.set_camera(base.view(*EYE, hsize=7, vsize=5, usteps=3, vsteps=3))
        _same_canvas(*_both(lambda: r.render()), "7x5 3x3")
        _same_canvas(*_both(lambda: r.render(batch_samples=2 * 9)), "7x5 3x3, two pixels per batch")

        r.set_camera(base.view(*EYE, hsize=16, vsize=9, usteps=8, vsteps=8))
        whole, _ = _both(lambda: r.render())
        fast, slow = _both(lambda: r.render(batch_samples=320))
        _same_canvas(fast, slow, "16x9 8x8, 320 samples per batch")
        assert np.array_equal(fast, whole)

        r.set_camera(base.view(*EYE, hsize=30, vsize=17, usteps=3, vsteps=3))
        whole, slow = _both(lambda: r.render())
        _same_canvas(whole, slow, "30x17 3x3")
        fast, slow = _both(lambda: r.render(1, None, 3))
        _same_canvas(fast, slow, "30x17 3x3, rows 1::3")
        assert np.array_equal(fast, whole[1::3])
        fast, slow = _both(lambda: r.render(1, None, 3, batch_samples=1000))
        _same_canvas(fast, slow, "30x17 3x3, rows 1::3 in batches of 111 pixels")
        assert np.array_equal(fast, whole[1::3])
    finally:
        r.close()


@pytest.mark.parametrize("name", ["checkered_sphere_jitter_100", "checkered_sphere_dof_100"])
def test_jitter_and_thin_lens(built, name):
    """The jittered sub-pixel points (cmj_point takes the global pixel index) and the thin lens (aperture_point takes
    the global sample index; with an aperture every ray has an origin of its own: none is taken from the host)."""
    from fast_ray_tracer_amd.runtime import GpuRenderer
    r = GpuRenderer(load_scene(name))
    try:
        _same_canvas(*_both(lambda: r.render()), name)
    finally:
        r.close()


def test_reflection_keys_and_multi_row_light(built):
    """reflect_refract_test_150 seen from the side: the level-1 rays' keys are made from the level-0 keys, and
    primary misses return before any ray is made. cornell_shipped_48_4x4: each node's key draws its cache row of the
    multi-row light, and level 0 stores the keys camera_ray gives it; with FRT_HEAD_KEY0=0 every reader derives them
    through camera_key instead."""
    from fast_ray_tracer_amd.runtime import GpuRenderer
    base = load_scene("reflect_refract_test_150")
    r = GpuRenderer(base.view((5.0, 0.5, -0.5), (0, 0, 0), hsize=45, vsize=31))
    try:
        (fast, st), (slow, _) = _both(lambda: r.render(stats=True))
        assert st.secondary_rays > 0 and st.hits < st.primary_rays + st.secondary_rays
        _same_canvas(fast, slow, "reflect_refract side view")
    finally:
        r.close()
    r = GpuRenderer(load_scene("cornell_shipped_48_4x4"))
    saved = os.environ.pop("FRT_HEAD_KEY0", None)
    try:
        fast, slow = _both(lambda: r.render(seed=20260))
        _same_canvas(fast, slow, "cornell_shipped_48_4x4")
        assert not np.array_equal(fast, r.render(seed=20261))  # (the rows are drawn: the key matters)
        os.environ["FRT_HEAD_KEY0"] = "0"
        derived, derived_slow = _both(lambda: r.render(seed=20260, batch_samples=1000))
        _same_canvas(derived, derived_slow, "cornell_shipped_48_4x4, derived keys")
        assert np.array_equal(derived, fast)
    finally:
        os.environ.pop("FRT_HEAD_KEY0", None)
        if saved is not None:
            os.environ["FRT_HEAD_KEY0"] = saved
        r.close()


def test_strip_of_views_and_features(built):
    """A strip of three views (its rays come from the camera table with the 64-bit arithmetic either way) equals the
    three single-view frames, which take the fast path; and one render_features call: depth, normal and the id
    planes."""
    from fast_ray_tracer_amd.runtime import GpuRenderer
    base = load_scene("cornell_direct_64_4x4")
    eyes = [EYE, ((-0.4, 0.3, -1.6), (0.2, -0.2, 0.5)), ((0.0, -0.3, -2.4), (0, 0, 0))]
    views = [base.view(f, t, hsize=30, vsize=17, usteps=3, vsteps=3) for f, t in eyes]
    r = GpuRenderer(base)
    try:
        fast, slow = _both(lambda: r.render_views(views))
        _same_canvas(fast, slow, "strip of three views")
        for k, v in enumerate(views):
            r.set_camera(v)
            assert np.array_equal(fast[k], r.render()), k
        ffast, fslow = _both(lambda: r.render_features())
        assert ffast["coverage"].max() > 0 and (ffast["node"] >= 0).any()
        for plane in ("depth", "normal", "node", "material", "albedo", "coverage"):
            assert np.array_equal(ffast[plane], fslow[plane]), plane
    finally:
        r.close()
