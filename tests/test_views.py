"""Views: the camera of a resident scene moved (frt_scene_set_camera), K views in one strip frame
(frt_render_views*), and render_multi's reuse of its kept handles under another camera.

The references: the goldens' canvases where another golden is "the same world under another camera", a fresh upload
of that scene (bit for bit), and the CPU oracle for cameras no golden has (within 1e-4, the parity tests' bound)."""
import ctypes
import gc
import hashlib
import os

import numpy as np
import pytest

from conftest import golden_index, load_golden_canvas, load_scene

pytestmark = pytest.mark.gpu

TOL = 1e-4


def _renderer(scene):
    from fast_ray_tracer_amd.runtime import GpuRenderer
    return GpuRenderer(scene)


def _fresh(scene, **args):
    """A frame of a fresh upload of `scene` (a Scene, or a View: the same world uploaded under its camera)."""
    r = _renderer(scene)
    try:
        return r.render(**args)
    finally:
        r.close()


def test_goldens_through_set_camera(built):
    """One handle on cornell_direct_64_4x4 renders the goldens that differ from it in their camera lines only:
    within 1e-4 of their canvases, their 16-bit PPM values, and bit for bit a fresh upload of them; back under its
    own camera it repeats its first frame."""
    from fast_ray_tracer_amd.runtime import encode_ppm
    base = load_scene("cornell_direct_64_4x4")
    r = _renderer(base)
    try:
        first = r.render()
        for name in ("cornell_direct_128_1x1", "cornell_direct_240x135_8x8"):
            other = load_scene(name)
            r.set_camera(base.view_of(other))
            img = r.render()
            assert img.shape == (other.height, other.width, 4)
            diff = np.abs(img[:, :, :3] - load_golden_canvas(name))
            print(f"{name}: max|d|={diff.max():.3e}")
            assert diff.max() <= TOL
            assert hashlib.sha256(encode_ppm(img[:, :, :3])).hexdigest() == golden_index()[name]["ppm_sha256"]
            assert np.array_equal(img, _fresh(other))
        r.set_camera(base)
        assert np.array_equal(r.render(), first)
    finally:
        r.close()


def test_stochastic_cameras_through_set_camera(built):
    """Jitter and a lens aperture arrive with the camera: one handle on checkered_sphere_200 under the cameras of
    the jitter and depth-of-field goldens renders, at seed 7, what fresh uploads of those scenes render."""
    base = load_scene("checkered_sphere_200")
    r = _renderer(base)
    try:
        r.render()
        for name in ("checkered_sphere_jitter_100", "checkered_sphere_dof_100"):
            other = load_scene(name)
            r.set_camera(base.view_of(other))
            got = r.render(seed=7)
            want = _fresh(other, seed=7)
            assert np.array_equal(got, want), name
            assert not np.array_equal(got, r.render(seed=8)), name  # (the stochastic path is on)
    finally:
        r.close()


# three eyes per world: off the captured axis, inside the room / in free space, looking at the captured target
MOVED = {
    "cornell_direct_64_4x4": [((0.3, 0.2, -2.0), (0, 0, 0)), ((-0.4, 0.3, -1.6), (0.2, -0.2, 0.5)),
                              ((0.0, -0.3, -2.4), (0, 0.2, 0))],
    "csg_nested_96x64": [((3.0, 4.0, -9.0), (0.5, 1.0, 0.5)), ((-2.0, 6.0, -8.0), (0.5, 1.0, 0.5)),
                         ((0.5, 3.0, -12.0), (0.5, 1.0, 0.5))],
    "teapot_low_100": [((10.0, 5.0, -28.0), (0, 0, 0)), ((-8.0, 12.0, -25.0), (0, 0, 0)),
                       ((0.0, 8.0, -32.0), (0, 0, 0))],
    "reflect_refract_test_150": [((1.0, 0.5, -4.5), (0, 0, 0)), ((-1.2, 0.8, -4.0), (0, 0, 0)),
                                 ((0.3, 0.4, -5.5), (0, 0, 0))],
}


@pytest.mark.parametrize("name", sorted(MOVED))
def test_moved_cameras_match_the_oracle(built, name):
    """Three Scene.view viewpoints at 48 x 32 with the captured steps, on one handle, against the CPU oracle's
    render of the same view."""
    import oracle
    base = load_scene(name)
    r = _renderer(base)
    try:
        for from_, to in MOVED[name]:
            v = base.view(from_, to, hsize=48, vsize=32)
            r.set_camera(v)
            gpu = r.render()
            cpu = oracle.render(v)
            assert gpu.shape == cpu.shape == (32, 48, 4)
            diff = np.abs(gpu - cpu)
            print(f"{v.name}: max|d|={diff.max():.3e} mean={gpu[:, :, :3].mean():.4f}")
            assert gpu[:, :, :3].max() > 0
            assert diff.max() <= TOL, v.name
    finally:
        r.close()


def test_gi_keeps_its_photon_maps(built):
    """A GI scene's photon maps belong to the seed, not to the camera: after set_camera a frame at the same seed
    traces none (photon_pass == 0) and is bit for bit a fresh upload's frame of that view at that seed."""
    base = load_scene("cornell_gi_16")
    v = base.view((0.3, 0.2, -2.0), (0, 0, 0))
    r = _renderer(base)
    try:
        _, st = r.render(seed=5, stats=True)
        assert st.photon_pass == 1
        r.set_camera(v)
        img, st = r.render(seed=5, stats=True)
        assert st.photon_pass == 0 and st.photons[0] + st.photons[1] > 0
    finally:
        r.close()
    assert np.array_equal(img, _fresh(v, seed=5))


STRIP_WORLDS = ["cornell_direct_64_4x4", "csg_nested_96x64", "reflect_refract_test_150", "checkered_sphere_dof_100",
                "cornell_gi_16"]
STRIP_EYES = {"cornell_direct_64_4x4": MOVED["cornell_direct_64_4x4"], "csg_nested_96x64": MOVED["csg_nested_96x64"],
              "reflect_refract_test_150": MOVED["reflect_refract_test_150"],
              "checkered_sphere_dof_100": [((1.0, 0.5, -4.5), (0, 0, 0)), ((-1.2, 0.8, -4.0), (0, 0, 0)),
                                           ((0.3, 0.4, -5.5), (0, 0, 0))],
              "cornell_gi_16": MOVED["cornell_direct_64_4x4"]}


@pytest.mark.parametrize("name", STRIP_WORLDS)
def test_strip_equals_sequence(built, name):
    """render_views of K = 3 views equals, bit for bit, the three set_camera + render frames: 30 x 17 views of 3 x 3
    steps (4 590 samples each, no multiple of a wave, 9 samples per pixel), one view with another aperture size
    where the world's camera has an aperture; also in batches of 1000 samples (batch edges inside views and across
    them), over rows 1, 4, .., 13, and for K = 1; the handle's own camera renders unchanged afterwards."""
    from fast_ray_tracer_amd.runtime import host_lib
    base = load_scene(name)
    has_aperture = host_lib().frt_camera_aperture_size(base.camera) != 0.0
    views = [base.view(f, t, hsize=30, vsize=17, usteps=3, vsteps=3,
                       aperture_size=0.3 if has_aperture and k == 1 else None)
             for k, (f, t) in enumerate(STRIP_EYES[name])]
    seed = 7
    r = _renderer(base)
    try:
        own = r.render(seed=seed)
        for args in ({}, {"batch_samples": 1000}, {"row_begin": 1, "row_end": 16, "row_stride": 3}):
            seq = []
            for v in views:
                r.set_camera(v)
                seq.append(r.render(seed=seed, **args))
            r.set_camera(base)
            strip = r.render_views(views, seed=seed, **args)
            assert strip.shape == (3,) + seq[0].shape and strip.shape[2] == 30
            for k in range(3):
                assert np.array_equal(strip[k], seq[k]), (args, k)
            assert not np.array_equal(strip[0], strip[1]) and strip[:, :, :, :3].max() > 0
            if has_aperture:  # (the aperture size is the view's own)
                r.set_camera(base.view(*STRIP_EYES[name][1], hsize=30, vsize=17, usteps=3, vsteps=3))
                assert not np.array_equal(r.render(seed=seed, **args), strip[1])
                r.set_camera(base)
        one = r.render_views(views[2:], seed=seed)
        assert one.shape[0] == 1 and np.array_equal(one[0], seq_full(r, views[2], base, seed))
        assert r.frame is base and np.array_equal(r.render(seed=seed), own)
    finally:
        r.close()


def seq_full(r, view, base, seed):
    r.set_camera(view)
    try:
        return r.render(seed=seed)
    finally:
        r.set_camera(base)


def test_render_multi_reuses_kept_handles_under_another_camera(built, monkeypatch):
    """render_multi(scene) then render_multi(view) of the same world: the second call uploads nothing
    (phase "upload" 0.0) and returns the canvas a call without kept handles returns; another world uploads again.
    The C entry frt_render_views with two cameras returns what two render_multi calls return."""
    from fast_ray_tracer_amd.runtime import (host_lib, release_render_multi, render_multi, render_multi_phases)
    base = load_scene("cornell_direct_64_4x4")
    view = base.view((0.3, 0.2, -2.0), (0, 0, 0), hsize=48, vsize=32)
    other_world = load_scene("checkered_sphere_200")
    release_render_multi()
    monkeypatch.setenv("FRT_RM_KEEP", "0")
    want_base, want_view = np.array(render_multi(base, devices="0")), np.array(render_multi(view, devices="0"))
    assert render_multi_phases()["upload"] > 0.0
    monkeypatch.setenv("FRT_RM_KEEP", "1")
    try:
        a = np.array(render_multi(base, devices="0"))
        assert render_multi_phases()["upload"] > 0.0
        b = np.array(render_multi(view, devices="0"))
        assert render_multi_phases()["upload"] == 0.0
        assert b.shape == (32, 48, 4) and np.array_equal(a, want_base) and np.array_equal(b, want_view)
        c = np.array(render_multi(base.view_of(load_scene("cornell_direct_128_1x1")), devices="0"))  # (other steps)
        assert render_multi_phases()["upload"] == 0.0
        assert np.abs(c[:, :, :3] - load_golden_canvas("cornell_direct_128_1x1")).max() <= TOL
        render_multi(other_world, devices="0")
        assert render_multi_phases()["upload"] > 0.0

        # frt_render_views: two cameras of one size, one strip call
        lib = host_lib()
        vp = ctypes.c_void_p
        lib.frt_render_views.restype = ctypes.c_int
        lib.frt_render_views.argtypes = [ctypes.POINTER(vp), ctypes.c_size_t, vp, ctypes.c_size_t, ctypes.c_size_t,
                                         ctypes.c_bool, ctypes.POINTER(vp)]
        lib.frt_canvas_data.restype = ctypes.POINTER(ctypes.c_double)
        lib.frt_canvas_data.argtypes = [vp]
        lib.canvas_free.argtypes = [vp]
        lib.frt_render_multi_error.restype = ctypes.c_char_p
        view2 = base.view((-0.4, 0.3, -1.6), (0.2, -0.2, 0.5), hsize=48, vsize=32)
        cams, out = (vp * 2)(view.camera, view2.camera), (vp * 2)()
        monkeypatch.setenv("FRT_DEVICES", "0")
        rc = lib.frt_render_views(cams, 2, base.world, base.usteps, base.vsteps, base.jitter, out)
        got = [np.array(np.ctypeslib.as_array(lib.frt_canvas_data(out[k]), shape=(32, 48, 4))) for k in range(2)]
        for k in range(2):
            lib.canvas_free(out[k])
        assert rc == 0 and lib.frt_render_multi_error() == b""
        assert np.array_equal(got[0], want_view)
        assert np.array_equal(got[1], np.array(render_multi(view2, devices="0")))
        # a refusal: the reason, and zeroed canvases the caller still frees
        odd = base.view((0.3, 0.2, -2.0), (0, 0, 0), hsize=40, vsize=32)
        cams = (vp * 2)(view.camera, odd.camera)
        assert lib.frt_render_views(cams, 2, base.world, base.usteps, base.vsteps, base.jitter, out) == -1
        assert b"share one size" in lib.frt_render_multi_error()
        for k in range(2):
            assert not np.ctypeslib.as_array(lib.frt_canvas_data(out[k]), shape=(32, 48, 4)).any()
            lib.canvas_free(out[k])
    finally:
        release_render_multi()


def test_refusals_leave_the_handle_as_it_was(built):
    """set_camera with a zero size or step count, and render_views with views of different size or steps, fail
    with the reason; the handle's next frame is bit for bit the one before."""
    base = load_scene("cornell_direct_64_4x4")
    eye = ((0.3, 0.2, -2.0), (0, 0, 0))
    good = base.view(*eye, hsize=30, vsize=17)
    r = _renderer(base)
    try:
        r.set_camera(good)
        before = r.render()
        with pytest.raises(RuntimeError, match="hsize and vsize must be positive"):
            r.set_camera(base.view(*eye, hsize=0, vsize=17))
        assert r.frame is good and np.array_equal(r.render(), before)
        with pytest.raises(RuntimeError, match="usteps and vsteps must be positive"):
            r.set_camera(base.view(*eye, hsize=30, vsize=17, usteps=0))
        assert np.array_equal(r.render(), before)
        with pytest.raises(RuntimeError, match="share one size"):
            r.render_views([good, base.view(*eye, hsize=30, vsize=18)])
        assert np.array_equal(r.render(), before)
        with pytest.raises(RuntimeError, match="share their steps"):
            r.render_views([good, base.view(*eye, hsize=30, vsize=17, usteps=2, vsteps=2)])
        assert r.frame is good and np.array_equal(r.render(), before)
        with pytest.raises(ValueError, match="this renderer's world"):
            r.set_camera(load_scene("checkered_sphere_200"))
        assert np.array_equal(r.render(), before)
    finally:
        r.close()


def test_pinned_canvases_are_capped(built, monkeypatch):
    """At most FRT_PINNED_CANVASES page-locked canvases are out at once; one asked for beyond that is ordinary
    memory, and a freed one makes room again."""
    from fast_ray_tracer_amd.runtime import host_lib, release_render_multi
    lib = host_lib()
    vp = ctypes.c_void_p
    lib.frt_canvas_alloc_pinned.restype = vp
    lib.frt_canvas_alloc_pinned.argtypes = [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_bool, vp]
    lib.frt_canvas_is_pinned.restype = ctypes.c_int
    lib.frt_canvas_is_pinned.argtypes = [vp]
    lib.canvas_free.argtypes = [vp]
    gc.collect()
    release_render_multi()
    _renderer(load_scene("cornell_direct_64_4x4")).close()  # (a device context: page-locked memory can be had)
    monkeypatch.setenv("FRT_PINNED_CANVASES", "2")
    cs = [lib.frt_canvas_alloc_pinned(32, 16, False, None) for _ in range(3)]
    try:
        assert [lib.frt_canvas_is_pinned(c) for c in cs] == [1, 1, 0]
        lib.canvas_free(cs.pop(0))
        cs.append(lib.frt_canvas_alloc_pinned(32, 16, False, None))
        assert lib.frt_canvas_is_pinned(cs[-1]) == 1
    finally:
        for c in cs:
            lib.canvas_free(c)
        release_render_multi()
