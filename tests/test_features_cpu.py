"""Feature buffers, the half that needs no GPU: the ABI constant, the entry points' refusals, scene_nodes, and the
analytic sphere reference (tests/feature_ref.py) pinned against the CPU oracle."""
import ctypes

import numpy as np
import pytest

from conftest import load_scene

import feature_ref

EYE = ((0.0, 0.0, -5.0), (0.0, 0.0, 0.0))
STEPS = (1, 3, 4, 8, 17)


def _lib(built):
    from fast_ray_tracer_amd.runtime import host_lib
    lib = host_lib()
    lib.frt_last_error.restype = ctypes.c_char_p
    return lib


def test_geom_words(built):
    from fast_ray_tracer_amd.runtime import FEATURE_GEOM_WORDS
    lib = _lib(built)
    lib.frt_feature_geom_words.restype = ctypes.c_size_t
    assert lib.frt_feature_geom_words() == 8 == FEATURE_GEOM_WORDS


@pytest.mark.parametrize("fn,strip", [("frt_render_features_device", False), ("frt_render_features_host", False),
                                      ("frt_render_feature_views_device", True),
                                      ("frt_render_feature_views_host", True)])
def test_entry_points_refuse_null_arguments(built, fn, strip):
    """A null handle, and both buffers NULL, are refused with the reason before anything touches a device (the
    second with a pointer that is never dereferenced standing in for a handle)."""
    from fast_ray_tracer_amd.runtime import FeatureBuffers, FrameParams
    lib = _lib(built)
    f = getattr(lib, fn)
    params = FrameParams()
    geom = np.zeros(8, dtype=np.float64)
    some, none = FeatureBuffers(geom.ctypes.data, None), FeatureBuffers(None, None)
    cams = ctypes.create_string_buffer(240)
    lead = (cams, 1) if strip else ()
    assert f(None, *lead, ctypes.byref(params), ctypes.byref(some), None) == -1
    assert fn.encode() in lib.frt_last_error() and b"null argument" in lib.frt_last_error()
    fake = ctypes.c_void_p(ctypes.addressof(cams))
    assert f(fake, *lead, None, ctypes.byref(some), None) == -1
    assert b"null argument" in lib.frt_last_error()
    assert f(fake, *lead, ctypes.byref(params), ctypes.byref(none), None) == -1
    assert fn.encode() in lib.frt_last_error() and b"both feature buffers are NULL" in lib.frt_last_error()


def test_scene_nodes_of_the_sphere_world(built):
    from fast_ray_tracer_amd.runtime import scene_nodes
    n = scene_nodes(load_scene("checkered_sphere_200"))
    assert set(n) == {"type", "parent", "material"} and all(v.dtype == np.int32 for v in n.values())
    leaves = np.flatnonzero(n["type"] < 8)
    assert len(leaves) == 1 and n["type"][leaves[0]] == 5  # (one sphere)
    assert n["parent"][0] == -1 and n["material"][leaves[0]] == feature_ref.kd_pattern_colours(
        load_scene("checkered_sphere_200"))[0]


def test_reference_hit_mask_equals_the_oracle(built):
    """At 37 x 37, 1 x 1 the helper's hit mask is "the oracle's colour is non-zero": every hit of this scene has
    Ka > 0 and a miss is black. This pins the helper's rays against the pinned oracle."""
    import oracle
    base = load_scene("checkered_sphere_200")
    view = base.view(*EYE, hsize=37, vsize=37, usteps=1, vsteps=1)
    _, point, disc, hit = feature_ref.sphere_samples(view)
    img = oracle.render(view, threads=2)
    assert img.shape == (37, 37, 4)
    assert np.array_equal(hit[:, :, 0], (img[:, :, :3] != 0.0).any(axis=2))
    assert 0 < hit.sum() < hit.size
    assert np.abs(np.linalg.norm(point[hit], axis=-1) - 1.0).max() < 1e-12


def test_reference_discriminants_stay_clear_of_zero(built):
    """With the real sample tables no sample of the five step counts the GPU test uses is within 1e-7 of the
    sphere's silhouette (|discriminant| < 1e-7), so that test excludes nothing."""
    base = load_scene("checkered_sphere_200")
    for s in STEPS:
        _, _, disc, _ = feature_ref.sphere_samples(base.view(*EYE, hsize=37, vsize=37, usteps=s, vsteps=s))
        print("steps %d x %d: min |discriminant| = %.3e" % (s, s, np.abs(disc).min()))
        assert np.abs(disc).min() >= 1e-7
