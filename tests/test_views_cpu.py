"""Views, the host half (no GPU): the camera block of the flatten on its own, frt_camera_look_at against a captured
camera, and render_multi's split of "the same scene" into "the same world" and "the same camera"."""
import ctypes
import re

import pytest

from conftest import GOLDEN, golden_index, load_scene


def _lib(built):
    from fast_ray_tracer_amd.runtime import host_lib
    lib = host_lib()
    for fn in ("frt_scene_camera_offset", "frt_scene_table_offset", "frt_camera_size"):
        getattr(lib, fn).restype = ctypes.c_size_t
    lib.frt_flatten_camera.restype = ctypes.c_int
    lib.frt_flatten_camera.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_bool,
                                       ctypes.c_void_p, ctypes.POINTER(ctypes.POINTER(ctypes.c_double))]
    lib.frt_scenes_compare.restype = ctypes.c_int
    lib.frt_scenes_compare.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.free.argtypes = [ctypes.c_void_p]
    return lib


def _scene_camera(lib, fs, spp):
    """(camera bytes, sample table bytes) of a flattened scene (runtime._flat_scene's buffer)."""
    off, size = lib.frt_scene_camera_offset(), lib.frt_camera_size()
    table = ctypes.c_void_p.from_buffer(fs, lib.frt_scene_table_offset()).value
    return fs.raw[off:off + size], ctypes.string_at(table, 16 * spp)


def _flat_camera(lib, view):
    """(camera bytes, sample table bytes) of frt_flatten_camera for a Scene / View."""
    cam = ctypes.create_string_buffer(lib.frt_camera_size())
    table = ctypes.POINTER(ctypes.c_double)()
    assert lib.frt_flatten_camera(view.camera, view.usteps, view.vsteps, view.jitter, cam, ctypes.byref(table)) == 0
    try:
        return cam.raw, ctypes.string_at(table, 16 * view.usteps * view.vsteps)
    finally:
        lib.free(table)


@pytest.mark.parametrize("name", sorted(golden_index()))
def test_flatten_camera_reproduces_flatten_scene(built, name):
    """frt_flatten_camera gives the camera bytes and the sample table frt_flatten_scene gives (which calls it),
    for every golden scene."""
    from fast_ray_tracer_amd.runtime import _flat_scene
    lib = _lib(built)
    sc = load_scene(name)
    hl, fs = _flat_scene(sc)
    try:
        want = _scene_camera(lib, fs, sc.usteps * sc.vsteps)
    finally:
        hl.frt_flat_scene_free(fs)
    got = _flat_camera(lib, sc)
    assert len(want[0]) == 240 and got[0] == want[0]
    assert got[1] == want[1]


def test_look_at_reproduces_the_captured_camera(built):
    """Scene.view (frt_camera_look_at) with the from / to / up, field of view, distance and size written in
    cornell_direct_64_4x4.c flattens to the bytes of the camera that main.c built."""
    lib = _lib(built)
    src = open(GOLDEN + "/scenes/cornell_direct_64_4x4.c").read()
    vec = {k: [float(x) for x in re.search(r"(?:Point|Vector) %s = \{([^}]*)\}" % k, src).group(1).split(",")[:3]]
           for k in ("from", "to", "up")}
    m = re.search(r"Camera cam = camera\((\d+), (\d+), ([0-9.]+)/\*field_of_view\*/, ([0-9.]+)/\*distance\*/", src)
    hsize, vsize, fov, dist = int(m.group(1)), int(m.group(2)), float(m.group(3)), float(m.group(4))
    sc = load_scene("cornell_direct_64_4x4")
    v = sc.view(vec["from"], vec["to"], vec["up"], hsize=hsize, vsize=vsize, fov=fov, distance=dist)
    assert (v.width, v.height, v.usteps, v.vsteps, v.jitter) == (64, 64, 4, 4, False)
    assert _flat_camera(lib, v) == _flat_camera(lib, sc)
    # the defaults are the captured camera's own scalars
    assert _flat_camera(lib, sc.view(vec["from"], vec["to"], vec["up"])) == _flat_camera(lib, sc)
    # and a moved eye is another camera of the same size
    moved = _flat_camera(lib, sc.view((0.5, 0.25, -2.0), vec["to"]))
    assert moved[0] != _flat_camera(lib, sc)[0] and moved[1] == _flat_camera(lib, sc)[1]


def test_world_and_camera_equality(built):
    """render_multi's reuse test in its two halves (frt_scenes_compare: bit 0 the same world, bit 1 the same
    camera): two cornell goldens that differ in their camera lines share a world, not a camera; another scene
    shares neither; a View of a scene flattens to that scene's world."""
    from fast_ray_tracer_amd.runtime import _flat_scene
    lib = _lib(built)
    a = load_scene("cornell_direct_64_4x4")
    flat = {}
    try:
        for key, s in (("a", a), ("a2", a), ("b", load_scene("cornell_direct_128_1x1")),
                       ("c", load_scene("checkered_sphere_200")), ("view", a.view((0.5, 0.25, -2.0), (0, 0, 0)))):
            flat[key] = _flat_scene(s)[1]
        assert lib.frt_scenes_compare(flat["a"], flat["a2"]) == 3
        assert lib.frt_scenes_compare(flat["a"], flat["b"]) == 1
        assert lib.frt_scenes_compare(flat["a"], flat["c"]) & 1 == 0
        assert lib.frt_scenes_compare(flat["a"], flat["view"]) == 1
        assert lib.frt_scenes_compare(flat["b"], flat["view"]) == 1
    finally:
        for fs in flat.values():
            lib.frt_flat_scene_free(fs)


def test_view_carries_the_scene_attributes(built):
    """A View has the attributes of a Scene that the renderers and the oracle read."""
    a, b = load_scene("checkered_sphere_200"), load_scene("checkered_sphere_dof_100")
    v = a.view_of(b)
    assert (v.camera, v.world) == (b.camera, a.world)
    assert (v.usteps, v.vsteps, v.jitter, v.width, v.height) == (b.usteps, b.vsteps, b.jitter, b.width, b.height)
    assert v.drand48_state == b.drand48_state and v.spp == b.spp and v.base is a
    w = a.view((0, 1, -4), (0, 0, 0), hsize=48, vsize=32, aperture_size=0.25)
    assert (w.width, w.height, w.usteps, w.vsteps, w.world) == (48, 32, a.usteps, a.vsteps, a.world)
    assert all(hasattr(w, k) for k in ("camera", "world", "usteps", "vsteps", "jitter", "width", "height",
                                       "drand48_state", "name"))
