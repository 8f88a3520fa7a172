"""Reference for the feature buffers on checkered_sphere_200's world: the camera rays rebuilt on the host and
intersected with the unit sphere analytically (numpy only, no GPU).

The rays follow ray_for_pixel in fast_ray_tracer_amd/csrc/frt_camera.hpp for a point aperture without jitter, from
the flattened frt_camera and sample table of the view (runtime._flat_scene). The world is one sphere with the
identity transform, so a sample's closest hit is the smaller root of |o + t d|^2 = 1, its hit point is its normal,
and the camera at (0, 0, -5) is outside it (the normal already faces the eye).
"""
import ctypes

import numpy as np


class FlatCamera(ctypes.Structure):  # frt_camera (include/frt_device.h)
    _fields_ = [("hsize", ctypes.c_int64), ("vsize", ctypes.c_int64), ("usteps", ctypes.c_int64),
                ("vsteps", ctypes.c_int64), ("half_width", ctypes.c_double), ("half_height", ctypes.c_double),
                ("pixel_size", ctypes.c_double), ("canvas_distance", ctypes.c_double), ("inv", ctypes.c_double * 16),
                ("aperture_size", ctypes.c_double), ("aperture_type", ctypes.c_int32), ("jitter", ctypes.c_int32),
                ("aperture_args", ctypes.c_double * 4)]


def flat_camera(view):
    """(FlatCamera, sample table (spp, 2)) of a Scene / View, as frt_flatten_scene gives them."""
    from fast_ray_tracer_amd.runtime import _flat_scene
    lib, fs = _flat_scene(view)
    try:
        for fn in ("frt_scene_camera_offset", "frt_scene_table_offset", "frt_camera_size"):
            getattr(lib, fn).restype = ctypes.c_size_t
        assert lib.frt_camera_size() == ctypes.sizeof(FlatCamera)
        cam = FlatCamera.from_buffer_copy(fs, lib.frt_scene_camera_offset())
        table = ctypes.c_void_p.from_buffer(fs, lib.frt_scene_table_offset()).value
        spp = view.usteps * view.vsteps
        tab = np.frombuffer(ctypes.string_at(table, 16 * spp), dtype=np.float64).reshape(spp, 2).copy()
    finally:
        lib.frt_flat_scene_free(fs)
    return cam, tab


def kd_pattern_colours(view):
    """The two flattened colours of the uv-check pattern behind map_Kd of checkered_sphere_200's one material:
    (material index, (2, 3) float64). Offsets are those of frt_scene / frt_material / frt_pattern."""
    from fast_ray_tracer_amd.runtime import _flat_scene
    lib, fs = _flat_scene(view)
    try:
        nmat, npat = ctypes.c_int32.from_buffer(fs, 64).value, ctypes.c_int32.from_buffer(fs, 68).value
        mats = ctypes.string_at(ctypes.c_void_p.from_buffer(fs, 72).value, 184 * nmat)
        pats = ctypes.string_at(ctypes.c_void_p.from_buffer(fs, 80).value, 320 * npat)
    finally:
        lib.frt_flat_scene_free(fs)
    found = []
    for m in range(nmat):
        map_kd = int(np.frombuffer(mats, dtype="<i4", count=1, offset=184 * m + 156)[0])
        if map_kd < 0:
            continue
        faces = int(np.frombuffer(pats, dtype="<i4", count=1, offset=320 * map_kd + 12)[0])
        body = faces if faces >= 0 else map_kd
        found.append((m, np.frombuffer(pats, dtype="<f8", count=6, offset=320 * body + 176).reshape(2, 3).copy()))
    assert len(found) == 1, found
    return found[0]


def camera_rays(view):
    """The camera rays of the view in binary64, in (row, col, sub) order with sub = v * usteps + u: origin and
    direction, each (rows, w, spp, 3)."""
    cam, tab = flat_camera(view)
    assert cam.aperture_size == 0.0 and cam.jitter == 0
    h, w, spp = int(cam.vsize), int(cam.hsize), tab.shape[0]
    inv = np.array(list(cam.inv), dtype=np.float64).reshape(4, 4)
    py, px = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    xoff = (px[:, :, None] + tab[None, None, :, 0]) * cam.pixel_size
    yoff = (py[:, :, None] + tab[None, None, :, 1]) * cam.pixel_size
    wx, wy, wz = cam.half_width - xoff, cam.half_height - yoff, -cam.canvas_distance

    def xf_point(x, y, z):
        return np.stack([((inv[i, 0] * x + inv[i, 1] * y) + inv[i, 2] * z) + inv[i, 3] for i in range(3)], axis=-1)

    pixel = xf_point(wx, wy, wz)
    origin = xf_point(0.0, 0.0, 0.0)  # (point aperture: (0.5 - 0.5) * aperture_size)
    v = pixel - origin
    d = v / np.sqrt((v * v).sum(axis=-1, keepdims=True))
    return np.broadcast_to(origin, d.shape), d


def sphere_samples(view):
    """Per camera sample of the view, in (row, col, sub) order with sub = v * usteps + u: t (rows, w, spp; NaN for
    a miss), the hit point = normal (rows, w, spp, 3), the discriminant (rows, w, spp) and the hit mask."""
    o, d = camera_rays(view)
    a = (d * d).sum(axis=-1)
    b = 2.0 * (o * d).sum(axis=-1)
    c = (o * o).sum(axis=-1) - 1.0
    disc = b * b - 4.0 * a * c
    hit = disc >= 0.0
    t = np.where(hit, (-b - np.sqrt(np.where(hit, disc, 0.0))) / (2.0 * a), np.nan)
    point = o + d * np.where(hit, t, 0.0)[..., None]
    return t, point, disc, hit


def ordered_mean(values, hit):
    """Per pixel the sum of values over the hitting samples in sub-sample order divided by the hit count (0 where
    no sample hits): values (rows, w, spp[, k]), hit (rows, w, spp)."""
    vals = values.reshape(values.shape[:3] + (-1,))
    acc = np.zeros(vals.shape[:2] + vals.shape[3:], dtype=np.float64)
    for s in range(vals.shape[2]):  # (sequential: the engine's order of additions)
        acc = np.where(hit[:, :, s, None], acc + np.where(hit[:, :, s, None], vals[:, :, s], 0.0), acc)
    cnt = hit.sum(axis=2)
    out = np.where(cnt[..., None] > 0, acc / np.maximum(cnt, 1)[..., None], 0.0)
    return out.reshape(values.shape[:2] + values.shape[3:])
