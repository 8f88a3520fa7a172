"""ctypes bindings for the frt-mi355x host and device libraries.

A scene is a codegen main.c (``yaml_parser.py scene.yml > main.c``) compiled
unchanged in capture mode (``build.build_scene``): running its ``main`` builds
the scene through the drop-in C API and hands the Camera / World to
``frt_capture_render_multi`` instead of rendering. ``GpuRenderer`` then
flattens the captured scene once, uploads it to HBM and renders rows with the
HIP engine (``include/frt_device.h``). There is no CPU fallback: if
libfrt_device.so or a GPU is missing, construction raises.
"""
from __future__ import annotations

import ctypes
import numbers
import os
import weakref
import threading

import numpy as np

from . import build

_lock = threading.Lock()
_host = None


class FrameParams(ctypes.Structure):
    _fields_ = [("row_begin", ctypes.c_int64), ("row_end", ctypes.c_int64), ("row_stride", ctypes.c_int64),
                ("seed", ctypes.c_uint64), ("batch_samples", ctypes.c_int64),
                ("count_reference_rays", ctypes.c_int32), ("precision", ctypes.c_int32)]


# frt_frame_params.precision (include/frt_device.h enum frt_precision); None: the environment decides, else parity
PRECISION = {None: 0, "parity": 1, "fast32": 2}


class FrameStats(ctypes.Structure):
    _fields_ = [("primary_rays", ctypes.c_uint64), ("secondary_rays", ctypes.c_uint64),
                ("shadow_rays", ctypes.c_uint64), ("pruned_secondary", ctypes.c_uint64),
                ("hits", ctypes.c_uint64), ("errors", ctypes.c_uint64), ("render_ms", ctypes.c_double),
                ("kernel_ms", ctypes.c_double * 8), ("kernel_launches", ctypes.c_uint64 * 8),
                ("shadow_kernel_bytes", ctypes.c_double), ("gather_rays", ctypes.c_uint64),
                ("photons", ctypes.c_uint64 * 2), ("photon_ms", ctypes.c_double),
                ("shadow_jit", ctypes.c_int32), ("photon_pass", ctypes.c_int32),
                ("sub_ms", ctypes.c_double * 16), ("sub_launches", ctypes.c_uint64 * 16),
                ("shadow_rays_walked", ctypes.c_uint64), ("shadow_tile_pairs", ctypes.c_uint64),
                ("shadow_tile_mixed", ctypes.c_uint64), ("shadow_pairs", ctypes.c_uint64),
                ("shadow_pairs_mixed", ctypes.c_uint64), ("shadow_sub_pairs", ctypes.c_uint64),
                ("shadow_sub_mixed", ctypes.c_uint64), ("shadow_subtile_pairs", ctypes.c_uint64),
                ("shadow_subtile_mixed", ctypes.c_uint64), ("lit_nodes", ctypes.c_uint64),
                ("prepare_uniform_waves", ctypes.c_uint64)]

    def as_dict(self) -> dict:
        names = ["trace", "shadow", "shade", "combine", "resolve", "trace_primary", "prepare", "gi"]
        subs = ["frt_jit_beam", "frt_jit_shadow", "k_gather_est", "k_gather_hit", "frt_jit_tile", "frt_jit_sub",
                "frt_jit_subtile", "k_shade_lit", "k_lit_sort", "k_shade_lit32", "k_feature_resolve", "frt_jit_split"]
        return {
            "primary_rays": int(self.primary_rays), "secondary_rays": int(self.secondary_rays),
            "shadow_rays": int(self.shadow_rays), "pruned_secondary": int(self.pruned_secondary),
            "hits": int(self.hits), "errors": int(self.errors), "render_ms": float(self.render_ms),
            "shadow_kernel_bytes": float(self.shadow_kernel_bytes),
            "gather_rays": int(self.gather_rays), "photons": [int(self.photons[0]), int(self.photons[1])],
            "photon_ms": float(self.photon_ms), "shadow_jit": int(self.shadow_jit),
            "photon_pass": int(self.photon_pass),
            "kernel_ms": {names[i]: float(self.kernel_ms[i]) for i in range(8) if self.kernel_launches[i]},
            "kernel_launches": {names[i]: int(self.kernel_launches[i]) for i in range(8) if self.kernel_launches[i]},
            "sub_ms": {subs[i]: float(self.sub_ms[i]) for i in range(len(subs)) if self.sub_launches[i]},
            "sub_launches": {subs[i]: int(self.sub_launches[i]) for i in range(len(subs)) if self.sub_launches[i]},
            "shadow_rays_walked": int(self.shadow_rays_walked),
            "shadow_tile_pairs": int(self.shadow_tile_pairs), "shadow_tile_mixed": int(self.shadow_tile_mixed),
            "shadow_pairs": int(self.shadow_pairs), "shadow_pairs_mixed": int(self.shadow_pairs_mixed),
            "shadow_sub_pairs": int(self.shadow_sub_pairs), "shadow_sub_mixed": int(self.shadow_sub_mixed),
            "shadow_subtile_pairs": int(self.shadow_subtile_pairs),
            "shadow_subtile_mixed": int(self.shadow_subtile_mixed), "lit_nodes": int(self.lit_nodes),
            "prepare_uniform_waves": int(self.prepare_uniform_waves),
        }


class ShadowStageStats(ctypes.Structure):
    """frt_shadow_stage_stats (include/frt_device.h): the shadow pass's per-stage counters of a handle's last frame."""
    _fields_ = [(n, ctypes.c_uint64) for n in
                ("supertile", "tile_pairs", "tile_mixed", "sub_pairs", "sub_mixed", "split_pairs", "split_mixed",
                 "subtile_pairs", "subtile_mixed", "rays_walked", "split_launches")] + [("split_ms", ctypes.c_double)]

    def as_dict(self) -> dict:
        return {n: (float if t is ctypes.c_double else int)(getattr(self, n)) for n, t in self._fields_}


class FeatureBuffers(ctypes.Structure):
    """frt_feature_buffers (include/frt_device.h): either pointer may be null, not both."""
    _fields_ = [("geom", ctypes.c_void_p), ("ids", ctypes.c_void_p)]


FEATURE_GEOM_WORDS = 8  # doubles per pixel of FeatureBuffers.geom (frt_feature_geom_words)


def _feature_dict(geom: np.ndarray, ids: np.ndarray) -> dict:
    """The named planes of the two feature buffers (..., 8) float64 / (..., 2) int32, as views into them."""
    return {"depth": geom[..., 0], "normal": geom[..., 1:4], "albedo": geom[..., 4:7], "coverage": geom[..., 7],
            "node": ids[..., 0], "material": ids[..., 1]}


class EncodeStats(ctypes.Structure):
    """frt_encode_stats (include/frt_device.h)."""
    _fields_ = [("values", ctypes.c_uint64), ("undecided", ctypes.c_uint64), ("backend", ctypes.c_int32),
                ("decline", ctypes.c_int32), ("mode", ctypes.c_int32), ("device", ctypes.c_int32),
                ("rgb_max", ctypes.c_double * 3), ("srgb_max", ctypes.c_double * 3), ("upload_ms", ctypes.c_double),
                ("kernel_ms", ctypes.c_double), ("readback_ms", ctypes.c_double), ("patch_ms", ctypes.c_double),
                ("host_ms", ctypes.c_double)]

    def as_dict(self) -> dict:
        return {"values": int(self.values), "undecided": int(self.undecided),
                "backend": ENCODE_BACKENDS[self.backend], "decline": ENCODE_DECLINES[self.decline],
                "mode": ENCODE_MODES[self.mode], "device": int(self.device), "rgb_max": list(self.rgb_max),
                "srgb_max": list(self.srgb_max), "upload_ms": float(self.upload_ms),
                "kernel_ms": float(self.kernel_ms), "readback_ms": float(self.readback_ms),
                "patch_ms": float(self.patch_ms), "host_ms": float(self.host_ms)}


# enum frt_encode_mode / frt_encode_backend / frt_encode_decline (include/frt_device.h), by value
ENCODE_MODES = ("ppm_scaled", "ppm_clamped", "png")
ENCODE_BACKENDS = ("host", "device", "auto")
ENCODE_DECLINES = (None, "zero_max", "non_finite", "over_cap", "no_device", "too_large")


DENOISE_BACKENDS = ("host", "device", "auto")  # enum frt_denoise_backend, by value
DENOISE_MAX_ITERATIONS = 8


class DenoiseParams(ctypes.Structure):
    """frt_denoise_params (include/frt_device.h "Denoise"). DenoiseParams() holds the library's defaults
    (frt_denoise_defaults); keyword arguments replace single fields: DenoiseParams(iterations=3)."""
    _fields_ = [("iterations", ctypes.c_int32), ("normal_squarings", ctypes.c_int32), ("demodulate", ctypes.c_int32),
                ("match_material", ctypes.c_int32), ("sigma_color", ctypes.c_double), ("sigma_depth", ctypes.c_double),
                ("albedo_eps", ctypes.c_double)]

    def __init__(self, **fields):
        super().__init__()
        host_lib().frt_denoise_defaults(ctypes.byref(self))
        for k, v in fields.items():
            if k not in dict(self._fields_):
                raise TypeError("frt: DenoiseParams has no field %r" % (k,))
            setattr(self, k, v)

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class DenoiseStats(ctypes.Structure):
    """frt_denoise_stats (include/frt_device.h)."""
    _fields_ = [("pixels", ctypes.c_uint64), ("valid_pixels", ctypes.c_uint64), ("iterations", ctypes.c_int32),
                ("backend", ctypes.c_int32), ("device", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("upload_ms", ctypes.c_double), ("pack_ms", ctypes.c_double), ("atrous_ms", ctypes.c_double),
                ("atrous_iter_ms", ctypes.c_double * DENOISE_MAX_ITERATIONS), ("readback_ms", ctypes.c_double),
                ("host_ms", ctypes.c_double)]

    def as_dict(self) -> dict:
        return {"pixels": int(self.pixels), "valid_pixels": int(self.valid_pixels),
                "iterations": int(self.iterations), "backend": DENOISE_BACKENDS[self.backend],
                "device": int(self.device), "upload_ms": float(self.upload_ms), "pack_ms": float(self.pack_ms),
                "atrous_ms": float(self.atrous_ms),
                "atrous_iter_ms": [float(self.atrous_iter_ms[i]) for i in range(self.iterations)],
                "readback_ms": float(self.readback_ms), "host_ms": float(self.host_ms)}


class DenoiseVarParams(ctypes.Structure):
    """frt_denoise_var_params (include/frt_device.h "Variance-guided denoise"). DenoiseVarParams() holds the
    library's defaults (frt_denoise_var_defaults); keyword arguments replace single fields."""
    _fields_ = DenoiseParams._fields_ + [("var_eps", ctypes.c_double)]

    def __init__(self, **fields):
        super().__init__()
        host_lib().frt_denoise_var_defaults(ctypes.byref(self))
        for k, v in fields.items():
            if k not in dict(self._fields_):
                raise TypeError("frt: DenoiseVarParams has no field %r" % (k,))
            setattr(self, k, v)

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class DenoiseVarStats(DenoiseStats):
    """frt_denoise_var_stats (include/frt_device.h): frt_denoise_stats' fields, timed on the var kernels."""


class AccumStats(ctypes.Structure):
    """frt_accum_stats (include/frt_device.h "Accumulator")."""
    _fields_ = [("pixels", ctypes.c_uint64), ("frames", ctypes.c_uint64), ("skipped", ctypes.c_uint64),
                ("device", ctypes.c_int32), ("reserved", ctypes.c_int32), ("add_ms", ctypes.c_double),
                ("resolve_ms", ctypes.c_double)]

    def as_dict(self) -> dict:
        return {"pixels": int(self.pixels), "frames": int(self.frames), "skipped": int(self.skipped),
                "device": int(self.device), "add_ms": float(self.add_ms), "resolve_ms": float(self.resolve_ms)}


class FlatCamera(ctypes.Structure):
    """frt_camera (include/frt_device.h): a camera as the engine takes it (flat_camera(view))."""
    _fields_ = [("hsize", ctypes.c_int64), ("vsize", ctypes.c_int64), ("usteps", ctypes.c_int64),
                ("vsteps", ctypes.c_int64), ("half_width", ctypes.c_double), ("half_height", ctypes.c_double),
                ("pixel_size", ctypes.c_double), ("canvas_distance", ctypes.c_double), ("inv", ctypes.c_double * 16),
                ("aperture_size", ctypes.c_double), ("aperture_type", ctypes.c_int32), ("jitter", ctypes.c_int32),
                ("aperture_args", ctypes.c_double * 4)]


class ReprojectParams(ctypes.Structure):
    """frt_reproject_params (include/frt_device.h "Reprojection"). ReprojectParams() holds the library's defaults
    (frt_reproject_defaults); keyword arguments replace single fields: ReprojectParams(max_history=8)."""
    _fields_ = [("max_history", ctypes.c_int32), ("match_material", ctypes.c_int32), ("normal_cos", ctypes.c_double),
                ("sigma_depth", ctypes.c_double), ("min_weight", ctypes.c_double)]

    def __init__(self, **fields):
        super().__init__()
        host_lib().frt_reproject_defaults(ctypes.byref(self))
        for k, v in fields.items():
            if k not in dict(self._fields_):
                raise TypeError("frt: ReprojectParams has no field %r" % (k,))
            setattr(self, k, v)

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class ReprojectStats(ctypes.Structure):
    """frt_reproject_stats (include/frt_device.h "Reprojection")."""
    _fields_ = [("pixels", ctypes.c_uint64), ("reprojected", ctypes.c_uint64), ("missed", ctypes.c_uint64),
                ("no_history", ctypes.c_uint64), ("device", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("kernel_ms", ctypes.c_double), ("host_ms", ctypes.c_double)]

    def as_dict(self) -> dict:
        return {"pixels": int(self.pixels), "reprojected": int(self.reprojected), "missed": int(self.missed),
                "no_history": int(self.no_history), "device": int(self.device), "kernel_ms": float(self.kernel_ms),
                "host_ms": float(self.host_ms)}


class ReprojectGeometry(ctypes.Structure):
    """frt_reproject_geometry: what frt_reproject_setup derives from the two cameras (reproject_setup())."""
    _fields_ = [("o_cur", ctypes.c_double * 3), ("o_prev", ctypes.c_double * 3), ("prev_fwd", ctypes.c_double * 16)]


def host_lib(auto_build: bool = False) -> ctypes.CDLL:
    """Load libfrt_host.so (which pulls in libfrt_device.so) with global symbols."""
    global _host
    with _lock:
        if _host is not None:
            return _host
        if auto_build:
            build.build_host()
        if not os.path.exists(build.HOST_LIB) or not os.path.exists(build.DEVICE_LIB):
            raise RuntimeError("frt native libraries are not built: run __graft_entry__.build() "
                               "(expected %s and %s)" % (build.HOST_LIB, build.DEVICE_LIB))
        lib = ctypes.CDLL(build.HOST_LIB, mode=ctypes.RTLD_GLOBAL)
        vp = ctypes.c_void_p
        lib.frt_captured.restype = ctypes.c_int
        for fn in ("frt_captured_camera", "frt_captured_world"):
            getattr(lib, fn).restype = vp
        for fn in ("frt_captured_usteps", "frt_captured_vsteps"):
            getattr(lib, fn).restype = ctypes.c_size_t
        lib.frt_captured_jitter.restype = ctypes.c_int
        lib.frt_camera_hsize.restype = ctypes.c_size_t
        lib.frt_camera_hsize.argtypes = [vp]
        lib.frt_camera_vsize.restype = ctypes.c_size_t
        lib.frt_camera_vsize.argtypes = [vp]
        lib.frt_host_prepare.restype = vp
        lib.frt_host_prepare.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_bool, ctypes.c_int]
        lib.frt_host_last_error.restype = ctypes.c_char_p
        lib.frt_host_set_camera.restype = ctypes.c_int
        lib.frt_host_set_camera.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_bool]
        lib.frt_camera_look_at.restype = vp
        lib.frt_camera_look_at.argtypes = [ctypes.POINTER(ctypes.c_double)] * 3 + [
            ctypes.c_size_t, ctypes.c_size_t, ctypes.c_double, ctypes.c_double, vp]
        for fn in ("frt_camera_fov", "frt_camera_distance", "frt_camera_aperture_size"):
            getattr(lib, fn).restype = ctypes.c_double
            getattr(lib, fn).argtypes = [vp]
        lib.frt_camera_set_aperture_size.restype = None
        lib.frt_camera_set_aperture_size.argtypes = [vp, ctypes.c_double]
        lib.frt_camera_free.restype = None
        lib.frt_camera_free.argtypes = [vp]
        lib.frt_device_count.restype = ctypes.c_int
        lib.frt_last_error.restype = ctypes.c_char_p
        lib.frt_render_rows.restype = ctypes.c_int
        lib.frt_render_rows.argtypes = [vp, ctypes.POINTER(FrameParams), vp, ctypes.POINTER(FrameStats)]
        lib.frt_render_rows_device.restype = ctypes.c_int
        lib.frt_render_rows_device.argtypes = [vp, ctypes.POINTER(FrameParams), vp, ctypes.POINTER(FrameStats)]
        lib.frt_scene_release.argtypes = [vp]
        lib.frt_shadow_stages.restype = ctypes.c_size_t
        lib.frt_shadow_stages.argtypes = [vp, ctypes.POINTER(ShadowStageStats)]
        if lib.frt_shadow_stages(None, None) != ctypes.sizeof(ShadowStageStats):
            raise RuntimeError("frt: frt_shadow_stage_stats does not match runtime.py ShadowStageStats: rebuild")
        lib.frt_encode_ppm.restype = ctypes.c_size_t
        lib.frt_encode_ppm.argtypes = [vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, vp, ctypes.c_size_t]
        lib.frt_encode16.restype = ctypes.c_int
        lib.frt_encode16.argtypes = [vp, ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_int, vp, ctypes.POINTER(EncodeStats)]
        lib.frt_encode_last.restype = None
        lib.frt_encode_last.argtypes = [ctypes.POINTER(EncodeStats)]
        lib.frt_encode_stats_size.restype = ctypes.c_size_t
        if lib.frt_encode_stats_size() != ctypes.sizeof(EncodeStats):
            raise RuntimeError("frt: frt_encode_stats is %d bytes in %s, runtime.py EncodeStats %d: rebuild"
                               % (lib.frt_encode_stats_size(), build.HOST_LIB, ctypes.sizeof(EncodeStats)))
        lib.frt_srgb_max_full.restype = None
        lib.frt_srgb_max_full.argtypes = [vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(ctypes.c_double)]
        lib.frt_encode_selftest.restype = ctypes.c_int64
        lib.frt_encode_selftest.argtypes = [ctypes.c_int64, ctypes.c_uint64, ctypes.POINTER(ctypes.c_double),
                                            ctypes.c_int]
        lib.write_ppm_file.restype = ctypes.c_int
        lib.write_ppm_file.argtypes = [vp, ctypes.c_bool, ctypes.c_char_p]
        lib.write_png.restype = ctypes.c_int
        lib.write_png.argtypes = [vp, ctypes.c_char_p]
        lib.frt_frame_stats_size.restype = ctypes.c_size_t
        if lib.frt_frame_stats_size() != ctypes.sizeof(FrameStats):  # (a stale library against this mirror)
            raise RuntimeError("frt: frt_frame_stats is %d bytes in %s, runtime.py FrameStats %d: rebuild"
                               % (lib.frt_frame_stats_size(), build.DEVICE_LIB, ctypes.sizeof(FrameStats)))
        lib.frt_frame_params_size.restype = ctypes.c_size_t
        if lib.frt_frame_params_size() != ctypes.sizeof(FrameParams):
            raise RuntimeError("frt: frt_frame_params is %d bytes in %s, runtime.py FrameParams %d: rebuild"
                               % (lib.frt_frame_params_size(), build.DEVICE_LIB, ctypes.sizeof(FrameParams)))
        lib.frt_feature_geom_words.restype = ctypes.c_size_t
        if lib.frt_feature_geom_words() != FEATURE_GEOM_WORDS:
            raise RuntimeError("frt: frt_feature_buffers.geom has %d doubles per pixel in %s, runtime.py %d: rebuild"
                               % (lib.frt_feature_geom_words(), build.DEVICE_LIB, FEATURE_GEOM_WORDS))
        fb, fp, fs = ctypes.POINTER(FeatureBuffers), ctypes.POINTER(FrameParams), ctypes.POINTER(FrameStats)
        for fn in ("frt_render_features_device", "frt_render_features_host"):
            getattr(lib, fn).restype = ctypes.c_int
            getattr(lib, fn).argtypes = [vp, fp, fb, fs]
        for fn in ("frt_render_feature_views_device", "frt_render_feature_views_host"):
            getattr(lib, fn).restype = ctypes.c_int
            getattr(lib, fn).argtypes = [vp, vp, ctypes.c_int32, fp, fb, fs]
        for fn, mirror in (("frt_denoise_params_size", DenoiseParams), ("frt_denoise_stats_size", DenoiseStats)):
            getattr(lib, fn).restype = ctypes.c_size_t
            if getattr(lib, fn)() != ctypes.sizeof(mirror):
                raise RuntimeError("frt: %s() is %d bytes in %s, runtime.py %s %d: rebuild"
                                   % (fn, getattr(lib, fn)(), build.DEVICE_LIB, mirror.__name__,
                                      ctypes.sizeof(mirror)))
        dp, ds, i64 = ctypes.POINTER(DenoiseParams), ctypes.POINTER(DenoiseStats), ctypes.c_int64
        lib.frt_denoise_defaults.restype = None
        lib.frt_denoise_defaults.argtypes = [dp]
        lib.frt_denoise_host.restype = ctypes.c_int
        lib.frt_denoise_host.argtypes = [vp, vp, vp, i64, i64, i64, dp, vp, ds]
        lib.frt_denoise_device.restype = ctypes.c_int
        lib.frt_denoise_device.argtypes = [vp, vp, vp, ctypes.c_int, i64, i64, i64, dp, ctypes.c_int, vp, ds]
        lib.frt_denoise.restype = ctypes.c_int
        lib.frt_denoise.argtypes = [vp, vp, vp, ctypes.c_int, i64, i64, i64, dp, ctypes.c_int, ctypes.c_int, vp, ds]
        lib.frt_denoise_error.restype = ctypes.c_char_p
        lib.frt_denoise_release.restype = None
        for fn, mirror in (("frt_denoise_var_params_size", DenoiseVarParams), ("frt_accum_stats_size", AccumStats)):
            getattr(lib, fn).restype = ctypes.c_size_t
            if getattr(lib, fn)() != ctypes.sizeof(mirror):
                raise RuntimeError("frt: %s() is %d bytes in %s, runtime.py %s %d: rebuild"
                                   % (fn, getattr(lib, fn)(), build.DEVICE_LIB, mirror.__name__,
                                      ctypes.sizeof(mirror)))
        vdp, vds = ctypes.POINTER(DenoiseVarParams), ctypes.POINTER(DenoiseVarStats)
        lib.frt_denoise_var_defaults.restype = None
        lib.frt_denoise_var_defaults.argtypes = [vdp]
        lib.frt_denoise_var_host.restype = ctypes.c_int
        lib.frt_denoise_var_host.argtypes = [vp, vp, vp, vp, i64, i64, i64, vdp, vp, vp, vds]
        lib.frt_denoise_var_device.restype = ctypes.c_int
        lib.frt_denoise_var_device.argtypes = [vp, vp, vp, vp, ctypes.c_int, i64, i64, i64, vdp, ctypes.c_int, vp, vp,
                                               vds]
        lib.frt_denoise_var.restype = ctypes.c_int
        lib.frt_denoise_var.argtypes = [vp, vp, vp, vp, ctypes.c_int, i64, i64, i64, vdp, ctypes.c_int, ctypes.c_int,
                                        vp, vp, vds]
        lib.frt_denoise_var_release.restype = None
        lib.frt_accum_create.restype = ctypes.c_int
        lib.frt_accum_create.argtypes = [ctypes.c_int, i64, ctypes.POINTER(vp)]
        lib.frt_accum_reset.restype = ctypes.c_int
        lib.frt_accum_reset.argtypes = [vp]
        lib.frt_accum_add.restype = ctypes.c_int
        lib.frt_accum_add.argtypes = [vp, vp, ctypes.c_int]
        lib.frt_accum_resolve.restype = ctypes.c_int
        lib.frt_accum_resolve.argtypes = [vp, vp, vp, ctypes.c_int, ctypes.POINTER(AccumStats)]
        lib.frt_accum_release.restype = None
        lib.frt_accum_release.argtypes = [vp]
        lib.frt_accum_device_part.restype = vp
        lib.frt_accum_device_part.argtypes = [vp]
        lib.frt_accum_error.restype = ctypes.c_char_p
        lib.frt_render_rows_accumulate.restype = ctypes.c_int
        lib.frt_render_rows_accumulate.argtypes = [vp, fp, ctypes.c_int32, vp, fs]
        lib.frt_camera_size.restype = ctypes.c_size_t
        if lib.frt_camera_size() != ctypes.sizeof(FlatCamera):
            raise RuntimeError("frt: frt_camera is %d bytes in %s, runtime.py FlatCamera %d: rebuild"
                               % (lib.frt_camera_size(), build.HOST_LIB, ctypes.sizeof(FlatCamera)))
        for fn, mirror in (("frt_reproject_params_size", ReprojectParams), ("frt_reproject_stats_size", ReprojectStats)):
            getattr(lib, fn).restype = ctypes.c_size_t
            if getattr(lib, fn)() != ctypes.sizeof(mirror):
                raise RuntimeError("frt: %s() is %d bytes in %s, runtime.py %s %d: rebuild"
                                   % (fn, getattr(lib, fn)(), build.HOST_LIB, mirror.__name__, ctypes.sizeof(mirror)))
        rpp, rps, fcp = ctypes.POINTER(ReprojectParams), ctypes.POINTER(ReprojectStats), ctypes.POINTER(FlatCamera)
        lib.frt_reproject_defaults.restype = None
        lib.frt_reproject_defaults.argtypes = [rpp]
        lib.frt_reproject_setup.restype = ctypes.c_int
        lib.frt_reproject_setup.argtypes = [fcp, fcp, ctypes.POINTER(ReprojectGeometry)]
        lib.frt_accum_reproject.restype = ctypes.c_int
        lib.frt_accum_reproject.argtypes = [vp, vp, fcp, fcp, fb, fb, i64, i64, rpp, ctypes.c_int, rps]
        lib.frt_accum_reproject_cameras.restype = ctypes.c_int
        lib.frt_accum_reproject_cameras.argtypes = [vp, vp, vp, vp, fb, fb, i64, i64, rpp, ctypes.c_int, rps]
        lib.frt_accum_host_state.restype = ctypes.c_int
        lib.frt_accum_host_state.argtypes = [vp, ctypes.POINTER(i64)] + [ctypes.POINTER(vp)] * 5
        _host = lib
        return lib


class Scene:
    """A scene built by running a capture-mode generated main.c."""

    def __init__(self, scene_so: str, asset_root: str | None = None):
        lib = host_lib()
        self._so = ctypes.CDLL(scene_so, mode=ctypes.RTLD_GLOBAL)
        self._so.frt_scene_main.restype = ctypes.c_int
        cwd = os.getcwd()
        lib.frt_reset_libc_rng()
        try:
            if asset_root:
                os.chdir(asset_root)
            rc = self._so.frt_scene_main()
        finally:
            os.chdir(cwd)
        if rc != 0 or not lib.frt_captured():
            raise RuntimeError("scene main() did not reach render_multi (rc=%d): %s" % (rc, scene_so))
        self.camera = lib.frt_captured_camera()
        self.world = lib.frt_captured_world()
        self.usteps = int(lib.frt_captured_usteps())
        self.vsteps = int(lib.frt_captured_vsteps())
        self.jitter = bool(lib.frt_captured_jitter())
        st = (ctypes.c_ushort * 3)()
        lib.frt_captured_drand48(st)
        self.drand48_state = tuple(st)  # glibc drand48 state at the render_multi call (stochastic checks)
        self.width = int(lib.frt_camera_hsize(self.camera))
        self.height = int(lib.frt_camera_vsize(self.camera))
        self.name = os.path.splitext(os.path.basename(scene_so))[0]

    @property
    def spp(self) -> int:
        return self.usteps * self.vsteps

    def view(self, from_, to, up=(0.0, 1.0, 0.0), hsize: int | None = None, vsize: int | None = None,
             fov: float | None = None, distance: float | None = None, aperture_size: float | None = None,
             usteps: int | None = None, vsteps: int | None = None, name: str | None = None) -> "View":
        """This scene's world seen from `from_` towards `to`: a camera built by the host library as a generated
        main() builds its own (frt_camera_look_at: view_transform, then camera()), with this scene's aperture,
        steps and jitter; size, field of view, canvas distance, aperture size and the render call's steps default to
        the captured ones."""
        lib = host_lib()
        v3 = ctypes.c_double * 3
        cam = lib.frt_camera_look_at(v3(*from_), v3(*to), v3(*up),
                                     self.width if hsize is None else hsize, self.height if vsize is None else vsize,
                                     lib.frt_camera_fov(self.camera) if fov is None else fov,
                                     lib.frt_camera_distance(self.camera) if distance is None else distance,
                                     self.camera)
        if not cam:
            raise RuntimeError("frt: frt_camera_look_at failed")
        if aperture_size is not None:
            lib.frt_camera_set_aperture_size(cam, aperture_size)
        v = View(self, cam, self.usteps if usteps is None else usteps, self.vsteps if vsteps is None else vsteps,
                 self.jitter, self.drand48_state,
                 name or "%s@%s" % (self.name, ",".join("%g" % x for x in from_)))
        weakref.finalize(v, lib.frt_camera_free, cam)
        return v

    def view_of(self, other: "Scene") -> "View":
        """This scene's world under another capture's camera, steps, jitter and drand48 state (a golden that
        differs from this one only in its camera(...) / aperture(...) lines)."""
        return View(self, other.camera, other.usteps, other.vsteps, other.jitter, other.drand48_state,
                    "%s@%s" % (self.name, other.name), keep=other)


class View:
    """A camera over a captured Scene's world. It carries the attributes a Scene has (camera, world, usteps, vsteps,
    jitter, width, height, drand48_state, name), so whatever renders a Scene renders a View: render_multi(view),
    the oracle, GpuRenderer.set_camera(view) / render_views([...])."""

    def __init__(self, base: Scene, camera, usteps: int, vsteps: int, jitter: bool, drand48_state, name: str,
                 keep=None):
        lib = host_lib()
        self.base = base.base if isinstance(base, View) else base  # (keeps the world, and the aperture's tables, alive)
        self._keep = keep
        self.camera = camera
        self.world = base.world
        self.usteps = int(usteps)
        self.vsteps = int(vsteps)
        self.jitter = bool(jitter)
        self.drand48_state = tuple(drand48_state)
        self.width = int(lib.frt_camera_hsize(camera))
        self.height = int(lib.frt_camera_vsize(camera))
        self.name = name

    @property
    def spp(self) -> int:
        return self.usteps * self.vsteps


class GpuRenderer:
    """render_multi's device path for one captured scene on one HIP device."""

    def __init__(self, scene: Scene, device: int = 0):
        self.lib = host_lib()
        if self.lib.frt_device_count() <= 0:
            raise RuntimeError("frt: no HIP device visible; the GPU path has no CPU fallback")
        # the handles an earlier render_multi kept hold their device memory until released (GBs for a GI scene)
        release_render_multi()
        self.scene = scene
        self.frame = scene  # (whose camera the handle holds: the scene, or set_camera's view)
        self.device = device
        h = self.lib.frt_host_prepare(scene.camera, scene.world, scene.usteps, scene.vsteps, scene.jitter, device)
        if not h:
            raise RuntimeError("frt: scene upload failed: " + self.lib.frt_host_last_error().decode())
        self.handle = h

    def set_camera(self, view) -> None:
        """Move the resident scene's camera to `view` (a View of this scene's world, or the Scene itself to go
        back): frt_host_set_camera. Only the camera (and, for other steps, the sample table) goes to the device;
        the world, its kernels, the level state and a GI scene's photon maps stay. Later render / render_into /
        render_encoded calls produce view.height x view.width frames. On a refusal it raises, and the renderer
        keeps the camera it had."""
        if view.world != self.scene.world:
            raise ValueError("frt: set_camera needs a view of this renderer's world (Scene.view / Scene.view_of)")
        if self.lib.frt_host_set_camera(self.handle, view.camera, view.usteps, view.vsteps, view.jitter) != 0:
            raise RuntimeError("frt: set_camera failed: " + self.lib.frt_host_last_error().decode())
        self.frame = view

    def _strip_cams(self, who: str, views, allow_empty: bool = False):
        """The views of a strip as a list and as the flattened frt_camera table the engine takes."""
        views = list(views)
        if not views and not allow_empty:
            raise ValueError("frt: %s needs at least one view" % who)
        if any(v.world != self.scene.world for v in views):
            raise ValueError("frt: %s needs views of this renderer's world (Scene.view / Scene.view_of)" % who)
        lib = self.lib
        lib.frt_camera_size.restype = ctypes.c_size_t
        lib.frt_flatten_camera.restype = ctypes.c_int
        lib.frt_flatten_camera.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_bool,
                                           ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]
        size = lib.frt_camera_size()
        cams = ctypes.create_string_buffer(size * max(1, len(views)))
        for k, v in enumerate(views):
            table = ctypes.c_void_p()
            rc = lib.frt_flatten_camera(v.camera, v.usteps, v.vsteps, v.jitter, ctypes.addressof(cams) + k * size,
                                        ctypes.byref(table))
            lib.frt_camera_free(table)  # (free(): the strip uses the handle's table)
            if rc:
                raise RuntimeError("frt: out of host memory for a view's sample table")
        return views, cams

    def render_views(self, views, row_begin: int = 0, row_end: int | None = None, row_stride: int = 1,
                     seed: int = 0x5EED, batch_samples: int = 0, stats: bool = False, precision: str | None = None):
        """Render K views of this renderer's world in one frame, a strip (frt_render_views_host): an array
        (K, rows, width, 4) float64 in ordinary pageable memory, view k bit for bit what set_camera(views[k])
        followed by render(...) with the same arguments gives. The views share their size, steps and jitter; the row
        range and stride apply inside each view. The levels' launches and count read-backs are paid once for the
        strip, not once per view. The renderer's own camera is unchanged afterwards."""
        views, cams = self._strip_cams("render_views", views)
        lib = self.lib
        lib.frt_render_views_host.restype = ctypes.c_int
        lib.frt_render_views_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
                                              ctypes.POINTER(FrameParams), ctypes.c_void_p, ctypes.POINTER(FrameStats)]
        first, own = views[0], self.frame
        # the handle's sample table is the strip's: a strip of other steps borrows the handle for its first view
        borrow = (first.usteps, first.vsteps) != (own.usteps, own.vsteps)
        if borrow:
            self.set_camera(first)
        try:
            p = self._params(row_begin, first.height if row_end is None else row_end, row_stride, seed, batch_samples,
                             precision)
            n = self.rows_in(p.row_begin, p.row_end, row_stride)
            out = np.zeros((len(views), n, first.width, 4), dtype=np.float64)
            st = FrameStats()
            rc = lib.frt_render_views_host(self.handle, cams, len(views), ctypes.byref(p),
                                           out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(st) if stats else None)
            err = lib.frt_last_error().decode() if rc != 0 else ""
        finally:
            if borrow:
                self.set_camera(own)
        if rc != 0:
            raise RuntimeError("frt render_views failed: " + err)
        return (out, st) if stats else out

    def shadow_stages(self) -> dict:
        """The shadow pass's per-stage counters of this renderer's last frame (frt_shadow_stages): the beams each
        stage tested and left mixed, the rays walked one by one, the super-tile size in use (0: none), and the
        split stage's launches and HIP-event time where the frame was rendered with stats=True."""
        st = ShadowStageStats()
        self.lib.frt_shadow_stages(self.handle, ctypes.byref(st))
        return st.as_dict()

    def close(self) -> None:
        if getattr(self, "handle", None):
            self.lib.frt_scene_release(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _params(self, row_begin, row_end, row_stride, seed, batch_samples, precision=None):
        p = FrameParams()
        # (a name from PRECISION; an integer goes to the engine as it is, which refuses the ones it does not know)
        if not isinstance(precision, int) and precision not in PRECISION:
            raise ValueError("frt: precision %r is not supported (\"parity\", \"fast32\" or None)" % (precision,))
        p.precision = precision if isinstance(precision, int) else PRECISION[precision]
        p.row_begin = row_begin
        p.row_end = self.frame.height if row_end is None else row_end
        p.row_stride = row_stride
        p.seed = seed
        p.batch_samples = batch_samples
        return p

    @staticmethod
    def rows_in(row_begin, row_end, row_stride) -> int:
        return len(range(row_begin, row_end, row_stride))

    def render(self, row_begin: int = 0, row_end: int | None = None, row_stride: int = 1, seed: int = 0x5EED,
               batch_samples: int = 0, stats: bool = False, precision: str | None = None):
        """Render rows into a host array (rows, width, 4) float64. precision: "parity" (binary64 throughout, the
        default), "fast32" (the light-point loop in binary32) or None (FRT_PRECISION decides, else parity)."""
        p = self._params(row_begin, row_end, row_stride, seed, batch_samples, precision)
        n = self.rows_in(p.row_begin, p.row_end, row_stride)
        out = np.zeros((n, self.frame.width, 4), dtype=np.float64)
        st = FrameStats()
        rc = self.lib.frt_render_rows(self.handle, ctypes.byref(p), out.ctypes.data_as(ctypes.c_void_p),
                                      ctypes.byref(st) if stats else None)
        if rc != 0:
            raise RuntimeError("frt render failed: " + self.lib.frt_last_error().decode())
        return (out, st) if stats else out

    def render_into(self, device_ptr: int, row_begin: int = 0, row_end: int | None = None, row_stride: int = 1,
                    seed: int = 0x5EED, batch_samples: int = 0, stats: bool = False, precision: str | None = None):
        """Render rows into device memory (e.g. a torch.cuda tensor's data_ptr()); precision as in render."""
        p = self._params(row_begin, row_end, row_stride, seed, batch_samples, precision)
        st = FrameStats()
        rc = self.lib.frt_render_rows_device(self.handle, ctypes.byref(p), ctypes.c_void_p(device_ptr),
                                             ctypes.byref(st) if stats else None)
        if rc != 0:
            raise RuntimeError("frt render failed: " + self.lib.frt_last_error().decode())
        return st if stats else None

    def render_features(self, row_begin: int = 0, row_end: int | None = None, row_stride: int = 1,
                        seed: int = 0x5EED, batch_samples: int = 0, stats: bool = False):
        """First-hit feature buffers of the rows a render(...) call with the same arguments shades
        (frt_render_features_host): level 0 only, no shadow, shading or GI work. A dict of numpy arrays: depth
        (rows, w), normal (rows, w, 3), albedo (rows, w, 3), coverage (rows, w), all float64 and views into one
        (rows, w, 8) buffer ("geom"), and node, material (rows, w) int32, views into one (rows, w, 2) buffer
        ("ids"). Each value is the mean over the pixel's hitting samples in sub-sample order (coverage: hits / spp;
        node / material: the first hitting sample's; -1 and zeros where nothing is hit): include/frt_device.h
        frt_feature_buffers. scene_nodes() maps a node id back to the flattened tree."""
        p = self._params(row_begin, row_end, row_stride, seed, batch_samples)
        n = self.rows_in(p.row_begin, p.row_end, row_stride)
        geom = np.zeros((n, self.frame.width, FEATURE_GEOM_WORDS), dtype=np.float64)
        ids = np.zeros((n, self.frame.width, 2), dtype=np.int32)
        bufs = FeatureBuffers(geom.ctypes.data, ids.ctypes.data)
        st = FrameStats()
        rc = self.lib.frt_render_features_host(self.handle, ctypes.byref(p), ctypes.byref(bufs),
                                               ctypes.byref(st) if stats else None)
        if rc != 0:
            raise RuntimeError("frt render_features failed: " + self.lib.frt_last_error().decode())
        out = _feature_dict(geom, ids)
        return (out, st) if stats else out

    def render_features_into(self, geom_ptr: int | None, ids_ptr: int | None, row_begin: int = 0,
                             row_end: int | None = None, row_stride: int = 1, seed: int = 0x5EED,
                             batch_samples: int = 0, stats: bool = False):
        """render_features into device memory (frt_render_features_device): geom_ptr rows x w x 8 float64, ids_ptr
        rows x w x 2 int32 (e.g. torch.cuda tensors' data_ptr()); either may be None, not both."""
        p = self._params(row_begin, row_end, row_stride, seed, batch_samples)
        bufs = FeatureBuffers(geom_ptr or None, ids_ptr or None)
        st = FrameStats()
        rc = self.lib.frt_render_features_device(self.handle, ctypes.byref(p), ctypes.byref(bufs),
                                                 ctypes.byref(st) if stats else None)
        if rc != 0:
            raise RuntimeError("frt render_features failed: " + self.lib.frt_last_error().decode())
        return st if stats else None

    def render_feature_views(self, views, row_begin: int = 0, row_end: int | None = None, row_stride: int = 1,
                             seed: int = 0x5EED, batch_samples: int = 0, stats: bool = False):
        """render_features of K views of this renderer's world in one pass, a strip (frt_render_feature_views_host):
        render_features' dict with a leading K axis, view k bit for bit what set_camera(views[k]) followed by
        render_features(...) with the same arguments gives. The views share their size, steps and jitter, as
        render_views' do; the renderer's own camera is unchanged afterwards."""
        views, cams = self._strip_cams("render_feature_views", views, allow_empty=True)  # (none: the engine refuses)
        first, own = views[0] if views else self.frame, self.frame
        # the handle's sample table is the strip's: a strip of other steps borrows the handle for its first view
        borrow = (first.usteps, first.vsteps) != (own.usteps, own.vsteps)
        if borrow:
            self.set_camera(first)
        try:
            p = self._params(row_begin, first.height if row_end is None else row_end, row_stride, seed, batch_samples)
            n = self.rows_in(p.row_begin, p.row_end, row_stride)
            geom = np.zeros((len(views), n, first.width, FEATURE_GEOM_WORDS), dtype=np.float64)
            ids = np.zeros((len(views), n, first.width, 2), dtype=np.int32)
            bufs = FeatureBuffers(geom.ctypes.data, ids.ctypes.data)
            st = FrameStats()
            rc = self.lib.frt_render_feature_views_host(self.handle, cams, len(views), ctypes.byref(p),
                                                        ctypes.byref(bufs), ctypes.byref(st) if stats else None)
            err = self.lib.frt_last_error().decode() if rc != 0 else ""
        finally:
            if borrow:
                self.set_camera(own)
        if rc != 0:
            raise RuntimeError("frt render_feature_views failed: " + err)
        out = _feature_dict(geom, ids)
        return (out, st) if stats else out

    def render_encoded(self, mode: str = "ppm_scaled", **render_args):
        """Render the whole frame into device memory (a torch tensor, frt_render_rows_device) and encode it there
        (frt_encode16 from device memory: the canvas never crosses to the host). Returns ((h, w, 3) uint16, encode
        stats dict); render_args as render_into's (seed, batch_samples, precision)."""
        import torch
        with torch.cuda.device(self.device):
            frame = torch.empty((self.frame.height, self.frame.width, 4), dtype=torch.float64, device="cuda")
        self.render_into(frame.data_ptr(), **render_args)
        return _encode16(frame.data_ptr(), True, self.frame.width, self.frame.height, mode, "device", self.device)

    def render_denoised(self, params=None, **render_args):
        """Render the whole frame and its feature buffers into device memory (torch tensors: render_into,
        render_features_into) and denoise the frame there (frt_denoise on device buffers, in place): nothing crosses
        to the host in between. Returns ((h, w, 4) float64 array, denoise stats dict): bit for bit
        denoise(render(...), render_features(...)) with the same arguments. render_args as render_into's (seed,
        batch_samples, precision; the feature pass takes seed and batch_samples)."""
        import torch
        h, w = self.frame.height, self.frame.width
        with torch.cuda.device(self.device):
            frame = torch.empty((h, w, 4), dtype=torch.float64, device="cuda")
            geom = torch.empty((h, w, FEATURE_GEOM_WORDS), dtype=torch.float64, device="cuda")
            ids = torch.empty((h, w, 2), dtype=torch.int32, device="cuda")
        self.render_into(frame.data_ptr(), **render_args)
        self.render_features_into(geom.data_ptr(), ids.data_ptr(),
                                  **{k: v for k, v in render_args.items() if k in ("seed", "batch_samples")})
        st = _denoise(frame.data_ptr(), geom.data_ptr(), ids.data_ptr(), True, w, h, 1, params, "device", self.device,
                      frame.data_ptr())
        return frame.cpu().numpy(), st.as_dict()

    def render_denoised_views(self, views, params=None, **render_args):
        """render_denoised of K views of this renderer's world as one strip: render_views' and
        render_feature_views' passes into device memory, then one denoise call over the K images (a tap never
        leaves its own view). Returns ((K, h, w, 4) float64 array, denoise stats dict); view k is bit for bit
        set_camera(views[k]) + render_denoised(...)."""
        import torch
        unknown = set(render_args) - {"seed", "batch_samples", "precision"}
        if unknown:
            raise TypeError("frt: render_denoised_views takes seed, batch_samples and precision, not %s"
                            % sorted(unknown))
        views, cams = self._strip_cams("render_denoised_views", views)
        lib, first, own = self.lib, views[0], self.frame
        fb, fp, fs = ctypes.POINTER(FeatureBuffers), ctypes.POINTER(FrameParams), ctypes.POINTER(FrameStats)
        lib.frt_render_views_device.restype = ctypes.c_int
        lib.frt_render_views_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, fp, ctypes.c_void_p,
                                                fs]
        lib.frt_render_feature_views_device.restype = ctypes.c_int
        lib.frt_render_feature_views_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, fp, fb, fs]
        k, h, w = len(views), first.height, first.width
        with torch.cuda.device(self.device):
            frame = torch.empty((k, h, w, 4), dtype=torch.float64, device="cuda")
            geom = torch.empty((k, h, w, FEATURE_GEOM_WORDS), dtype=torch.float64, device="cuda")
            ids = torch.empty((k, h, w, 2), dtype=torch.int32, device="cuda")
        # the handle's sample table is the strip's: a strip of other steps borrows the handle for its first view
        borrow = (first.usteps, first.vsteps) != (own.usteps, own.vsteps)
        if borrow:
            self.set_camera(first)
        try:
            p = self._params(0, h, 1, render_args.get("seed", 0x5EED), render_args.get("batch_samples", 0),
                             render_args.get("precision"))
            rc = lib.frt_render_views_device(self.handle, cams, k, ctypes.byref(p), ctypes.c_void_p(frame.data_ptr()),
                                             None)
            if rc == 0:
                bufs = FeatureBuffers(geom.data_ptr(), ids.data_ptr())
                p.precision = 0
                rc = lib.frt_render_feature_views_device(self.handle, cams, k, ctypes.byref(p), ctypes.byref(bufs),
                                                         None)
            err = lib.frt_last_error().decode() if rc != 0 else ""
        finally:
            if borrow:
                self.set_camera(own)
        if rc != 0:
            raise RuntimeError("frt render_denoised_views failed: " + err)
        st = _denoise(frame.data_ptr(), geom.data_ptr(), ids.data_ptr(), True, w, h, k, params, "device", self.device,
                      frame.data_ptr())
        return frame.cpu().numpy(), st.as_dict()

    def _accumulate(self, acc: "Accumulator", frames: int, seed, batch_samples, precision, stats: bool):
        if frames < 1:
            raise ValueError("frt: render_accumulated needs frames >= 1, not %r" % (frames,))
        p = self._params(0, None, 1, seed, batch_samples, precision)
        st = FrameStats()
        rc = self.lib.frt_render_rows_accumulate(self.handle, ctypes.byref(p), frames,
                                                 self.lib.frt_accum_device_part(acc._acc),
                                                 ctypes.byref(st) if stats else None)
        if rc != 0:
            raise RuntimeError("frt render_accumulated failed: " + self.lib.frt_last_error().decode())
        return st

    def render_accumulated(self, frames: int, seed: int = 0x5EED, batch_samples: int = 0,
                           precision: str | None = None, stats: bool = False):
        """Render the whole frame `frames` times under the seeds seed, seed + 1, .. (wrapping uint64) into a device
        accumulator (frt_render_rows_accumulate: the frames never leave the device) and resolve it. Returns (mean
        (h, w, 4), var (h, w, 4)) float64: bit for bit what a host Accumulator fed render(seed=seed + k) for
        k < frames resolves to. var[..., :3] is the variance of the mean (0 where fewer than two frames counted),
        var[..., 3] the number of frames counted. With stats=True: and the summed FrameStats."""
        h, w = self.frame.height, self.frame.width
        acc = Accumulator((h, w), device=self.device)
        try:
            st = self._accumulate(acc, frames, seed, batch_samples, precision, stats)
            mean, var = acc.resolve()
        finally:
            acc.close()
        return (mean, var, st) if stats else (mean, var)

    def render_accumulated_denoised(self, frames: int, params=None, **render_args):
        """render_accumulated, render_features_into and the variance-guided denoise (frt_denoise_var) on device
        buffers, in place: nothing crosses to the host in between. Returns (rgba (h, w, 4), var (h, w, 4), denoise
        stats dict): bit for bit denoise_var(*render_accumulated(frames, ...), render_features(...)). It needs
        frames >= 2: one frame has no variance, and it raises rather than pass the frame through. render_args: seed,
        batch_samples, precision (the feature pass takes seed and batch_samples)."""
        import torch
        unknown = set(render_args) - {"seed", "batch_samples", "precision"}
        if unknown:
            raise TypeError("frt: render_accumulated_denoised takes seed, batch_samples and precision, not %s"
                            % sorted(unknown))
        if frames < 2:
            raise ValueError("frt: render_accumulated_denoised needs frames >= 2 (one frame has no variance), not %r"
                             % (frames,))
        h, w = self.frame.height, self.frame.width
        with torch.cuda.device(self.device):
            mean = torch.empty((h, w, 4), dtype=torch.float64, device="cuda")
            var = torch.empty((h, w, 4), dtype=torch.float64, device="cuda")
            geom = torch.empty((h, w, FEATURE_GEOM_WORDS), dtype=torch.float64, device="cuda")
            ids = torch.empty((h, w, 2), dtype=torch.int32, device="cuda")
        acc = Accumulator((h, w), device=self.device)
        try:
            self._accumulate(acc, frames, render_args.get("seed", 0x5EED), render_args.get("batch_samples", 0),
                             render_args.get("precision"), False)
            acc.resolve_into(mean.data_ptr(), var.data_ptr())
        finally:
            acc.close()
        self.render_features_into(geom.data_ptr(), ids.data_ptr(),
                                  **{k: v for k, v in render_args.items() if k in ("seed", "batch_samples")})
        st = _denoise_var(mean.data_ptr(), var.data_ptr(), geom.data_ptr(), ids.data_ptr(), True, w, h, 1, params,
                          "device", self.device, mean.data_ptr(), var.data_ptr())
        return mean.cpu().numpy(), var.cpu().numpy(), st.as_dict()

    def temporal(self, params=None, seed: int = 0x5EED) -> "TemporalAccumulator":
        """A TemporalAccumulator over this renderer: accumulation that follows a moving camera. Each of its render()
        calls moves the camera, reprojects the accumulated history into the new view on the device
        (frt_accum_reproject) and adds the call's frames. params: a ReprojectParams, a dict of its fields, or None."""
        return TemporalAccumulator(self, params, seed)


def render_multi(scene: Scene, devices: str | None = None) -> np.ndarray:
    """The drop-in entry point itself: ``render_multi(cam, world, usteps, vsteps, jitter)``
    (host/frt_render.c; reference renderer.c:244) on the captured scene — flatten, upload
    (incl. the scene-specialised kernel's compile), render over the selected devices
    (``FRT_DEVICES`` list, e.g. "0,0"; default every visible GPU), copy to the host canvas.
    A call whose world, config, knobs and devices equal the previous call's and whose camera alone differs (a
    View of the same Scene) moves the camera of the handles it kept and uploads nothing.
    Returns the (height, width, 4) canvas. The array is the canvas's own memory, not a copy: for up to
    FRT_PINNED_CANVASES (default 4) canvases alive at once it aliases page-locked (hipHostMalloc) memory, which goes
    back to the library's pool when the array is collected; canvases kept beyond that number are ordinary malloc'd
    memory. Copy an array you mean to keep for long (np.array(c)). render_multi's failures are logged by it and
    leave the canvas zeroed (the reference has no error return); ``frt_render_multi_error``
    (host/frt_render.c) names the failure, and it raises here."""
    lib = host_lib()
    vp = ctypes.c_void_p
    lib.render_multi.restype = vp
    lib.render_multi.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_bool]
    lib.canvas_free.argtypes = [vp]
    old = os.environ.get("FRT_DEVICES")
    if devices is not None:
        os.environ["FRT_DEVICES"] = devices
    try:
        c = lib.render_multi(scene.camera, scene.world, scene.usteps, scene.vsteps, scene.jitter)
    finally:
        if devices is not None:
            if old is None:
                os.environ.pop("FRT_DEVICES", None)
            else:
                os.environ["FRT_DEVICES"] = old
    # the canvas's array itself, not a copy (a 1920x1080 canvas is 66 MB): the returned array owns the canvas, and
    # canvas_free runs when it is collected (render_multi's array goes back to host/frt_canvas.c's pinned pool)
    try:
        # struct canvas (canvas.h): Color *arr; size_t width, height; ... — read via the helper
        lib.frt_canvas_data.restype = ctypes.POINTER(ctypes.c_double)
        lib.frt_canvas_data.argtypes = [vp]
        ptr = lib.frt_canvas_data(c)
        out = np.ctypeslib.as_array(ptr, shape=(scene.height, scene.width, 4))
        weakref.finalize(out, lib.canvas_free, c)
    except BaseException:
        lib.canvas_free(c)
        raise
    lib.frt_render_multi_error.restype = ctypes.c_char_p
    err = lib.frt_render_multi_error()
    global _release_registered
    if not _release_registered:  # (the kept handles go before the interpreter's teardown, not during it)
        import atexit
        lib.frt_render_multi_release.restype = None
        atexit.register(lib.frt_render_multi_release)
        _release_registered = True
    if err:
        raise RuntimeError("frt: render_multi failed: " + err.decode(errors="replace"))
    return out


_release_registered = False


def release_render_multi() -> None:
    """Release the device handles render_multi keeps between calls (host/frt_render.c frt_render_multi_release:
    the scene, its compiled kernels and level state on every device of the last call). Registered to run at exit."""
    global _release_registered
    lib = host_lib()
    lib.frt_render_multi_release.restype = None
    lib.frt_render_multi_release()
    if not _release_registered:
        import atexit
        atexit.register(lib.frt_render_multi_release)
        _release_registered = True


RENDER_MULTI_PHASES = ("flatten", "upload", "upload.device_select", "upload.scene_buffers", "upload.walk_records_meshes",
                       "upload.jit_source", "upload.jit_code_object", "upload.jit_module_load", "upload.rest",
                       "upload.total", "render_rows_and_copy", "place_rows", "release", "total", "device_warmup",
                       "device_warmup_wait")


def render_multi_phases() -> dict:
    """The phases of this process's last render_multi in ms (host/frt_render.c frt_render_multi_phases):
    flatten, the slowest device's upload and its sub-phases (frt_upload_phases), render incl. the copy to
    host memory, placing the rows into the canvas, release, total."""
    lib = host_lib()
    lib.frt_render_multi_phases.restype = ctypes.c_int
    lib.frt_render_multi_phases.argtypes = [ctypes.c_void_p, ctypes.c_int]
    out = (ctypes.c_double * 16)()
    lib.frt_render_multi_phases(out, 16)
    return {k: round(float(v), 3) for k, v in zip(RENDER_MULTI_PHASES, out)}


def cpu_share() -> int:
    """The host CPUs this process may use: the cgroup's CPU quota (cpu.max) when one is set, else the
    CPUs in its affinity mask. On the GPU box os.cpu_count() reports the whole machine (256) while the
    quota per GPU is 16."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) // int(period))))
    except (OSError, ValueError):
        pass
    return max(1, n)


def jit_cache_stats() -> dict:
    """Counters of the scene-specialised kernels' code-object cache (include/frt_device.h
    frt_jit_cache_stats) since the library was loaded."""
    lib = host_lib()
    lib.frt_jit_cache_stats.restype = ctypes.c_int
    lib.frt_jit_cache_stats.argtypes = [ctypes.c_void_p, ctypes.c_int]
    out = (ctypes.c_int64 * 5)()
    lib.frt_jit_cache_stats(out, 5)
    return dict(zip(("compiles", "disk_hits", "disk_writes", "module_loads", "module_hits"), map(int, out)))


def _flat_scene(scene: Scene):
    """The scene flattened by the host library (frt_flatten_scene); free with frt_flat_scene_free."""
    lib = host_lib()
    vp = ctypes.c_void_p
    lib.frt_flatten_scene.restype = ctypes.c_int
    lib.frt_flatten_scene.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_bool, vp, ctypes.c_char_p,
                                      ctypes.c_size_t]
    lib.frt_flat_scene_free.argtypes = [vp]
    fs = ctypes.create_string_buffer(4096)  # frt_scene (a few hundred bytes)
    err = ctypes.create_string_buffer(512)
    if lib.frt_flatten_scene(scene.camera, scene.world, scene.usteps, scene.vsteps, scene.jitter, fs, err, 512):
        raise RuntimeError("frt: flatten failed: " + err.value.decode())
    return lib, fs


# frt_node (include/frt_device.h): 8 int32 and the 6 doubles of its box, 80 bytes
_NODE_DTYPE = np.dtype([("type", "<i4"), ("skip", "<i4"), ("parent", "<i4"), ("tparent", "<i4"), ("xform", "<i4"),
                        ("material", "<i4"), ("prim", "<i4"), ("right", "<i4"), ("bbox", "<f8", (6,))])


def scene_nodes(scene: Scene) -> dict:
    """The flattened object tree of a scene (or view) in pre-order, as the device holds it: {"type" (enum
    frt_node_type: 8 CSG and 9 group are the composites, everything else a leaf), "parent" (-1: a world shape),
    "material" (index into the flattened materials; leaves)}, int32 arrays of one entry per node. A `node` id of
    GpuRenderer.render_features indexes them."""
    lib, fs = _flat_scene(scene)
    try:
        num = ctypes.c_int32.from_buffer(fs, 4).value  # frt_scene: abi_version, num_nodes, nodes
        ptr = ctypes.c_void_p.from_buffer(fs, 8).value
        nodes = np.frombuffer(ctypes.string_at(ptr, num * _NODE_DTYPE.itemsize), dtype=_NODE_DTYPE) if num > 0 \
            else np.zeros(0, dtype=_NODE_DTYPE)
        return {k: np.array(nodes[k], dtype=np.int32) for k in ("type", "parent", "material")}
    finally:
        lib.frt_flat_scene_free(fs)


def jit_check(scene: Scene) -> tuple[int, str, str]:
    """Generate and compile (hiprtc, no device needed) the scene-specialised shadow
    kernel frt_scene_upload would use for this scene: (rc, log, source) with rc 0
    compiled, 1 not eligible (generic walk), -1 compile error (include/frt_device.h)."""
    hl, fs = _flat_scene(scene)
    lib = hl
    lib.frt_jit_check.restype = ctypes.c_int
    lib.frt_jit_check.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p,
                                  ctypes.c_size_t]
    log = ctypes.create_string_buffer(1 << 16)
    src = ctypes.create_string_buffer(1 << 22)
    try:
        rc = lib.frt_jit_check(fs, log, len(log), src, len(src))
    finally:
        hl.frt_flat_scene_free(fs)
    return rc, log.value.decode(errors="replace"), src.value.decode(errors="replace")


def mesh_check(scene: Scene) -> tuple[int, dict]:
    """The meshes frt_scene_upload would search per lane in BVHs of their own, built
    and checked on the host (include/frt_device.h frt_mesh_check, no device needed):
    (violations, {"meshes", "triangles", "bvh_nodes", "depth"})."""
    hl, fs = _flat_scene(scene)
    lib = hl
    lib.frt_mesh_check.restype = ctypes.c_int
    lib.frt_mesh_check.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    out = (ctypes.c_int64 * 4)()
    try:
        bad = lib.frt_mesh_check(fs, out, 4)
    finally:
        hl.frt_flat_scene_free(fs)
    return bad, dict(zip(("meshes", "triangles", "bvh_nodes", "depth"), map(int, out)))


def encode_ppm(rgba: np.ndarray, use_scaling: bool = True) -> bytes:
    """16-bit P6 PPM bytes of a (h, w, 3|4) float64 canvas, encoded by the host
    library exactly as write_ppm_file(c, use_scaling, path) writes them."""
    lib = host_lib()
    h, w = rgba.shape[:2]
    buf = np.zeros((h, w, 4), dtype=np.float64)
    buf[:, :, :rgba.shape[2]] = rgba[:, :, :min(4, rgba.shape[2])]
    if rgba.shape[2] == 3:
        buf[:, :, 3] = 0.0
    n = lib.frt_encode_ppm(buf.ctypes.data_as(ctypes.c_void_p), w, h, int(use_scaling), None, 0)
    out = np.zeros(n, dtype=np.uint8)
    lib.frt_encode_ppm(buf.ctypes.data_as(ctypes.c_void_p), w, h, int(use_scaling),
                       out.ctypes.data_as(ctypes.c_void_p), n)
    return out.tobytes()


def ppm_values(rgba: np.ndarray, use_scaling: bool = True) -> np.ndarray:
    """The (h, w, 3) 16-bit channel values encode_ppm writes (big-endian after the header, one newline at the end)."""
    h, w = rgba.shape[:2]
    data = encode_ppm(rgba, use_scaling)
    return np.frombuffer(data[len(data) - 1 - 6 * h * w:len(data) - 1], dtype=">u2").reshape(h, w, 3).astype(np.int64)


def _encode16(ptr: int, on_device: bool, w: int, h: int, mode: str, backend: str, device: int):
    lib = host_lib()
    if mode not in ENCODE_MODES or backend not in ENCODE_BACKENDS:
        raise ValueError("frt: encode mode %r / backend %r is not supported" % (mode, backend))
    out = np.zeros((h, w, 3), dtype=">u2")
    st = EncodeStats()
    rc = lib.frt_encode16(ctypes.c_void_p(ptr), int(on_device), w, h, ENCODE_MODES.index(mode),
                          ENCODE_BACKENDS.index(backend), device, out.ctypes.data_as(ctypes.c_void_p),
                          ctypes.byref(st))
    if rc != 0:
        raise RuntimeError("frt: encode16 failed (rc %d)" % rc)
    return out.astype(np.uint16), st.as_dict()


def _rgba64(rgba: np.ndarray) -> np.ndarray:
    h, w = rgba.shape[:2]
    buf = np.zeros((h, w, 4), dtype=np.float64)
    buf[:, :, :min(4, rgba.shape[2])] = rgba[:, :, :min(4, rgba.shape[2])]
    return buf


def encode16(rgba: np.ndarray, mode: str = "ppm_scaled", backend: str = "device", device: int = 0):
    """The 16-bit values write_ppm_file(c, true / false, ..) ("ppm_scaled" / "ppm_clamped") or write_png ("png")
    write for a (h, w, 3|4) float64 canvas: ((h, w, 3) uint16, stats dict). backend "device": the HIP encode
    (frt_encode.hip), falling back to the host pass with the reason in stats["decline"]; "host": the host pass;
    "auto": the device once this process has rendered on one. Either way the values are the host pass's."""
    _, buf = _canvas_of(rgba)  # (a float64 h x w x 4 array as it is: render_multi's page-locked canvas)
    return _encode16(buf.ctypes.data, False, buf.shape[1], buf.shape[0], mode, backend, device)


def encode_last() -> dict:
    """What this thread's last encode did (frt_encode_last): write_ppm / write_png / encode16."""
    st = EncodeStats()
    host_lib().frt_encode_last(ctypes.byref(st))
    return st.as_dict()


def srgb_max_full(rgba: np.ndarray) -> list:
    """construct_ppm's srgb_max by its two full host passes (frt_srgb_max_full)."""
    buf = _rgba64(rgba)
    out = (ctypes.c_double * 3)()
    host_lib().frt_srgb_max_full(buf.ctypes.data_as(ctypes.c_void_p), buf.shape[1], buf.shape[0], out)
    return list(out)


def encode_selftest(n: int, seed: int = 1):
    """frt_encode_selftest on the current device: (failed lanes, [worst sRGB deviation, worst pow deviation,
    lanes whose sRGB value differs from the host's])."""
    out = (ctypes.c_double * 3)()
    bad = host_lib().frt_encode_selftest(n, seed, out, 3)
    return int(bad), list(out)


def _denoise_params(params) -> DenoiseParams:
    if params is None:
        return DenoiseParams()
    if isinstance(params, DenoiseParams):
        return params
    if isinstance(params, dict):
        return DenoiseParams(**params)
    raise TypeError("frt: denoise params must be a DenoiseParams, a dict of its fields or None")


def _denoise(rgba: int, geom: int, ids: int, on_device: bool, w: int, h: int, nimages: int, params, backend: str,
             device: int, out: int) -> DenoiseStats:
    """frt_denoise on raw pointers (all on the host or all on `device`); raises with the library's reason."""
    lib = host_lib()
    if backend not in DENOISE_BACKENDS:
        raise ValueError("frt: denoise backend %r is not supported (%s)" % (backend, ", ".join(DENOISE_BACKENDS)))
    p = _denoise_params(params)
    st = DenoiseStats()
    rc = lib.frt_denoise(ctypes.c_void_p(rgba), ctypes.c_void_p(geom), ctypes.c_void_p(ids), int(on_device), w, h,
                         nimages, ctypes.byref(p), DENOISE_BACKENDS.index(backend), device, ctypes.c_void_p(out),
                         ctypes.byref(st))
    if rc != 0:
        raise RuntimeError("frt: denoise failed: " + lib.frt_denoise_error().decode())
    return st


def _feature_buffers(features):
    """(geom (..., 8) float64, ids (..., 2) int32), C-contiguous, from render_features' dict or a (geom, ids) pair."""
    if isinstance(features, dict):
        geom = features["depth"].base if isinstance(features.get("depth"), np.ndarray) else None
        ids = features["node"].base if isinstance(features.get("node"), np.ndarray) else None
        shape = features["depth"].shape
        if geom is None or geom.shape != shape + (FEATURE_GEOM_WORDS,) or geom.dtype != np.float64:
            geom = np.concatenate([features["depth"][..., None], features["normal"], features["albedo"],
                                   features["coverage"][..., None]], axis=-1)
        if ids is None or ids.shape != shape + (2,) or ids.dtype != np.int32:
            ids = np.stack([features["node"], features["material"]], axis=-1)
    else:
        geom, ids = features
    return (np.ascontiguousarray(geom, dtype=np.float64), np.ascontiguousarray(ids, dtype=np.int32))


def denoise(rgba: np.ndarray, features, params=None, backend: str = "device", device: int = 0, stats: bool = False):
    """Denoise a colour frame with its first-hit feature buffers (frt_denoise: an edge-avoiding a-trous filter
    guided by depth, normal, albedo and material id; include/frt_device.h "Denoise"). rgba: (h, w, 4) float64, or
    (K, h, w, 4) for K stacked views, which are filtered independently; features: render_features' /
    render_feature_views' dict, or a (geom (..., 8) float64, ids (..., 2) int32) pair. params: a DenoiseParams, a
    dict of its fields, or None for the defaults. backend "device": the HIP pass (frt_denoise.hip); "host": the C
    pass, which is the definition; "auto": the device once this process has rendered on one. The two give the same
    bits. A missing device is an error, not a fall-back. Returns a new array like rgba (with stats=True: and the
    DenoiseStats). Pixels without a hit, or with a non-finite colour, come back as they are."""
    rgba = np.ascontiguousarray(rgba, dtype=np.float64)
    if rgba.ndim not in (3, 4) or rgba.shape[-1] != 4:
        raise ValueError("frt: denoise needs an (h, w, 4) or (K, h, w, 4) canvas, not %r" % (rgba.shape,))
    geom, ids = _feature_buffers(features)
    if geom.shape != rgba.shape[:-1] + (FEATURE_GEOM_WORDS,) or ids.shape != rgba.shape[:-1] + (2,):
        raise ValueError("frt: denoise needs feature buffers of the canvas's shape: geom %r, ids %r, canvas %r"
                         % (geom.shape, ids.shape, rgba.shape))
    k = rgba.shape[0] if rgba.ndim == 4 else 1
    h, w = rgba.shape[-3], rgba.shape[-2]
    out = np.empty_like(rgba)
    st = _denoise(rgba.ctypes.data, geom.ctypes.data, ids.ctypes.data, False, w, h, k, params, backend, device,
                  out.ctypes.data)
    return (out, st) if stats else out


def denoise_release() -> None:
    """Free the device pass's buffers (frt_denoise_release); the next call allocates them again."""
    host_lib().frt_denoise_release()


def _denoise_var_params(params) -> DenoiseVarParams:
    if params is None:
        return DenoiseVarParams()
    if isinstance(params, DenoiseVarParams):
        return params
    if isinstance(params, dict):
        return DenoiseVarParams(**params)
    raise TypeError("frt: denoise_var params must be a DenoiseVarParams, a dict of its fields or None")


def _denoise_var(rgba: int, var: int, geom: int, ids: int, on_device: bool, w: int, h: int, nimages: int, params,
                 backend: str, device: int, out: int, out_var: int | None) -> DenoiseVarStats:
    """frt_denoise_var on raw pointers (all on the host or all on `device`); raises with the library's reason."""
    lib = host_lib()
    if backend not in DENOISE_BACKENDS:
        raise ValueError("frt: denoise backend %r is not supported (%s)" % (backend, ", ".join(DENOISE_BACKENDS)))
    p = _denoise_var_params(params)
    st = DenoiseVarStats()
    rc = lib.frt_denoise_var(ctypes.c_void_p(rgba), ctypes.c_void_p(var), ctypes.c_void_p(geom), ctypes.c_void_p(ids),
                             int(on_device), w, h, nimages, ctypes.byref(p), DENOISE_BACKENDS.index(backend), device,
                             ctypes.c_void_p(out), ctypes.c_void_p(out_var) if out_var else None, ctypes.byref(st))
    if rc != 0:
        raise RuntimeError("frt: denoise_var failed: " + lib.frt_denoise_error().decode())
    return st


def denoise_var(rgba: np.ndarray, var: np.ndarray, features, params=None, backend: str = "device", device: int = 0,
                stats: bool = False):
    """Denoise an accumulated mean guided by the variance of that mean (frt_denoise_var: the a-trous filter of
    denoise() with its colour term scaled by the locally pre-filtered variance, and the variance filtered alongside;
    include/frt_device.h "Variance-guided denoise"). rgba, var: (h, w, 4) float64 as Accumulator.resolve() /
    GpuRenderer.render_accumulated return them, or (K, h, w, 4) stacks; features, backend, device as denoise's;
    params: a DenoiseVarParams, a dict of its fields, or None. Returns (rgba, var) as new arrays (with stats=True:
    and the DenoiseVarStats). A pixel whose variance and whose neighbours' variance are 0 comes back as it is, as do
    pixels without a hit or with a non-finite colour or variance."""
    rgba = np.ascontiguousarray(rgba, dtype=np.float64)
    var = np.ascontiguousarray(var, dtype=np.float64)
    if rgba.ndim not in (3, 4) or rgba.shape[-1] != 4:
        raise ValueError("frt: denoise_var needs an (h, w, 4) or (K, h, w, 4) canvas, not %r" % (rgba.shape,))
    if var.shape != rgba.shape:
        raise ValueError("frt: denoise_var needs a variance of the canvas's shape %r, not %r" % (rgba.shape, var.shape))
    geom, ids = _feature_buffers(features)
    if geom.shape != rgba.shape[:-1] + (FEATURE_GEOM_WORDS,) or ids.shape != rgba.shape[:-1] + (2,):
        raise ValueError("frt: denoise_var needs feature buffers of the canvas's shape: geom %r, ids %r, canvas %r"
                         % (geom.shape, ids.shape, rgba.shape))
    k = rgba.shape[0] if rgba.ndim == 4 else 1
    h, w = rgba.shape[-3], rgba.shape[-2]
    out, out_var = np.empty_like(rgba), np.empty_like(var)
    st = _denoise_var(rgba.ctypes.data, var.ctypes.data, geom.ctypes.data, ids.ctypes.data, False, w, h, k, params,
                      backend, device, out.ctypes.data, out_var.ctypes.data)
    return (out, out_var, st) if stats else (out, out_var)


def denoise_var_release() -> None:
    """Free the variance-guided device pass's buffers (frt_denoise_var_release)."""
    host_lib().frt_denoise_var_release()


class Accumulator:
    """A per-pixel running mean and variance over frames (frt_accum: Welford's update; include/frt_device.h
    "Accumulator"). npixels_or_shape: a pixel count, or (h, w), which resolve() then shapes its arrays by. device: a
    HIP device (the state lives there; add() takes numpy arrays or device pointers) or None for the host pass, which
    is the definition (numpy arrays only). The two resolve to the same bits."""

    def __init__(self, npixels_or_shape, device: int | None = 0):
        self.lib = host_lib()
        self.shape = (int(npixels_or_shape),) if np.isscalar(npixels_or_shape) else tuple(
            int(n) for n in npixels_or_shape)
        self.npixels = int(np.prod(self.shape, dtype=np.int64)) if self.shape else 0
        self.device = device
        acc = ctypes.c_void_p()
        if self.lib.frt_accum_create(-1 if device is None else device, self.npixels, ctypes.byref(acc)) != 0:
            raise RuntimeError("frt: accumulator: " + self.lib.frt_accum_error().decode())
        self._acc = acc

    def _check(self, rc: int) -> None:
        if rc != 0:
            raise RuntimeError("frt: accumulator: " + self.lib.frt_accum_error().decode())

    def add(self, sample) -> None:
        """One sample per pixel: a float64 array of npixels x 4 values (any shape), or an int, the address of as
        many doubles in device memory on the accumulator's device (a torch.cuda tensor's data_ptr())."""
        if isinstance(sample, int):
            self._check(self.lib.frt_accum_add(self._acc, ctypes.c_void_p(sample), 1))
            return
        a = np.ascontiguousarray(sample, dtype=np.float64)
        if a.size != self.npixels * 4:
            raise ValueError("frt: accumulator of %d pixels given %d values (4 per pixel)" % (self.npixels, a.size))
        self._check(self.lib.frt_accum_add(self._acc, a.ctypes.data, 0))

    def resolve(self, stats: bool = False):
        """(mean, var), float64 arrays of shape + (4,): var[..., :3] the variance of the mean (0.0 under two samples),
        var[..., 3] the samples counted. With stats=True: and the AccumStats."""
        mean = np.empty(self.shape + (4,), dtype=np.float64)
        var = np.empty(self.shape + (4,), dtype=np.float64)
        st = AccumStats()
        self._check(self.lib.frt_accum_resolve(self._acc, mean.ctypes.data, var.ctypes.data, 0, ctypes.byref(st)))
        return (mean, var, st) if stats else (mean, var)

    def resolve_into(self, mean_ptr: int | None, var_ptr: int | None) -> AccumStats:
        """resolve into device memory on the accumulator's device (npixels x 4 doubles each; either may be None)."""
        st = AccumStats()
        self._check(self.lib.frt_accum_resolve(self._acc, ctypes.c_void_p(mean_ptr) if mean_ptr else None,
                                               ctypes.c_void_p(var_ptr) if var_ptr else None, 1, ctypes.byref(st)))
        return st

    def reset(self) -> None:
        self._check(self.lib.frt_accum_reset(self._acc))

    def state(self):
        """A host accumulator's state as copies: (n (npixels,) int32, mean (npixels, 4), m2 (npixels, 3)). A device
        accumulator's state stays on the device: resolve() is its way out."""
        vp = ctypes.c_void_p
        npx, ptr = ctypes.c_int64(), [vp() for _ in range(5)]
        if self.lib.frt_accum_host_state(self._acc, ctypes.byref(npx), *[ctypes.byref(q) for q in ptr]) != 0:
            raise RuntimeError("frt: accumulator: state() needs a host accumulator (device=None)")
        n = np.ctypeslib.as_array(ctypes.cast(ptr[0], ctypes.POINTER(ctypes.c_int32)), (npx.value,)).copy()
        mean = np.ctypeslib.as_array(ctypes.cast(ptr[1], ctypes.POINTER(ctypes.c_double)), (npx.value, 4)).copy()
        m2 = np.ctypeslib.as_array(ctypes.cast(ptr[2], ctypes.POINTER(ctypes.c_double)), (npx.value, 3)).copy()
        return n, mean, m2

    def close(self) -> None:
        if getattr(self, "_acc", None):
            self.lib.frt_accum_release(self._acc)
            self._acc = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def flat_camera(view) -> FlatCamera:
    """A Scene's or View's camera as the engine's frt_camera (frt_flatten_camera, without a sample table); a
    FlatCamera comes back as it is."""
    if isinstance(view, FlatCamera):
        return view
    lib = host_lib()
    lib.frt_flatten_camera.restype = ctypes.c_int
    lib.frt_flatten_camera.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_bool,
                                       ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]
    cam, table = FlatCamera(), ctypes.c_void_p()
    if lib.frt_flatten_camera(view.camera, 0, 0, False, ctypes.addressof(cam), ctypes.byref(table)) != 0:
        raise RuntimeError("frt: frt_flatten_camera failed")
    return cam


def reproject_setup(prev_view, cur_view) -> ReprojectGeometry:
    """frt_reproject_setup: the two lens centres and the previous camera's forward matrix, as both passes take them.
    It raises for cameras whose sizes differ or whose matrices are not finite."""
    lib = host_lib()
    g = ReprojectGeometry()
    if lib.frt_reproject_setup(ctypes.byref(flat_camera(prev_view)), ctypes.byref(flat_camera(cur_view)),
                               ctypes.byref(g)) != 0:
        raise RuntimeError("frt: reproject: " + lib.frt_accum_error().decode())
    return g


def _reproject_params(params) -> ReprojectParams:
    if params is None:
        return ReprojectParams()
    if isinstance(params, ReprojectParams):
        return params
    if isinstance(params, dict):
        return ReprojectParams(**params)
    raise TypeError("frt: reproject params must be a ReprojectParams, a dict of its fields or None")


def _reproject_features(features, npixels: int, keep: list):
    """(FeatureBuffers, on_device) of render_features' dict, a (geom, ids) pair of arrays, or a (geom, ids) pair of
    device pointers."""
    if not isinstance(features, dict) and all(isinstance(x, numbers.Integral) for x in features):
        return FeatureBuffers(int(features[0]) or None, int(features[1]) or None), True
    geom, ids = _feature_buffers(features)
    if geom.size != npixels * FEATURE_GEOM_WORDS or ids.size != npixels * 2:
        raise ValueError("frt: reproject needs feature buffers of the cameras' %d pixels: geom %r, ids %r"
                         % (npixels, geom.shape, ids.shape))
    keep += [geom, ids]
    return FeatureBuffers(geom.ctypes.data, ids.ctypes.data), False


def reproject(dst: "Accumulator", src: "Accumulator", prev_view, prev_features, cur_view, cur_features, params=None,
              stats: bool = False):
    """Carry src's state, accumulated under prev_view, to cur_view's pixels in dst (frt_accum_reproject: SVGF's
    reprojection step; include/frt_device.h "Reprojection"). dst and src are two Accumulators of the views' size,
    both on the host (the C pass, which is the definition) or both on one device (k_accum_reproject); the two give
    the same bits. prev_view / cur_view: a Scene, a View or a FlatCamera; the features are the dicts render_features
    returns under each view (or (geom, ids) arrays), or for device accumulators (geom_ptr, ids_ptr) pairs of device
    memory. dst's earlier contents are gone afterwards; later add()s continue from the reprojected state. A pixel
    whose surface the previous view did not see starts over with n = 0. params: a ReprojectParams, a dict of its
    fields, or None. Returns None (with stats=True: the ReprojectStats)."""
    lib = host_lib()
    prev, cur = flat_camera(prev_view), flat_camera(cur_view)
    w, h = int(cur.hsize), int(cur.vsize)
    keep = []
    pf, pdev = _reproject_features(prev_features, w * h, keep)
    cf, cdev = _reproject_features(cur_features, w * h, keep)
    if pdev != cdev:
        raise ValueError("frt: reproject needs both views' features on the host or both on the device")
    p = _reproject_params(params)
    st = ReprojectStats()
    rc = lib.frt_accum_reproject(dst._acc, src._acc, ctypes.byref(prev), ctypes.byref(cur), ctypes.byref(pf),
                                 ctypes.byref(cf), w, h, ctypes.byref(p), int(pdev), ctypes.byref(st))
    if rc != 0:
        raise RuntimeError("frt: reproject: " + lib.frt_accum_error().decode())
    return st if stats else None


class TemporalAccumulator:
    """Accumulation over a sequence of views of one resident scene (GpuRenderer.temporal()): every render() call
    reprojects the history into the call's view and adds the call's frames to it, all on the device.

    The contract: the result of a sequence of render() calls is bit for bit the same composition done by hand with a
    host Accumulator pair: for call j with view v_j, frames f_j and first frame index k_j (the frames of the object's
    life so far), feats_j = render_features(seed=seed + k_j, batch_samples=...) under v_j; reproject(dst, src,
    v_{j-1}, feats_{j-1}, v_j, feats_j, params) (skipped on the first call and after a restart); dst.add(render(
    seed=seed + k_j + i, ...)) for i < f_j; dst.resolve(). Frame k of the object's life uses seed + k, wrapping at 64
    bits. A view whose size differs from the history's restarts the history (counted in `restarts`)."""

    def __init__(self, renderer: "GpuRenderer", params=None, seed: int = 0x5EED):
        self.r = renderer
        self.params = _reproject_params(params)
        self.seed = int(seed)
        self.frames_done = 0
        self.restarts = 0
        self._accs = [None, None]
        self._feats = [None, None]
        self._cur = 0
        self._prev_cam = None
        self._shape = None

    def reset(self) -> None:
        """Forget the history (the seeds run on)."""
        self._prev_cam = None
        for a in self._accs:
            if a is not None:
                a.reset()

    def close(self) -> None:
        for a in self._accs:
            if a is not None:
                a.close()
        self._accs = [None, None]
        self._feats = [None, None]
        self._prev_cam = None
        self._shape = None

    def _allocate(self, h: int, w: int) -> None:
        import torch
        self.close()
        self._accs = [Accumulator((h, w), device=self.r.device) for _ in range(2)]
        with torch.cuda.device(self.r.device):
            self._feats = [(torch.empty((h, w, FEATURE_GEOM_WORDS), dtype=torch.float64, device="cuda"),
                            torch.empty((h, w, 2), dtype=torch.int32, device="cuda")) for _ in range(2)]
        self._shape = (h, w)

    def render(self, view=None, frames: int = 1, batch_samples: int = 0, precision: str | None = None, denoise=None,
               stats: bool = False):
        """Move the camera to `view` (None: where it is), reproject the history into it, add `frames` frames and
        resolve: (mean (h, w, 4), var (h, w, 4)) as render_accumulated returns them, var[..., 3] the samples a pixel
        holds (the reprojected history's and the new frames'). denoise: None, or True / a DenoiseVarParams / a dict
        of its fields to run the variance-guided denoise on the device buffers before they come back; it needs
        frames >= 2 and raises otherwise, as render_accumulated_denoised does. With stats=True a third value: a dict
        with "reproject" (ReprojectStats.as_dict(), None when nothing was reprojected), "frame" (the summed
        FrameStats), "restarts", "first_frame" and, with denoise, "denoise"."""
        import torch
        if frames < 1:
            raise ValueError("frt: temporal render needs frames >= 1, not %r" % (frames,))
        if denoise is not None and denoise is not False and frames < 2:
            raise ValueError("frt: temporal render with denoise needs frames >= 2 (one frame has no variance), not %r"
                             % (frames,))
        r = self.r
        if view is not None:
            r.set_camera(view)
        h, w = r.frame.height, r.frame.width
        cam = flat_camera(r.frame)
        if self._shape is not None and self._shape != (h, w):
            self.restarts += 1
            self._prev_cam = None
        if self._shape != (h, w):
            self._allocate(h, w)
        seed0 = (self.seed + self.frames_done) & 0xFFFFFFFFFFFFFFFF
        src, dst = self._cur, self._cur ^ 1
        geom, ids = self._feats[dst]
        r.render_features_into(geom.data_ptr(), ids.data_ptr(), seed=seed0, batch_samples=batch_samples)
        rst = None
        if self._prev_cam is not None:
            pgeom, pids = self._feats[src]
            rst = reproject(self._accs[dst], self._accs[src], self._prev_cam, (pgeom.data_ptr(), pids.data_ptr()),
                            cam, (geom.data_ptr(), ids.data_ptr()), self.params, stats=True)
        else:
            self._accs[dst].reset()
        fst = r._accumulate(self._accs[dst], frames, seed0, batch_samples, precision, stats)
        self.frames_done += frames
        self._cur, self._prev_cam = dst, cam
        with torch.cuda.device(r.device):
            mean = torch.empty((h, w, 4), dtype=torch.float64, device="cuda")
            var = torch.empty((h, w, 4), dtype=torch.float64, device="cuda")
        self._accs[dst].resolve_into(mean.data_ptr(), var.data_ptr())
        dst_stats = None
        if denoise is not None and denoise is not False:
            dst_stats = _denoise_var(mean.data_ptr(), var.data_ptr(), geom.data_ptr(), ids.data_ptr(), True, w, h, 1,
                                     None if denoise is True else denoise, "device", r.device, mean.data_ptr(),
                                     var.data_ptr())
        out = (mean.cpu().numpy(), var.cpu().numpy())
        if not stats:
            return out
        info = {"reproject": rst.as_dict() if rst is not None else None, "frame": fst, "restarts": self.restarts,
                "first_frame": self.frames_done - frames}
        if dst_stats is not None:
            info["denoise"] = dst_stats.as_dict()
        return out + (info,)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _CanvasStruct(ctypes.Structure):  # struct canvas (host/src/libs/canvas/canvas.h)
    _fields_ = [("arr", ctypes.c_void_p), ("width", ctypes.c_size_t), ("height", ctypes.c_size_t),
                ("super_sample", ctypes.c_bool), ("color_space_fn", ctypes.c_void_p)]


def _canvas_of(rgba: np.ndarray):
    if rgba.dtype == np.float64 and rgba.ndim == 3 and rgba.shape[2] == 4 and rgba.flags["C_CONTIGUOUS"]:
        buf = rgba  # (render_multi's page-locked array as it is)
    else:
        buf = _rgba64(rgba)
    return _CanvasStruct(buf.ctypes.data, buf.shape[1], buf.shape[0], False, None), buf


def write_ppm(path: str, rgba: np.ndarray, use_scaling: bool = True) -> dict:
    """write_ppm_file(canvas, use_scaling, path) of the host library (it appends ".ppm"; FRT_ENCODE selects the
    encode's backend); returns what the encode did."""
    c, keep = _canvas_of(rgba)
    if host_lib().write_ppm_file(ctypes.byref(c), bool(use_scaling), os.fsencode(path)) != 0:
        raise RuntimeError("frt: write_ppm_file failed: " + path)
    del keep
    return encode_last()


def write_png(path: str, rgba: np.ndarray) -> dict:
    """write_png(canvas, path) of the host library (it appends ".png"); returns what the encode did."""
    c, keep = _canvas_of(rgba)
    if host_lib().write_png(ctypes.byref(c), os.fsencode(path)) != 0:
        raise RuntimeError("frt: write_png failed: " + path)
    del keep
    return encode_last()
