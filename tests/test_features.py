"""First-hit feature buffers (frt_render_features*, GpuRenderer.render_features / render_feature_views): depth,
normal, albedo, coverage and the leaf / material ids of level 0, resolved per pixel by k_feature_resolve.

The references: the analytic unit sphere of tests/feature_ref.py (pinned against the oracle in
test_features_cpu.py), the pass against itself under every placement and kernel path (bit for bit), and the CPU
oracle's image for which pixels are hit at all."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import load_scene

import feature_ref

pytestmark = pytest.mark.gpu

KEYS = ("depth", "normal", "albedo", "coverage", "node", "material")

# the captured cameras' from / to (tests/golden/scenes/<name>.c)
EYES = {
    "checkered_sphere_200": ((0.0, 0.0, -5.0), (0.0, 0.0, 0.0)),
    "cornell_direct_64_4x4": ((0.0, 0.0, -2.75), (0.0, 0.0, 0.0)),
    "cornell_gi_24": ((0.0, 0.0, -2.75), (0.0, 0.0, 0.0)),
    "patterns_160x80": ((0.0, 2.2, -6.0), (0.0, 0.6, 0.0)),
    "csg_ops_96x64": ((0.0, 9.0, -11.0), (0.0, 0.5, 0.0)),
    "bump_map_100": ((0.0, 0.0, -2.0), (0.0, 0.0, 0.0)),
    "checkered_sphere_dof_100": ((0.0, 0.0, -5.0), (0.0, 0.0, 0.0)),
    "checkered_sphere_jitter_100": ((0.0, 0.0, -5.0), (0.0, 0.0, 0.0)),
    "teapot_low_100": ((0.0, 0.0, -30.0), (0.0, 0.0, 0.0)),
    "test_scene_120": ((-2.0, 3.0, -6.0), (0.0, 0.0, 0.0)),
    "group_test_150x50": ((0.0, 0.0, -9.0), (0.0, 0.0, 0.0)),
    "csg_nested_96x64": ((0.5, 5.0, -10.0), (0.5, 1.0, 0.5)),
    "reflect_refract_160x80": ((-2.6, 1.5, -3.9), (-0.6, 1.0, -0.8)),
    "checkered_torus_120": ((0.0, 5.0, -10.0), (0.0, 0.0, 0.0)),
    "primitives_edge_64x48": ((1.02, 7.1, -13.0), (0.2, 0.8, 0.3)),
}


def _renderer(scene):
    from fast_ray_tracer_amd.runtime import GpuRenderer
    return GpuRenderer(scene)


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in KEYS)


def _buffers(f):
    """The two buffers behind a feature dict (its arrays are views into them)."""
    return f["depth"].base, f["node"].base


# ---------------------------------------------------------------------------------------------------------------
# 1. analytic: the sphere

@pytest.fixture(scope="module")
def sphere(built):
    base = load_scene("checkered_sphere_200")
    r = _renderer(base)
    yield base, r
    r.close()


@pytest.mark.parametrize("steps", [1, 3, 4, 8, 17])
def test_sphere_against_the_analytic_reference(sphere, steps):
    """37 x 37 views at 1, 9, 16, 64 and 289 samples per pixel: ppb = 256, 28 (idle lanes), 16, 4 and the
    spp > 256 path; 37 * 37 pixels are no multiple of any of them. coverage equals the reference's hits / spp
    exactly; depth and normal are within 1e-9 of its ordered means (t is 4..5 and the discriminant at least 1e-5,
    so t's error is about 1e-14 / (2 sqrt(disc)) = 2e-12); ids are the sphere's where anything is hit."""
    from fast_ray_tracer_amd.runtime import scene_nodes
    base, r = sphere
    view = base.view(*EYES["checkered_sphere_200"], hsize=37, vsize=37, usteps=steps, vsteps=steps)
    t, point, disc, hit = feature_ref.sphere_samples(view)
    assert np.abs(disc).min() >= 1e-7  # (nothing to exclude: test_features_cpu.py)
    r.set_camera(view)
    f = r.render_features()
    spp = steps * steps
    cov = hit.sum(axis=2) / np.float64(spp)
    assert np.array_equal(f["coverage"], cov)
    assert 0 < (cov == 0).sum() and 0 < (cov == 1).sum()
    if steps > 1:
        assert ((cov > 0) & (cov < 1)).any()
    d_depth = np.abs(f["depth"] - feature_ref.ordered_mean(np.where(hit, t, 0.0), hit)).max()
    d_normal = np.abs(f["normal"] - feature_ref.ordered_mean(point, hit)).max()
    print("steps %d: max |depth - ref| = %.3e, max |normal - ref| = %.3e" % (steps, d_depth, d_normal))
    assert d_depth <= 1e-9 and d_normal <= 1e-9
    nodes = scene_nodes(base)
    leaf = int(np.flatnonzero(nodes["type"] == 5)[0])
    mat, colours = feature_ref.kd_pattern_colours(base)
    anyhit = cov > 0
    assert np.array_equal(f["node"], np.where(anyhit, leaf, -1))
    assert np.array_equal(f["material"], np.where(anyhit, mat, -1))
    for k in ("depth", "normal", "albedo"):  # (a pixel without a hit: +0.0 in every plane)
        z = f[k][~anyhit]
        assert not z.any() and not np.signbit(z).any()
    if steps == 1:  # albedo: one of the Kd pattern's two colours, bit for bit, and both occur
        a = f["albedo"][anyhit]
        is0, is1 = (a == colours[0]).all(axis=1), (a == colours[1]).all(axis=1)
        assert (is0 | is1).all() and is0.any() and is1.any()
    else:  # a mean of the two colours
        lo, hi = np.minimum(colours[0], colours[1]), np.maximum(colours[0], colours[1])
        a = f["albedo"][anyhit]
        assert (a >= lo - 1e-12).all() and (a <= hi + 1e-12).all()


# ---------------------------------------------------------------------------------------------------------------
# 2. placement

@pytest.mark.parametrize("name,size", [("cornell_direct_64_4x4", None), ("patterns_160x80", (48, 40))])
def test_features_are_a_placement(built, name, size):
    """One batch, batches of seven pixels (edges inside rows), batches of one sample's worth (one pixel), and the
    frame as three interleaved row sets of stride 3: the same two buffers bit for bit. cornell's walls are CSG (the
    scene-specialised closest hit runs), patterns_160x80 takes its albedo from the NodeColors columns."""
    base = load_scene(name)
    r = _renderer(base)
    try:
        if size:
            r.set_camera(base.view(*EYES[name], hsize=size[0], vsize=size[1]))
        h, spp = r.frame.height, r.frame.spp
        whole = r.render_features(batch_samples=1 << 24)
        assert (whole["coverage"] > 0).any() and np.isfinite(whole["depth"]).all()
        if name == "patterns_160x80":
            assert len(np.unique(whole["albedo"].reshape(-1, 3), axis=0)) > 4
        for batch in (7 * spp, 1):
            assert _same(r.render_features(batch_samples=batch), whole), batch
        geom, ids = (np.zeros_like(b) for b in _buffers(whole))
        for off in range(3):
            part = r.render_features(row_begin=off, row_end=h, row_stride=3)
            g, i = _buffers(part)
            assert g.shape[0] == len(range(off, h, 3))
            geom[off::3], ids[off::3] = g, i
        assert np.array_equal(geom, _buffers(whole)[0]) and np.array_equal(ids, _buffers(whole)[1])
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------------------------
# 3. kernel paths agree (fresh processes: the switches are read at upload)

PATH_SCENES = {"cornell_direct_64_4x4": (64, 64), "csg_ops_96x64": (48, 32), "bump_map_100": (48, 48),
               "checkered_sphere_dof_100": (32, 32), "checkered_sphere_jitter_100": (32, 32),
               "teapot_low_100": (40, 40), "primitives_edge_64x48": (64, 48)}
PATH_ENVS = {"default": {}, "jit_trace_off": {"FRT_JIT_TRACE": "0"}, "uniform_off": {"FRT_PREPARE_UNIFORM": "0"},
             "mesh_off": {"FRT_MESH": "0"}}

_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, {tests!r})
from conftest import load_scene
from fast_ray_tracer_amd.runtime import GpuRenderer
out = {{}}
for name, (eye, size) in {scenes!r}.items():
    base = load_scene(name)
    r = GpuRenderer(base)
    r.set_camera(base.view(eye[0], eye[1], hsize=size[0], vsize=size[1]))
    f, st = r.render_features(seed=11, stats=True)
    assert st.errors == 0
    out[name + ".geom"], out[name + ".ids"] = f["depth"].base, f["node"].base
    r.close()
np.savez({out!r}, **out)
"""


@pytest.fixture(scope="module")
def path_renders(built, tmp_path_factory):
    """{setting: the buffers of every PATH_SCENES frame}: one fresh process per setting renders all of them."""
    here = os.path.dirname(os.path.abspath(__file__))
    tmp = tmp_path_factory.mktemp("feature_paths")
    procs = {}
    for key, env in PATH_ENVS.items():  # (the four processes side by side)
        names = ["teapot_low_100"] if key == "mesh_off" else sorted(PATH_SCENES)
        penv = dict(os.environ)
        for k in ("FRT_JIT_TRACE", "FRT_PREPARE_UNIFORM", "FRT_MESH"):
            penv.pop(k, None)
        penv.update(env)
        out = str(tmp / (key + ".npz"))
        code = _CHILD.format(tests=here, out=out, scenes={n: (EYES[n], PATH_SCENES[n]) for n in names})
        procs[key] = (out, subprocess.Popen([sys.executable, "-c", code], env=penv, stdout=subprocess.DEVNULL,
                                            stderr=subprocess.PIPE, text=True))
    got = {}
    for key, (out, p) in procs.items():
        _, err = p.communicate(timeout=600)
        assert p.returncode == 0, (key, err[-3000:])
        got[key] = dict(np.load(out))
    return got


@pytest.mark.parametrize("name", sorted(PATH_SCENES))
def test_kernel_paths_agree(path_renders, name):
    """The generic closest hit (FRT_JIT_TRACE=0), k_prepare's per-lane path (FRT_PREPARE_UNIFORM=0) and, for the
    mesh, the tree walk without the mesh BVH (FRT_MESH=0) give the default's buffers bit for bit: CSG, a bump map,
    a lens aperture, jitter (seed 11) and smooth triangles."""
    want = path_renders["default"]
    assert (want[name + ".geom"][..., 7] > 0).any()
    others = ["jit_trace_off", "uniform_off"] + (["mesh_off"] if name == "teapot_low_100" else [])
    for key in others:
        for buf in (".geom", ".ids"):
            assert np.array_equal(path_renders[key][name + buf], want[name + buf]), (key, buf)


# ---------------------------------------------------------------------------------------------------------------
# 4. / 5. against the oracle's image, and invariants

ORACLE_SCENES = {"test_scene_120": (48, 48), "group_test_150x50": (45, 15), "csg_nested_96x64": (48, 32),
                 "reflect_refract_160x80": (64, 32), "checkered_torus_120": (48, 48)}
_golden_cache = {}


def _golden_features(name):
    """{steps: (view, features)} at 1 x 1 and 3 x 3 steps on one handle, rendered once per session."""
    if name not in _golden_cache:
        base = load_scene(name)
        r = _renderer(base)
        try:
            got = {}
            for steps in (1, 3):
                v = base.view(*EYES[name], hsize=ORACLE_SCENES[name][0], vsize=ORACLE_SCENES[name][1], usteps=steps,
                              vsteps=steps)
                r.set_camera(v)
                got[steps] = (v, r.render_features())
        finally:
            r.close()
        _golden_cache[name] = got
    return _golden_cache[name]


@pytest.mark.parametrize("name", sorted(ORACLE_SCENES))
def test_coverage_against_the_oracle_image(built, name):
    """One direction each, at 1 spp: a pixel whose sample hits nothing is exactly black in the oracle's frame, and
    a pixel the oracle colours is hit."""
    import oracle
    view, f = _golden_features(name)[1]
    img = oracle.render(view, threads=4)[:, :, :3]
    assert f["coverage"].shape == img.shape[:2]
    assert not img[f["coverage"] == 0].any()
    lit = (img > 0).any(axis=2)
    assert lit.any() and (f["coverage"][lit] == 1).all()


@pytest.mark.parametrize("name", sorted(ORACLE_SCENES))
def test_invariants(built, name):
    from fast_ray_tracer_amd.runtime import scene_nodes
    nodes = scene_nodes(load_scene(name))
    for steps, (view, f) in _golden_features(name).items():
        spp = steps * steps
        hits = f["coverage"] * spp
        assert np.array_equal(hits, np.rint(hits)) and hits.min() >= 0 and hits.max() <= spp
        hit = hits > 0
        assert hit.any()
        norm = np.linalg.norm(f["normal"], axis=2)
        if spp == 1:
            assert np.abs(norm[hit] - 1.0).max() <= 1e-12
        assert norm.max() <= 1.0 + 1e-12
        assert (f["depth"][hit] > 0).all() and np.isfinite(f["depth"]).all()
        assert np.array_equal(f["node"] >= 0, hit) and np.array_equal(f["material"] >= 0, hit)
        assert f["node"][hit].max() < len(nodes["type"]) and (nodes["type"][f["node"][hit]] < 8).all()
        assert np.array_equal(f["material"][hit], nodes["material"][f["node"][hit]])
        assert (f["albedo"] >= 0).all()


# ---------------------------------------------------------------------------------------------------------------
# 6. the handle is left as it was

def _photon_passes():
    from fast_ray_tracer_amd.runtime import host_lib
    lib = host_lib()
    lib.frt_photon_pass_stats.restype = ctypes.c_int
    lib.frt_photon_pass_stats.argtypes = [ctypes.c_void_p, ctypes.c_int]
    out = (ctypes.c_int64 * 2)()
    lib.frt_photon_pass_stats(out, 2)
    return list(out)


@pytest.mark.parametrize("name", ["cornell_direct_64_4x4", "cornell_gi_24"])
def test_colour_frames_around_a_features_pass(built, name):
    """colour frame, features, colour frame: the two frames are bit-identical, and with global illumination the
    pass traces no photons and the frame after it reuses its maps."""
    r = _renderer(load_scene(name))
    try:
        first, st0 = r.render(seed=5, stats=True)
        passes = _photon_passes()
        f, fst = r.render_features(seed=5, stats=True)
        assert _photon_passes() == passes and fst.photon_pass == 0 and fst.photon_ms == 0.0
        assert (f["coverage"] > 0).any()
        second, st1 = r.render(seed=5, stats=True)
        assert np.array_equal(first, second)
        assert st1.photon_pass == 0 and _photon_passes() == passes
        if name == "cornell_gi_24":
            assert st0.photon_pass == 1 and st1.photons[0] + st1.photons[1] > 0
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------------------------
# 7. strips

STRIP_EYES = [((0.3, 0.2, -2.0), (0, 0, 0)), ((-0.4, 0.3, -1.6), (0.2, -0.2, 0.5)), ((0.0, -0.3, -2.4), (0, 0.2, 0)),
              ((0.0, 0.0, -2.75), (0, 0, 0))]


def test_feature_strips(built):
    """Four 40 x 30 views of the cornell world through render_feature_views: view k is bit for bit set_camera +
    render_features (also in batches that cross views, and over a strided row set); the renderer's camera is its
    own afterwards; views of other steps than the handle's borrow it; mixed sizes and no views are refused with the
    engine's reason."""
    base = load_scene("cornell_direct_64_4x4")
    r = _renderer(base)
    try:
        own = r.render_features()
        for steps in (4, 3):  # (3 x 3: not the handle's steps, the borrow path)
            views = [base.view(f, t, hsize=40, vsize=30, usteps=steps, vsteps=steps) for f, t in STRIP_EYES]
            for args in ({}, {"batch_samples": 1000}, {"row_begin": 1, "row_end": 29, "row_stride": 3}):
                strip = r.render_feature_views(views, **args)
                assert r.frame is base
                assert strip["normal"].shape[:1] + strip["normal"].shape[2:] == (4, 40, 3)
                for k, v in enumerate(views):
                    r.set_camera(v)
                    one = r.render_features(**args)
                    assert all(np.array_equal(strip[key][k], one[key]) for key in KEYS), (steps, args, k)
                r.set_camera(base)
                assert not np.array_equal(strip["depth"][0], strip["depth"][1])
        assert r.frame is base and _same(r.render_features(), own)
        with pytest.raises(RuntimeError, match="share one size"):
            r.render_feature_views([views[0], base.view(*STRIP_EYES[0], hsize=40, vsize=31, usteps=3, vsteps=3)])
        with pytest.raises(RuntimeError, match="number of views must be positive"):
            r.render_feature_views([])
        assert r.frame is base and _same(r.render_features(), own)
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------------------------
# 8. stats, and the device variant

def _device_buffer(lib, nbytes):
    """hipMalloc'd memory on device 0, filled with 0xF9 bytes: (pointer, fetch() -> bytes, free())."""
    hip = ctypes.CDLL("libamdhip64.so")
    ptr = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(ptr), ctypes.c_size_t(nbytes)) == 0
    lib.frt_encode_fetch.restype = ctypes.c_int
    lib.frt_encode_fetch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]

    def fetch():
        host = np.zeros(nbytes, dtype=np.uint8)
        assert lib.frt_encode_fetch(host.ctypes.data, ptr, nbytes, 0) == 0
        return host

    def fill():
        assert hip.hipMemset(ptr, 0xF9, ctypes.c_size_t(nbytes)) == 0 and hip.hipDeviceSynchronize() == 0

    fill()
    return ptr.value, fetch, fill, lambda: hip.hipFree(ptr)


def test_stats_and_device_buffers(built):
    base = load_scene("cornell_direct_64_4x4")
    r = _renderer(base)
    try:
        f, st = r.render_features(row_begin=3, row_end=50, row_stride=2, stats=True)
        rows = len(range(3, 50, 2))
        assert f["depth"].shape == (rows, 64) and f["node"].dtype == np.int32
        assert st.primary_rays == rows * 64 * 16 and st.errors == 0 and st.render_ms > 0
        assert st.sub_launches[10] >= 1 and st.sub_ms[10] > 0
        assert st.kernel_launches[5] >= 1 and st.kernel_launches[6] >= 1
        assert [st.kernel_ms[k] for k in (1, 2, 3)] == [0.0, 0.0, 0.0]
        assert [st.kernel_launches[k] for k in (0, 1, 2, 3, 4, 7)] == [0] * 6
        assert "k_feature_resolve" in st.as_dict()["sub_ms"]
        # device memory, and either buffer alone
        whole = r.render_features()
        want_geom, want_ids = _buffers(whole)
        geom, geom_fetch, geom_fill, geom_free = _device_buffer(r.lib, want_geom.nbytes)
        ids, ids_fetch, ids_fill, ids_free = _device_buffer(r.lib, want_ids.nbytes)
        try:
            r.render_features_into(geom, ids)
            assert geom_fetch().tobytes() == want_geom.tobytes() and ids_fetch().tobytes() == want_ids.tobytes()
            geom_fill(), ids_fill()
            r.render_features_into(geom, None)
            assert geom_fetch().tobytes() == want_geom.tobytes() and (ids_fetch() == 0xF9).all()
            geom_fill()
            r.render_features_into(None, ids)
            assert ids_fetch().tobytes() == want_ids.tobytes() and (geom_fetch() == 0xF9).all()
        finally:
            geom_free(), ids_free()
        with pytest.raises(RuntimeError, match="both feature buffers are NULL"):
            r.render_features_into(None, None)
    finally:
        r.close()
