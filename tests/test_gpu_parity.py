"""GPU parity: the HIP engine against the reference's own output.

Tolerance (north star): every canvas channel within 1e-4 of the reference's
binary64 canvas, and the 16-bit PPM bytes identical (integer canvas
indexing). Differences below that come only from libm transcendentals (pow in
the microfacet term, atan2/acos in UV maps) evaluated by the device library
instead of glibc; the mismatch fraction is printed for the record.
"""
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ASSETS, GOLDEN, canvas_goldens, golden_index, load_golden_canvas, load_scene

pytestmark = pytest.mark.gpu

TOL = 1e-4
NEEDS_UNIMPLEMENTED = {}

_renderers = {}


def renderer(name):
    from fast_ray_tracer_amd.runtime import GpuRenderer
    if name not in _renderers:
        _renderers[name] = GpuRenderer(load_scene(name))
    return _renderers[name]


@pytest.mark.parametrize("name", [n for n in canvas_goldens()
                                  if n not in NEEDS_UNIMPLEMENTED and not golden_index()[n].get("stochastic")])
def test_gpu_matches_reference_canvas_and_ppm(built, name):
    from fast_ray_tracer_amd.runtime import encode_ppm
    img = renderer(name).render()[:, :, :3]
    ref = load_golden_canvas(name)
    diff = np.abs(img - ref)
    print(f"{name}: max|d|={diff.max():.3e} mismatching channels={(diff > 0).mean():.4%}")
    assert diff.max() <= TOL
    assert hashlib.sha256(encode_ppm(img)).hexdigest() == golden_index()[name]["ppm_sha256"]


def test_unimplemented_features_fail_loudly(built):
    """Configurations the reference cannot render are refused at upload with the reason, never
    rendered wrong: global illumination with photon-count 0 (the reference reads a NULL photon map)."""
    from fast_ray_tracer_amd.runtime import GpuRenderer
    scene = load_scene("cornell_gi_nomaps_16")
    with pytest.raises(RuntimeError, match="not (supported|implemented)"):
        GpuRenderer(scene)


def test_gpu_matches_oracle_on_benchmark_scene_rows(built):
    """cornell_box 800x800, 4x4 CMJ, full recursion (BASELINE configs[2]): a row band vs the oracle, within 1e-4
    and with identical 16-bit PPM values (the shading's refined estimates, FMA dot products and specular-tail test
    move a channel by ulps: no quantised value may flip)."""
    import oracle
    r = renderer("cornell_direct_800_4x4")
    gpu = r.render(392, 400)
    cpu = oracle.render(load_scene("cornell_direct_800_4x4"), 392, 400, threads=8)
    assert np.abs(gpu - cpu).max() <= TOL
    assert encode_band(gpu) == encode_band(cpu)


def test_gpu_full_frame_determinism_and_split_invariance(built):
    """Full-size properties: repeat runs, row interleaving (the multi-GPU split)
    and batch size do not change a single bit."""
    r = renderer("cornell_direct_800_4x4")
    full = r.render()
    assert np.array_equal(full, r.render())
    even = r.render(0, None, 2)
    odd = r.render(1, None, 2)
    assert np.array_equal(full[0::2], even)
    assert np.array_equal(full[1::2], odd)
    small_batches = r.render(batch_samples=1 << 16)
    assert np.array_equal(full, small_batches)
    assert np.isfinite(full).all()


@pytest.mark.parametrize("name", ["csg_nested_96x64", "csg_unsorted_64x48"])
def test_csg_scenes_split_and_batch_invariance(built, name):
    """CSG units through the generated kernels (csg_nested_96x64) and through the generic list walk
    (csg_unsorted_64x48): the 2-way and 3-way row interleave and batches of 2^12 samples (tiles of 64 nodes cut
    in the middle of a unit's pixels) leave every bit of the full frame unchanged."""
    r = renderer(name)
    full = r.render()
    assert np.isfinite(full).all() and full[:, :, :3].max() > 0
    for n in (2, 3):
        for k in range(n):
            assert np.array_equal(full[k::n], r.render(k, None, n)), (n, k)
    assert np.array_equal(full, r.render(batch_samples=1 << 12))


def test_drop_in_executable_renders_reference_ppm(built, tmp_path):
    """The unmodified generated main.c, linked against libfrt_host, renders on the
    GPU through render_multi and writes the reference's PPM bytes at full size."""
    name = "checkered_sphere_800"
    main_c = os.path.join(GOLDEN, "scenes", name + ".c")
    exe = tmp_path / name
    built.build_scene_executable(main_c, str(exe))
    out_base = re.search(r'global_config.output.file_path = "([^"]+)"', open(main_c).read()).group(1)
    os.makedirs(os.path.dirname(out_base), exist_ok=True)
    stats = tmp_path / "stats.json"
    subprocess.run([str(exe)], cwd=ASSETS, check=True, stdout=subprocess.DEVNULL,
                   env=dict(os.environ, FRT_STATS_OUT=str(stats)))
    e = golden_index()[name]
    assert hashlib.sha256(open(out_base + ".ppm", "rb").read()).hexdigest() == e["ppm_sha256"]
    assert hashlib.sha256(open(out_base + ".png", "rb").read()).hexdigest() == e["png_sha256"]
    st = json.load(open(stats))
    assert st["primary_rays"] == 800 * 800 and st["errors"] == 0


# ---- round 2: the north-star headline configuration at full size ----
HEADLINE = "cornell_direct_1920x1080_8x8"


def test_gpu_matches_oracle_on_headline_rows(built):
    """cornell_box 1920x1080, 8x8 CMJ (64 spp), full recursion — the bench workload: 24 rows spread over
    the frame (every 45th from row 22: walls, window, both spheres, floor) against the oracle at 1e-4,
    the oracle on every CPU of this process's share (one row job per thread). The reference itself is
    pinned on the same camera at 240x135 (golden cornell_direct_240x135_8x8)."""
    import oracle
    from fast_ray_tracer_amd.runtime import cpu_share
    gpu = renderer(HEADLINE).render(22, None, 45)
    assert gpu.shape[0] == 24
    cpu = oracle.render(load_scene(HEADLINE), 22, None, threads=cpu_share(), row_stride=45)
    diff = np.abs(gpu - cpu)
    print(f"24 rows: max|d|={diff.max():.3e} mismatching={(diff > 0).mean():.4%}")
    assert diff.max() <= TOL
    # the canvas's 16-bit PPM indexing of these rows (the rows' own max scaling)
    assert encode_band(gpu) == encode_band(cpu)


def test_gpu_matches_oracle_on_headline_dense_band(built):
    """32 consecutive rows of the headline frame across the window's penumbra on the floor and walls (rows
    700-731: the rows where the shadow pass's pair decisions and the shading's per-point arithmetic vary most)
    against the oracle: every channel within 1e-4 and the band's 16-bit PPM values identical — the count of
    differing values is printed (0 required), so a drift of the shading's refined estimates that flips a
    quantised value anywhere in the band fails here."""
    import oracle
    from fast_ray_tracer_amd.runtime import cpu_share, encode_ppm
    gpu = renderer(HEADLINE).render(700, 732)
    cpu = oracle.render(load_scene(HEADLINE), 700, 732, threads=cpu_share())
    diff = np.abs(gpu - cpu)
    pg = np.frombuffer(encode_ppm(gpu[:, :, :3]), dtype=np.uint8)
    pc = np.frombuffer(encode_ppm(cpu[:, :, :3]), dtype=np.uint8)
    flips = int((pg != pc).sum())
    print(f"rows 700-731: max|d|={diff.max():.3e} mismatching channels={(diff > 0).mean():.4%} PPM bytes differing={flips}")
    assert diff.max() <= TOL
    assert flips == 0


def encode_band(rgba):
    from fast_ray_tracer_amd.runtime import encode_ppm
    return hashlib.sha256(encode_ppm(rgba[:, :, :3])).hexdigest()


def test_gpu_headline_full_frame_determinism_and_split_invariance(built):
    """The full 1920x1080x64 frame: repeat runs, the row interleave of every multi-GPU split
    (2, 3 and 8 ranks) and the batch size leave every bit unchanged."""
    r = renderer(HEADLINE)
    full = r.render()
    assert full.shape == (1080, 1920, 4) and np.isfinite(full).all()
    assert np.array_equal(full, r.render())
    for n in (2, 3, 8):
        for k in range(n):
            assert np.array_equal(full[k::n], r.render(k, None, n)), (n, k)
    assert np.array_equal(full, r.render(batch_samples=1 << 19))
    # the image is not trivially empty: its mean agrees with the reference's render of the same camera at
    # 1/64 of the pixels (golden cornell_direct_240x135_8x8: 6.137e-4; the scene is dim apart from the lit
    # faces), and as many pixels are lit
    ref = load_golden_canvas("cornell_direct_240x135_8x8")
    assert abs(full[:, :, :3].mean() / ref.mean() - 1.0) < 0.02
    assert abs((full[:, :, :3] > 0).mean() - (ref > 0).mean()) < 0.02


def test_render_multi_two_handles_on_one_device_bit_identical(built):
    """render_multi's in-process multi-GPU split (host/frt_render.c: one thread, handle and stream
    per device, interleaved rows placed into the caller's canvas) with two handles on device 0,
    against one device and against the engine's direct row render."""
    from fast_ray_tracer_amd.runtime import render_multi
    sc = load_scene("cornell_direct_800_4x4")
    one = render_multi(sc, devices="0")
    two = render_multi(sc, devices="0,0")
    three = render_multi(sc, devices="0,0,0")
    assert np.array_equal(one, two) and np.array_equal(one, three)
    assert np.array_equal(one, renderer("cornell_direct_800_4x4").render())


def test_render_multi_shares_photon_maps_across_devices(built):
    """render_multi over several devices of one process traces and balances the photon maps once (frt_engine.hip
    build_photon_maps: the first handle traces, the others upload the same host arrays): the GI canvas over two
    and three handles on device 0 equals the canvas with every handle tracing its own maps (FRT_SHARE_PHOTONS=0)
    bit for bit, and the counters show the passes traced and shared (the maps' host arrays are held only while a
    handle of the call still uploads them, so a later call with the same seed traces again)."""
    import ctypes
    from fast_ray_tracer_amd.runtime import host_lib, render_multi
    lib = host_lib()
    lib.frt_photon_pass_stats.restype = ctypes.c_int

    def passes():
        out = (ctypes.c_int64 * 2)()
        lib.frt_photon_pass_stats(out, 2)
        return int(out[0]), int(out[1])

    sc = load_scene("cornell_gi_24")
    saved = {k: os.environ.get(k) for k in ("FRT_SHARE_PHOTONS", "FRT_SEED", "FRT_RM_KEEP")}
    os.environ["FRT_SEED"] = "424242"  # (a seed no other test renders this scene with: no maps kept from before)
    os.environ["FRT_RM_KEEP"] = "0"  # (every call uploads: a kept handle would reuse its maps)
    try:
        os.environ["FRT_SHARE_PHOTONS"] = "0"
        t0, s0 = passes()
        own = render_multi(sc, devices="0,0")  # every handle traces its own maps
        t1, s1 = passes()
        del os.environ["FRT_SHARE_PHOTONS"]
        two = render_multi(sc, devices="0,0")  # one pass for both handles
        t2, s2 = passes()
        three = render_multi(sc, devices="0,0,0")  # the same scene and seed again: traced anew (the host arrays
        # are freed after the last handle of a call uploads them), shared by the three handles
        t3, s3 = passes()
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert (t1 - t0, s1 - s0) == (2, 0), (t0, s0, t1, s1)
    assert (t2 - t1, s2 - s1) == (1, 1), (t1, s1, t2, s2)
    assert (t3 - t2, s3 - s2) == (1, 2), (t2, s2, t3, s3)
    assert np.isfinite(own).all() and own[:, :, :3].max() > 0
    assert np.array_equal(own, two) and np.array_equal(own, three)


def test_render_multi_failure_returns_zero_canvas(built):
    """The reference has no error return: a failing render_multi logs and returns a zeroed canvas
     instead of exiting the process; frt_render_multi_error names the failure (a
    canvas may be black without one)."""
    import ctypes
    from fast_ray_tracer_amd.runtime import host_lib, render_multi
    sc = load_scene("cornell_gi_nomaps_16")
    with pytest.raises(RuntimeError, match="render_multi failed: .*not supported"):
        render_multi(sc, devices="0")
    lib = host_lib()
    lib.frt_render_multi_error.restype = ctypes.c_char_p
    render_multi(load_scene("checkered_sphere_200"), devices="0")
    assert lib.frt_render_multi_error() == b""


_JIT_CACHE_PROBE = r"""
import json, os, sys, time
sys.path.insert(0, {tests!r})
from conftest import load_scene
from fast_ray_tracer_amd.runtime import GpuRenderer, jit_cache_stats, render_multi
sc = load_scene("cornell_direct_64_4x4")
out = {{}}
t = time.perf_counter(); render_multi(sc, devices="0,0"); out["cold_ms"] = 1e3 * (time.perf_counter() - t)
out["after_render_multi"] = jit_cache_stats()
t = time.perf_counter(); render_multi(sc, devices="0,0"); out["warm_ms"] = 1e3 * (time.perf_counter() - t)
a, b = GpuRenderer(sc), GpuRenderer(sc)
a.close(); b.close()
out["after_handles"] = jit_cache_stats()
print("JSON" + json.dumps(out))
"""


def test_jit_compiled_once_and_cached_on_disk(built, tmp_path):
    """The scene-specialised kernels' code object is compiled once per process and shared by every
    device and handle (frt_jit.hip frt_jit_compile): render_multi over two handles on device 0 and two
    more scene handles compile once; a second process finds the code object in the on-disk cache and
    compiles nothing, so its first render_multi costs about what a warm one does."""
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, FRT_JIT_CACHE_DIR=str(tmp_path / "co"), FRT_JIT="1")

    def probe():
        p = subprocess.run([sys.executable, "-c", _JIT_CACHE_PROBE.format(tests=here)], env=env, cwd=here,
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-3000:]
        return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("JSON")][-1][4:])

    first = probe()
    print("first process", first)
    assert first["after_render_multi"]["compiles"] == 1 and first["after_render_multi"]["disk_writes"] == 1
    assert first["after_render_multi"]["module_loads"] == 1  # one device: one module, the second handle hits it
    assert first["after_handles"]["compiles"] == 1 and first["after_handles"]["module_loads"] == 1
    assert os.listdir(tmp_path / "co")
    second = probe()
    print("second process", second)
    assert second["after_handles"]["compiles"] == 0 and second["after_render_multi"]["disk_hits"] == 1
    # a cold render_multi in a new process compiles nothing (the counters above); its wall time is printed for
    # the record only (the process's first module load and allocations vary by box: bench.py reports the
    # phases of a second process's render_multi, render_multi_phases_second_process)
    # (no bound on it here: it depends on the box's load; bench.py reports the phases)
    print("second process: cold %.1f ms, warm %.1f ms" % (second["cold_ms"], second["warm_ms"]))
    # a corrupt cached object (its payload checksum fails) is dropped and compiled again, and renders
    co = [f for f in os.listdir(tmp_path / "co") if f.endswith(".co")]
    assert len(co) == 1
    path = tmp_path / "co" / co[0]
    data = bytearray(open(path, "rb").read())
    data[-100] ^= 0xFF
    open(path, "wb").write(bytes(data))
    third = probe()
    print("third process (corrupt cache)", third)
    assert third["after_render_multi"]["compiles"] == 1 and third["after_render_multi"]["disk_hits"] == 0
    assert third["after_render_multi"]["disk_writes"] == 1


def test_gpu_matches_oracle_on_cfg4_rows(built):
    """cfg4 stand-in: bounding_boxes (6 dragons, 140 940 triangles, BVH) at 800x1000 with a 4x4 CMJ
    grid — row bands against the oracle at 1e-4 and with identical 16-bit PPM values (the reference is pinned at
    100x125x16 by the bounding_boxes_100x125_4x4 golden)."""
    import oracle
    name = "bounding_boxes_800x1000_4x4"
    for rows in ((400, 404), (700, 703)):
        gpu = renderer(name).render(*rows)
        cpu = oracle.render(load_scene(name), *rows, threads=16)
        assert np.abs(gpu - cpu).max() <= TOL, rows
        assert encode_band(gpu) == encode_band(cpu), rows  # (the band's 16-bit PPM values identical)


def test_path_length_limit_is_refused(built, tmp_path):
    """Path lengths beyond the engine's 12-bit path-node code are refused with the reason."""
    import ctypes
    from fast_ray_tracer_amd.runtime import GpuRenderer, host_lib
    sc = load_scene("checkered_sphere_200")
    lib = host_lib()
    lib.frt_world_path_length.restype = ctypes.c_int
    lib.frt_world_path_length.argtypes = [ctypes.c_void_p, ctypes.c_int]
    old = lib.frt_world_path_length(sc.world, 12)
    try:
        with pytest.raises(RuntimeError, match="path-length 12 is not supported"):
            GpuRenderer(sc)
    finally:
        lib.frt_world_path_length(sc.world, old)
    GpuRenderer(sc).close()


def _render_env(name, env, **kw):
    """Render with environment switches that the engine reads at upload."""
    from fast_ray_tracer_amd.runtime import GpuRenderer
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        r = GpuRenderer(load_scene(name))
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    try:
        return r.render(**kw)
    finally:
        r.close()


def _render_frame_env(name, env, **kw):
    """Render with environment switches that the engine reads per frame (set around the render only)."""
    from fast_ray_tracer_amd.runtime import GpuRenderer
    r = GpuRenderer(load_scene(name))
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return r.render(**kw)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
        r.close()


@pytest.mark.parametrize("name", ["cornell_direct_64_4x4", "reflect_refract_test_150", "patterns_160x80",
                                  "csg_noshadow_glass_64x48"])
def test_lazy_ambient_equals_stored_surface(built, name):
    """Without GI the path nodes no light sample reaches are not written by k_shade: k_combine computes their
    ambient terms where it would read them (frt_engine.hip ambient_node). The canvas must equal the one with
    every node's terms stored (FRT_SHADE_LAZY=0), bit for bit — patterned materials (per-node colours) too."""
    lazy = _render_frame_env(name, {"FRT_SHADE_LAZY": "1"})
    stored = _render_frame_env(name, {"FRT_SHADE_LAZY": "0"})
    assert np.array_equal(lazy, stored)


def test_gather_queue_equals_static_ranges(built):
    """The final-gather estimate's request queue (k_gather_est's work counter) only schedules: the GI canvas
    at one seed must equal the one with fixed request ranges per wave (FRT_GATHER_QUEUE=0), bit for bit."""
    queued = _render_frame_env("cornell_gi_24", {"FRT_GATHER_QUEUE": "1"})
    ranges = _render_frame_env("cornell_gi_24", {"FRT_GATHER_QUEUE": "0"})
    assert np.isfinite(queued).all()
    assert np.array_equal(queued, ranges)


def test_gather_order_equals_request_order(built):
    """The final-gather estimate's requests sorted by the Morton key of their points and dealt to the XCD groups
    (k_gather_keys, perm) only reorder independent queries: the GI canvas must equal the one estimated in gather
    order (FRT_GATHER_SORT=0), bit for bit."""
    ordered = _render_frame_env("cornell_gi_24", {"FRT_GATHER_SORT": "1"})
    plain = _render_frame_env("cornell_gi_24", {"FRT_GATHER_SORT": "0"})
    assert np.isfinite(ordered).all()
    assert np.array_equal(ordered, plain)


def test_gather_rays_jit_equals_generic_walk(built):
    """The final gather's hemisphere rays through the scene-specialised closest hit (frt_jit_trace with k_trace_redo
    for the rays it cannot decide; the default since round 6) must give the GI canvas of the generic walk
    (FRT_GATHER_JIT=0), bit for bit: the hit records are the same, only the kernel that finds them changes."""
    jit = _render_frame_env("cornell_gi_24", {"FRT_GATHER_JIT": "1"})
    plain = _render_frame_env("cornell_gi_24", {"FRT_GATHER_JIT": "0"})
    assert np.isfinite(jit).all()
    assert np.array_equal(jit, plain)


@pytest.mark.parametrize("name", ["bounding_boxes_800x1000_4x4", "bounding_boxes_100x125_4x4", "teapot_low_100",
                                  "nave_120x150_4x4", "degenerate_mesh_48"])
def test_mesh_search_equals_generic_walk(built, name):
    """Mesh subtrees (groups of triangles, frt_traverse.hpp MeshDesc) are searched per lane in a BVH of their
    own, closest hit and the shadow walk's first-in-pre-order entry alike; the answer must be the generic
    walk's (which follows the reference's group tree and box tests), every pixel bit for bit. cfg4's
    stand-in at full size (800x1000, 4x4 CMJ: 6 dragons, 140 940 triangles) and the mesh goldens."""
    fast = _render_env(name, {"FRT_MESH": "1"})
    plain = _render_env(name, {"FRT_MESH": "0"})
    assert np.array_equal(fast, plain)


def test_math_core_sequences_bit_identical(built):
    """The core binary64 sequences (frt_math.hpp sqrt_core / recip_core: the compiler's sequences without their
    range steps) give the compiler's own sqrt and division results bit for bit (normalize3), and the
    shading's Newton-refined estimates (rsqrt_nr, recip_shade, div_shade) stay within 2^-46 relative of the
    IEEE operations, on 4M lanes of vectors spanning 2^-320..2^320 (fast path and fallback waves)."""
    import ctypes
    from fast_ray_tracer_amd.runtime import host_lib
    lib = host_lib()
    lib.frt_math_selftest.restype = ctypes.c_int64
    lib.frt_math_selftest.argtypes = [ctypes.c_int64, ctypes.c_uint64]
    for seed in (1, 0x5eed):
        assert lib.frt_math_selftest(1 << 22, seed) == 0


@pytest.mark.parametrize("name,rows", [("cornell_shipped_48_4x4", None), ("cornell_gi_24", None),
                                       ("cornell_shipped_1920x1080_8x8", (520, 528))])
def test_row_sorted_shading_equals_list_order(built, name, rows):
    """With a multi-row light (the shipped 65 535-row cache) the lit nodes are shaded in the order of the light row
    their shading draw picks (k_lit_stage / k_lit_rows and a radix sort), so a wave mostly shares one row and reads it through the
    scalar cache. Each lane still shades its own node, so the canvas equals the one in list order (FRT_SHADE_SORT=0)
    bit for bit: the shipped direct configuration, a GI one and a band of the shipped 1920x1080x64 frame."""
    kw = {} if rows is None else {"row_begin": rows[0], "row_end": rows[1]}
    sorted_ = _render_env(name, {"FRT_SHADE_SORT": "1"}, **kw)
    plain = _render_env(name, {"FRT_SHADE_SORT": "0"}, **kw)
    assert np.isfinite(sorted_).all() and sorted_[:, :, :3].max() > 0
    assert np.array_equal(sorted_, plain)
    # the row-ordered shading's three modes (frt_engine.hip FRT_SHADE_STAGE), each set explicitly: 2 (the default)
    # reads the node records in row order and writes its triples in row order (combine through spos); 1 also stages
    # the records in list order first (k_lit_stage) and shades from the staged copies; 0 reads and writes by node,
    # as round 5 did
    for mode in ("0", "1", "2"):
        other = _render_env(name, {"FRT_SHADE_SORT": "1", "FRT_SHADE_STAGE": mode}, **kw)
        assert np.array_equal(other, plain), mode


def test_render_multi_keeps_handles_between_calls(built):
    """render_multi keeps the last call's device handles (host/frt_render.c g_kept): a call with the same flattened
    scene and devices renders on them without an upload; another scene or device list releases them first. The
    canvases equal fresh uploads bit for bit (FRT_RM_KEEP=0), through a sequence that switches scenes and device
    lists, and the reuse shows in the phases (no upload time on a repeated call)."""
    from fast_ray_tracer_amd.runtime import release_render_multi, render_multi, render_multi_phases
    a, b = load_scene("cornell_direct_64_4x4"), load_scene("checkered_sphere_200")
    saved = os.environ.get("FRT_RM_KEEP")
    try:
        os.environ["FRT_RM_KEEP"] = "0"
        ref_a, ref_b = render_multi(a, devices="0"), render_multi(b, devices="0")
        ref_a2 = render_multi(a, devices="0,0")
        os.environ["FRT_RM_KEEP"] = "1"
        outs = []
        for sc, devs in ((a, "0"), (a, "0"), (b, "0"), (b, "0"), (a, "0,0"), (a, "0,0"), (a, "0")):
            outs.append(render_multi(sc, devices=devs))
            if len(outs) in (2, 4, 6):  # (a repeat of the previous call: the kept handles, no upload)
                assert render_multi_phases()["upload"] == 0.0, render_multi_phases()
            if len(outs) in (1, 3, 5, 7):
                assert render_multi_phases()["upload"] > 0.0, render_multi_phases()
        # an upload-time knob changed between two calls with the same scene: the kept handles (built under the old
        # knobs) are not reused; the same knobs again reuse the new ones; frt_render_multi_release drops them
        os.environ["FRT_JIT_BEAM"] = "0"
        outs.append(render_multi(a, devices="0"))
        assert render_multi_phases()["upload"] > 0.0, render_multi_phases()
        outs.append(render_multi(a, devices="0"))
        assert render_multi_phases()["upload"] == 0.0, render_multi_phases()
        del os.environ["FRT_JIT_BEAM"]
        release_render_multi()
        release_render_multi()  # (nothing kept: a no-op)
        outs.append(render_multi(a, devices="0"))
        assert render_multi_phases()["upload"] > 0.0, render_multi_phases()
    finally:
        os.environ.pop("FRT_JIT_BEAM", None)
        if saved is None:
            os.environ.pop("FRT_RM_KEEP", None)
        else:
            os.environ["FRT_RM_KEEP"] = saved
    for got, ref in zip(outs, (ref_a, ref_a, ref_b, ref_b, ref_a2, ref_a2, ref_a, ref_a, ref_a, ref_a)):
        assert np.array_equal(got, ref)


def test_render_multi_concurrent_calls(built):
    """render_multi's kept handles and phases are process-wide: two Python threads calling it at once (ctypes drops
    the GIL) are serialised by its lock and both get the right canvas."""
    import threading
    from fast_ray_tracer_amd.runtime import render_multi
    a, b = load_scene("cornell_direct_64_4x4"), load_scene("checkered_sphere_200")
    ref = {0: render_multi(a, devices="0"), 1: render_multi(b, devices="0")}
    got, errs = {}, []

    def run(k, sc):
        try:
            for _ in range(3):
                got.setdefault(k, []).append(render_multi(sc, devices="0"))
        except Exception as e:  # (reported below)
            errs.append(e)

    ts = [threading.Thread(target=run, args=(0, a)), threading.Thread(target=run, args=(1, b))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    for k in (0, 1):
        assert len(got[k]) == 3 and all(np.array_equal(g, ref[k]) for g in got[k])


def test_render_multi_canvas_is_pinned_and_pooled(built):
    """render_multi's canvas array is page-locked and pooled (host/frt_canvas.c frt_canvas_alloc_pinned): a freed
    canvas's array is taken again by the next canvas of the same size, never while a canvas still holds it; the array
    runtime.render_multi returns is the canvas itself (no copy) and its canvas is freed when it is collected."""
    import ctypes
    import gc
    from fast_ray_tracer_amd.runtime import host_lib, release_render_multi, render_multi
    lib = host_lib()
    vp = ctypes.c_void_p
    lib.frt_canvas_alloc_pinned.restype = vp
    lib.frt_canvas_alloc_pinned.argtypes = [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_bool, vp]
    lib.canvas_free.argtypes = [vp]
    lib.frt_canvas_data.restype = vp
    lib.frt_canvas_data.argtypes = [vp]
    release_render_multi()  # (an empty pool)
    c1 = lib.frt_canvas_alloc_pinned(64, 32, False, None)
    c2 = lib.frt_canvas_alloc_pinned(64, 32, False, None)
    a1, a2 = lib.frt_canvas_data(c1), lib.frt_canvas_data(c2)
    assert a1 and a2 and a1 != a2
    lib.canvas_free(c1)
    c3 = lib.frt_canvas_alloc_pinned(64, 32, False, None)
    assert lib.frt_canvas_data(c3) == a1  # (c1's array, from the pool)
    c4 = lib.frt_canvas_alloc_pinned(16, 16, False, None)  # (another size, the pool empty: a fresh array)
    assert lib.frt_canvas_data(c4) not in (a1, a2)
    for c in (c2, c3, c4):
        lib.canvas_free(c)
    sc = load_scene("cornell_direct_64_4x4")
    x = render_multi(sc, devices="0")
    y = render_multi(sc, devices="0")
    px = x.ctypes.data
    assert y.ctypes.data != px and np.array_equal(x, y)
    del x
    gc.collect()
    z = render_multi(sc, devices="0")
    assert z.ctypes.data == px and np.array_equal(z, y)
    release_render_multi()


@pytest.mark.parametrize("name,rows", [("reflect_refract_test_150", None), ("cornell_direct_64_4x4", None),
                                       ("cornell_gi_24", None), ("cornell_shipped_48_4x4", None),
                                       ("cornell_direct_1920x1080_8x8", (700, 708)),
                                       ("csg_noshadow_glass_64x48", None)])
def test_queue_order_equals_segment_order(built, name, rows):
    """The secondary levels' nodes in parent order (FRT_QUEUE_SORT): 2 (default) children at fixed slots n * slot +
    node compacted in order, 1 the segmented queue radix-sorted by (slot, parent), 0 the segments' append order.
    Node order decides only which nodes share a wave or a beam tile, never what a node computes (keys carry the
    sample and heap code, the combine writes through parent and slot), so the canvases are equal bit for bit:
    reflection and refraction, a GI scene, the multi-row light and a band of the headline frame."""
    kw = {} if rows is None else {"row_begin": rows[0], "row_end": rows[1]}
    ref = _render_env(name, {"FRT_QUEUE_SORT": "0"}, **kw)
    assert np.isfinite(ref).all() and ref[:, :, :3].max() > 0
    for mode in ("1", "2"):
        assert np.array_equal(_render_env(name, {"FRT_QUEUE_SORT": mode}, **kw), ref), mode
