"""k_prepare's scalar path for waves whose lanes all hit one leaf (frt_engine.hip prepare_node, frt_shade.hpp
uniform_view; FRT_PREPARE_UNIFORM, default on).

The uniform path runs the same functions on the same values in the same order, with the leaf's node, transform
chain, primitive data and material read through the scalar cache: every canvas must equal the per-lane path's
(FRT_PREPARE_UNIFORM=0) bit for bit. The switch is read at upload, so each setting renders in a fresh process.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

_RENDER = r"""
import sys, numpy as np
sys.path.insert(0, {tests!r})
from conftest import load_scene
from fast_ray_tracer_amd.runtime import GpuRenderer
r = GpuRenderer(load_scene({name!r}))
img, st = r.render(stats=True, **{kw!r})
d = st.as_dict()
np.save({out!r}, img)
print("STATS", d["prepare_uniform_waves"], d["primary_rays"], d["secondary_rays"], d["hits"], d["errors"])
"""


def _render_process(name, env, out, **kw):
    """(canvas, [uniform waves, primary rays, secondary rays, hits, errors]) of a statistics frame in a fresh process."""
    here = os.path.dirname(os.path.abspath(__file__))
    penv = dict(os.environ)
    penv.pop("FRT_PREPARE_UNIFORM", None)
    penv.update(env)
    p = subprocess.run([sys.executable, "-c", _RENDER.format(tests=here, name=name, out=str(out), kw=kw)],
                       env=penv, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    stats = [ln.split()[1:] for ln in p.stdout.splitlines() if ln.startswith("STATS")][-1]
    return np.load(str(out)), [int(x) for x in stats]


def _both(name, tmp_path, nonblack=True, **kw):
    on, st_on = _render_process(name, {}, tmp_path / "on.npy", **kw)
    off, st_off = _render_process(name, {"FRT_PREPARE_UNIFORM": "0"}, tmp_path / "off.npy", **kw)
    print(name, "uniform waves", st_on[0], "of path nodes", st_on[1] + st_on[2], "hits", st_on[3])
    assert st_on[4] == 0 and st_off[4] == 0
    assert np.isfinite(on).all()
    if nonblack:
        assert float(on[..., :3].max()) > 0.0
    assert np.array_equal(on, off)
    assert st_off[0] == 0  # the switch keeps every wave on the per-lane path
    return st_on, st_off


@pytest.mark.gpu
@pytest.mark.parametrize("name", [
    "cornell_direct_64_4x4",        # 16 spp: four pixels per wave, both paths in one launch
    "cornell_direct_128_1x1",       # 1 spp: mostly mixed waves
    "group_test_150x50",            # transform chains two and three deep
    "csg_nested_96x64",             # CSG
    "teapot_low_100",               # smooth triangles: the (u, v) recomputation
    "bounding_boxes_100x125_4x4",
    "patterns_160x80",              # kPat
    "bump_map_100",
    "checkered_torus_120",          # leaf types with prim data
    "checkered_cylinder_120",
    "reflect_refract_test_150",     # secondary levels, misses, Schlick
    "cornell_shipped_48_4x4",       # the multi-row light: the key through the head
])
def test_uniform_path_equals_per_lane_path(built, name, tmp_path):
    st_on, _ = _both(name, tmp_path)
    if name == "cornell_direct_64_4x4":  # (walls wider than four pixels: the uniform path must have run)
        assert st_on[0] > 0


@pytest.mark.gpu
def test_uniform_path_on_headline_rows(built, tmp_path):
    """The headline at 64 spp: a level-0 wave is one pixel's samples. The band crosses object edges, so the waves on
    the uniform path stay below the number of waves that ran (per level ceil(nodes / 64); the levels below 0 hold
    the secondary rays, at most one partial wave per level, 11 levels at the most).

    Rows 400-408 of this frame are black in every build (981 544 of its 983 040 samples hit a surface no light
    sample reaches: the canvas is all zeros before this path existed too), so "not black" cannot hold there; it is
    asserted on rows 700-708 (the window's light on the floor) instead, with every other check on both bands."""
    _both("cornell_direct_1920x1080_8x8", tmp_path, row_begin=700, row_end=708)
    st_on, _ = _both("cornell_direct_1920x1080_8x8", tmp_path, nonblack=False, row_begin=400, row_end=408)
    uniform, primary, secondary = st_on[0], st_on[1], st_on[2]
    assert primary == 8 * 1920 * 64
    waves = (primary + 63) // 64 + ((secondary + 63) // 64 + 11 if secondary else 0)
    print("headline rows 400-408: uniform fraction of k_prepare waves >= %.4f" % (uniform / waves))
    assert 0 < uniform < waves
