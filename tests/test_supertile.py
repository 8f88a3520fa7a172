"""Super-tiles in the shadow hierarchy (FRT_JIT_SUPERTILE, csrc/frt_jit.hip and frt_engine.hip launch_shadow).

frt_jit_tile and frt_jit_sub first decide runs of 128 .. 1024 consecutive path nodes from the union of their tile
boxes (k_sup_boxes); frt_jit_split re-decides the (super-tile, sample) pairs they leave per 64-node tile of the run,
from the tile's own box and the pair's resume point; the later stages run as before. Every proof holds for the
narrower beams below it and the counts are integer sums, so each canvas equals, bit for bit, the one without
super-tiles (FRT_JIT_SUPERTILE=0) and the generic walk's (FRT_JIT=0). The split stage's own counters
(GpuRenderer.shadow_stages) show that it ran. The rays walked one by one are printed, not compared: a finer beam that
resumes from a coarser beam's point and flags may leave a slightly different set undecided.
"""
import contextlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import load_scene

_RENDER = r"""
import json, sys, numpy as np
sys.path.insert(0, {tests!r})
from conftest import load_scene
from fast_ray_tracer_amd.runtime import GpuRenderer
r = GpuRenderer(load_scene({name!r}))
img, st = r.render(stats=True, **{kw!r})
d = st.as_dict()
s = r.shadow_stages()
s["shadow_jit"] = d["shadow_jit"]
s["frame_tile_pairs"], s["frame_sub_pairs"] = d["shadow_tile_pairs"], d["shadow_sub_pairs"]
np.save({out!r}, img)
print("STAGES", json.dumps(s))
"""


def _render(name, env, out, **kw):
    """Render in a fresh process under `env` (tests/test_jit.py _render_env_process): the canvas and the stage
    counters of the frame."""
    here = os.path.dirname(os.path.abspath(__file__))
    penv = dict(os.environ, **env)
    p = subprocess.run([sys.executable, "-c", _RENDER.format(tests=here, name=name, out=str(out), kw=kw)],
                       env=penv, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    st = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("STAGES")][-1][7:])
    return np.load(str(out)), st


_generic = {}


def _generic_walk(name, tmp_path, **kw):
    """The generic walk's canvas, rendered once per scene and band; read-only for the cases that share it."""
    key = (name, tuple(sorted(kw.items())))
    if key not in _generic:
        img, st = _render(name, {"FRT_JIT": "0"}, tmp_path / "generic.npy", **kw)
        assert st["shadow_jit"] == 0
        img.setflags(write=False)
        _generic[key] = img
    return _generic[key]


def _check(name, env, tmp_path, **kw):
    """`env` (with a super-tile size) against the same settings without super-tiles and against the generic walk."""
    ref = _generic_walk(name, tmp_path, **kw)
    on, st_on = _render(name, env, tmp_path / "on.npy", **kw)
    off, st_off = _render(name, dict(env, FRT_JIT_SUPERTILE="0"), tmp_path / "off.npy", **kw)
    print(name, env, "rays walked one by one: with super-tiles %d, without %d" % (st_on["rays_walked"],
                                                                                 st_off["rays_walked"]))
    print(name, env, "stages", st_on)
    assert st_on["shadow_jit"] == 1 and st_off["shadow_jit"] == 1
    assert st_off["supertile"] == 0 and st_off["split_pairs"] == 0
    assert st_on["supertile"] == int(env["FRT_JIT_SUPERTILE"])
    assert st_on["split_pairs"] > 0 and st_on["split_launches"] > 0, st_on
    assert st_on["frame_tile_pairs"] > 0 and st_on["frame_sub_pairs"] > 0
    # (the first stage's lanes: a quarter and less of the tiles')
    assert st_on["tile_pairs"] < st_off["tile_pairs"]
    assert np.array_equal(on, off), (name, env)
    assert np.array_equal(on, ref), (name, env)


SCENES = ["cornell_direct_64_4x4", "cornell_shipped_48_4x4", "reflect_refract_test_150", "test_scene_120",
          "csg_ties_64x48"]

# (settings, the scenes each runs on): every setting on at least two scenes, every scene at the default size
CASES = [({"FRT_JIT_SUPERTILE": "256"}, SCENES),
         ({"FRT_JIT_SUPERTILE": "128"}, ["cornell_direct_64_4x4", "reflect_refract_test_150", "csg_ties_64x48"]),
         ({"FRT_JIT_SUPERTILE": "1024"}, ["cornell_direct_64_4x4", "reflect_refract_test_150", "cornell_shipped_48_4x4"]),
         ({"FRT_JIT_SUPERTILE": "256", "FRT_JIT_TILE": "16", "FRT_JIT_SUBTILE": "4"},
          ["cornell_direct_64_4x4", "test_scene_120", "cornell_shipped_48_4x4"]),
         ({"FRT_JIT_SUPERTILE": "256", "FRT_JIT_SUBTILE": "0"}, ["cornell_direct_64_4x4", "reflect_refract_test_150"]),
         ({"FRT_JIT_SUPERTILE": "256", "FRT_JIT_NODE_BEAM": "1"},
          ["cornell_direct_64_4x4", "cornell_shipped_48_4x4", "csg_ties_64x48"]),
         ({"FRT_JIT_SUPERTILE": "256", "FRT_JIT_NODE_MAJOR": "4"}, ["cornell_shipped_48_4x4", "test_scene_120"]),
         ({"FRT_JIT_SUPERTILE": "256", "FRT_JIT_MAX_PAIRS": "4099"},
          ["cornell_direct_64_4x4", "reflect_refract_test_150", "cornell_shipped_48_4x4"]),
         ({"FRT_JIT_SUPERTILE": "256", "FRT_JIT_ORDER": "2"}, ["cornell_direct_64_4x4", "csg_ties_64x48"]),
         ({"FRT_JIT_SUPERTILE": "256", "FRT_JIT_SUPERTILE_DEEP": "0"}, ["reflect_refract_test_150", "test_scene_120"]),
         ({"FRT_JIT_SUPERTILE": "256", "FRT_JIT_SUPERTILE_DEEP": "1"}, ["reflect_refract_test_150", "test_scene_120"])]


def _id(env):
    return ",".join("%s=%s" % (k[8:], v) for k, v in env.items())


@pytest.mark.gpu
@pytest.mark.parametrize("name,env", [pytest.param(n, e, id=n + "-" + _id(e)) for e, names in CASES for n in names])
def test_supertile_equals_tiles_and_generic_walk(built, name, env, tmp_path):
    _check(name, env, tmp_path)


@pytest.mark.gpu
def test_deep_levels_knob_selects_the_levels(built, tmp_path):
    """FRT_JIT_SUPERTILE_DEEP=0 keeps the super-tiles to level 0: fewer split lanes than with every level, more than
    none, on a scene with reflected and refracted levels."""
    name = "reflect_refract_test_150"
    _, deep = _render(name, {"FRT_JIT_SUPERTILE": "256", "FRT_JIT_SUPERTILE_DEEP": "1"}, tmp_path / "d.npy")
    _, top = _render(name, {"FRT_JIT_SUPERTILE": "256", "FRT_JIT_SUPERTILE_DEEP": "0"}, tmp_path / "t.npy")
    print("split lanes: every level %d, level 0 only %d" % (deep["split_pairs"], top["split_pairs"]))
    assert 0 < top["split_pairs"] < deep["split_pairs"]
    # (the deeper levels of the second frame tested tiles, not super-tiles)
    assert top["tile_pairs"] > deep["tile_pairs"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell_direct_64_4x4", "reflect_refract_test_150"])
@pytest.mark.parametrize("env", [{"FRT_JIT_SUPERTILE": "32", "FRT_JIT_TILE": "64"},
                                 {"FRT_JIT_SUPERTILE": "256", "FRT_JIT_SUB": "0"}], ids=_id)
def test_supertile_off_where_it_cannot_apply(built, name, env, tmp_path):
    """A super-tile no larger than the tile, or no sub-part stage: no split kernel, its counters at 0, the canvas the
    generic walk's."""
    ref = _generic_walk(name, tmp_path)
    img, st = _render(name, env, tmp_path / "x.npy")
    assert st["shadow_jit"] == 1 and st["frame_tile_pairs"] > 0
    assert st["supertile"] == 0 and st["split_pairs"] == 0 and st["split_launches"] == 0, st
    assert np.array_equal(img, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [{"row_begin": 400, "row_end": 408},
                                {"row_begin": 400, "row_end": 464, "row_stride": 8}], ids=["rows400-408", "stride8"])
def test_supertile_on_headline_rows(built, kw, tmp_path):
    """The headline workload (cornell 1920x1080, 8x8 CMJ): a band of rows, and rows 8 apart (consecutive nodes of
    rows that are not neighbours: large boxes, the same result), with super-tiles, without, and through the generic
    walk."""
    _check("cornell_direct_1920x1080_8x8", {"FRT_JIT_SUPERTILE": "256"}, tmp_path, **kw)


@pytest.mark.gpu
def test_supertile_on_shipped_band(built, tmp_path):
    """Rows 300 to 306 of the shipped frame (the multi-row light) at a fixed seed: super-tiles on against off."""
    kw = {"row_begin": 300, "row_end": 306, "seed": 0x5EED}
    name = "cornell_shipped_1920x1080_8x8"
    on, st_on = _render(name, {"FRT_JIT_SUPERTILE": "256"}, tmp_path / "on.npy", **kw)
    off, st_off = _render(name, {"FRT_JIT_SUPERTILE": "0"}, tmp_path / "off.npy", **kw)
    print("rays walked one by one: with super-tiles %d, without %d" % (st_on["rays_walked"], st_off["rays_walked"]))
    assert st_on["shadow_jit"] == 1 and st_on["split_pairs"] > 0 and st_off["split_pairs"] == 0
    assert np.array_equal(on, off)


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.mark.gpu
def test_supertile_follows_the_upload(built):
    """FRT_JIT_SUPERTILE is an upload knob: two handles of one process, the size set around each construction only.
    The second handle has the split stage, the first has none, and the canvases are equal."""
    from fast_ray_tracer_amd.runtime import GpuRenderer
    scene = load_scene("cornell_direct_64_4x4")
    out = []
    for sup in ("0", "256"):
        with _env(FRT_JIT_SUPERTILE=sup):
            r = GpuRenderer(scene)
        try:
            img = r.render(stats=True)[0]
            out.append((img, r.shadow_stages()))
        finally:
            r.close()
    (img0, st0), (img1, st1) = out
    assert st0["supertile"] == 0 and st0["split_pairs"] == 0
    assert st1["supertile"] == 256 and st1["split_pairs"] > 0
    assert st1["tile_pairs"] < st0["tile_pairs"]
    assert np.array_equal(img0, img1)


@pytest.mark.gpu
def test_supertile_is_part_of_the_generated_source(built):
    """The super-tile size is a literal of the generated source (and so of the code-object cache's key): each size
    gives another source with a split kernel, 0 gives none, and the same size gives the same source back."""
    from fast_ray_tracer_amd.runtime import jit_check
    scene = load_scene("cornell_direct_64_4x4")
    srcs = {}
    for sup in ("0", "128", "256", "1024", "256b"):
        with _env(FRT_JIT_SUPERTILE=sup[:-1] if sup.endswith("b") else sup):
            rc, log, src = jit_check(scene)
        assert rc == 0, log[-2000:]
        srcs[sup] = src
    assert "frt_jit_split(" not in srcs["0"]
    assert all("frt_jit_split(" in srcs[k] for k in ("128", "256", "1024"))
    assert len({srcs[k] for k in ("0", "128", "256", "1024")}) == 4
    assert srcs["256b"] == srcs["256"]
