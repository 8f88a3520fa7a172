"""The engine's FRT_* knobs (fast_ray_tracer_amd/csrc/frt_knobs.hpp): read in one place, each with the lifetime of
its struct. An upload knob set around a handle's construction shapes that handle; a frame knob set around a render
shapes that frame; nothing is frozen for the life of the process.
"""
import contextlib
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_scene

SCENE = "cornell_direct_64_4x4"
CSRC = os.path.join(ROOT, "fast_ray_tracer_amd", "csrc")


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


def test_tile_size_follows_each_jit_check(built):
    """FRT_JIT_TILE is an upload knob: frt_jit_check reads it at every call, so one process generates the 64-node
    and the 32-node tile kernels in turn, and 64 again gives the first source back."""
    from fast_ray_tracer_amd.runtime import jit_check
    scene = load_scene(SCENE)
    srcs = []
    for tile in ("64", "32", "64"):
        with _env(FRT_JIT_TILE=tile):
            rc, log, src = jit_check(scene)
        assert rc == 0, log[-2000:]
        srcs.append(src)
    assert srcs[0] != srcs[1]
    assert srcs[2] == srcs[0]


def test_engine_reads_the_environment_in_one_file():
    """No engine source but frt_knobs.hpp reads the environment."""
    readers = []
    for f in sorted(os.listdir(CSRC)):
        with open(os.path.join(CSRC, f), errors="replace") as fh:
            if re.search(r"getenv", fh.read()):
                readers.append(f)
    assert readers == ["frt_knobs.hpp"]


@pytest.mark.gpu
def test_upload_knobs_follow_the_upload(built):
    """Two handles of one process, the tile size set around each construction only: the second has the smaller tiles
    (more tile pairs for the same nodes), and the canvases are equal."""
    from fast_ray_tracer_amd.runtime import GpuRenderer
    scene = load_scene(SCENE)
    out = []
    for tile in ("64", "32"):
        with _env(FRT_JIT_TILE=tile):
            r = GpuRenderer(scene)
        try:
            out.append(r.render(stats=True))
        finally:
            r.close()
    (img64, st64), (img32, st32) = out
    assert st64.shadow_jit == 1 and st32.shadow_jit == 1
    assert np.array_equal(img64, img32)
    assert st32.shadow_tile_pairs > st64.shadow_tile_pairs > 0


@pytest.mark.gpu
def test_frame_knobs_follow_the_frame(built):
    """One handle, FRT_JIT_MIN_PAIRS set around each render only: the beam stages run, are skipped (no level has
    2^40 pairs), and run again; the canvases are equal."""
    from fast_ray_tracer_amd.runtime import GpuRenderer
    r = GpuRenderer(load_scene(SCENE))
    try:
        out = []
        for min_pairs in ("0", "1099511627776", "0"):
            with _env(FRT_JIT_MIN_PAIRS=min_pairs):
                out.append(r.render(stats=True))
    finally:
        r.close()
    pairs = [st.shadow_tile_pairs for _, st in out]
    assert pairs[0] > 0 and pairs[1] == 0 and pairs[2] > 0, pairs
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][0], out[2][0])
