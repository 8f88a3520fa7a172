"""The shadow pass's per-node columns (frt_shadow.hpp HeadCols): over_point as three columns of the level's capacity,
the key column only where a key cannot be derived (levels >= 1, strips of views, GI), the level-0 key derived from
the batch and the node index (frt_camera.hpp camera_key), and "the node has a hit" read from the path-node record's
material word.

Every value is the one the array-of-structs head held, so GPU canvases are compared with the CPU oracle under the
parity tests' bound (1e-4 per channel), and two GPU renders of one frame are compared bit for bit: however the frame
is cut into batches, node ranges or interleaved rows. The shapes are small on purpose: levels of fewer than 64 nodes,
levels that are no multiple of a wave, batches that end inside a 64-node tile.
"""
import os

import numpy as np
import pytest

from conftest import golden_index, load_scene

pytestmark = pytest.mark.gpu

TOL = 1e-4  # (tests/test_gpu_parity.py)


def _renderer(scene, env=None):
    """A renderer of `scene` (a Scene or a View) uploaded under environment switches that are read at upload."""
    from fast_ray_tracer_amd.runtime import GpuRenderer
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return GpuRenderer(scene)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


_oracle = {}


def _cpu(view):
    """The oracle's frame of a view, computed once and shared (never written to)."""
    import oracle
    if view.name not in _oracle:
        img = oracle.render(view)
        img.setflags(write=False)
        _oracle[view.name] = img
    return _oracle[view.name]


def _cuts(r, full, spp, **kw):
    """`full` again in batches that end inside a wave and inside a 64-node tile, and as interleaved rows."""
    for batch in (7 * spp, 1000):  # (whole pixels per batch: 7 pixels, and 1000 // spp pixels)
        assert np.array_equal(full, r.render(batch_samples=batch, **kw)), batch
    for n in (1, 3):
        for k in range(n):
            assert np.array_equal(full[k::n], r.render(k, None, n, **kw)), (n, k)
            assert np.array_equal(full[k::n], r.render(k, None, n, batch_samples=1000, **kw)), (n, k)


# (name, eye, target, hsize, vsize, usteps, vsteps)
ODD = [
    ("cornell_direct_64_4x4", (0.3, 0.2, -2.0), (0, 0, 0), 30, 17, 3, 3),  # 4 590 nodes: 71 waves and 46 lanes
    ("cornell_direct_64_4x4", (0.3, 0.2, -2.0), (0, 0, 0), 5, 3, 1, 1),    # 15 nodes: one partial wave
]


@pytest.mark.parametrize("name,eye,to,w,h,u,v", ODD)
def test_odd_levels_match_the_oracle(built, name, eye, to, w, h, u, v):
    """A level whose node count is no multiple of 64, and one of fewer than 64 nodes: the columns' stride is the
    level's capacity, not its node count, and the last wave is partial."""
    base = load_scene(name)
    view = base.view(eye, to, hsize=w, vsize=h, usteps=u, vsteps=v, name="%s_%dx%d_%dx%d" % (name, w, h, u, v))
    r = _renderer(view)
    try:
        gpu, st = r.render(stats=True)
        cpu = _cpu(view)
        diff = np.abs(gpu - cpu)
        print(f"{view.name}: max|d|={diff.max():.3e} hits {st.hits} of {st.primary_rays + st.secondary_rays} nodes")
        assert st.errors == 0 and st.primary_rays == w * h * u * v and st.primary_rays % 64 != 0
        assert gpu.shape == cpu.shape == (h, w, 4) and gpu[:, :, :3].max() > 0
        assert diff.max() <= TOL
        _cuts(r, gpu, u * v)
    finally:
        r.close()


def test_generic_shadow_walk_reads_the_columns(built):
    """The generic k_shadow (shadow_lane) on the odd-sized frame: FRT_JIT=0 at upload, against the oracle and, bit for
    bit, against the scene-specialised kernels' frame."""
    name, eye, to, w, h, u, v = ODD[0]
    view = load_scene(name).view(eye, to, hsize=w, vsize=h, usteps=u, vsteps=v,
                                 name="%s_%dx%d_%dx%d" % (name, w, h, u, v))
    rg, rj = _renderer(view, {"FRT_JIT": "0"}), _renderer(view, {"FRT_JIT": "1"})
    try:
        generic, st_g = rg.render(stats=True)
        jit, st_j = rj.render(stats=True)
        assert st_g.shadow_jit == 0 and st_j.shadow_jit == 1
        diff = np.abs(generic - _cpu(view))
        print(f"{view.name} generic walk: max|d|={diff.max():.3e}")
        assert diff.max() <= TOL
        assert np.array_equal(generic, jit)
        _cuts(rg, generic, u * v)
    finally:
        rg.close()
        rj.close()


def test_derived_level0_key_does_not_depend_on_the_cut(built):
    """cornell_shipped_48_4x4: the multi-row light, whose cache row a node's key picks (the shadow pass's draw and the
    shading's). With such a light level 0 keeps its key column (the per-ray kernel reads it in every lane);
    FRT_HEAD_KEY0=0, read per frame, makes level 0 store none, so every reader derives the keys from the batch and
    the node index. Stored or derived, in one batch, in batches that end inside a tile, in node ranges of the shadow
    pass (FRT_JIT_MAX_PAIRS, read per launch), in the row interleaves of stride 1 and 3 and under the generic walk:
    the same bits at one seed."""
    name = "cornell_shipped_48_4x4"
    sc = load_scene(name)
    seed = 20260
    saved = os.environ.pop("FRT_HEAD_KEY0", None)
    r = _renderer(sc)
    try:
        full, st = r.render(seed=seed, stats=True)
        assert st.errors == 0 and st.shadow_jit == 1
        assert np.isfinite(full).all() and full[:, :, :3].max() > 0
        assert not np.array_equal(full, r.render(seed=seed + 1))  # (the rows are drawn: the key matters)
        _cuts(r, full, sc.spp, seed=seed)
        os.environ["FRT_HEAD_KEY0"] = "0"
        _cuts(r, full, sc.spp, seed=seed)
        os.environ["FRT_JIT_MAX_PAIRS"] = "4099"
        _cuts(r, full, sc.spp, seed=seed)
    finally:
        os.environ.pop("FRT_JIT_MAX_PAIRS", None)
        os.environ.pop("FRT_HEAD_KEY0", None)
        r.close()
    rg = _renderer(sc, {"FRT_JIT": "0"})
    try:
        assert np.array_equal(full, rg.render(seed=seed))
        os.environ["FRT_HEAD_KEY0"] = "0"
        assert np.array_equal(full, rg.render(seed=seed))
        assert np.array_equal(full[1::3], rg.render(1, None, 3, seed=seed, batch_samples=1000))
    finally:
        os.environ.pop("FRT_HEAD_KEY0", None)
        if saved is not None:
            os.environ["FRT_HEAD_KEY0"] = saved
        rg.close()


def test_secondary_levels_and_misses(built):
    """Two glass spheres (reflective, Tr 0.9) in front of a wall, seen from the side so that half the frame is sky:
    primary and secondary misses (no head words are written for them: the material word of the path-node record
    says so) and the stored key column of the levels >= 1. Against the oracle, and the same bits for every cut."""
    base = load_scene("reflect_refract_test_150")
    view = base.view((5.0, 0.5, -0.5), (0, 0, 0), hsize=45, vsize=31, name="reflect_refract_side_45x31")
    r = _renderer(view)
    try:
        gpu, st = r.render(stats=True)
        cpu = _cpu(view)
        nodes = st.primary_rays + st.secondary_rays
        black = int((gpu[:, :, :3].sum(axis=-1) == 0).sum())
        diff = np.abs(gpu - cpu)
        print(f"{view.name}: max|d|={diff.max():.3e} nodes {nodes} hits {st.hits} black pixels {black}")
        assert st.errors == 0 and st.secondary_rays > 0
        assert 0 < black < 45 * 31  # primary misses (1 spp: a missed pixel is exactly black) and hits
        assert nodes - st.hits > black  # more misses than black pixels: secondary rays missed too
        assert diff.max() <= TOL
        _cuts(r, gpu, 1)
    finally:
        r.close()


def _refs(name):
    from conftest import GOLDEN
    return np.load(os.path.join(GOLDEN, golden_index()[name]["canvas"]))["refs"]


def test_gi_readers(built):
    """cornell_gi_24, the smallest GI golden: the shading, gather and photon kernels read over_point and the key
    through the path-node record (with GI level 0 stores its keys: the gather kernels have no batch to derive them
    from). Under tests/test_gpu_stochastic.py's gate against the reference's six renders, and one seed's frame the
    same bits in two batch sizes."""
    name = "cornell_gi_24"
    refs = _refs(name)
    k = refs.shape[0]
    sc = load_scene(name)
    r = _renderer(sc)
    try:
        gpus = [r.render(seed=sd) for sd in (0x5EED, 0xC0FFEE, 11, 12)]
        assert np.array_equal(gpus[0], r.render(seed=0x5EED, batch_samples=1000))
        assert np.array_equal(gpus[0], r.render(seed=0x5EED, batch_samples=7 * sc.spp))
    finally:
        r.close()
    gpus = [g[:, :, :3] for g in gpus]
    rmse = lambda a, b: float(np.sqrt(np.mean((a - b) ** 2)))
    pairs = [(i, j) for i in range(k) for j in range(i + 1, k)]
    d_ref = np.mean([rmse(refs[i], refs[j]) for i, j in pairs])
    d_gpu = np.mean([rmse(g, refs[i]) for g in gpus for i in range(k)])
    a_ref = np.mean([np.abs(refs[i] - refs[j]).mean() for i, j in pairs])
    a_gpu = np.mean([np.abs(g - refs[i]).mean() for g in gpus for i in range(k)])
    m_ref = np.array([x.mean() for x in refs])
    m_gpu = np.array([g.mean() for g in gpus])
    tol = 4 * m_ref.std(ddof=1) * np.sqrt(1.0 / k + 1.0 / len(gpus)) + 1e-12
    bias = float(m_gpu.mean() - m_ref.mean())
    print(f"{name}: mad ratio={a_gpu / a_ref:.3f} rmse ratio={d_gpu / d_ref:.3f} bias={bias:.3e} (tol {tol:.3e})")
    assert d_ref > 0 and a_ref > 0
    assert a_gpu <= 1.15 * a_ref
    assert d_gpu <= 1.6 * d_ref
    assert abs(bias) <= tol
