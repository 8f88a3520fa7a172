"""The device's first hits (GpuRenderer.render_features at 1 x 1 steps: depth is the closest hit's t, normal is
comps.normalv, node the leaf) value by value against two references: the CPU oracle's first hits (oracle.first_hits,
CSG scenes included) and the extended-precision reference of tests/first_hit_ref.py, on the views of
tests/first_hit_views.py. tests/test_first_hit_cpu.py pins the two references against each other on the CPU.

Against the oracle: coverage, node and material on every sample; depth and normal bit for bit wherever the hit leaf
is not a toroid and its material has no bump map (everything built from + - * / sqrt). On toroid
hits solve_cubic calls cbrt, acos and cos, where the device's and glibc's libm may differ: the difference is printed
and bounded through the reference. Against the reference, over its decided samples: the hit mask and leaf are equal,
t and the normal are within the recorded per-type bounds (tests/golden/first_hit_bounds.json), the toroid within
4 x its bound."""
import numpy as np
import pytest

import feature_ref
import first_hit_ref as ref
import first_hit_views as views

pytestmark = pytest.mark.gpu

TOROID_FACTOR = 4.0
CSG_KEYS = ["csg:" + n for n in views.CSG_VIEWS]
_renderers = {}


@pytest.fixture(scope="module")
def renderer_of(built):
    """One renderer per scene for the module; set_camera per view."""
    from fast_ray_tracer_amd.runtime import GpuRenderer

    def get(key):
        scene = views.scene_of(key)
        if scene.name not in _renderers:
            _renderers[scene.name] = GpuRenderer(scene)
        return _renderers[scene.name]

    yield get
    for r in _renderers.values():
        r.close()
    _renderers.clear()


@pytest.fixture(scope="module")
def bounds():
    return views.load_bounds()


def _features(renderer_of, key):
    view = views.view_of(key)[0]
    r = renderer_of(key)
    r.set_camera(view)
    f, st = r.render_features(stats=True)
    assert st.errors == 0
    return view, f


def _materials(view):
    from fast_ray_tracer_amd.runtime import scene_nodes
    tree = ref.flat_tree(view)
    nodes = scene_nodes(view)
    return nodes, tree["bump"]


def _against_oracle(key, view, f):
    """coverage, ids and (off toroids and bump maps) depth and normal against the oracle, at 1 x 1 steps; returns the
    largest |t_gpu - t_oracle| / max(1, t) and |n_gpu - n_oracle| over the toroid hits (None without any)."""
    t, normal, leaf = (a[:, :, 0] for a in views.oracle_of(key))
    nodes, bump = _materials(view)
    hit = leaf >= 0
    assert hit.any()
    assert np.array_equal(f["coverage"], hit.astype(np.float64))
    assert np.array_equal(f["node"], leaf)
    assert np.array_equal(f["material"], np.where(hit, nodes["material"][np.maximum(leaf, 0)], -1))
    types = np.where(hit, nodes["type"][np.maximum(leaf, 0)], -1)
    exact = hit & (types != ref.TOROID) & ~bump[np.maximum(f["material"], 0)]
    differ = exact & ((f["depth"] != t) | (f["normal"] != normal).any(axis=2))
    if differ.any():
        i = tuple(np.argwhere(differ)[0])
        print("%s: %d of %d samples differ from the oracle; first at %s, leaf %d (type %d): t %r / %r, normal %r / %r"
              % (key, differ.sum(), exact.sum(), i, leaf[i], types[i], f["depth"][i], t[i], f["normal"][i], normal[i]))
    assert np.array_equal(f["depth"][exact], t[exact]) and np.array_equal(f["normal"][exact], normal[exact])
    tor = hit & (types == ref.TOROID)
    if not tor.any():
        return None
    dt = (np.abs(f["depth"][tor] - t[tor]) / np.maximum(1, t[tor])).max()
    dn = np.abs(f["normal"][tor] - normal[tor]).max()
    print("%s: %d toroid hits, |t_gpu - t_oracle| / max(1, t) <= %.3e, |n_gpu - n_oracle| <= %.3e, %d bit-identical"
          % (key, tor.sum(), dt, dn, (f["depth"][tor] == t[tor]).sum()))
    return float(dt), float(dn)


def _limit(bounds, name, what):
    return bounds["types"][name][what] * (TOROID_FACTOR if name == "toroid" else 1.0)


@pytest.mark.parametrize("key", [k for k in views.KEYS if k != "fixture:a3"])
def test_device_first_hits(renderer_of, bounds, key):
    view, f = _features(renderer_of, key)
    _against_oracle(key, view, f)
    # the reference, on its decided samples
    r = {k: (v[:, :, 0] if k != "branch" else v) for k, v in views.reference_of(key).items()}
    t = np.where(f["node"] >= 0, f["depth"], -1.0)
    mask_ok, leaf_ok, dev = views.deviations(r, t, f["normal"], f["node"])
    assert mask_ok and leaf_ok
    for name, d in sorted(dev.items()):
        lt, ln = _limit(bounds, name, "t"), _limit(bounds, name, "normal")
        print("%s %-16s %5d hits  |t_gpu - t_ref| / max(1, t) %.3e (%.2f of the limit)  |n_gpu - n_ref| %.3e (%.2f)"
              % (key, name, d["hits"], d["t"], d["t"] / lt, d["normal"], d["normal"] / ln))
        assert d["t"] <= lt and d["normal"] <= ln, (name, d)


@pytest.mark.parametrize("key", CSG_KEYS)
def test_device_first_hits_csg(renderer_of, key):
    view, f = _features(renderer_of, key)
    _against_oracle(key, view, f)


def test_ordered_means(renderer_of, bounds):
    """The overview at 3 x 3 steps: coverage equals the reference's hits / spp, depth and normal are within the
    per-type bounds of feature_ref.ordered_mean of the reference's per-sample values, on the pixels without an
    undecided sample. A pixel's limit is the largest of its samples' limits (a mean of deviations is no larger than
    their maximum) plus the rounding of the two binary64 sums: 2 spp 2^-53 of the largest term."""
    key = "fixture:a3"
    view, f = _features(renderer_of, key)
    r = views.reference_of(key)
    spp = view.spp
    clean = ~r["undecided"].any(axis=2)
    hit = r["hit"]
    assert clean.mean() >= 1 - spp * views.MAX_UNDECIDED
    cov = hit.sum(axis=2) / np.float64(spp)
    assert np.array_equal(f["coverage"][clean], cov[clean])
    t64, n64 = r["t"].astype(np.float64), r["normal"].astype(np.float64)
    lim_t, lim_n = np.zeros(hit.shape), np.zeros(hit.shape)
    for typ, name in ref.TYPE_NAMES.items():
        lim_t = np.where(r["type"] == typ, _limit(bounds, name, "t"), lim_t)
        lim_n = np.where(r["type"] == typ, _limit(bounds, name, "normal"), lim_n)
    tmax = np.where(hit, t64, 0.0).max(axis=2)
    allow_t = (lim_t * np.maximum(1, t64) * hit).max(axis=2) + 2 * spp * 2.0 ** -53 * tmax
    allow_n = (lim_n * hit).max(axis=2) + 2 * spp * 2.0 ** -53
    d_depth = np.abs(f["depth"] - feature_ref.ordered_mean(np.where(hit, t64, 0.0), hit))
    d_normal = np.abs(f["normal"] - feature_ref.ordered_mean(np.where(hit[..., None], n64, 0.0), hit)).max(axis=2)
    mixed = clean & (np.array([len(set(p)) for p in r["leaf"].reshape(-1, spp)]).reshape(clean.shape) > 1)
    print("a3: %d clean pixels (%d with more than one leaf), depth within %.2f of its limit, normal within %.2f"
          % (clean.sum(), mixed.sum(), (d_depth / np.maximum(allow_t, 1e-300))[clean & (cov > 0)].max(),
             (d_normal / np.maximum(allow_n, 1e-300))[clean & (cov > 0)].max()))
    assert mixed.sum() >= views.MIN_HITS
    assert (d_depth[clean] <= allow_t[clean]).all() and (d_normal[clean] <= allow_n[clean]).all()
    first = np.where(hit.any(axis=2), np.take_along_axis(r["leaf"], hit.argmax(axis=2)[..., None], axis=2)[..., 0], -1)
    assert np.array_equal(f["node"][clean], first[clean])
