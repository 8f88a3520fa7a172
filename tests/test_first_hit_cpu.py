"""The extended-precision first-hit reference (tests/first_hit_ref.py) against the CPU oracle's first hits
(oracle.first_hits), on the CPU: every view of tests/first_hit_views.py over the primitives fixture scene and the
CSG-free goldens. Over the decided samples the hit mask and the leaf are equal and t and the normal deviate by no more
than tests/golden/first_hit_bounds.json records (python tests/golden/make_first_hit_bounds.py); every type but the
toroid is within 1e-9 in t. The conditions on the views (undecided share, decided hits per listed type, decided
samples in the epsilon branches) are checked on the reference alone. tests/test_first_hit.py holds the device to the
same reference."""
import numpy as np
import pytest

import first_hit_ref as ref
import first_hit_views as views


def _mpf(x):
    import mpmath
    hi = float(x)
    return mpmath.mpf(hi) + mpmath.mpf(float(x - ref.LD(hi)))  # (a longdouble is two binary64 terms, exactly)


def test_quartic_roots_against_mpmath():
    """200 seeded rays through the two toroids of the fixture scene (r1 = 1, r2 = 0.35 and r1 = 0.6, r2 = 0.5), from
    outside and from inside the tube: the longdouble-refined real roots against mpmath.polyroots of the same
    coefficients at 50 digits: the same number of real roots, each within 1e-15 relative."""
    import mpmath
    rng = np.random.default_rng(20240607)
    worst, count, rays = 0.0, 0, 0
    with mpmath.workdps(50):
        while rays < 200:
            r1, r2 = ((1.0, 0.35), (0.6, 0.5))[rays % 2]
            if rays % 4 < 2:  # from outside towards a point of the centre circle's disc
                o = rng.normal(size=3)
                o = o / np.linalg.norm(o) * rng.uniform(2.0, 12.0)
                ang, rad = rng.uniform(0, 2 * np.pi), rng.uniform(0, r1 + r2)
                target = np.array([rad * np.cos(ang), rng.uniform(-r2, r2), rad * np.sin(ang)])
            else:  # from inside the tube
                ang = rng.uniform(0, 2 * np.pi)
                o = np.array([r1 * np.cos(ang), 0.0, r1 * np.sin(ang)]) + rng.uniform(-0.4, 0.4, size=3) * r2
                target = o + rng.normal(size=3)
            d = (target - o) / np.linalg.norm(target - o)
            c = ref.quartic_coeffs(o.astype(ref.LD), d.astype(ref.LD), ref.LD(r1), ref.LD(r2))
            roots, clear, clear_im, _ = ref.quartic_real_roots(c)
            exact = mpmath.polyroots([_mpf(x) for x in c[::-1]], maxsteps=500, extraprec=400)
            real = sorted(z.real for z in exact if abs(z.imag) <= mpmath.mpf(10) ** -30 * (1 + abs(z.real)))
            if not real:
                assert not roots
                continue
            rays += 1
            assert len(roots) == len(real), (o, d, roots, real)
            for x, y in zip(roots, real):
                worst = max(worst, float(abs(_mpf(x) - y) / abs(y)))
                count += 1
    print("quartic: %d roots of %d rays, worst relative deviation from mpmath %.3e" % (count, rays, worst))
    assert worst <= 1e-15


def test_reference_refuses_csg(built):
    from conftest import load_scene
    with pytest.raises(ValueError, match="CSG is out of scope"):
        ref.first_hits(load_scene("csg_ops_96x64"))


@pytest.fixture(scope="module")
def bounds():
    return views.load_bounds()


@pytest.mark.parametrize("key", views.KEYS)
def test_reference_against_oracle(built, bounds, key):
    view, types, branches = views.view_of(key)
    r = views.reference_of(key)
    t, normal, leaf = views.oracle_of(key)
    dec = ~r["undecided"]
    # the view's conditions, on the reference alone
    share = float(r["undecided"].mean())
    counts = {views.type_name(k): int((dec & (r["type"] == k)).sum()) for k in np.unique(r["type"][r["hit"]])}
    taken = {k: int((b & dec).sum()) for k, b in r["branch"].items()}
    print("%s %dx%dx%d: undecided %.4f, decided hits %s, branches %s" % (key, view.width, view.height, view.spp, share,
                                                                       counts, taken))
    assert share <= views.MAX_UNDECIDED
    for typ in types:
        assert counts.get(views.type_name(typ), 0) >= views.MIN_HITS, (views.type_name(typ), counts)
    for b in branches:
        assert taken[b] >= 1, (b, taken)
    assert r["hit"].any() and np.isfinite(r["t"].astype(np.float64)).all()
    assert np.abs(np.sqrt((r["normal"] ** 2).sum(axis=-1))[r["hit"]] - 1).max() <= 1e-15
    if key == "fixture:f":
        assert r["t"].max() >= 900  # (t up to about 1e3)
    if key == "fixture:h":  # the cap's outermost ring, 1e-6 wide in x^2 + z^2, holds decided samples
        ring = int((views.rim_ring(r, ref.flat_tree(view)) & dec).sum())
        print("  %d decided samples in the cap's ring" % ring)
        assert ring >= views.MIN_HITS
    # against the oracle, over the decided samples
    mask_ok, leaf_ok, dev = views.deviations(r, t, normal, leaf)
    assert mask_ok and leaf_ok
    for name, d in sorted(dev.items()):
        print("  %-16s %5d hits  |t - t_ref| / max(1, t) %.3e  |n - n_ref| %.3e" % (name, d["hits"], d["t"], d["normal"]))
        assert d["t"] <= bounds["types"][name]["t"] and d["normal"] <= bounds["types"][name]["normal"], (name, d)
    assert share <= bounds["undecided"][key]


def test_recorded_bounds(bounds):
    """Every type but the toroid is pinned within 1e-9 in t (the sphere test's bound at the same discriminant
    clearance); every leaf type is recorded."""
    assert sorted(bounds["types"]) == sorted(ref.TYPE_NAMES.values())
    for name, d in bounds["types"].items():
        print("%-16s t %.3e normal %.3e" % (name, d["t"], d["normal"]))
        assert name == "toroid" or d["t"] <= 1e-9, (name, d)
    assert sorted(bounds["undecided"]) == sorted(views.KEYS)


def test_quad_has_no_gap(built):
    """View g, straight at the quad: every decided sample whose ray passes inside the quad's outline (its four corners
    projected from the eye, clear of the outline by 1e-9) hits one of its two triangles, in the reference and in the
    oracle: no gap along the shared edge; samples on both sides of that edge occur."""
    view, _, _ = views.view_of("fixture:g")
    r = views.reference_of("fixture:g")
    tree = ref.flat_tree(view)
    inside = views.inside_quad(view, tree) & ~r["undecided"]
    tris, _ = views.quad_world(tree)
    assert inside.sum() >= 500
    assert np.isin(r["leaf"][inside], tris).all()
    assert np.isin(views.oracle_of("fixture:g")[2][inside], tris).all()
    assert all((r["leaf"][inside] == k).sum() >= views.MIN_HITS for k in tris)
