"""The views of the first-hit tests (test_first_hit_cpu.py, test_first_hit.py, golden/make_first_hit_bounds.py):
cameras over primitives_edge_64x48 and over the CSG-free goldens, each with the leaf types it must show at least
MIN_HITS decided hits of and the epsilon branches it must enter on a decided sample. No GPU."""
import math

import numpy as np

import first_hit_ref as ref
from first_hit_ref import CONE, CUBE, CYLINDER, PLANE, SMOOTH_TRIANGLE, SPHERE, TOROID, TRIANGLE

FIXTURE = "primitives_edge_64x48"
MIN_HITS = 20
MAX_UNDECIDED = 0.01
EVERY = (CONE, CUBE, CYLINDER, PLANE, SMOOTH_TRIANGLE, SPHERE, TOROID, TRIANGLE)

# name: (scene, view arguments or None for the captured camera, steps, leaf types, branches)
#   a  the overview (the scene's own camera), at 1 x 1 and at 3 x 3 steps
#   b  along +z at an odd size: the centre column has |d_x|, the centre row |d_y| of rounding size. The column runs
#      through the cube, which turns about x only (the slab's infinity branch on its x axis); the row through the
#      closed cylinder, which turns about y only (feq(d_y, 0) skips the caps), and above the floor (the plane's
#      parallel miss)
#   c  straight down with up = z, the centre column through the cube
#   d  the centre ray at 45 degrees to the plain cone's axis: a = d_x^2 + d_z^2 - d_y^2 of rounding size
#   e_* a camera inside each closed shape (eyes: inside_eyes())
#   f  from 0.05 above the floor, nearly horizontal: t up to about 1e3
#   g  straight at the quad (eye: quad_eye())
#   h  the rim of the closed cylinder's top cap through a field of view of 5e-7 (rim_eye()): a pixel is 1.6e-7 wide,
#      so the ring 1 - 1e-6 <= x^2 + z^2 < 1 of the cap, 3e-7 wide in the world, holds samples: a cap test that
#      is off by 1e-6 drops their hits
# f looks up by half a pixel less 5e-5: the sample row under the centre runs 5e-5 below the horizontal and meets
# the floor at t = 0.05 / 5e-5 (the scene's field of view is 0.9; |d_y| stays above EPSILON)
F_RISE = math.hypot(14.0, 21.0) * (0.5 * 2.0 * math.tan(0.45) / 64 - 5e-5)
FIXTURE_VIEWS = {
    "a": (None, 1, EVERY, ()),
    "a3": (None, 3, EVERY, ()),
    "b": (dict(from_=(-2.5, 1.15, -12.0), to=(-2.5, 1.15, 0.0), hsize=63, vsize=47), 1,
          (CUBE, CYLINDER, PLANE, CONE, TOROID), ("slab_parallel", "caps_skipped", "plane_parallel")),
    "c": (dict(from_=(-2.5, 14.0, 0.4), to=(-2.5, 0.0, 0.4), up=(0.0, 0.0, 1.0), hsize=63, vsize=47), 1,
          (CUBE, CYLINDER, PLANE, SPHERE, TOROID, CONE), ("slab_parallel",)),
    "d": (dict(from_=(5.3, 4.0, -1.0), to=(5.3, 1.0, 2.0), hsize=33, vsize=33), 1, (CONE, PLANE),
          ("cone_a_zero", "cone_single_root")),
    "f": (dict(from_=(-8.0, 0.05, -12.0), to=(6.0, 0.05 + F_RISE, 9.0), hsize=64, vsize=48), 1,
          (PLANE, CUBE, CYLINDER, CONE, TOROID), ()),
}
INSIDE = {"e_sphere": SPHERE, "e_cube": CUBE, "e_cylinder": CYLINDER, "e_cone": CONE, "e_toroid": TOROID,
          "e_toroid_fat": TOROID}
GOLDEN_VIEWS = {  # the captured cameras (from, to) at a reduced size
    "group_test_150x50": (((0.0, 0.0, -9.0), (0.0, 0.0, 0.0)), (45, 15), (CONE, CYLINDER, PLANE)),
    "checkered_cube_160x80": (((0.0, 0.0, -20.0), (0.0, 0.0, 0.0)), (40, 20), (CUBE,)),
    "checkered_cylinder_120": (((0.0, 5.0, -10.0), (0.0, 0.0, 0.0)), (40, 40), (CYLINDER,)),
    "checkered_torus_120": (((0.0, 5.0, -10.0), (0.0, 0.0, 0.0)), (48, 48), (TOROID,)),
    "bounding_boxes_100x125_4x4": (((0.0, 2.5, -10.0), (0.0, 1.0, 0.0)), (40, 50), (CUBE, CYLINDER, SMOOTH_TRIANGLE)),
    "teapot_low_100": (((0.0, 0.0, -30.0), (0.0, 0.0, 0.0)), (40, 40), (SMOOTH_TRIANGLE,)),
}
CSG_VIEWS = {  # the device against the oracle only (the oracle does CSG)
    "cornell_direct_64_4x4": (((0.0, 0.0, -2.75), (0.0, 0.0, 0.0)), (64, 64)),
    "csg_ops_96x64": (((0.0, 9.0, -11.0), (0.0, 0.5, 0.0)), (48, 32)),
    "csg_nested_96x64": (((0.5, 5.0, -10.0), (0.5, 1.0, 0.5)), (48, 32)),
    "test_scene_120": (((-2.0, 3.0, -6.0), (0.0, 0.0, 0.0)), (48, 48)),
}


def _to_world(tree, node):
    """The binary64 matrix from a node's space to the world's (the product of the inverses of its chain)."""
    nodes, m, x = tree["nodes"], np.eye(4), int(node)
    while x >= 0:
        if nodes["xform"][x] >= 0:
            m = np.linalg.inv(tree["xforms"][nodes["xform"][x]]) @ m
        x = int(nodes["tparent"][x])
    return m


def _leaves(tree, typ):
    return [int(k) for k in np.flatnonzero(tree["nodes"]["type"] == typ)]


def inside_eyes(tree):
    """{view name: (eye, look-at)} in the world: a point inside each closed shape of the fixture, and a point off it
    in a direction that is parallel to no axis of the shape."""
    nodes, prim = tree["nodes"], tree["prim"]
    closed = [k for k in _leaves(tree, CYLINDER) + _leaves(tree, CONE) if prim[nodes["prim"][k] + 2] != 0.0]
    cyl = [k for k in closed if nodes["type"][k] == CYLINDER][0]
    cone = [k for k in closed if nodes["type"][k] == CONE][0]
    tor = {prim[nodes["prim"][k]]: k for k in _leaves(tree, TOROID)}  # by r1
    local = {"e_sphere": (_leaves(tree, SPHERE)[0], (0.1, -0.2, 0.15)), "e_cube": (_leaves(tree, CUBE)[0], (0.2, 0.1, -0.3)),
             "e_cylinder": (cyl, (0.1, 0.6, -0.2)), "e_cone": (cone, (0.05, -0.6, 0.1)),
             "e_toroid": (tor[1.0], (1.0, 0.05, 0.1)), "e_toroid_fat": (tor[0.6], (0.1, -0.1, 0.65))}
    out = {}
    for name, (leaf, p) in local.items():
        m = _to_world(tree, leaf)
        eye = m @ np.array(p + (1.0,))
        to = m @ np.array((p[0] + 0.35, p[1] + 0.45, p[2] + 0.8, 1.0))
        out[name] = (tuple(eye[:3]), tuple(to[:3]))
    return out


def quad_world(tree):
    """The quad's two triangle leaves and its four corners a, b, c, d in the world (the triangles are a b c and
    a c d), binary64."""
    nodes, prim = tree["nodes"], tree["prim"]
    t1, t2 = _leaves(tree, TRIANGLE)
    m = _to_world(tree, t1)
    assert np.array_equal(tree["xforms"][nodes["xform"][t1]], tree["xforms"][nodes["xform"][t2]])
    p1, q1 = prim[nodes["prim"][t1]:nodes["prim"][t1] + 9], prim[nodes["prim"][t2]:nodes["prim"][t2] + 9]
    a, b, c, d = p1[0:3], p1[0:3] + p1[3:6], p1[0:3] + p1[6:9], q1[0:3] + q1[6:9]
    assert np.array_equal(q1[0:3], a) and np.allclose(q1[0:3] + q1[3:6], c, rtol=0, atol=1e-15)
    return (t1, t2), [(m @ np.append(v, 1.0))[:3] for v in (a, b, c, d)]


def quad_eye(tree):
    _, (a, b, c, d) = quad_world(tree)
    centre = (a + b + c + d) / 4
    n = np.cross(c - a, d - b)
    n = n / np.linalg.norm(n)
    if n[2] > 0:  # (the side the scene's camera is on)
        n = -n
    return tuple(centre + 4.0 * n + np.array((0.013, 0.021, 0.0))), tuple(centre)


def closed_cylinder(tree):
    nodes, prim = tree["nodes"], tree["prim"]
    return [k for k in _leaves(tree, CYLINDER) if prim[nodes["prim"][k] + 2] != 0.0][0]


def rim_eye(tree):
    """An eye 10 away from a point of the closed cylinder's top rim, above the cap's inner side, and that point:
    the rays run outwards and down, so those that pass the rim meet no wall (a wall hit within EPSILON of the top has
    x^2 + z^2 = 1 to rounding, where the normal's dist < 1 rule decides nothing)."""
    m = _to_world(tree, closed_cylinder(tree))
    c, s = math.cos(-1.9), math.sin(-1.9)
    rim = np.array((c, 1.5, s, 1.0))
    p = (m @ rim)[:3]
    off = (m @ (rim + np.array((-0.5 * c - 0.3 * s, 1.0, -0.5 * s + 0.3 * c, 0.0))))[:3] - p
    return tuple(p + 10.0 * off / np.linalg.norm(off)), tuple(p)


def rim_ring(r, tree):
    """The samples of a reference result that hit the closed cylinder's top cap in the ring
    1 - 1e-6 <= x^2 + z^2 < 1."""
    x, y, z = (r["local"][..., k] for k in range(3))
    rr = x * x + z * z
    return (r["leaf"] == closed_cylinder(tree)) & (np.abs(y - 1.5) < 1e-9) & (rr >= 1 - 1e-6) & (rr < 1)


def fixture_views(scene):
    """{name: (View, leaf types, branches)} over the captured fixture scene."""
    from fast_ray_tracer_amd.runtime import View
    tree = ref.flat_tree(scene)
    out = {}
    for name, (args, steps, types, branches) in FIXTURE_VIEWS.items():
        if args is None:  # the captured camera at other steps
            v = View(scene, scene.camera, steps, steps, False, scene.drand48_state, "%s@%s" % (scene.name, name))
        else:
            v = scene.view(usteps=steps, vsteps=steps, **args)
        out[name] = (v, types, branches)
    for name, (eye, to) in inside_eyes(tree).items():
        out[name] = (scene.view(eye, to, hsize=32, vsize=24, fov=1.3, usteps=1, vsteps=1), (INSIDE[name],), ("inside",))
    eye, to = quad_eye(tree)
    out["g"] = (scene.view(eye, to, hsize=48, vsize=36, fov=0.6, usteps=1, vsteps=1), (TRIANGLE,), ())
    eye, to = rim_eye(tree)
    out["h"] = (scene.view(eye, to, hsize=32, vsize=32, fov=5e-7, usteps=1, vsteps=1), (CYLINDER,), ())
    return out


def golden_view(scene, name):
    (eye, to), (w, h), types = GOLDEN_VIEWS[name]
    return scene.view(eye, to, hsize=w, vsize=h, usteps=1, vsteps=1, aperture_size=0.0), types, ()


def inside_quad(view, tree):
    """Per sample of a view: its ray passes inside the quad's outline as seen from the eye, clear of it by 1e-9
    relative (longdouble; the corners projected from the eye onto the plane through them across the view axis)."""
    import feature_ref
    o, d = feature_ref.camera_rays(view)
    _, corners = quad_world(tree)
    LD = ref.LD
    eye = o.reshape(-1, 3)[0].astype(LD)
    rel = [np.asarray(c, dtype=LD) - eye for c in corners]
    axis = sum(rel) / 4
    axis = axis / np.sqrt((axis * axis).sum())
    e1 = np.cross(axis.astype(np.float64), (0.0, 1.0, 0.0)).astype(LD)
    e1 = e1 / np.sqrt((e1 * e1).sum())
    e2 = np.array([axis[1] * e1[2] - axis[2] * e1[1], axis[2] * e1[0] - axis[0] * e1[2],
                   axis[0] * e1[1] - axis[1] * e1[0]], dtype=LD)

    def project(v):
        w = (v * axis).sum(axis=-1)
        return np.stack([(v * e1).sum(axis=-1) / w, (v * e2).sum(axis=-1) / w], axis=-1)

    q = [project(r) for r in rel]
    p = project(d.astype(LD))
    sides = []
    for k in range(4):
        a, b = q[k], q[(k + 1) % 4]
        cr = (b[0] - a[0]) * (p[..., 1] - a[1]) - (b[1] - a[1]) * (p[..., 0] - a[0])
        size = np.abs((b[0] - a[0]) * (p[..., 1] - a[1])) + np.abs((b[1] - a[1]) * (p[..., 0] - a[0]))
        sides.append(np.where(np.abs(cr) > LD(1e-9) * size, np.sign(cr), 0))
    sides = np.stack(sides)
    return (sides == 1).all(axis=0) | (sides == -1).all(axis=0)


def type_name(t):
    return ref.TYPE_NAMES[int(t)]


# ---------------------------------------------------------------------------------------------------------------
# the views by key, their references (computed once per process) and the deviations between two sets of first hits

KEYS = (["fixture:" + n for n in list(FIXTURE_VIEWS) + list(INSIDE) + ["g", "h"]] + ["golden:" + n for n in GOLDEN_VIEWS])
_views, _refs, _oracle = {}, {}, {}


def scene_of(key):
    from conftest import load_scene
    kind, name = key.split(":")
    return load_scene(FIXTURE if kind == "fixture" else name)


def view_of(key):
    """(View, leaf types the view is listed for, branches it must enter)."""
    if key not in _views:
        kind, name = key.split(":")
        scene = scene_of(key)
        if kind == "fixture":
            _views.update({"fixture:" + n: v for n, v in fixture_views(scene).items()})
        elif kind == "golden":
            _views[key] = golden_view(scene, name)
        else:
            (eye, to), (w, h) = CSG_VIEWS[name]
            _views[key] = (scene.view(eye, to, hsize=w, vsize=h, usteps=1, vsteps=1, aperture_size=0.0), (), ())
    return _views[key]


def reference_of(key):
    if key not in _refs:
        _refs[key] = ref.first_hits(view_of(key)[0])
    return _refs[key]


def oracle_of(key):
    import oracle
    if key not in _oracle:
        _oracle[key] = oracle.first_hits(view_of(key)[0])
    return _oracle[key]


def deviations(r, t, normal, leaf):
    """A set of first hits (t, normal, leaf as oracle.first_hits gives them) against the reference r over its
    decided samples: (the hit masks agree, the leaves agree, {type name: {"t": max |t_ref - t| / max(1, t_ref),
    "normal": max |n_ref - n|, "hits": decided hits}})."""
    dec = ~r["undecided"]
    mask_ok = np.array_equal(r["hit"][dec], (leaf >= 0)[dec])
    leaf_ok = np.array_equal(r["leaf"][dec], leaf[dec])
    both = dec & r["hit"] & (leaf == r["leaf"])
    out = {}
    for typ in np.unique(r["type"][both]):
        m = both & (r["type"] == typ)
        dt = (np.abs(r["t"][m] - t[m]) / np.maximum(1, r["t"][m])).max()
        dn = np.abs(r["normal"][m] - normal[m]).max()
        out[type_name(typ)] = {"t": float(dt), "normal": float(dn), "hits": int(m.sum())}
    return mask_ok, leaf_ok, out


def load_bounds():
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "first_hit_bounds.json")) as f:
        return json.load(f)
