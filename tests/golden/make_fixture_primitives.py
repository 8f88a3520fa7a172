#!/usr/bin/env python3
"""Write the primitives conformance scene: tests/golden/scenes/primitives_edge_64x48.c.

Every leaf type but CSG in one frame, for the first-hit tests (tests/test_first_hit_cpu.py, tests/test_first_hit.py:
t, normal and leaf of every camera sample against an extended-precision reference and the oracle) and, through its
golden, for the image tests. The C is this project's own text against the drop-in headers, written with
make_fixture_csg.py's emitter; the golden comes from the real reference (make_golden.py, source kind "c:<name>").

Settings as for the CSG scenes: 64x48, 2x2 CMJ without jitter, a point aperture, path_length 5, GI off, one
reference thread, one point light and one 4x4 area light with a single cached row.

Leaves: a floor plane; a sphere; a cube; a closed cylinder [-0.5, 1.5] and an open one; a closed cone [-1, 0.5]
(spans the apex: both nappes) and an open truncated one [0.25, 1]; a toroid r1 = 1, r2 = 0.35 and a fat one
r1 = 0.6, r2 = 0.5; two flat triangles sharing an edge (a quad) and a smooth triangle with three distinct vertex
normals. Every leaf but the plane is under rotation, non-uniform scale and translation, with three exceptions made
for the tests' axis-aligned views: the cube turns about x only and the closed cylinder about y only, so a ray with
a direction component of rounding size keeps it in their frames (the slab's infinity branch, the skipped caps), and
the closed cone has only a uniform scale and a translation, so a ray at 45 degrees to its axis meets feq(a, 0).
The three triangles sit two groups deep with a transform on each group and on themselves: a tparent chain of 3.

The reference turns a ray inside a cube's face plane into NaN (make_fixture_csg.py); check_directions() asserts
that no camera sample of the scene's own camera has a direction component under 3 x EPSILON in the world's, a
group's or the cube's frame, so the infinity branch of cube.c / bounding_box.c is never entered in the golden.

  python tests/golden/make_fixture_primitives.py
  python tests/golden/make_golden.py primitives_edge_64x48
"""
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_fixture_csg as base  # noqa: E402
from make_fixture_csg import S, T, grp, leaf, matte, nums  # noqa: E402

NAME = "primitives_edge_64x48"
CAMERA = {"from": (1.02, 7.1, -13.0), "to": (0.2, 0.8, 0.3), "size": (64, 48), "fov": 0.9}
LIGHTS = {"point": (-6, 10, -8), "corner": (3, 9, -5), "uvec": (2, 0, 0), "vvec": (0, 0, 2)}
GREY, PINK, TEAL = matte(0.6, 0.6, 0.65), matte(0.9, 0.5, 0.6), matte(0.15, 0.6, 0.55)


def smooth_tri(material, pts, normals, *xf):
    return {"kind": "smooth_triangle", "mat": material, "xf": xf, "pts": pts, "normals": normals, "fields": {}}


class Emitter(base.Emitter):
    def shape(self, node, dst):
        k = node["kind"]
        if k == "smooth_triangle":
            names = []
            for p in node["pts"]:
                names.append(self.fresh("p"))
                self.out("Point %s = { %s, 1.0 };" % (names[-1], nums(*p)))
            for v in node["normals"]:
                names.append(self.fresh("n"))
                self.out("Vector %s = { %s, 0.0 };" % (names[-1], nums(*v)))
            self.out("smooth_triangle(%s, %s);" % (dst, ", ".join(names)))
            self.material(node, dst)
            self.transform(dst, node["xf"])
        elif k == "toroid":
            self.out("toroid(%s);" % dst)
            self.material(node, dst)
            for name, v in node["fields"].items():
                self.out("(%s)->fields.toroid.%s = %s;" % (dst, name, base.num(v)))
            self.transform(dst, node["xf"])
        else:
            super().shape(node, dst)

    def material(self, node, dst):
        (r, g, b), ka, kd, ks, refl, tr, ni, shadow = node["mat"]
        self.out("shape_set_material(%s, mat(%s, %s));" % (dst, nums(r, g, b, ka, kd, ks, refl, tr, ni),
                                                            "true" if shadow else "false"))


def unit(x, y, z):
    n = math.sqrt(x * x + y * y + z * z)
    return (x / n, y / n, z / n)


def shapes():
    quad_xf = (S(1.5, 1.2, 1.0), ("rx", 0.2), T(0, 0.3, 0))
    a, b, c, d = (-0.75, 0.0, 0.1), (0.75, 0.0, -0.1), (0.8, 1.25, 0.15), (-0.7, 1.0, -0.05)
    quad = [base.tri(base.YELLOW, a, b, c, *quad_xf), base.tri(base.ORANGE, a, c, d, *quad_xf)]
    smooth = smooth_tri(base.CYAN, ((-0.6, 0.0, 0.0), (0.6, 0.1, 0.0), (0.1, 1.1, 0.2)),
                        (unit(-0.4, 0.1, -1.0), unit(0.5, -0.2, -1.0), unit(0.05, 0.6, -1.0)),
                        S(1.7, 1.4, 1.0), ("ry", -0.3), T(0.2, 1.55, 1.4))
    deep = grp([grp(quad + [smooth], S(1.2, 1.0, 0.9), ("rz", 0.1), T(0, 0.15, 0))], ("ry", 0.3), T(4.6, 0, -2.0))
    return [
        base.floor(),
        leaf("sphere", base.RED, S(0.9, 0.7, 0.8), ("ry", 0.4), ("rz", 0.2), T(-5.0, 1.0, 2.5)),
        leaf("cube", base.GREEN, S(0.9, 0.7, 0.8), ("rx", 0.3), T(-2.5, 1.2, 2.5)),
        leaf("cylinder", base.BLUE, S(0.6, 0.7, 0.5), ("ry", 0.5), T(0.0, 1.0, 2.5),
             minimum=-0.5, maximum=1.5, closed=True),
        leaf("cylinder", base.MAGENTA, S(0.5, 0.8, 0.6), ("rx", 0.9), ("rz", -0.3), T(2.5, 1.3, 2.5),
             minimum=-1.0, maximum=1.0, closed=False),
        leaf("cone", base.WHITE, S(0.8), T(5.0, 1.0, 2.5), minimum=-1.0, maximum=0.5, closed=True),
        leaf("cone", PINK, S(0.9, 1.2, 0.7), ("ry", 0.6), ("rz", 0.25), T(-4.0, 0.5, -2.0),
             minimum=0.25, maximum=1.0, closed=False),
        leaf("toroid", TEAL, S(0.7, 0.75, 0.65), ("rx", 0.5), ("ry", 0.3), T(-1.0, 0.9, -2.0), r1=1.0, r2=0.35),
        leaf("toroid", GREY, S(0.75, 0.8, 0.85), ("rx", -0.4), ("rz", 0.3), T(2.0, 1.0, -2.0), r1=0.6, r2=0.5),
        deep,
    ]


def check_directions():
    """The smallest |direction component| over the camera samples of the written scene (captured and flattened by
    the host library, rays as tests/feature_ref.py builds them) in the world's frame and, taken through the
    inverse transforms above it, in every group's and the cube's frame. At 3 x EPSILON or more (the components are
    exact to 1e-16; 12288 samples in five frames leave no eye with much more room) no sample enters the infinity
    branch of cube.c / bounding_box.c."""
    import numpy as np
    root = os.path.dirname(os.path.dirname(HERE))
    sys.path[:0] = [root, os.path.join(root, "tests")]
    import feature_ref
    import first_hit_ref
    from fast_ray_tracer_amd import build
    from fast_ray_tracer_amd.runtime import Scene
    scene = Scene(build.build_scene(os.path.join(base.SCENES_DIR, NAME + ".c"), force=True))
    tree = first_hit_ref.flat_tree(scene)
    d = feature_ref.camera_rays(scene)[1].reshape(-1, 3)
    nodes, smallest = tree["nodes"], np.abs(d).min()
    for k in np.flatnonzero((nodes["type"] == first_hit_ref.GROUP) | (nodes["type"] == first_hit_ref.CUBE)):
        chain, x = [], int(k)
        while x >= 0:
            if nodes["xform"][x] >= 0:
                chain.append(tree["xforms"][nodes["xform"][x]][:3, :3])
            x = int(nodes["tparent"][x])
        local = d
        for m in reversed(chain):  # (the outermost transform first)
            local = local @ m.T
        smallest = min(smallest, np.abs(local).min())
    assert smallest >= 3 * 1e-5, smallest
    return smallest


def main():
    tree = shapes()
    base.Emitter = Emitter  # (write_scene builds its emitter itself)
    base.write_scene(NAME, "every leaf type but CSG, transformed and grouped, for the first-hit tests", tree, CAMERA,
                     LIGHTS)
    print("smallest |direction component| in a slab frame: %.3e" % check_directions())


if __name__ == "__main__":
    main()
