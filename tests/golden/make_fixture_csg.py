#!/usr/bin/env python3
"""Write the CSG conformance scenes: tests/golden/scenes/csg_*.c.

The suite's other scenes hold two CSG trees, the cornell wall ((cube U cube) - cube, axis-aligned leaves) and
test_scene_120's cube - sphere. These scene programs (the seven the suite's lists name and one variant) cover what those leave out of the generated kernels
(frt_jit.hip Gen) and of the generic walk (frt_traverse.hpp): CSG_INTERSECT, CSG nodes as right operands, groups
inside units, one-slot leaves (plane, triangle), rotated and non-uniformly scaled leaves and units, exactly equal
t across leaves, members that cast no shadow, refraction through a CSG, units with unsorted-list leaves
(cylinder, cone, torus: the generator must refuse them) and the 32-entry limit of a unit from both sides.

The C is this project's own text against the drop-in headers (fast_ray_tracer_amd/host/src): a helper for
materials and one main() per scene, emitted from the small tree descriptions below. Every file compiles
unchanged in capture mode (build.build_scene) and against the reference sources (oracle/build_ref.sh); the
goldens come from the real reference (make_golden.py, source kind "c:<name>").

Common settings, the smallest at which every stage still runs: at most 96x64 pixels, 2x2 CMJ without jitter, a
point aperture, path_length 5, GI off, one reference thread, a floor plane, one point light and one rectangular
area light of 4x4 samples with a single cached row (one 16-sample light part).

csg_ties_64x48: the camera sits on the z axis with up = y and looks along it but for a pitch of 1/8 pixel
(0.0016 rad). Looking exactly along the axis, no ray would come near a zero component: the 2x2 grid without
jitter samples a pixel at 1/8, 3/8, 5/8 and 7/8 (sampler.c:426), so at even sizes the smallest |direction x| or
|direction y| is 1.6e-3, far above the reference's EPSILON of 1e-5 (linalg.h:7). The pitch turns the sample row
1/8 pixel above the centre into the plane y = 0: its 64 x 2 camera rays have |direction y| of rounding size
and cross all three units, taking the +-INFINITY branch of cube.c:24 and bounding_box.c:132 on the y axis
(counted in a scratch build of the reference: 0 entries into cube.c's branch without the pitch). No face lies
in y = 0. Taken out: the same turn about y, a sample column in the plane x = 0 of the shared face. The
reference cannot render it: a ray that runs in a cube's face plane gets 0 * INFINITY on that slab and the
reference's canvas holds NaN for those pixels, so there is nothing to compare against. scene_ties() checks the
row's direction before it writes the scene.

  python tests/golden/make_fixture_csg.py
  python tests/golden/make_golden.py csg_ops_96x64 csg_nested_96x64 csg_ties_64x48 csg_noshadow_glass_64x48 \
      csg_unsorted_64x48 csg_wide32_48 csg_wide34_48 csg_nested_nogroup_96x64
"""
import math
import os

HERE = os.path.dirname(os.path.abspath(__file__))
SCENES_DIR = os.path.join(HERE, "scenes")

HEADER = """\
/* %(name)s: %(purpose)s
 * Written by tests/golden/make_fixture_csg.py; edit the generator, not this file. */
#include <stdio.h>
#include <stdbool.h>
#include <math.h>

#include "src/libs/canvas/canvas.h"
#include "src/libs/linalg/linalg.h"
#include "src/color/color.h"
#include "src/renderer/camera.h"
#include "src/renderer/config.h"
#include "src/renderer/renderer.h"
#include "src/renderer/world.h"
#include "src/light/light.h"
#include "src/material/material.h"
#include "src/shapes/shapes.h"
#include "src/shapes/cone.h"
#include "src/shapes/csg.h"
#include "src/shapes/cube.h"
#include "src/shapes/cylinder.h"
#include "src/shapes/group.h"
#include "src/shapes/plane.h"
#include "src/shapes/sphere.h"
#include "src/shapes/toroid.h"
#include "src/shapes/triangle.h"

/* colour (r, g, b) weighted into Ka / Kd / Ks, one grey level for reflection and for the transmission filter */
static Material
mat(double r, double g, double b, double ka, double kd, double ks, double refl, double tr, double ni, bool shadow)
{
    Material m = material_alloc();
    m->Ka[0] = r * ka; m->Ka[1] = g * ka; m->Ka[2] = b * ka;
    m->Kd[0] = r * kd; m->Kd[1] = g * kd; m->Kd[2] = b * kd;
    m->Ks[0] = ks; m->Ks[1] = ks; m->Ks[2] = ks;
    m->refl[0] = m->refl[1] = m->refl[2] = refl;
    m->Tf[0] = m->Tf[1] = m->Tf[2] = tr;
    m->reflective = refl > 0.0;
    m->Tr = tr;
    m->Ni = ni;
    m->Ns = 50.0;
    m->casts_shadow = shadow;
    return m;
}

int
main()
{
    struct global_config cfg;
    cfg.illumination.include_direct = true;
    cfg.illumination.include_global = false;
    cfg.illumination.debug_visualize_photon_map = false;
    cfg.illumination.debug_visualize_soft_indirect = false;
    cfg.illumination.di.include_ambient = true;
    cfg.illumination.di.include_diffuse = true;
    cfg.illumination.di.include_specular_highlight = true;
    cfg.illumination.di.include_specular = true;
    cfg.illumination.di.path_length = 5;
    cfg.illumination.gi.include_caustics = false;
    cfg.illumination.gi.include_final_gather = false;
    cfg.illumination.gi.usteps = 1;
    cfg.illumination.gi.vsteps = 1;
    cfg.illumination.gi.irradiance_estimate_num = 200;
    cfg.illumination.gi.irradiance_estimate_radius = 0.1;
    cfg.illumination.gi.irradiance_estimate_cone_filter_k = 1.0;
    cfg.illumination.gi.photon_count = 0;
    cfg.illumination.gi.path_length = 5;
    cfg.threading.num_threads = 1;
    cfg.scene.divide_threshold = %(divide)d;
    cfg.output.file_path = "/tmp/frt_golden/out/%(name)s";
    cfg.output.color_space = SRGB;

    struct aperture ap;
    aperture(POINT_APERTURE, 0.0, 1, 1, false, &ap);
    Point from = { %(from)s, 1.0 };
    Point to = { %(to)s, 1.0 };
    Vector up = { %(up)s, 0.0 };
    Matrix view;
    view_transform(from, to, up, view);
    Camera cam = camera(%(w)d, %(h)d, %(fov)s, 1.0, 2, 2, &ap, view);

    Light lights = array_of_lights(2);
    Point point_at = { %(point)s, 1.0 };
    Color point_power = color(%(point_i)s, %(point_i)s, %(point_i)s);
    point_light(point_at, point_power, lights + 0);
    Point area_corner = { %(corner)s, 1.0 };
    Vector area_u = vector_init(%(uvec)s);
    Vector area_v = vector_init(%(vvec)s);
    Color area_power = color(%(area_i)s, %(area_i)s, %(area_i)s);
    area_light(area_corner, area_u, 4, area_v, 4, true, 1, area_power, lights + 1);

    Matrix t, u;
"""

FOOTER = """\

    Shape top = array_of_shapes(1);
    group(top, all, %(n)d);
    top->divide(top, cfg.scene.divide_threshold);

    World w = world();
    w->lights = lights;
    w->lights_num = 2;
    w->shapes = top;
    w->shapes_num = 1;
    w->global_config = &cfg;
    w->photon_maps = NULL;

    Canvas c = render_multi(cam, w, cam->usteps, cam->vsteps, cam->aperture.jitter);
    write_ppm_file(c, true, cfg.output.file_path);
    write_png(c, cfg.output.file_path);
    canvas_free(c);
    return 0;
}
"""


def num(x):
    return repr(float(x))


def nums(*xs):
    return ", ".join(num(x) for x in xs)


# ---- materials: (r, g, b), Ka, Kd, Ks, refl, Tr, Ni, casts_shadow ----
def matte(r, g, b, shadow=True):
    return ((r, g, b), 0.15, 0.75, 0.3, 0.0, 0.0, 1.0, shadow)


GLASS = ((1.0, 1.0, 1.0), 0.0, 0.05, 0.9, 0.9, 1.0, 1.5, True)
FLOOR = matte(0.8, 0.8, 0.75)
RED, GREEN, BLUE = matte(0.9, 0.2, 0.15), matte(0.2, 0.8, 0.25), matte(0.2, 0.3, 0.9)
YELLOW, CYAN, MAGENTA = matte(0.9, 0.85, 0.2), matte(0.2, 0.85, 0.85), matte(0.85, 0.25, 0.8)
ORANGE, WHITE = matte(0.95, 0.55, 0.15), matte(0.9, 0.9, 0.9)


# ---- tree descriptions ----
# transform: a tuple of steps applied in order, ("s", x, y, z) ("rx" | "ry" | "rz", angle) ("t", x, y, z)
def leaf(kind, material, *xf, **fields):
    return {"kind": kind, "mat": material, "xf": xf, "fields": fields}


def tri(material, p1, p2, p3, *xf):
    return {"kind": "triangle", "mat": material, "xf": xf, "pts": (p1, p2, p3), "fields": {}}


def csg(op, left, right, *xf):
    return {"kind": "csg", "op": op, "left": left, "right": right, "xf": xf}


def grp(children, *xf):
    return {"kind": "group", "children": children, "xf": xf}


def S(x, y=None, z=None):
    return ("s", x, x if y is None else y, x if z is None else z)


def T(x, y, z):
    return ("t", x, y, z)


class Emitter:
    def __init__(self):
        self.lines = []
        self.n = 0

    def out(self, s):
        self.lines.append("    " + s)

    def fresh(self, p):
        self.n += 1
        return "%s%d" % (p, self.n)

    def transform(self, dst, xf):
        if not xf:
            return
        self.out("matrix_identity(t);")
        for st in xf:
            if st[0] == "s":
                self.out("matrix_scale(%s, u);" % nums(*st[1:]))
            elif st[0] == "t":
                self.out("matrix_translate(%s, u);" % nums(*st[1:]))
            else:
                self.out("matrix_rotate_%s(%s, u);" % (st[0][1], num(st[1])))
            self.out("transform_chain(u, t);")
        self.out("shape_set_transform(%s, t);" % dst)

    def shape(self, node, dst):
        k = node["kind"]
        if k == "csg":
            kids = self.fresh("k")
            self.out("Shape %s = array_of_shapes(2);" % kids)
            self.shape(node["left"], kids + " + 0")
            self.shape(node["right"], kids + " + 1")
            self.out("csg(%s, CSG_%s, %s + 0, %s + 1);" % (dst, node["op"], kids, kids))
        elif k == "group":
            kids = self.fresh("g")
            self.out("Shape %s = array_of_shapes(%d);" % (kids, len(node["children"])))
            for i, c in enumerate(node["children"]):
                self.shape(c, "%s + %d" % (kids, i))
            self.out("group(%s, %s, %d);" % (dst, kids, len(node["children"])))
        else:
            if k == "triangle":
                names = []
                for p in node["pts"]:
                    names.append(self.fresh("p"))
                    self.out("Point %s = { %s, 1.0 };" % (names[-1], nums(*p)))
                self.out("triangle(%s, %s);" % (dst, ", ".join(names)))
            else:
                self.out("%s(%s);" % (k, dst))
            (r, g, b), ka, kd, ks, refl, tr, ni, shadow = node["mat"]
            self.out("shape_set_material(%s, mat(%s, %s));" % (dst, nums(r, g, b, ka, kd, ks, refl, tr, ni),
                                                                "true" if shadow else "false"))
            field = "cone" if k == "cone" else "cylinder"
            for name, v in node["fields"].items():
                val = ("true" if v else "false") if isinstance(v, bool) else num(v)
                self.out("(%s)->fields.%s.%s = %s;" % (dst, field, name, val))
        self.transform(dst, node["xf"])


def write_scene(name, purpose, shapes, cam, lights, divide=100000):
    em = Emitter()
    em.out("Shape all = array_of_shapes(%d);" % len(shapes))
    for i, s in enumerate(shapes):
        em.out("/* top-level shape %d */" % i)
        em.shape(s, "all + %d" % i)
    head = HEADER % {
        "name": name, "purpose": purpose, "divide": divide,
        "from": nums(*cam["from"]), "to": nums(*cam["to"]), "up": nums(*cam.get("up", (0, 1, 0))),
        "w": cam["size"][0], "h": cam["size"][1], "fov": num(cam["fov"]),
        "point": nums(*lights["point"]), "point_i": num(lights.get("point_i", 0.5)),
        "corner": nums(*lights["corner"]), "uvec": nums(*lights["uvec"]), "vvec": nums(*lights["vvec"]),
        "area_i": num(lights.get("area_i", 0.5)),
    }
    with open(os.path.join(SCENES_DIR, name + ".c"), "w") as f:
        f.write(head + "\n".join(em.lines) + "\n" + FOOTER % {"n": len(shapes)})


def floor(y=0.0):
    return leaf("plane", FLOOR, T(0, y, 0)) if y else leaf("plane", FLOOR)


def scene_ops():
    """{UNION, INTERSECT, DIFFERENCE} x {(cube, sphere), (sphere, cube), (sphere, sphere)}, partly overlapping;
    in each row one unit's cube is rotated about y and z and scaled non-uniformly (the general-frame path)."""
    shapes = [floor()]
    for row, op in enumerate(("UNION", "INTERSECT", "DIFFERENCE")):
        z = 3.5 - 3.5 * row
        turned = (0, 1, 0)[row]  # the column whose cube is rotated
        for col in range(3):
            x = -3.5 + 3.5 * col
            if col == 0:
                cube_xf = ((S(0.8, 0.6, 0.7), ("ry", 0.5), ("rz", 0.3), T(x, 0.85, z)) if turned == 0
                           else (S(0.75), T(x, 0.75, z)))
                unit = csg(op, leaf("cube", RED, *cube_xf), leaf("sphere", BLUE, S(0.9), T(x + 0.5, 1.25, z - 0.25)))
            elif col == 1:
                cube_xf = ((S(0.5, 0.8, 0.6), ("ry", -0.7), ("rz", 0.4), T(x + 0.5, 1.2, z - 0.5)) if turned == 1
                           else (S(0.6), T(x + 0.5, 1.2, z - 0.5)))
                unit = csg(op, leaf("sphere", GREEN, S(0.9), T(x, 0.9, z)), leaf("cube", YELLOW, *cube_xf))
            else:
                unit = csg(op, leaf("sphere", CYAN, S(0.9), T(x - 0.4, 0.9, z)),
                           leaf("sphere", MAGENTA, S(0.8), T(x + 0.4, 1.1, z - 0.25)))
            shapes.append(unit)
    write_scene("csg_ops_96x64", "the three CSG ops over ordered leaf pairs", shapes,
                {"from": (0, 9, -11), "to": (0, 0.5, 0), "size": (96, 64), "fov": 0.72},
                {"point": (-6, 10, -8), "corner": (3, 9, -5), "uvec": (2, 0, 0), "vvec": (0, 0, 2)})


def scene_nested(with_group=True):
    """CSG nodes as right operands at two levels, a group as an operand, plane and triangle leaves, a unit with
    its own rotation and scale over transformed children; divide_threshold 1 reshapes the top level.

    with_group=False writes csg_nested_nogroup_96x64, the same scene without the unit that holds the group: the
    closest-hit generator (frt_jit.hip closest_ok) writes no kernel for a scene with a group inside a unit, so
    only this variant takes the nested units, the one-slot leaves and the transformed unit through frt_jit_trace."""
    a = leaf("sphere", RED, T(-4, 1, 0))
    b = leaf("cube", GREEN, S(0.8), T(-4, 1, 0))
    c = leaf("sphere", BLUE, S(0.6), T(-4, 1.5, -0.75))
    d = leaf("cube", YELLOW, S(0.9, 0.7, 0.7), T(-3, 0.7, 0.5))
    e = leaf("sphere", CYAN, S(0.5), T(-3, 1.4, 0.5))
    f = leaf("sphere", MAGENTA, S(0.5), T(-2.4, 0.9, -0.2))
    n1 = csg("UNION", csg("INTERSECT", a, csg("DIFFERENCE", b, c)), csg("DIFFERENCE", d, csg("UNION", e, f)))
    n2 = csg("DIFFERENCE",
             grp([leaf("sphere", ORANGE, S(0.8), T(-0.5, 0.8, 0)), leaf("sphere", WHITE, S(0.8), T(0.5, 0.8, 0))]),
             leaf("cube", BLUE, S(0.5), T(0, 1.2, -0.6)))
    n3 = csg("INTERSECT", leaf("sphere", GREEN, T(2.5, 1, 0)), leaf("plane", YELLOW, T(0, 1, 0)))
    n4 = csg("DIFFERENCE", leaf("sphere", CYAN, T(5, 1, 0)),
             tri(RED, (3.5, 0.25, -1.5), (6.5, 0.5, -0.5), (5, 2.5, -0.25)))
    n5 = csg("DIFFERENCE", leaf("cube", MAGENTA, S(0.7), ("ry", 0.3)),
             leaf("sphere", ORANGE, S(0.6), T(0.4, 0.4, -0.4)),
             S(1.2, 0.8, 1.0), ("ry", 0.4), ("rz", 0.2), T(0.5, 1.2, 3.5))
    write_scene("csg_nested_96x64" if with_group else "csg_nested_nogroup_96x64",
                "nesting, groups in units, one-slot leaves, transformed units" if with_group
                else "csg_nested_96x64 without the group unit (a scene the closest-hit generator accepts)",
                [floor(), n1, n2, n3, n4, n5] if with_group else [floor(), n1, n3, n4, n5],
                {"from": (0.5, 5, -10), "to": (0.5, 1, 0.5), "size": (96, 64), "fov": 1.0},
                {"point": (-5, 9, -7), "corner": (3, 8, -5), "uvec": (2, 0, 0), "vvec": (0, 0, 2)}, divide=1)


def scene_ties():
    """Exact ties: every shape coordinate is a multiple of 1/4. cube - cube with the cut's top (y = 1) and front
    (z = -1) faces in the planes of the outer cube's; cube U cube sharing the face x = 0, which also holds the
    camera and the point light; a sphere inside a cube, tangent to its top and front faces, under INTERSECT.

    No camera ray and no shadow ray to the point light crosses the shared face x = 0 (both start in its plane):
    the equal-t exit / entry pair there comes from the area light's shadow rays. The pitched sample row (see
    the module docstring) runs in the plane y = 0, which holds no face."""
    fov, width, height = 0.78, 64, 48
    # the camera's own arithmetic (camera.c:122-138, ray_for_pixel camera.c:96-110): world_y of row 23's sample
    # at 7/8 is half_height - 23.875 * pixel_size = pixel_size / 8; aim the camera at that slope
    half_width = math.tan(fov * 0.5)
    half_height = half_width / (width / height)
    pixel_size = half_width * 2.0 / width
    world_y = half_height - (23 + 0.875) * pixel_size
    to_y = 12.0 * world_y
    # the pitched row's direction y: (., world_y, -1) turned by the pitch, about 1e-17 where EPSILON is 1e-5
    norm = math.hypot(to_y, 12.0)
    assert abs(world_y * 12.0 / norm - to_y / norm) < 1e-12 and abs(world_y) > 100 * 1e-5
    t1 = csg("DIFFERENCE", leaf("cube", RED, T(-3, 0, 0)), leaf("cube", YELLOW, S(0.25), T(-3, 0.75, -0.75)))
    t2 = csg("UNION", leaf("cube", GREEN, S(0.5, 1, 1), T(-0.5, 0, 0)),
             leaf("cube", BLUE, S(0.5, 0.75, 0.75), T(0.5, 0, 0)))
    t3 = csg("INTERSECT", leaf("cube", CYAN, T(3, 0, 0)), leaf("sphere", MAGENTA, S(0.75), T(3, 0.25, -0.25)))
    write_scene("csg_ties_64x48", "coincident faces and tangent leaves: equal t across leaves",
                [floor(-1.5), t1, t2, t3],
                {"from": (0, 0, -12), "to": (0, to_y, 0), "size": (width, height), "fov": fov},
                {"point": (0, 6, -6), "corner": (-2, 6, -4), "uvec": (4, 0, 0), "vvec": (0, 0, 2)})


def scene_noshadow_glass():
    """One operand that casts no shadow per op; a non-casting sphere listed ahead of a casting cube, between it
    and the point light; a glass cube - sphere; a glass sphere inside a glass cube U cube."""
    def ghost(m):
        return m[:7] + (False,)
    u1 = csg("UNION", leaf("sphere", RED, S(0.7), T(-3, 0.7, 2)), leaf("cube", ghost(YELLOW), S(0.5), T(-2.5, 1.0, 1.75)))
    u2 = csg("INTERSECT", leaf("cube", ghost(GREEN), S(0.75), T(0, 0.75, 2)), leaf("sphere", BLUE, S(0.9), T(0.25, 1.0, 1.75)))
    u3 = csg("DIFFERENCE", leaf("cube", CYAN, S(0.75), T(3, 0.75, 2)), leaf("sphere", ghost(MAGENTA), S(0.7), T(3.25, 1.25, 1.5)))
    shield = leaf("sphere", ghost(ORANGE), S(0.6), T(-3, 3, -2))
    lit = leaf("cube", WHITE, S(0.5), T(-3, 0.5, -2))
    g1 = csg("DIFFERENCE", leaf("cube", GLASS, S(0.8), T(0, 0.8, -2.5)), leaf("sphere", GLASS, S(0.6), T(0.25, 1.25, -3.0)))
    g2 = csg("UNION", leaf("cube", GLASS, S(0.8), T(3, 0.8, -2.5)), leaf("cube", GLASS, S(0.6), T(3.5, 1.0, -2.5)))
    inner = leaf("sphere", GLASS, S(0.3), T(3, 0.8, -2.5))
    write_scene("csg_noshadow_glass_64x48", "members that cast no shadow; refraction through CSG units",
                [floor(), u1, u2, u3, shield, lit, g1, g2, inner],
                {"from": (0, 5, -11), "to": (0, 1, 0), "size": (64, 48), "fov": 0.8},
                {"point": (-3, 9, -2), "corner": (2, 8, -6), "uvec": (2, 0, 0), "vvec": (0, 0, 2)})


def scene_unsorted():
    """Units whose leaves return unsorted lists: closed cylinder - sphere, cube ^ cone, torus U cube, and
    sphere - open cylinder with min / max. The generator refuses the scene; the generic walk renders it."""
    s1 = csg("DIFFERENCE", leaf("cylinder", RED, S(0.8, 1.6, 0.8), T(-4.5, 0, 0), minimum=0.0, maximum=1.0, closed=True),
             leaf("sphere", YELLOW, S(0.6), T(-4.5, 1.6, -0.4)))
    s2 = csg("INTERSECT", leaf("cube", GREEN, S(0.8), T(-1.5, 0.8, 0)),
             leaf("cone", BLUE, S(1, 1.6, 1), T(-1.5, 1.8, 0), minimum=-1.0, maximum=0.0, closed=True))
    s3 = csg("UNION", leaf("toroid", CYAN, T(1.5, 0.5, 0)), leaf("cube", MAGENTA, S(0.3, 0.6, 0.3), T(1.5, 0.6, 0)))
    s4 = csg("DIFFERENCE", leaf("sphere", ORANGE, T(4.5, 1, 0)),
             leaf("cylinder", WHITE, S(0.4, 1, 0.4), ("rz", 0.5), T(4.5, 1, 0), minimum=-2.0, maximum=2.0, closed=False))
    write_scene("csg_unsorted_64x48", "units with cylinder, cone and torus leaves (the generic list walk)",
                [floor(), s1, s2, s3, s4],
                {"from": (0, 4, -11), "to": (0, 0.8, 0), "size": (64, 48), "fov": 0.9},
                {"point": (-5, 9, -7), "corner": (3, 8, -5), "uvec": (2, 0, 0), "vvec": (0, 0, 2)})


def scene_wide(count, name, purpose):
    """A left-deep UNION chain of small overlapping cubes, two entries each."""
    def cube(i):
        return leaf("cube", (RED, GREEN, BLUE, YELLOW)[i % 4], S(0.3), T(-3.0 + 0.375 * i, 0.3 + 0.125 * (i % 3), 0.25 * (i % 2)))
    chain = cube(0)
    for i in range(1, count):
        chain = csg("UNION", chain, cube(i))
    write_scene(name, purpose, [floor(), chain],
                {"from": (0, 3, -9), "to": (0, 0.5, 0), "size": (48, 48), "fov": 0.75},
                {"point": (-4, 8, -6), "corner": (2, 7, -4), "uvec": (2, 0, 0), "vvec": (0, 0, 2)})


def main():
    scene_ops()
    scene_nested()
    scene_nested(with_group=False)
    scene_ties()
    scene_noshadow_glass()
    scene_unsorted()
    scene_wide(16, "csg_wide32_48", "a unit of exactly 32 entries (16 cubes): the generator's limit")
    scene_wide(17, "csg_wide34_48", "a unit of 34 entries (17 cubes): one leaf over the generator's limit")


if __name__ == "__main__":
    main()
