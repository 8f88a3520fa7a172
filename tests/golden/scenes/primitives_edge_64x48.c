/* primitives_edge_64x48: every leaf type but CSG, transformed and grouped, for the first-hit tests
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
    cfg.scene.divide_threshold = 100000;
    cfg.output.file_path = "/tmp/frt_golden/out/primitives_edge_64x48";
    cfg.output.color_space = SRGB;

    struct aperture ap;
    aperture(POINT_APERTURE, 0.0, 1, 1, false, &ap);
    Point from = { 1.02, 7.1, -13.0, 1.0 };
    Point to = { 0.2, 0.8, 0.3, 1.0 };
    Vector up = { 0.0, 1.0, 0.0, 0.0 };
    Matrix view;
    view_transform(from, to, up, view);
    Camera cam = camera(64, 48, 0.9, 1.0, 2, 2, &ap, view);

    Light lights = array_of_lights(2);
    Point point_at = { -6.0, 10.0, -8.0, 1.0 };
    Color point_power = color(0.5, 0.5, 0.5);
    point_light(point_at, point_power, lights + 0);
    Point area_corner = { 3.0, 9.0, -5.0, 1.0 };
    Vector area_u = vector_init(2.0, 0.0, 0.0);
    Vector area_v = vector_init(0.0, 0.0, 2.0);
    Color area_power = color(0.5, 0.5, 0.5);
    area_light(area_corner, area_u, 4, area_v, 4, true, 1, area_power, lights + 1);

    Matrix t, u;
    Shape all = array_of_shapes(10);
    /* top-level shape 0 */
    plane(all + 0);
    shape_set_material(all + 0, mat(0.8, 0.8, 0.75, 0.15, 0.75, 0.3, 0.0, 0.0, 1.0, true));
    /* top-level shape 1 */
    sphere(all + 1);
    shape_set_material(all + 1, mat(0.9, 0.2, 0.15, 0.15, 0.75, 0.3, 0.0, 0.0, 1.0, true));
    matrix_identity(t);
    matrix_scale(0.9, 0.7, 0.8, u);
    transform_chain(u, t);
    matrix_rotate_y(0.4, u);
    transform_chain(u, t);
    matrix_rotate_z(0.2, u);
    transform_chain(u, t);
    matrix_translate(-5.0, 1.0, 2.5, u);
    transform_chain(u, t);
    shape_set_transform(all + 1, t);
    /* top-level shape 2 */
    cube(all + 2);
    shape_set_material(all + 2, mat(0.2, 0.8, 0.25, 0.15, 0.75, 0.3, 0.0, 0.0, 1.0, true));
    matrix_identity(t);
    matrix_scale(0.9, 0.7, 0.8, u);
    transform_chain(u, t);
    matrix_rotate_x(0.3, u);
    transform_chain(u, t);
    matrix_translate(-2.5, 1.2, 2.5, u);
    transform_chain(u, t);
    shape_set_transform(all + 2, t);
    /* top-level shape 3 */
    cylinder(all + 3);
    shape_set_material(all + 3, mat(0.2, 0.3, 0.9, 0.15, 0.75, 0.3, 0.0, 0.0, 1.0, true));
    (all + 3)->fields.cylinder.minimum = -0.5;
    (all + 3)->fields.cylinder.maximum = 1.5;
    (all + 3)->fields.cylinder.closed = true;
    matrix_identity(t);
    matrix_scale(0.6, 0.7, 0.5, u);
    transform_chain(u, t);
    matrix_rotate_y(0.5, u);
    transform_chain(u, t);
    matrix_translate(0.0, 1.0, 2.5, u);
    transform_chain(u, t);
    shape_set_transform(all + 3, t);
    /* top-level shape 4 */
    cylinder(all + 4);
    shape_set_material(all + 4, mat(0.85, 0.25, 0.8, 0.15, 0.75, 0.3, 0.0, 0.0, 1.0, true));
    (all + 4)->fields.cylinder.minimum = -1.0;
    (all + 4)->fields.cylinder.maximum = 1.0;
    (all + 4)->fields.cylinder.closed = false;
    matrix_identity(t);
    matrix_scale(0.5, 0.8, 0.6, u);
    transform_chain(u, t);
    matrix_rotate_x(0.9, u);
    transform_chain(u, t);
    matrix_rotate_z(-0.3, u);
    transform_chain(u, t);
    matrix_translate(2.5, 1.3, 2.5, u);
    transform_chain(u, t);
    shape_set_transform(all + 4, t);
    /* top-level shape 5 */
    cone(all + 5);
    shape_set_material(all + 5, mat(0.9, 0.9, 0.9, 0.15, 0.75, 0.3, 0.0, 0.0, 1.0, true));
    (all + 5)->fields.cone.minimum = -1.0;
    (all + 5)->fields.cone.maximum = 0.5;
    (all + 5)->fields.cone.closed = true;
    matrix_identity(t);
    matrix_scale(0.8, 0.8, 0.8, u);
    transform_chain(u, t);
    matrix_translate(5.0, 1.0, 2.5, u);
    transform_chain(u, t);
    shape_set_transform(all + 5, t);
    /* top-level shape 6 */
    cone(all + 6);
    shape_set_material(all + 6, mat(0.9, 0.5, 0.6, 0.15, 0.75, 0.3, 0.0, 0.0, 1.0, true));
    (all + 6)->fields.cone.minimum = 0.25;
    (all + 6)->fields.cone.maximum = 1.0;
    (all + 6)->fields.cone.closed = false;
    matrix_identity(t);
    matrix_scale(0.9, 1.2, 0.7, u);
    transform_chain(u, t);
    matrix_rotate_y(0.6, u);
    transform_chain(u, t);
    matrix_rotate_z(0.25, u);
    transform_chain(u, t);
    matrix_translate(-4.0, 0.5, -2.0, u);
    transform_chain(u, t);
    shape_set_transform(all + 6, t);
    /* top-level shape 7 */
    toroid(all + 7);
    shape_set_material(all + 7, mat(0.15, 0.6, 0.55, 0.15, 0.75, 0.3, 0.0, 0.0, 1.0, true));
    (all + 7)->fields.toroid.r1 = 1.0;
    (all + 7)->fields.toroid.r2 = 0.35;
    matrix_identity(t);
    matrix_scale(0.7, 0.75, 0.65, u);
    transform_chain(u, t);
    matrix_rotate_x(0.5, u);
    transform_chain(u, t);
    matrix_rotate_y(0.3, u);
    transform_chain(u, t);
    matrix_translate(-1.0, 0.9, -2.0, u);
    transform_chain(u, t);
    shape_set_transform(all + 7, t);
    /* top-level shape 8 */
    toroid(all + 8);
    shape_set_material(all + 8, mat(0.6, 0.6, 0.65, 0.15, 0.75, 0.3, 0.0, 0.0, 1.0, true));
    (all + 8)->fields.toroid.r1 = 0.6;
    (all + 8)->fields.toroid.r2 = 0.5;
    matrix_identity(t);
    matrix_scale(0.75, 0.8, 0.85, u);
    transform_chain(u, t);
    matrix_rotate_x(-0.4, u);
    transform_chain(u, t);
    matrix_rotate_z(0.3, u);
    transform_chain(u, t);
    matrix_translate(2.0, 1.0, -2.0, u);
    transform_chain(u, t);
    shape_set_transform(all + 8, t);
    /* top-level shape 9 */
    Shape g1 = array_of_shapes(1);
    Shape g2 = array_of_shapes(3);
    Point p3 = { -0.75, 0.0, 0.1, 1.0 };
    Point p4 = { 0.75, 0.0, -0.1, 1.0 };
    Point p5 = { 0.8, 1.25, 0.15, 1.0 };
    triangle(g2 + 0, p3, p4, p5);
    shape_set_material(g2 + 0, mat(0.9, 0.85, 0.2, 0.15, 0.75, 0.3, 0.0, 0.0, 1.0, true));
    matrix_identity(t);
    matrix_scale(1.5, 1.2, 1.0, u);
    transform_chain(u, t);
    matrix_rotate_x(0.2, u);
    transform_chain(u, t);
    matrix_translate(0.0, 0.3, 0.0, u);
    transform_chain(u, t);
    shape_set_transform(g2 + 0, t);
    Point p6 = { -0.75, 0.0, 0.1, 1.0 };
    Point p7 = { 0.8, 1.25, 0.15, 1.0 };
    Point p8 = { -0.7, 1.0, -0.05, 1.0 };
    triangle(g2 + 1, p6, p7, p8);
    shape_set_material(g2 + 1, mat(0.95, 0.55, 0.15, 0.15, 0.75, 0.3, 0.0, 0.0, 1.0, true));
    matrix_identity(t);
    matrix_scale(1.5, 1.2, 1.0, u);
    transform_chain(u, t);
    matrix_rotate_x(0.2, u);
    transform_chain(u, t);
    matrix_translate(0.0, 0.3, 0.0, u);
    transform_chain(u, t);
    shape_set_transform(g2 + 1, t);
    Point p9 = { -0.6, 0.0, 0.0, 1.0 };
    Point p10 = { 0.6, 0.1, 0.0, 1.0 };
    Point p11 = { 0.1, 1.1, 0.2, 1.0 };
    Vector n12 = { -0.3698001308168195, 0.09245003270420488, -0.9245003270420487, 0.0 };
    Vector n13 = { 0.4402254531628119, -0.1760901812651248, -0.8804509063256238, 0.0 };
    Vector n14 = { 0.042835293687811936, 0.5140235242537432, -0.8567058737562386, 0.0 };
    smooth_triangle(g2 + 2, p9, p10, p11, n12, n13, n14);
    shape_set_material(g2 + 2, mat(0.2, 0.85, 0.85, 0.15, 0.75, 0.3, 0.0, 0.0, 1.0, true));
    matrix_identity(t);
    matrix_scale(1.7, 1.4, 1.0, u);
    transform_chain(u, t);
    matrix_rotate_y(-0.3, u);
    transform_chain(u, t);
    matrix_translate(0.2, 1.55, 1.4, u);
    transform_chain(u, t);
    shape_set_transform(g2 + 2, t);
    group(g1 + 0, g2, 3);
    matrix_identity(t);
    matrix_scale(1.2, 1.0, 0.9, u);
    transform_chain(u, t);
    matrix_rotate_z(0.1, u);
    transform_chain(u, t);
    matrix_translate(0.0, 0.15, 0.0, u);
    transform_chain(u, t);
    shape_set_transform(g1 + 0, t);
    group(all + 9, g1, 1);
    matrix_identity(t);
    matrix_rotate_y(0.3, u);
    transform_chain(u, t);
    matrix_translate(4.6, 0.0, -2.0, u);
    transform_chain(u, t);
    shape_set_transform(all + 9, t);

    Shape top = array_of_shapes(1);
    group(top, all, 10);
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
