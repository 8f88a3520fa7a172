/* csg_noshadow_glass_64x48: members that cast no shadow; refraction through CSG units
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
    cfg.output.file_path = "/tmp/frt_golden/out/csg_noshadow_glass_64x48";
    cfg.output.color_space = SRGB;

    struct aperture ap;
    aperture(POINT_APERTURE, 0.0, 1, 1, false, &ap);
    Point from = { 0.0, 5.0, -11.0, 1.0 };
    Point to = { 0.0, 1.0, 0.0, 1.0 };
    Vector up = { 0.0, 1.0, 0.0, 0.0 };
    Matrix view;
    view_transform(from, to, up, view);
    Camera cam = camera(64, 48, 0.8, 1.0, 2, 2, &ap, view);

    Light lights = array_of_lights(2);
    Point point_at = { -3.0, 9.0, -2.0, 1.0 };
    Color point_power = color(0.5, 0.5, 0.5);
    point_light(point_at, point_power, lights + 0);
    Point area_corner = { 2.0, 8.0, -6.0, 1.0 };
    Vector area_u = vector_init(2.0, 0.0, 0.0);
    Vector area_v = vector_init(0.0, 0.0, 2.0);
    Color area_power = color(0.5, 0.5, 0.5);
    area_light(area_corner, area_u, 4, area_v, 4, true, 1, area_power, lights + 1);

    Matrix t, u;
    Shape all = array_of_shapes(9);
    /* top-level shape 0 */
    plane(all + 0);
    shape_set_material(all + 0, mat(0.8, 0.8, 0.75, 0.15, 0.75, 0.3, 0.0, 0.0, 1.0, true));
    /* top-level shape 1 */
    Shape k1 = array_of_shapes(2);
    sphere(k1 + 0);
    shape_set_material(k1 + 0, mat(0.9, 0.2, 0.15, 0.15, 0.75, 0.3, 0.0, 0.0, 1.0, true));
    matrix_identity(t);
    matrix_scale(0.7, 0.7, 0.7, u);
    transform_chain(u, t);
    matrix_translate(-3.0, 0.7, 2.0, u);
    transform_chain(u, t);
    shape_set_transform(k1 + 0, t);
    cube(k1 + 1);
    shape_set_material(k1 + 1, mat(0.9, 0.85, 0.2, 0.15, 0.75, 0.3, 0.0, 0.0, 1.0, false));
    matrix_identity(t);
    matrix_scale(0.5, 0.5, 0.5, u);
    transform_chain(u, t);
    matrix_translate(-2.5, 1.0, 1.75, u);
    transform_chain(u, t);
    shape_set_transform(k1 + 1, t);
    csg(all + 1, CSG_UNION, k1 + 0, k1 + 1);
    /* top-level shape 2 */
    Shape k2 = array_of_shapes(2);
    cube(k2 + 0);
    shape_set_material(k2 + 0, mat(0.2, 0.8, 0.25, 0.15, 0.75, 0.3, 0.0, 0.0, 1.0, false));
    matrix_identity(t);
    matrix_scale(0.75, 0.75, 0.75, u);
    transform_chain(u, t);
    matrix_translate(0.0, 0.75, 2.0, u);
    transform_chain(u, t);
    shape_set_transform(k2 + 0, t);
    sphere(k2 + 1);
    shape_set_material(k2 + 1, mat(0.2, 0.3, 0.9, 0.15, 0.75, 0.3, 0.0, 0.0, 1.0, true));
    matrix_identity(t);
    matrix_scale(0.9, 0.9, 0.9, u);
    transform_chain(u, t);
    matrix_translate(0.25, 1.0, 1.75, u);
    transform_chain(u, t);
    shape_set_transform(k2 + 1, t);
    csg(all + 2, CSG_INTERSECT, k2 + 0, k2 + 1);
    /* top-level shape 3 */
    Shape k3 = array_of_shapes(2);
    cube(k3 + 0);
    shape_set_material(k3 + 0, mat(0.2, 0.85, 0.85, 0.15, 0.75, 0.3, 0.0, 0.0, 1.0, true));
    matrix_identity(t);
    matrix_scale(0.75, 0.75, 0.75, u);
    transform_chain(u, t);
    matrix_translate(3.0, 0.75, 2.0, u);
    transform_chain(u, t);
    shape_set_transform(k3 + 0, t);
    sphere(k3 + 1);
    shape_set_material(k3 + 1, mat(0.85, 0.25, 0.8, 0.15, 0.75, 0.3, 0.0, 0.0, 1.0, false));
    matrix_identity(t);
    matrix_scale(0.7, 0.7, 0.7, u);
    transform_chain(u, t);
    matrix_translate(3.25, 1.25, 1.5, u);
    transform_chain(u, t);
    shape_set_transform(k3 + 1, t);
    csg(all + 3, CSG_DIFFERENCE, k3 + 0, k3 + 1);
    /* top-level shape 4 */
    sphere(all + 4);
    shape_set_material(all + 4, mat(0.95, 0.55, 0.15, 0.15, 0.75, 0.3, 0.0, 0.0, 1.0, false));
    matrix_identity(t);
    matrix_scale(0.6, 0.6, 0.6, u);
    transform_chain(u, t);
    matrix_translate(-3.0, 3.0, -2.0, u);
    transform_chain(u, t);
    shape_set_transform(all + 4, t);
    /* top-level shape 5 */
    cube(all + 5);
    shape_set_material(all + 5, mat(0.9, 0.9, 0.9, 0.15, 0.75, 0.3, 0.0, 0.0, 1.0, true));
    matrix_identity(t);
    matrix_scale(0.5, 0.5, 0.5, u);
    transform_chain(u, t);
    matrix_translate(-3.0, 0.5, -2.0, u);
    transform_chain(u, t);
    shape_set_transform(all + 5, t);
    /* top-level shape 6 */
    Shape k4 = array_of_shapes(2);
    cube(k4 + 0);
    shape_set_material(k4 + 0, mat(1.0, 1.0, 1.0, 0.0, 0.05, 0.9, 0.9, 1.0, 1.5, true));
    matrix_identity(t);
    matrix_scale(0.8, 0.8, 0.8, u);
    transform_chain(u, t);
    matrix_translate(0.0, 0.8, -2.5, u);
    transform_chain(u, t);
    shape_set_transform(k4 + 0, t);
    sphere(k4 + 1);
    shape_set_material(k4 + 1, mat(1.0, 1.0, 1.0, 0.0, 0.05, 0.9, 0.9, 1.0, 1.5, true));
    matrix_identity(t);
    matrix_scale(0.6, 0.6, 0.6, u);
    transform_chain(u, t);
    matrix_translate(0.25, 1.25, -3.0, u);
    transform_chain(u, t);
    shape_set_transform(k4 + 1, t);
    csg(all + 6, CSG_DIFFERENCE, k4 + 0, k4 + 1);
    /* top-level shape 7 */
    Shape k5 = array_of_shapes(2);
    cube(k5 + 0);
    shape_set_material(k5 + 0, mat(1.0, 1.0, 1.0, 0.0, 0.05, 0.9, 0.9, 1.0, 1.5, true));
    matrix_identity(t);
    matrix_scale(0.8, 0.8, 0.8, u);
    transform_chain(u, t);
    matrix_translate(3.0, 0.8, -2.5, u);
    transform_chain(u, t);
    shape_set_transform(k5 + 0, t);
    cube(k5 + 1);
    shape_set_material(k5 + 1, mat(1.0, 1.0, 1.0, 0.0, 0.05, 0.9, 0.9, 1.0, 1.5, true));
    matrix_identity(t);
    matrix_scale(0.6, 0.6, 0.6, u);
    transform_chain(u, t);
    matrix_translate(3.5, 1.0, -2.5, u);
    transform_chain(u, t);
    shape_set_transform(k5 + 1, t);
    csg(all + 7, CSG_UNION, k5 + 0, k5 + 1);
    /* top-level shape 8 */
    sphere(all + 8);
    shape_set_material(all + 8, mat(1.0, 1.0, 1.0, 0.0, 0.05, 0.9, 0.9, 1.0, 1.5, true));
    matrix_identity(t);
    matrix_scale(0.3, 0.3, 0.3, u);
    transform_chain(u, t);
    matrix_translate(3.0, 0.8, -2.5, u);
    transform_chain(u, t);
    shape_set_transform(all + 8, t);

    Shape top = array_of_shapes(1);
    group(top, all, 9);
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
