/*
 * The reprojection's host pass (host/frt_reproject.c, built with FRT_REPROJECT_STANDALONE, and the matrix inverse it
 * calls) under the address and undefined-behaviour sanitizers, without Python in the process: the cases whose tap
 * coordinates would leave the image or overflow an integer conversion if the range test came late. Exits 0 and prints
 * "OK ..." when every case ran and counted what it must.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "frt_reproject.h"

static void
look(frt_camera *c, int64_t w, int64_t h, double fx, double fy, double fz, double yaw)
{
    /* the inverse of a view transform: a rotation about y by yaw, then a translation to (fx, fy, fz) */
    memset(c, 0, sizeof(*c));
    c->hsize = w;
    c->vsize = h;
    c->usteps = c->vsteps = 1;
    c->canvas_distance = 1.0;
    c->half_width = tan(0.5);
    c->half_height = c->half_width * (double)h / (double)w;
    c->pixel_size = c->half_width * 2.0 / (double)w;
    const double cs = cos(yaw), sn = sin(yaw);
    const double m[16] = {cs, 0, sn, fx, 0, 1, 0, fy, -sn, 0, cs, fz, 0, 0, 0, 1};
    memcpy(c->inv, m, sizeof(m));
}

static int failures = 0;

#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            printf("FAILED line %d: %s\n", __LINE__, #cond);           \
            failures += 1;                                             \
        }                                                              \
    } while (0)

static void
run(const char *name, const frt_camera *prev, const frt_camera *cur, int64_t w, int64_t h, double depth,
    double prev_depth, frt_reproject_stats *st)
{
    const size_t npx = (size_t)(w * h);
    int32_t *sn = malloc(npx * sizeof(int32_t)), *dn = malloc(npx * sizeof(int32_t));
    double *smean = malloc(npx * 4 * sizeof(double)), *dmean = malloc(npx * 4 * sizeof(double));
    double *sm2 = malloc(npx * 3 * sizeof(double)), *dm2 = malloc(npx * 3 * sizeof(double));
    double *pg = calloc(npx * 8, sizeof(double)), *cg = calloc(npx * 8, sizeof(double));
    int32_t *pi = calloc(npx * 2, sizeof(int32_t)), *ci = calloc(npx * 2, sizeof(int32_t));
    for (size_t i = 0; i < npx; ++i) {
        sn[i] = (int32_t)(i % 5);
        for (int k = 0; k < 4; ++k) {
            smean[4 * i + k] = 0.25 * (double)((i + (size_t)k) % 7);
        }
        for (int k = 0; k < 3; ++k) {
            sm2[3 * i + k] = 0.125 * (double)(i % 3);
        }
        /* every sixth current depth is a NaN, an infinity or a huge or tiny number (1e150: its square is finite) */
        const double odd[6] = {depth, NAN, depth, INFINITY, 1e150, 1e-300};
        cg[8 * i] = odd[i % 6];
        pg[8 * i] = i % 7 == 3 ? NAN : prev_depth;
        cg[8 * i + 3] = pg[8 * i + 3] = 1.0;
        ci[2 * i] = i % 11 == 10 ? -1 : 0;
    }
    frt_reproject_params p;
    frt_reproject_defaults(&p);
    frt_reproject_geometry g;
    CHECK(frt_reproject_setup(prev, cur, &g) == 0);
    memset(st, 0, sizeof(*st));
    const int rc = frt_reproject_host(dn, dmean, dm2, sn, smean, sm2, prev, cur, &g, pg, pi, cg, ci, w, h, &p, st);
    CHECK(rc == 0);
    CHECK(st->reprojected + st->missed + st->no_history == npx);
    for (size_t i = 0; i < npx; ++i) {
        CHECK(dn[i] >= 0 && dn[i] <= p.max_history);
        CHECK(isfinite(dmean[4 * i]) && isfinite(dm2[3 * i]));
    }
    printf("%-28s reprojected %llu missed %llu no_history %llu\n", name, (unsigned long long)st->reprojected,
           (unsigned long long)st->missed, (unsigned long long)st->no_history);
    free(sn), free(dn), free(smean), free(dmean), free(sm2), free(dm2), free(pg), free(cg), free(pi), free(ci);
}

int
main(void)
{
    frt_camera a, b;
    frt_reproject_stats st;
    const int64_t w = 37, h = 5;

    /* the same camera: the finite depths come back */
    look(&a, w, h, 0, 0, 5, 0);
    run("identical", &a, &a, w, h, 5.0, 5.0, &st);
    CHECK(st.reprojected > 0 && st.missed > 0);

    /* out of range: the previous camera looks far to the side, and a huge depth lands astronomically far outside */
    look(&b, w, h, 0, 0, 5, 1.2);
    run("rotated out of range", &b, &a, w, h, 5.0, 5.0, &st);
    CHECK(st.reprojected == 0 && st.no_history > 0);
    look(&b, w, h, 1e6, -1e6, 5, 0);
    run("panned far out of range", &b, &a, w, h, 5.0, 5.0, &st);
    CHECK(st.reprojected == 0);

    /* behind the previous camera: it stands beyond the surface, looking the same way */
    look(&b, w, h, 0, 0, -3, 0);
    run("behind the camera", &b, &a, w, h, 5.0, 5.0, &st);
    CHECK(st.reprojected == 0 && st.no_history > 0);
    /* on the previous camera's plane: c.z == 0, the division's infinity never reaches a conversion */
    look(&b, w, h, 0, 0, 0, 0);
    run("on the camera plane", &b, &a, w, h, 5.0, 5.0, &st);

    /* NaN depths in the previous frame alone */
    run("NaN previous depths", &a, &a, w, h, 5.0, NAN, &st);
    CHECK(st.reprojected == 0);

    /* the refusals this build can reach */
    frt_reproject_geometry g;
    b = a;
    b.hsize = w + 1;
    CHECK(frt_reproject_setup(&a, &b, &g) == -1);
    b = a;
    b.inv[3] = NAN;
    CHECK(frt_reproject_setup(&b, &a, &g) == -1 && frt_reproject_standalone_error()[0] != 0);
    memset(b.inv, 0, sizeof(b.inv));
    CHECK(frt_reproject_setup(&b, &a, &g) == -1);

    if (failures != 0) {
        printf("%d checks failed\n", failures);
        return 1;
    }
    printf("OK reprojection host pass under the sanitizers\n");
    return 0;
}
