/*
 * frt-mi355x: the reprojection's host pass, which is its definition (include/frt_device.h "Reprojection", DESIGN.md
 * "Temporal reprojection").
 *
 * An accumulator's state carried from the previous camera's pixels to the current camera's: per destination pixel the
 * world point of its centre ray at the first-hit depth, that point's place in the previous frame, and a bilinear
 * gather of the four states around it that pass the id, depth and normal tests. Binary64 with + - * /, sqrt, floor
 * and comparisons only, in the order written here (this file is compiled with -ffp-contract=off), so the device pass
 * (csrc/frt_accum.hip k_accum_reproject) repeats it bit for bit: rp_pixel here, k_accum_reproject there.
 *
 * With FRT_REPROJECT_STANDALONE the file builds without libfrt_device and the accumulator objects: the setup and the
 * pass on plain arrays alone (it then needs matrix_inverse, host/frt_linalg.c, and nothing else).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "frt_reproject.h"
#include "src/libs/linalg/linalg.h"

#ifdef FRT_REPROJECT_STANDALONE
static const char *s_error = "";

const char *
frt_reproject_standalone_error(void)
{
    return s_error;
}

static int
refuse(const char *what)
{
    s_error = what;
    return -1;
}
#else
#include "frt_flatten.h"

static int
refuse(const char *what)
{
    frt_accum_set_error(what);
    return -1;
}
#endif

static double
clock_ms(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec * 1e3 + (double)ts.tv_nsec * 1e-6;
}

size_t
frt_reproject_params_size(void)
{
    return sizeof(frt_reproject_params);
}

size_t
frt_reproject_stats_size(void)
{
    return sizeof(frt_reproject_stats);
}

void
frt_reproject_defaults(frt_reproject_params *p)
{
    if (p == NULL) {
        return;
    }
    p->max_history = 32;
    p->match_material = 1;
    p->normal_cos = 0.9;
    p->sigma_depth = 0.02;
    p->min_weight = 0x1p-6;
}

const char *
frt_reproject_params_reason(const frt_reproject_params *p)
{
    if (p->max_history < 1 || p->max_history > (1 << 20)) {
        return "frt_reproject: max_history must be 1 .. 2^20";
    }
    if (p->match_material != 0 && p->match_material != 1) {
        return "frt_reproject: match_material must be 0 or 1";
    }
    if (!(isfinite(p->normal_cos) && p->normal_cos > 0.0 && p->normal_cos <= 1.0)) {
        return "frt_reproject: normal_cos must be in (0, 1]";
    }
    if (!(isfinite(p->sigma_depth) && p->sigma_depth > 0.0)) {
        return "frt_reproject: sigma_depth must be finite and > 0";
    }
    if (!(isfinite(p->min_weight) && p->min_weight > 0.0 && p->min_weight <= 1.0)) {
        return "frt_reproject: min_weight must be in (0, 1]";
    }
    return NULL;
}

/* matrix_point_multiply on three coordinates, in the engine's xf_point grouping */
static void
xf_point(const double *m, const double *p, double *r)
{
    const double x = ((m[0] * p[0] + m[1] * p[1]) + m[2] * p[2]) + m[3];
    const double y = ((m[4] * p[0] + m[5] * p[1]) + m[6] * p[2]) + m[7];
    const double z = ((m[8] * p[0] + m[9] * p[1]) + m[10] * p[2]) + m[11];
    r[0] = x;
    r[1] = y;
    r[2] = z;
}

static double
dot3(const double *a, const double *b)
{
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

static int
camera_finite(const frt_camera *c)
{
    for (int i = 0; i < 16; ++i) {
        if (!isfinite(c->inv[i])) {
            return 0;
        }
    }
    return isfinite(c->half_width) && isfinite(c->half_height) && isfinite(c->pixel_size) &&
           isfinite(c->canvas_distance);
}

int
frt_reproject_setup(const frt_camera *prev, const frt_camera *cur, frt_reproject_geometry *out)
{
    if (prev == NULL || cur == NULL || out == NULL) {
        return refuse("frt_reproject_setup: a null pointer");
    }
    if (prev->hsize <= 0 || prev->vsize <= 0 || prev->hsize != cur->hsize || prev->vsize != cur->vsize) {
        return refuse("frt_reproject_setup: the two cameras' sizes differ (or are not positive)");
    }
    if (!camera_finite(prev) || !camera_finite(cur)) {
        return refuse("frt_reproject_setup: a camera's matrix or scalars are not finite");
    }
    frt_reproject_geometry g;
    const double zero[3] = {0.0, 0.0, 0.0};
    xf_point(cur->inv, zero, g.o_cur);
    xf_point(prev->inv, zero, g.o_prev);
    Matrix fwd;
    matrix_inverse(prev->inv, fwd);
    for (int i = 0; i < 16; ++i) {
        if (!isfinite(fwd[i])) {
            return refuse("frt_reproject_setup: the previous camera's matrix has no finite inverse");
        }
        g.prev_fwd[i] = fwd[i];
    }
    *out = g;
    return 0;
}

typedef struct rp_view {
    const frt_camera *prev, *cur;
    const frt_reproject_geometry *g;
    const frt_reproject_params *p;
    const int32_t *sn;
    const double *smean, *sm2;
    const double *pgeom, *cgeom;
    const int32_t *pids, *cids;
    int32_t w, h;
    double cos2;
} rp_view;

/* one destination pixel: its state into n, mean[4], m2[3]; returns the outcome code */
static int
rp_pixel(const rp_view *v, int32_t px, int32_t py, int32_t *n, double *mean, double *m2)
{
    *n = 0;
    mean[0] = mean[1] = mean[2] = mean[3] = 0.0;
    m2[0] = m2[1] = m2[2] = 0.0;
    const int32_t i = py * v->w + px;
    /* 1 */
    const int32_t node = v->cids[2 * (size_t)i], mat = v->cids[2 * (size_t)i + 1];
    const double *cg = v->cgeom + 8 * (size_t)i;
    const double d = cg[0];
    if (!(node >= 0 && isfinite(d) && d > 0.0)) {
        return 1;
    }
    /* 2 */
    const frt_camera *cur = v->cur, *prev = v->prev;
    const double xoff = ((double)px + 0.5) * cur->pixel_size;
    const double yoff = ((double)py + 0.5) * cur->pixel_size;
    const double cp[3] = {cur->half_width - xoff, cur->half_height - yoff, -cur->canvas_distance};
    double P[3];
    xf_point(cur->inv, cp, P);
    const double *oc = v->g->o_cur, *op = v->g->o_prev;
    const double vv[3] = {P[0] - oc[0], P[1] - oc[1], P[2] - oc[2]};
    const double inv = 1.0 / sqrt(dot3(vv, vv));
    double W[3];
    for (int k = 0; k < 3; ++k) {
        const double dir = vv[k] * inv;
        const double t = d * dir;
        W[k] = oc[k] + t;
    }
    /* 3 */
    double c[3];
    xf_point(v->g->prev_fwd, W, c);
    if (!(isfinite(c[2]) && c[2] < 0.0)) {
        return 2;
    }
    const double s = -prev->canvas_distance / c[2];
    double fx = (prev->half_width - c[0] * s) / prev->pixel_size - 0.5;
    double fy = (prev->half_height - c[1] * s) / prev->pixel_size - 0.5;
    const double rx = floor(fx + 0.5), ry = floor(fy + 0.5);
    if (fabs(fx - rx) <= 0x1p-20) {
        fx = rx;
    }
    if (fabs(fy - ry) <= 0x1p-20) {
        fy = ry;
    }
    if (!(fx >= -1.0 && fx < (double)v->w && fy >= -1.0 && fy < (double)v->h)) {
        return 2;
    }
    const double flx = floor(fx), fly = floor(fy);
    const int32_t x0 = (int32_t)flx, y0 = (int32_t)fly;
    const double tx = fx - flx, ty = fy - fly;
    /* 4 */
    const double u[3] = {W[0] - op[0], W[1] - op[1], W[2] - op[2]};
    const double e = sqrt(dot3(u, u));
    const double tol = v->p->sigma_depth * e;
    const double *np_ = cg + 1;
    const double nnp = dot3(np_, np_);
    /* 5, 6 */
    const double ux = 1.0 - tx, uy = 1.0 - ty;
    const double wt[4] = {ux * uy, tx * uy, ux * ty, tx * ty};
    double ws = 0.0, an = 0.0, am[4] = {0.0, 0.0, 0.0, 0.0}, av[3] = {0.0, 0.0, 0.0};
    for (int t = 0; t < 4; ++t) {
        const int32_t qx = x0 + (t & 1), qy = y0 + (t >> 1);
        if (qx < 0 || qx >= v->w || qy < 0 || qy >= v->h) {
            continue;
        }
        const int32_t q = qy * v->w + qx;
        const int32_t nq = v->sn[q];
        if (!(nq > 0)) {
            continue;
        }
        if (v->pids[2 * (size_t)q] != node || (v->p->match_material && v->pids[2 * (size_t)q + 1] != mat)) {
            continue;
        }
        const double *qg = v->pgeom + 8 * (size_t)q;
        const double zq = qg[0];
        if (!(isfinite(zq) && zq > 0.0)) {
            continue;
        }
        if (!(fabs(zq - e) <= tol)) {
            continue;
        }
        const double dn = dot3(np_, qg + 1);
        const double nnq = dot3(qg + 1, qg + 1);
        if (!(dn > 0.0 && dn * dn >= v->cos2 * (nnp * nnq))) {
            continue;
        }
        const double w = wt[t], dq = (double)nq;
        ws = ws + w;
        for (int ch = 0; ch < 4; ++ch) {
            am[ch] = am[ch] + w * v->smean[4 * (size_t)q + ch];
        }
        for (int ch = 0; ch < 3; ++ch) {
            av[ch] = av[ch] + w * (v->sm2[3 * (size_t)q + ch] / dq);
        }
        an = an + w * dq;
    }
    if (!(ws >= v->p->min_weight)) {
        return 2;
    }
    /* 7 */
    const double r = an / ws + 0.5;
    int32_t nn = r >= (double)v->p->max_history ? v->p->max_history : (int32_t)r;
    if (nn < 1) {
        nn = 1;
    }
    *n = nn;
    for (int ch = 0; ch < 4; ++ch) {
        mean[ch] = am[ch] / ws;
    }
    for (int ch = 0; ch < 3; ++ch) {
        m2[ch] = (av[ch] / ws) * (double)nn;
    }
    return 0;
}

static int
check_common(const frt_camera *prev, const frt_camera *cur, int64_t w, int64_t h, const frt_reproject_params *p)
{
    if (w <= 0 || h <= 0 || w > 0x7fffffffll || h > 0x7fffffffll || w * h > 0x7fffffffll) {
        return refuse("frt_reproject: w and h must be positive, with at most 2^31 - 1 pixels");
    }
    if (prev->hsize != w || prev->vsize != h || cur->hsize != w || cur->vsize != h) {
        return refuse("frt_reproject: the two cameras must both be w x h");
    }
    const char *why = frt_reproject_params_reason(p);
    return why != NULL ? refuse(why) : 0;
}

int
frt_reproject_host(int32_t *dst_n, double *dst_mean, double *dst_m2, const int32_t *src_n, const double *src_mean,
                   const double *src_m2, const frt_camera *prev, const frt_camera *cur, const frt_reproject_geometry *g,
                   const double *prev_geom, const int32_t *prev_ids, const double *cur_geom, const int32_t *cur_ids,
                   int64_t w, int64_t h, const frt_reproject_params *p, frt_reproject_stats *st)
{
    if (dst_n == NULL || dst_mean == NULL || dst_m2 == NULL || src_n == NULL || src_mean == NULL || src_m2 == NULL ||
        prev == NULL || cur == NULL || g == NULL || prev_geom == NULL || prev_ids == NULL || cur_geom == NULL ||
        cur_ids == NULL || p == NULL) {
        return refuse("frt_reproject: a null pointer");
    }
    if (dst_n == src_n || dst_mean == src_mean || dst_m2 == src_m2) {
        return refuse("frt_reproject: the destination is the source");
    }
    if (check_common(prev, cur, w, h, p) != 0) {
        return -1;
    }
    const double t0 = clock_ms();
    rp_view v = {prev, cur, g, p, src_n, src_mean, src_m2, prev_geom, cur_geom, prev_ids, cur_ids, (int32_t)w,
                 (int32_t)h, p->normal_cos * p->normal_cos};
    uint64_t count[3] = {0, 0, 0};
    for (int32_t py = 0; py < v.h; ++py) {
        for (int32_t px = 0; px < v.w; ++px) {
            const size_t i = (size_t)py * (size_t)v.w + (size_t)px;
            count[rp_pixel(&v, px, py, dst_n + i, dst_mean + 4 * i, dst_m2 + 3 * i)] += 1;
        }
    }
    if (st != NULL) {
        memset(st, 0, sizeof(*st));
        st->pixels = (uint64_t)(w * h);
        st->reprojected = count[0];
        st->missed = count[1];
        st->no_history = count[2];
        st->device = -1;
        st->host_ms = clock_ms() - t0;
    }
    return 0;
}

#ifndef FRT_REPROJECT_STANDALONE

int
frt_accum_reproject(frt_accum *dst, frt_accum *src, const frt_camera *prev, const frt_camera *cur,
                    const frt_feature_buffers *pf, const frt_feature_buffers *cf, int64_t w, int64_t h,
                    const frt_reproject_params *p, int on_device, frt_reproject_stats *st)
{
    if (dst == NULL || src == NULL || prev == NULL || cur == NULL || pf == NULL || cf == NULL || p == NULL ||
        pf->geom == NULL || pf->ids == NULL || cf->geom == NULL || cf->ids == NULL) {
        return refuse("frt_accum_reproject: a null pointer (both buffers of both views are needed)");
    }
    if (dst == src) {
        return refuse("frt_accum_reproject: the destination is the source");
    }
    frt_accum_dev *ddev = frt_accum_device_part(dst), *sdev = frt_accum_device_part(src);
    if ((ddev == NULL) != (sdev == NULL)) {
        return refuse("frt_accum_reproject: one host and one device accumulator (different devices)");
    }
    if (check_common(prev, cur, w, h, p) != 0) {
        return -1;
    }
    frt_reproject_geometry g;
    if (ddev != NULL) {
        /* (the device entry point refuses sizes and devices that differ before the setup's message could mislead) */
        if (frt_accum_dev_npixels(ddev) != w * h || frt_accum_dev_npixels(sdev) != w * h) {
            return refuse("frt_accum_reproject: w * h is not the accumulators' npixels");
        }
        if (frt_reproject_setup(prev, cur, &g) != 0) {
            return -1;
        }
        return frt_accum_dev_reproject(ddev, sdev, prev, cur, &g, pf, cf, w, h, p, on_device, st);
    }
    if (on_device) {
        return refuse("frt_accum_reproject: device memory given to a host accumulator");
    }
    int64_t dnpx = 0, snpx = 0;
    int32_t *dn, *sn;
    double *dmean, *dm2, *smean, *sm2;
    uint64_t *dframes, *dskipped, *sframes, *sskipped;
    frt_accum_host_state(dst, &dnpx, &dn, &dmean, &dm2, &dframes, &dskipped);
    frt_accum_host_state(src, &snpx, &sn, &smean, &sm2, &sframes, &sskipped);
    if (dnpx != w * h || snpx != w * h) {
        return refuse("frt_accum_reproject: w * h is not the accumulators' npixels");
    }
    if (frt_reproject_setup(prev, cur, &g) != 0) {
        return -1;
    }
    if (frt_reproject_host(dn, dmean, dm2, sn, smean, sm2, prev, cur, &g, pf->geom, pf->ids, cf->geom, cf->ids, w, h,
                           p, st) != 0) {
        return -1;
    }
    *dframes = *sframes < (uint64_t)p->max_history ? *sframes : (uint64_t)p->max_history;
    *dskipped = 0;
    return 0;
}

int
frt_accum_reproject_cameras(frt_accum *dst, frt_accum *src, Camera prev_cam, Camera cur_cam,
                            const frt_feature_buffers *pf, const frt_feature_buffers *cf, int64_t w, int64_t h,
                            const frt_reproject_params *p, int on_device, frt_reproject_stats *st)
{
    if (prev_cam == NULL || cur_cam == NULL) {
        return refuse("frt_accum_reproject: a null pointer (both buffers of both views are needed)");
    }
    frt_camera prev, cur;
    double *tp = NULL, *tc = NULL;
    if (frt_flatten_camera(prev_cam, 0, 0, false, &prev, &tp) != 0) {
        return refuse("frt_accum_reproject: out of memory");
    }
    if (frt_flatten_camera(cur_cam, 0, 0, false, &cur, &tc) != 0) {
        free(tp);
        return refuse("frt_accum_reproject: out of memory");
    }
    free(tp);
    free(tc);
    return frt_accum_reproject(dst, src, &prev, &cur, pf, cf, w, h, p, on_device, st);
}

#endif
