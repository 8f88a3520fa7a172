/*
 * frt-mi355x: the variance-guided denoise's host pass, which is its definition (include/frt_device.h "Variance-guided
 * denoise", DESIGN.md "Accumulation and the variance-guided denoise").
 *
 * The a-trous filter of host/frt_denoise.c with its colour term scaled by the locally pre-filtered variance of the
 * mean, and the variance filtered alongside the colour (the spatial part of SVGF). Every value is built from
 * + - * /, comparisons and nothing else, in binary64 and in the order written here (-ffp-contract=off), so the device
 * pass (csrc/frt_denoise_var.hip) repeats it bit for bit: one function per step here, one of the same name there.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "frt_denoise.h"
#include "frt_denoise_var.h"

#define DV_INVALID INT32_MIN /* the material column's value of an invalid pixel */

/* the guides, the demodulated colour and its variance of one image, as columns */
typedef struct dv_planes {
    double *n0, *n1, *n2, *inv_nn, *iz, *z;
    int32_t *mat;
    double *x[2][3]; /* ping-pong */
    double *v[2][3];
} dv_planes;

typedef struct dv_consts {
    double kz, kc, eps, var_eps;
    int squarings, demodulate, match_material;
} dv_consts;

static const double DV_K[3] = {3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0};
static const double DV_G[2] = {1.0 / 2.0, 1.0 / 4.0};

static double
clock_ms(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec * 1e3 + (double)ts.tv_nsec * 1e-6;
}

static void
dv_make_consts(const frt_denoise_var_params *p, dv_consts *c)
{
    c->kz = 1.0 / (p->sigma_depth * p->sigma_depth);
    c->kc = 1.0 / (p->sigma_color * p->sigma_color);
    c->eps = p->albedo_eps;
    c->var_eps = p->var_eps;
    c->squarings = p->normal_squarings;
    c->demodulate = p->demodulate;
    c->match_material = p->match_material;
}

static int
dv_valid(const double *rgba, const double *var, const double *geom, const int32_t *ids)
{
    return ids[0] >= 0 && ids[1] != DV_INVALID && isfinite(geom[0]) && geom[0] > 0 && isfinite(rgba[0]) &&
           isfinite(rgba[1]) && isfinite(rgba[2]) && isfinite(var[0]) && var[0] >= 0 && isfinite(var[1]) &&
           var[1] >= 0 && isfinite(var[2]) && var[2] >= 0;
}

/* a[ch]: what the colour is divided by before the filter and multiplied by after it */
static double
dv_albedo(const double *geom, int ch, const dv_consts *c)
{
    return c->demodulate ? geom[4 + ch] + c->eps : 1.0;
}

static void
dv_pack(const double *rgba, const double *var, const double *geom, const int32_t *ids, size_t i, const dv_consts *c,
        const dv_planes *P)
{
    if (!dv_valid(rgba, var, geom, ids)) {
        P->mat[i] = DV_INVALID;
        return;
    }
    for (int ch = 0; ch < 3; ++ch) {
        const double a = dv_albedo(geom, ch, c);
        P->x[0][ch][i] = rgba[ch] / a;
        P->v[0][ch][i] = var[ch] / (a * a);
    }
    const double n0 = geom[1], n1 = geom[2], n2 = geom[3];
    const double nn = (n0 * n0 + n1 * n1) + n2 * n2;
    P->n0[i] = n0;
    P->n1[i] = n1;
    P->n2[i] = n2;
    P->inv_nn[i] = nn > 0 ? 1.0 / nn : 0.0;
    P->z[i] = geom[0];
    P->iz[i] = 1.0 / geom[0];
    P->mat[i] = ids[1];
}

/* g_p: the summed variance pre-filtered over the 3 x 3 neighbours at distance 1 */
static double
dv_guide(const dv_planes *P, const double *const v[3], int64_t w, int64_t h, int64_t px, int64_t py)
{
    double sum = 0.0, sg = 0.0;
    for (int dy = -1; dy <= 1; ++dy) {
        const int64_t qy = py + dy;
        if (qy < 0 || qy >= h) {
            continue;
        }
        for (int dx = -1; dx <= 1; ++dx) {
            const int64_t qx = px + dx;
            if (qx < 0 || qx >= w) {
                continue;
            }
            const size_t q = (size_t)(qy * w + qx);
            if (P->mat[q] == DV_INVALID) {
                continue;
            }
            const double g = DV_G[dx < 0 ? -dx : dx] * DV_G[dy < 0 ? -dy : dy];
            const double vs = (v[0][q] + v[1][q]) + v[2][q];
            sum += g * vs;
            sg += g;
        }
    }
    return sum / sg;
}

/* the weight of tap q != p for pixel p (both valid), or a negative value when the tap is skipped */
static double
dv_weight(const dv_planes *P, const double *const x[3], size_t p, size_t q, double hk, double kc_p, const dv_consts *c)
{
    if (c->match_material && P->mat[q] != P->mat[p]) {
        return -1.0;
    }
    const double d = (P->n0[p] * P->n0[q] + P->n1[p] * P->n1[q]) + P->n2[p] * P->n2[q];
    if (d <= 0) {
        return -1.0;
    }
    const double m = (d * d) * (P->inv_nn[p] * P->inv_nn[q]);
    double t = m < 1.0 ? m : 1.0;
    for (int k = 0; k < c->squarings; ++k) {
        t = t * t;
    }
    const double r = P->z[p] - P->z[q];
    const double xz = ((r * r) * c->kz) * (P->iz[p] * P->iz[q]);
    const double dc0 = x[0][p] - x[0][q], dc1 = x[1][p] - x[1][q], dc2 = x[2][p] - x[2][q];
    const double xc = ((dc0 * dc0 + dc1 * dc1) + dc2 * dc2) * kc_p;
    const double u = (1.0 + xz) * (1.0 + xc);
    return (hk * t) / (u * u);
}

/* one iteration for pixel (px, py) of a w x h image: x_{i+1}, v_{i+1} from x_i, v_i */
static void
dv_atrous_pixel(const dv_planes *P, const double *const x[3], const double *const v[3], double *const y[3],
                double *const vy[3], int64_t w, int64_t h, int64_t px, int64_t py, int64_t s, const dv_consts *c)
{
    const size_t p = (size_t)(py * w + px);
    const double kc_p = c->kc / (dv_guide(P, v, w, h, px, py) + c->var_eps);
    double acc[3] = {0.0, 0.0, 0.0}, vacc[3] = {0.0, 0.0, 0.0}, ws = 0.0;
    for (int dy = -2; dy <= 2; ++dy) {
        const int64_t qy = py + s * dy;
        if (qy < 0 || qy >= h) {
            continue;
        }
        for (int dx = -2; dx <= 2; ++dx) {
            const int64_t qx = px + s * dx;
            if (qx < 0 || qx >= w) {
                continue;
            }
            const size_t q = (size_t)(qy * w + qx);
            if (P->mat[q] == DV_INVALID) {
                continue;
            }
            const double hk = DV_K[dx < 0 ? -dx : dx] * DV_K[dy < 0 ? -dy : dy];
            double wgt = hk;
            if (dx != 0 || dy != 0) {
                wgt = dv_weight(P, x, p, q, hk, kc_p, c);
                if (wgt < 0) {
                    continue;
                }
            }
            const double w2 = wgt * wgt;
            for (int ch = 0; ch < 3; ++ch) {
                acc[ch] += wgt * x[ch][q];
                vacc[ch] += w2 * v[ch][q];
            }
            ws += wgt;
        }
    }
    const double ws2 = ws * ws;
    for (int ch = 0; ch < 3; ++ch) {
        y[ch][p] = acc[ch] / ws;
        vy[ch][p] = vacc[ch] / ws2;
    }
}

/* the outputs' pixel: the filtered colour times a, the filtered variance times a * a, alpha and var[3] copied; an
 * invalid pixel's inputs as they are */
static void
dv_unpack(const double *rgba, const double *var, const double *geom, size_t i, const dv_consts *c, const dv_planes *P,
          const double *const x[3], const double *const v[3], double *out, double *out_var)
{
    if (P->mat[i] == DV_INVALID) {
        memmove(out, rgba, 4 * sizeof(double));
        if (out_var != NULL) {
            memmove(out_var, var, 4 * sizeof(double));
        }
        return;
    }
    const double alpha = rgba[3], count = var[3];
    for (int ch = 0; ch < 3; ++ch) {
        const double a = dv_albedo(geom, ch, c);
        out[ch] = x[ch][i] * a;
        if (out_var != NULL) {
            out_var[ch] = v[ch][i] * (a * a);
        }
    }
    out[3] = alpha;
    if (out_var != NULL) {
        out_var[3] = count;
    }
}

static void
dv_image(const double *rgba, const double *var, const double *geom, const int32_t *ids, int64_t w, int64_t h,
         const dv_consts *c, int iterations, const dv_planes *P, double *out, double *out_var, uint64_t *valid)
{
    const size_t npx = (size_t)(w * h);
    for (size_t i = 0; i < npx; ++i) {
        dv_pack(rgba + 4 * i, var + 4 * i, geom + 8 * i, ids + 2 * i, i, c, P);
        *valid += P->mat[i] != DV_INVALID;
    }
    int cur = 0;
    for (int it = 0; it < iterations; ++it) {
        const double *const x[3] = {P->x[cur][0], P->x[cur][1], P->x[cur][2]};
        const double *const v[3] = {P->v[cur][0], P->v[cur][1], P->v[cur][2]};
        double *const y[3] = {P->x[cur ^ 1][0], P->x[cur ^ 1][1], P->x[cur ^ 1][2]};
        double *const vy[3] = {P->v[cur ^ 1][0], P->v[cur ^ 1][1], P->v[cur ^ 1][2]};
        const int64_t s = (int64_t)1 << it;
        for (int64_t py = 0; py < h; ++py) {
            for (int64_t px = 0; px < w; ++px) {
                if (P->mat[py * w + px] != DV_INVALID) {
                    dv_atrous_pixel(P, x, v, y, vy, w, h, px, py, s, c);
                }
            }
        }
        cur ^= 1;
    }
    const double *const x[3] = {P->x[cur][0], P->x[cur][1], P->x[cur][2]};
    const double *const v[3] = {P->v[cur][0], P->v[cur][1], P->v[cur][2]};
    for (size_t i = 0; i < npx; ++i) {
        dv_unpack(rgba + 4 * i, var + 4 * i, geom + 8 * i, i, c, P, x, v, out + 4 * i,
                  out_var != NULL ? out_var + 4 * i : NULL);
    }
}

int
frt_denoise_var_host(const double *rgba, const double *var, const double *geom, const int32_t *ids, int64_t w,
                     int64_t h, int64_t nimages, const frt_denoise_var_params *params, double *out, double *out_var,
                     frt_denoise_var_stats *stats)
{
    if (frt_denoise_var_check(rgba, var, geom, ids, w, h, nimages, params, out) != 0) {
        return -1;
    }
    frt_denoise_var_stats local;
    frt_denoise_var_stats *st = stats != NULL ? stats : &local;
    memset(st, 0, sizeof(*st));
    st->pixels = (uint64_t)(w * h * nimages);
    st->iterations = params->iterations;
    st->backend = FRT_DENOISE_HOST;
    st->device = -1;
    const double t0 = clock_ms();
    const size_t npx = (size_t)(w * h);
    /* one image's columns: 6 guides, 2 x 3 colour planes, 2 x 3 variance planes, the material */
    double *planes = (double *)malloc(npx * 18 * sizeof(double));
    int32_t *mat = (int32_t *)malloc(npx * sizeof(int32_t));
    if (planes == NULL || mat == NULL) {
        free(planes);
        free(mat);
        frt_denoise_set_error("frt_denoise_var_host: out of memory");
        return -1;
    }
    dv_planes P;
    P.n0 = planes;
    P.n1 = planes + npx;
    P.n2 = planes + 2 * npx;
    P.inv_nn = planes + 3 * npx;
    P.iz = planes + 4 * npx;
    P.z = planes + 5 * npx;
    for (int k = 0; k < 6; ++k) {
        P.x[k / 3][k % 3] = planes + (size_t)(6 + k) * npx;
        P.v[k / 3][k % 3] = planes + (size_t)(12 + k) * npx;
    }
    P.mat = mat;
    dv_consts c;
    dv_make_consts(params, &c);
    for (int64_t img = 0; img < nimages; ++img) {
        const size_t o = (size_t)img * npx;
        dv_image(rgba + 4 * o, var + 4 * o, geom + 8 * o, ids + 2 * o, w, h, &c, params->iterations, &P, out + 4 * o,
                 out_var != NULL ? out_var + 4 * o : NULL, &st->valid_pixels);
    }
    free(planes);
    free(mat);
    st->host_ms = clock_ms() - t0;
    return 0;
}

int frt_encode_hint_device(void); /* frt_canvas.c: the device this process last rendered on, -1 while none */

int
frt_denoise_var(const double *rgba, const double *var, const double *geom, const int32_t *ids, int on_device, int64_t w,
                int64_t h, int64_t nimages, const frt_denoise_var_params *params, int backend, int device, double *out,
                double *out_var, frt_denoise_var_stats *stats)
{
    if (frt_denoise_var_check(rgba, var, geom, ids, w, h, nimages, params, out) != 0) {
        return -1;
    }
    if (backend < FRT_DENOISE_HOST || backend > FRT_DENOISE_AUTO) {
        frt_denoise_set_error("frt_denoise_var: unknown backend");
        return -1;
    }
    const int hint = frt_encode_hint_device();
    if (backend == FRT_DENOISE_AUTO) {
        backend = on_device || hint >= 0 ? FRT_DENOISE_DEVICE : FRT_DENOISE_HOST;
    }
    if (device < 0) {
        device = hint >= 0 ? hint : 0;
    }
    if (backend == FRT_DENOISE_DEVICE) {
        return frt_denoise_var_device(rgba, var, geom, ids, on_device, w, h, nimages, params, device, out, out_var,
                                      stats);
    }
    if (!on_device) {
        return frt_denoise_var_host(rgba, var, geom, ids, w, h, nimages, params, out, out_var, stats);
    }
    /* the host pass on device buffers: fetch the four, filter in place, put the outputs back */
    const size_t npx = (size_t)(w * h * nimages);
    double *h_rgba = (double *)malloc(npx * 4 * sizeof(double));
    double *h_var = (double *)malloc(npx * 4 * sizeof(double));
    double *h_geom = (double *)malloc(npx * 8 * sizeof(double));
    int32_t *h_ids = (int32_t *)malloc(npx * 2 * sizeof(int32_t));
    int rc = -1;
    if (h_rgba == NULL || h_var == NULL || h_geom == NULL || h_ids == NULL) {
        frt_denoise_set_error("frt_denoise_var: out of memory");
    } else if (frt_encode_fetch(h_rgba, rgba, npx * 4 * sizeof(double), device) != 0 ||
               frt_encode_fetch(h_var, var, npx * 4 * sizeof(double), device) != 0 ||
               frt_encode_fetch(h_geom, geom, npx * 8 * sizeof(double), device) != 0 ||
               frt_encode_fetch(h_ids, ids, npx * 2 * sizeof(int32_t), device) != 0) {
        frt_denoise_set_error(frt_encode_error());
    } else {
        rc = frt_denoise_var_host(h_rgba, h_var, h_geom, h_ids, w, h, nimages, params, h_rgba, h_var, stats);
        if (rc == 0 && frt_denoise_store(out, h_rgba, npx * 4 * sizeof(double), device) != 0) {
            rc = -1;
        }
        if (rc == 0 && out_var != NULL && frt_denoise_store(out_var, h_var, npx * 4 * sizeof(double), device) != 0) {
            rc = -1;
        }
    }
    free(h_rgba);
    free(h_var);
    free(h_geom);
    free(h_ids);
    return rc;
}
