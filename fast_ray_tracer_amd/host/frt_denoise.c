/*
 * frt-mi355x: the denoise's host pass, which is its definition (include/frt_device.h "Denoise", DESIGN.md "Denoise").
 *
 * An edge-avoiding a-trous filter over a colour frame, guided by the first-hit feature buffers. Every weight is built
 * from + - * /, comparisons and nothing else, in binary64 and in the order written here (this file is compiled with
 * -ffp-contract=off), so the device pass (csrc/frt_denoise.hip) repeats it bit for bit: one function per step here,
 * one of the same name there.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "frt_denoise.h"

#define DN_INVALID INT32_MIN /* the material column's value of an invalid pixel */

/* the guides and the demodulated colour of one image, as columns */
typedef struct dn_planes {
    double *n0, *n1, *n2, *inv_nn, *iz, *z;
    int32_t *mat;
    double *x[2][3]; /* ping-pong */
} dn_planes;

typedef struct dn_consts {
    double kz;
    double kc[FRT_DENOISE_MAX_ITERATIONS];
    double eps;
    int squarings, demodulate, match_material;
} dn_consts;

static const double DN_K[3] = {3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0};

static double
clock_ms(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec * 1e3 + (double)ts.tv_nsec * 1e-6;
}

static void
dn_make_consts(const frt_denoise_params *p, dn_consts *c)
{
    c->kz = 1.0 / (p->sigma_depth * p->sigma_depth);
    const double kc = 1.0 / (p->sigma_color * p->sigma_color);
    for (int i = 0; i < FRT_DENOISE_MAX_ITERATIONS; ++i) {
        c->kc[i] = ldexp(kc, 2 * i);
    }
    c->eps = p->albedo_eps;
    c->squarings = p->normal_squarings;
    c->demodulate = p->demodulate;
    c->match_material = p->match_material;
}

static int
dn_valid(const double *rgba, const double *geom, const int32_t *ids)
{
    return ids[0] >= 0 && ids[1] != DN_INVALID && isfinite(geom[0]) && geom[0] > 0 && isfinite(rgba[0]) &&
           isfinite(rgba[1]) && isfinite(rgba[2]);
}

/* a[ch]: what the colour is divided by before the filter and multiplied by after it */
static double
dn_albedo(const double *geom, int ch, const dn_consts *c)
{
    return c->demodulate ? geom[4 + ch] + c->eps : 1.0;
}

static void
dn_pack(const double *rgba, const double *geom, const int32_t *ids, size_t i, const dn_consts *c, const dn_planes *P)
{
    if (!dn_valid(rgba, geom, ids)) {
        P->mat[i] = DN_INVALID;
        return;
    }
    for (int ch = 0; ch < 3; ++ch) {
        P->x[0][ch][i] = rgba[ch] / dn_albedo(geom, ch, c);
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

/* the weight of tap q != p for pixel p (both valid), or a negative value when the tap is skipped */
static double
dn_weight(const dn_planes *P, const double *const x[3], size_t p, size_t q, double hk, double kc, const dn_consts *c)
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
    const double xc = ((dc0 * dc0 + dc1 * dc1) + dc2 * dc2) * kc;
    const double u = (1.0 + xz) * (1.0 + xc);
    return (hk * t) / (u * u);
}

/* one iteration for pixel (px, py) of a w x h image: x_{i+1} from x_i */
static void
dn_atrous_pixel(const dn_planes *P, const double *const x[3], double *const y[3], int64_t w, int64_t h, int64_t px,
                int64_t py, int64_t s, double kc, const dn_consts *c)
{
    const size_t p = (size_t)(py * w + px);
    double acc[3] = {0.0, 0.0, 0.0}, ws = 0.0;
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
            if (P->mat[q] == DN_INVALID) {
                continue;
            }
            const double hk = DN_K[dx < 0 ? -dx : dx] * DN_K[dy < 0 ? -dy : dy];
            double wgt = hk;
            if (dx != 0 || dy != 0) {
                wgt = dn_weight(P, x, p, q, hk, kc, c);
                if (wgt < 0) {
                    continue;
                }
            }
            for (int ch = 0; ch < 3; ++ch) {
                acc[ch] += wgt * x[ch][q];
            }
            ws += wgt;
        }
    }
    for (int ch = 0; ch < 3; ++ch) {
        y[ch][p] = acc[ch] / ws;
    }
}

/* out's pixel: the filtered colour times a[ch], alpha copied; an invalid pixel's input as it is */
static void
dn_unpack(const double *rgba, const double *geom, size_t i, const dn_consts *c, const dn_planes *P,
          const double *const x[3], double *out)
{
    if (P->mat[i] == DN_INVALID) {
        memmove(out, rgba, 4 * sizeof(double));
        return;
    }
    const double alpha = rgba[3];
    for (int ch = 0; ch < 3; ++ch) {
        out[ch] = x[ch][i] * dn_albedo(geom, ch, c);
    }
    out[3] = alpha;
}

static int
dn_image(const double *rgba, const double *geom, const int32_t *ids, int64_t w, int64_t h, const dn_consts *c,
         int iterations, const dn_planes *P, double *out, uint64_t *valid)
{
    const size_t npx = (size_t)(w * h);
    for (size_t i = 0; i < npx; ++i) {
        dn_pack(rgba + 4 * i, geom + 8 * i, ids + 2 * i, i, c, P);
        *valid += P->mat[i] != DN_INVALID;
    }
    int cur = 0;
    for (int it = 0; it < iterations; ++it) {
        const double *const x[3] = {P->x[cur][0], P->x[cur][1], P->x[cur][2]};
        double *const y[3] = {P->x[cur ^ 1][0], P->x[cur ^ 1][1], P->x[cur ^ 1][2]};
        const int64_t s = (int64_t)1 << it;
        for (int64_t py = 0; py < h; ++py) {
            for (int64_t px = 0; px < w; ++px) {
                if (P->mat[py * w + px] != DN_INVALID) {
                    dn_atrous_pixel(P, x, y, w, h, px, py, s, c->kc[it], c);
                }
            }
        }
        cur ^= 1;
    }
    const double *const x[3] = {P->x[cur][0], P->x[cur][1], P->x[cur][2]};
    for (size_t i = 0; i < npx; ++i) {
        dn_unpack(rgba + 4 * i, geom + 8 * i, i, c, P, x, out + 4 * i);
    }
    return 0;
}

static void
dn_stats_init(frt_denoise_stats *st, int64_t w, int64_t h, int64_t nimages, const frt_denoise_params *params)
{
    memset(st, 0, sizeof(*st));
    st->pixels = (uint64_t)(w * h * nimages);
    st->iterations = params->iterations;
    st->backend = FRT_DENOISE_HOST;
    st->device = -1;
}

int
frt_denoise_host(const double *rgba, const double *geom, const int32_t *ids, int64_t w, int64_t h, int64_t nimages,
                 const frt_denoise_params *params, double *out, frt_denoise_stats *stats)
{
    if (frt_denoise_check(rgba, geom, ids, w, h, nimages, params, out) != 0) {
        return -1;
    }
    frt_denoise_stats local;
    frt_denoise_stats *st = stats != NULL ? stats : &local;
    dn_stats_init(st, w, h, nimages, params);
    const double t0 = clock_ms();
    const size_t npx = (size_t)(w * h);
    /* one image's columns: 6 guides, 2 x 3 colour planes, the material */
    double *planes = (double *)malloc(npx * 12 * sizeof(double));
    int32_t *mat = (int32_t *)malloc(npx * sizeof(int32_t));
    if (planes == NULL || mat == NULL) {
        free(planes);
        free(mat);
        frt_denoise_set_error("frt_denoise_host: out of memory");
        return -1;
    }
    dn_planes P;
    P.n0 = planes;
    P.n1 = planes + npx;
    P.n2 = planes + 2 * npx;
    P.inv_nn = planes + 3 * npx;
    P.iz = planes + 4 * npx;
    P.z = planes + 5 * npx;
    for (int k = 0; k < 6; ++k) {
        P.x[k / 3][k % 3] = planes + (size_t)(6 + k) * npx;
    }
    P.mat = mat;
    dn_consts c;
    dn_make_consts(params, &c);
    for (int64_t img = 0; img < nimages; ++img) {
        const size_t o = (size_t)img * npx;
        dn_image(rgba + 4 * o, geom + 8 * o, ids + 2 * o, w, h, &c, params->iterations, &P, out + 4 * o,
                 &st->valid_pixels);
    }
    free(planes);
    free(mat);
    st->host_ms = clock_ms() - t0;
    return 0;
}

int frt_encode_hint_device(void); /* frt_canvas.c: the device this process last rendered on, -1 while none */

int
frt_denoise(const double *rgba, const double *geom, const int32_t *ids, int on_device, int64_t w, int64_t h,
            int64_t nimages, const frt_denoise_params *params, int backend, int device, double *out,
            frt_denoise_stats *stats)
{
    if (frt_denoise_check(rgba, geom, ids, w, h, nimages, params, out) != 0) {
        return -1;
    }
    if (backend < FRT_DENOISE_HOST || backend > FRT_DENOISE_AUTO) {
        frt_denoise_set_error("frt_denoise: unknown backend");
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
        return frt_denoise_device(rgba, geom, ids, on_device, w, h, nimages, params, device, out, stats);
    }
    if (!on_device) {
        return frt_denoise_host(rgba, geom, ids, w, h, nimages, params, out, stats);
    }
    /* the host pass on device buffers: fetch the three, filter, put out back */
    const size_t npx = (size_t)(w * h * nimages);
    double *h_rgba = (double *)malloc(npx * 4 * sizeof(double));
    double *h_geom = (double *)malloc(npx * 8 * sizeof(double));
    int32_t *h_ids = (int32_t *)malloc(npx * 2 * sizeof(int32_t));
    int rc = -1;
    if (h_rgba == NULL || h_geom == NULL || h_ids == NULL) {
        frt_denoise_set_error("frt_denoise: out of memory");
    } else if (frt_encode_fetch(h_rgba, rgba, npx * 4 * sizeof(double), device) != 0 ||
               frt_encode_fetch(h_geom, geom, npx * 8 * sizeof(double), device) != 0 ||
               frt_encode_fetch(h_ids, ids, npx * 2 * sizeof(int32_t), device) != 0) {
        frt_denoise_set_error(frt_encode_error());
    } else {
        rc = frt_denoise_host(h_rgba, h_geom, h_ids, w, h, nimages, params, h_rgba, stats);
        if (rc == 0 && frt_denoise_store(out, h_rgba, npx * 4 * sizeof(double), device) != 0) {
            rc = -1;
        }
    }
    free(h_rgba);
    free(h_geom);
    free(h_ids);
    return rc;
}
