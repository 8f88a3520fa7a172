/*
 * frt-mi355x: the accumulator's host pass, which is its definition (include/frt_device.h "Accumulator", DESIGN.md
 * "Accumulation and the variance-guided denoise").
 *
 * Welford's running mean and sum of squared deviations per pixel, in binary64 with + - * / and comparisons only, in
 * the order written here (this file is compiled with -ffp-contract=off), so the device pass (csrc/frt_accum.hip)
 * repeats it bit for bit: ac_add and ac_resolve here, k_accum_add and k_accum_resolve there.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "frt_accum.h"

struct frt_accum {
    frt_accum_dev *dev; /* a device accumulator, or NULL and the host state below */
    int64_t npixels;
    int32_t *n;
    double *mean; /* 4 per pixel */
    double *m2;   /* 3 per pixel */
    uint64_t frames, skipped;
};

static double
clock_ms(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec * 1e3 + (double)ts.tv_nsec * 1e-6;
}

static int
refuse(const char *what)
{
    frt_accum_set_error(what);
    return -1;
}

/* one sample into one pixel's state; returns 1 when it was skipped */
static int
ac_add(const double *x, int32_t *n, double *mean, double *m2)
{
    if (!(isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]) && isfinite(x[3]))) {
        return 1;
    }
    *n += 1;
    const double dn = (double)*n;
    for (int ch = 0; ch < 4; ++ch) {
        const double d = x[ch] - mean[ch];
        mean[ch] = mean[ch] + d / dn;
        if (ch < 3) {
            m2[ch] = m2[ch] + d * (x[ch] - mean[ch]);
        }
    }
    return 0;
}

static void
ac_resolve(int32_t n, const double *mean, const double *m2, double *mean_rgba, double *var)
{
    if (mean_rgba != NULL) {
        for (int ch = 0; ch < 4; ++ch) {
            mean_rgba[ch] = n == 0 ? 0.0 : mean[ch];
        }
    }
    if (var != NULL) {
        for (int ch = 0; ch < 3; ++ch) {
            var[ch] = n < 2 ? 0.0 : (m2[ch] / (double)(n - 1)) / (double)n;
        }
        var[3] = (double)n;
    }
}

int
frt_accum_create(int device, int64_t npixels, frt_accum **out)
{
    if (out == NULL) {
        return refuse("frt_accum_create: a null pointer");
    }
    if (npixels <= 0 || npixels > 0x7fffffffll) {
        return refuse("frt_accum_create: npixels must be 1 .. 2^31 - 1 (the columns' index is 32-bit)");
    }
    frt_accum *a = (frt_accum *)calloc(1, sizeof(*a));
    if (a == NULL) {
        return refuse("frt_accum_create: out of memory");
    }
    a->npixels = npixels;
    if (device >= 0) {
        if (frt_accum_dev_create(device, npixels, &a->dev) != 0) {
            free(a);
            return -1;
        }
    } else {
        a->n = (int32_t *)calloc((size_t)npixels, sizeof(int32_t));
        a->mean = (double *)calloc((size_t)npixels * 4, sizeof(double));
        a->m2 = (double *)calloc((size_t)npixels * 3, sizeof(double));
        if (a->n == NULL || a->mean == NULL || a->m2 == NULL) {
            frt_accum_release(a);
            return refuse("frt_accum_create: out of memory");
        }
    }
    *out = a;
    return 0;
}

int
frt_accum_reset(frt_accum *acc)
{
    if (acc == NULL) {
        return refuse("frt_accum_reset: a null pointer");
    }
    if (acc->dev != NULL) {
        return frt_accum_dev_reset(acc->dev);
    }
    memset(acc->n, 0, (size_t)acc->npixels * sizeof(int32_t));
    memset(acc->mean, 0, (size_t)acc->npixels * 4 * sizeof(double));
    memset(acc->m2, 0, (size_t)acc->npixels * 3 * sizeof(double));
    acc->frames = acc->skipped = 0;
    return 0;
}

int
frt_accum_add(frt_accum *acc, const double *rgba, int on_device)
{
    if (acc == NULL || rgba == NULL) {
        return refuse("frt_accum_add: a null pointer");
    }
    if (acc->dev != NULL) {
        return frt_accum_dev_add(acc->dev, rgba, on_device);
    }
    if (on_device) {
        return refuse("frt_accum_add: device memory given to a host accumulator");
    }
    for (int64_t i = 0; i < acc->npixels; ++i) {
        acc->skipped += (uint64_t)ac_add(rgba + 4 * i, acc->n + i, acc->mean + 4 * i, acc->m2 + 3 * i);
    }
    acc->frames += 1;
    return 0;
}

int
frt_accum_resolve(frt_accum *acc, double *mean_rgba, double *var, int on_device, frt_accum_stats *stats)
{
    if (acc == NULL || (mean_rgba == NULL && var == NULL)) {
        return refuse("frt_accum_resolve: a null pointer (the accumulator and one of mean_rgba, var are needed)");
    }
    if (acc->dev != NULL) {
        return frt_accum_dev_resolve(acc->dev, mean_rgba, var, on_device, stats);
    }
    if (on_device) {
        return refuse("frt_accum_resolve: device memory given to a host accumulator");
    }
    const double t0 = clock_ms();
    for (int64_t i = 0; i < acc->npixels; ++i) {
        ac_resolve(acc->n[i], acc->mean + 4 * i, acc->m2 + 3 * i, mean_rgba != NULL ? mean_rgba + 4 * i : NULL,
                   var != NULL ? var + 4 * i : NULL);
    }
    if (stats != NULL) {
        memset(stats, 0, sizeof(*stats));
        stats->pixels = (uint64_t)acc->npixels;
        stats->frames = acc->frames;
        stats->skipped = acc->skipped;
        stats->device = -1;
        stats->resolve_ms = clock_ms() - t0;
    }
    return 0;
}

void
frt_accum_release(frt_accum *acc)
{
    if (acc == NULL) {
        return;
    }
    frt_accum_dev_release(acc->dev);
    free(acc->n);
    free(acc->mean);
    free(acc->m2);
    free(acc);
}

frt_accum_dev *
frt_accum_device_part(frt_accum *acc)
{
    return acc != NULL ? acc->dev : NULL;
}

int
frt_accum_host_state(frt_accum *acc, int64_t *npixels, int32_t **n, double **mean, double **m2, uint64_t **frames,
                     uint64_t **skipped)
{
    if (acc == NULL || acc->dev != NULL) {
        return -1;
    }
    *npixels = acc->npixels;
    *n = acc->n;
    *mean = acc->mean;
    *m2 = acc->m2;
    *frames = &acc->frames;
    *skipped = &acc->skipped;
    return 0;
}
