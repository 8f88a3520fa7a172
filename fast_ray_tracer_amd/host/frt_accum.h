#ifndef FRT_ACCUM_H
#define FRT_ACCUM_H

#include "frt_device.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * libfrt_host's side of the accumulator (host/frt_accum.c; include/frt_device.h "Accumulator" has the definition and
 * the statistics). An frt_accum is a host accumulator (device -1: the C pass that is the definition, state in host
 * memory, host buffers only) or a device accumulator (device >= 0: csrc/frt_accum.hip, which takes host or device
 * buffers). Refusals return -1 with the reason in frt_accum_error() and leave every output untouched: a null pointer,
 * npixels <= 0 or more than 2^31 - 1, no such device, device buffers given to a host accumulator.
 */
typedef struct frt_accum frt_accum;

int frt_accum_create(int device, int64_t npixels, frt_accum **out);
int frt_accum_reset(frt_accum *acc);
int frt_accum_add(frt_accum *acc, const double *rgba, int on_device);
/* mean_rgba or var may be NULL (not both); stats may be NULL */
int frt_accum_resolve(frt_accum *acc, double *mean_rgba, double *var, int on_device, frt_accum_stats *stats);
void frt_accum_release(frt_accum *acc);
/* the device accumulator inside (frt_render_rows_accumulate takes it), NULL for a host accumulator */
frt_accum_dev *frt_accum_device_part(frt_accum *acc);
/* a host accumulator's state in place (n, 4 x mean, 3 x m2 per pixel) and its two counters, for the passes of
 * libfrt_host that write one (host/frt_reproject.c); -1 for NULL or a device accumulator */
int frt_accum_host_state(frt_accum *acc, int64_t *npixels, int32_t **n, double **mean, double **m2, uint64_t **frames,
                         uint64_t **skipped);

#ifdef __cplusplus
}
#endif

#endif
