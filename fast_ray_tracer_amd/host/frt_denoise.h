#ifndef FRT_DENOISE_H
#define FRT_DENOISE_H

#include "frt_device.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * libfrt_host's side of the denoise (host/frt_denoise.c; include/frt_device.h "Denoise" has the definition, the
 * parameters and the statistics): the host pass on host buffers, one CPU thread, and the entry point that picks
 * a backend as frt_encode16 does: FRT_DENOISE_HOST (device buffers are fetched and out written back),
 * FRT_DENOISE_DEVICE, or FRT_DENOISE_AUTO (the device when the buffers are there or this process has rendered on
 * one, else the host). device < 0: the device last rendered on, else 0. Same refusals and return values as above.
 */
int frt_denoise_host(const double *rgba, const double *geom, const int32_t *ids, int64_t w, int64_t h, int64_t nimages,
                     const frt_denoise_params *params, double *out, frt_denoise_stats *stats);
int frt_denoise(const double *rgba, const double *geom, const int32_t *ids, int on_device, int64_t w, int64_t h,
                int64_t nimages, const frt_denoise_params *params, int backend, int device, double *out,
                frt_denoise_stats *stats);

#ifdef __cplusplus
}
#endif

#endif
