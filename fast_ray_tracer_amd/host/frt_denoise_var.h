#ifndef FRT_DENOISE_VAR_H
#define FRT_DENOISE_VAR_H

#include "frt_device.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * libfrt_host's side of the variance-guided denoise (host/frt_denoise_var.c; include/frt_device.h "Variance-guided
 * denoise" has the definition and the parameters): the host pass on host buffers, one CPU thread, and the entry point
 * that picks a backend as frt_denoise does (FRT_DENOISE_HOST / _DEVICE / _AUTO; device < 0: the device last rendered
 * on, else 0). out may be rgba, out_var may be var or NULL. Same refusals and return values as frt_denoise.
 */
int frt_denoise_var_host(const double *rgba, const double *var, const double *geom, const int32_t *ids, int64_t w,
                         int64_t h, int64_t nimages, const frt_denoise_var_params *params, double *out,
                         double *out_var, frt_denoise_var_stats *stats);
int frt_denoise_var(const double *rgba, const double *var, const double *geom, const int32_t *ids, int on_device,
                    int64_t w, int64_t h, int64_t nimages, const frt_denoise_var_params *params, int backend,
                    int device, double *out, double *out_var, frt_denoise_var_stats *stats);

#ifdef __cplusplus
}
#endif

#endif
