#ifndef FRT_REPROJECT_H
#define FRT_REPROJECT_H

#include "frt_device.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * libfrt_host's side of the reprojection (host/frt_reproject.c; include/frt_device.h "Reprojection" has the
 * definition, the parameters and the statistics). Refusals return -1 with the reason in frt_accum_error() and leave
 * every output untouched.
 */
size_t frt_reproject_params_size(void);
size_t frt_reproject_stats_size(void);
void frt_reproject_defaults(frt_reproject_params *params);

/* NULL when params are in range, else the reason (no device needed) */
const char *frt_reproject_params_reason(const frt_reproject_params *params);

/* O_cur, O_prev and prev_fwd of the two cameras; refuses (-1) a null pointer, sizes that differ or are not positive,
 * and a camera matrix, scalar or inverse that is not finite */
int frt_reproject_setup(const frt_camera *prev_cam, const frt_camera *cur_cam, frt_reproject_geometry *out);

/*
 * The host pass on plain arrays, which is the definition: the source state (src_n npixels int32, src_mean 4 and
 * src_m2 3 doubles per pixel) into the destination state, laid out alike, every pixel of which is written. The
 * feature buffers hold 8 doubles and 2 int32 per pixel. stats may be NULL. It refuses (-1) a null pointer, a
 * destination array that is its source array, w or h <= 0 or more than 2^31 - 1 pixels, cameras that are not w x h
 * and parameters out of range.
 */
int frt_reproject_host(int32_t *dst_n, double *dst_mean, double *dst_m2, const int32_t *src_n, const double *src_mean,
                       const double *src_m2, const frt_camera *prev_cam, const frt_camera *cur_cam,
                       const frt_reproject_geometry *geometry, const double *prev_geom, const int32_t *prev_ids,
                       const double *cur_geom, const int32_t *cur_ids, int64_t w, int64_t h,
                       const frt_reproject_params *params, frt_reproject_stats *stats);

#ifndef FRT_REPROJECT_STANDALONE
#include "frt_accum.h"
#include "src/renderer/camera.h"

/*
 * src's state under prev_cam into dst under cur_cam. Host accumulators run frt_reproject_host (host feature buffers
 * only: on_device must be 0); device accumulators forward to frt_accum_dev_reproject (csrc/frt_accum.hip), with the
 * feature buffers in host memory (on_device 0) or on the accumulators' device. Both buffers of both views are needed.
 * On top of the refusals above: dst == src, one host and one device accumulator, accumulators on different devices,
 * w * h != npixels, device buffers given to host accumulators.
 */
int frt_accum_reproject(frt_accum *dst, frt_accum *src, const frt_camera *prev_cam, const frt_camera *cur_cam,
                        const frt_feature_buffers *prev_features, const frt_feature_buffers *cur_features, int64_t w,
                        int64_t h, const frt_reproject_params *params, int on_device, frt_reproject_stats *stats);

/* the same with the host library's Camera objects, flattened by frt_flatten_camera (without steps: the pass reads no
 * sample table) */
int frt_accum_reproject_cameras(frt_accum *dst, frt_accum *src, Camera prev_cam, Camera cur_cam,
                                const frt_feature_buffers *prev_features, const frt_feature_buffers *cur_features,
                                int64_t w, int64_t h, const frt_reproject_params *params, int on_device,
                                frt_reproject_stats *stats);
#else
/* without libfrt_device (a stand-alone build of this file alone with matrix_inverse): the last refusal's reason */
const char *frt_reproject_standalone_error(void);
#endif

#ifdef __cplusplus
}
#endif

#endif
