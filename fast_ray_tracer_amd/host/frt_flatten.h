/*
 * frt-mi355x host: flattening of the pointer-linked scene graph into the
 * device layout declared in include/frt_device.h.
 */
#ifndef FRT_FLATTEN_H
#define FRT_FLATTEN_H

#include "frt_device.h"
#include "src/renderer/renderer.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Build a host-memory frt_scene for (cam, w). Returns 0 on success; on failure
 * writes a message into err (size errlen). Free with frt_flat_scene_free. */
int frt_flatten_scene(Camera cam, World w, size_t usteps, size_t vsteps, bool jitter,
                      frt_scene *out, char *err, size_t errlen);
void frt_flat_scene_free(frt_scene *s);

/* The camera half of frt_flatten_scene alone (which calls it): cam with the render call's steps and jitter as the
 * engine's frt_camera, and the non-jittered CMJ table of usteps x vsteps (2 * usteps * vsteps doubles, malloc'd: the
 * caller frees it; NULL when a step count is 0, which the engine refuses). Returns 0, or -1 when out of memory. */
int frt_flatten_camera(Camera cam, size_t usteps, size_t vsteps, bool jitter, frt_camera *out, double **table);

/* host/frt_render.c: flatten + upload (NULL: frt_host_last_error), and the move of a resident handle's camera
 * (0, or -1 with the reason in frt_host_last_error and the handle as it was) */
frt_scene_handle *frt_host_prepare(Camera cam, World w, size_t usteps, size_t vsteps, bool jitter, int device);
int frt_host_set_camera(frt_scene_handle *h, Camera cam, size_t usteps, size_t vsteps, bool jitter);
const char *frt_host_last_error(void);

/* diagnostics: bit 0 the two flattened scenes hold the same world, bit 1 the same camera (render_multi's reuse) */
int frt_scenes_compare(const frt_scene *a, const frt_scene *b);

#ifdef __cplusplus
}
#endif

#endif
