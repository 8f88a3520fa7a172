/*
 * frt-mi355x host API: render entry points.
 *
 * render_multi() is the drop-in boundary (reference src/renderer/renderer.h:46-47,
 * called by generated main() at yaml_parser/yaml_parser.py:218). It flattens
 * the scene and renders on MI355X through the device C-ABI declared in
 * include/frt_device.h; there is no CPU fallback.
 */
#ifndef FRT_RENDERER_H
#define FRT_RENDERER_H

#include <stdbool.h>
#include <stdlib.h>

#include "../libs/linalg/linalg.h"
#include "../libs/canvas/canvas.h"
#include "../color/color.h"
#include "../light/light.h"
#include "../shapes/shapes.h"
#include "../intersection/intersection.h"
#include "world.h"
#include "camera.h"
#include "ray.h"

Canvas render(Camera cam, World w, size_t usteps, size_t vsteps, bool jitter);
Canvas render_multi(Camera cam, World w, size_t usteps, size_t vsteps, bool jitter);

/* frt extensions (no reference counterpart; main.c does not call them): the reason the last render_multi
 * failed ("" after a successful call), and the release of the device handles render_multi keeps between calls
 * for a repeat of the same scene (host/frt_render.c) */
const char *frt_render_multi_error(void);
void frt_render_multi_release(void);

/* A camera at `from` looking at `to` (view_transform, then camera(): the order a generated main() uses) with the
 * aperture and steps of `like`; released with free(), and not to outlive `like` (it shares the aperture's sampler
 * tables). A main() that loops over such cameras and calls render_multi for each keeps its world on the device:
 * only the first call uploads (host/frt_render.c, INTEGRATION.md "Views"). */
/* n cameras of one size over one world as one strip frame on one device: out[k] receives a fresh canvas for cams[k]
 * (the caller frees each), what render_multi(cams[k], w, usteps, vsteps, jitter) returns on that device, bit for
 * bit. Returns 0, or -1 with the reason in frt_render_multi_error and the canvases zeroed (host/frt_render.c). */
int frt_render_views(Camera *cams, size_t n, World w, size_t usteps, size_t vsteps, bool jitter, Canvas *out);

Camera frt_camera_look_at(const double from[3], const double to[3], const double up[3], size_t hsize, size_t vsize,
                          double fov, double distance, Camera like);

#endif
