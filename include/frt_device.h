/*
 * frt_device.h — C ABI of the MI355X (gfx950) render engine.
 *
 * This is the thin boundary between the C11 host library (the drop-in
 * scene API under fast_ray_tracer_amd/host/src/...) and the hand-written HIP
 * kernels in fast_ray_tracer_amd/csrc. Plain structs, pointers and sizes only.
 *
 * What it replaces in the reference:
 *   frt_render_rows / frt_render_rows_device  -> the body of
 *       Canvas render_multi(Camera, World, size_t, size_t, bool)
 *       (reference src/renderer/renderer.h:47, renderer.c:244-281): the
 *       row-per-job pthread pool over per-thread deep world copies, and the
 *       per-sample recursion color_at -> intersect_world -> shade_hit
 *       (renderer.c:74-979, world.c:163-197).
 *   frt_scene                                 -> the pointer-linked object
 *       tree (struct shape, shapes.h:85-118), materials (material.h:196-220),
 *       patterns (pattern.h:119-142), lights (light.h:57-76), camera
 *       (camera.h:60-73) and config (config.h:56-62), flattened by
 *       fast_ray_tracer_amd/host/frt_flatten.c.
 *
 * How the reference's render_multi binds to it: see INTEGRATION.md.
 * All scene arithmetic is IEEE binary64, matching the reference.
 */
#ifndef FRT_DEVICE_H
#define FRT_DEVICE_H

#ifndef __HIPCC_RTC__
#include <stddef.h>
#include <stdint.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define FRT_ABI_VERSION 3u  /* 3: frt_frame_stats grew the beam-stage counters (round 4) */

/* node kinds: same numbering as the reference's enum shape_enum (shapes.h:16-27) */
enum frt_node_type {
    FRT_CONE = 0,
    FRT_CUBE = 1,
    FRT_CYLINDER = 2,
    FRT_PLANE = 3,
    FRT_SMOOTH_TRIANGLE = 4,
    FRT_SPHERE = 5,
    FRT_TOROID = 6,
    FRT_TRIANGLE = 7,
    FRT_CSG = 8,
    FRT_GROUP = 9
};

/*
 * One node of the object tree in depth-first pre-order (the reference's child
 * order, which its shadow-ray semantics depend on). A subtree occupies
 * [index, skip). For a CSG node the left operand starts at index+1 and the
 * right operand at right.
 */
typedef struct frt_node {
    int32_t type;      /* enum frt_node_type */
    int32_t skip;      /* first pre-order index after this subtree */
    int32_t parent;    /* parent node, -1 for a world shape */
    int32_t tparent;   /* nearest strict ancestor with a transform, -1 if none */
    int32_t xform;     /* index into frt_scene.xforms (16 doubles, the inverse), -1 = identity */
    int32_t material;  /* index into frt_scene.materials (leaves) */
    int32_t prim;      /* offset into frt_scene.prim_data (leaves), CSG: operation (enum csg_ops_enum) */
    int32_t right;     /* CSG: pre-order index of the right operand */
    double bbox[6];    /* groups and CSG: own-space bounds min xyz, max xyz */
} frt_node;

/* per-leaf parameters in prim_data (doubles), by type:
 *   cylinder / cone : minimum, maximum, closed
 *   toroid          : r1, r2
 *   triangle        : p1[3] e1[3] e2[3] normal[3] t1[2] t2[2] t3[2] use_textures
 *   smooth triangle : p1[3] e1[3] e2[3] n1[3] n2[3] n3[3] t1[2] t2[2] t3[2] use_textures */
#define FRT_TRI_P1 0
#define FRT_TRI_E1 3
#define FRT_TRI_E2 6
#define FRT_TRI_N 9
#define FRT_TRI_N2 12
#define FRT_TRI_N3 15
#define FRT_TRI_UV_FLAT 12
#define FRT_TRI_UV_SMOOTH 18

typedef struct frt_material {
    double Ka[3], Kd[3], Ks[3], Tf[3], refl[3];
    double Ns, Ni, Tr;
    int32_t reflective;
    int32_t casts_shadow;
    /* pattern indices (frt_scene.patterns) or -1 */
    int32_t map_Ka, map_Kd, map_Ks, map_Ns, map_d, map_bump, map_refl;
    int32_t pad;
} frt_material;

/* pattern kinds: same numbering as the reference's enum pattern_type (pattern.h:23-41) */
typedef struct frt_pattern {
    int32_t type;
    int32_t transform_identity;
    int32_t uv_map;        /* texture map: enum uv_map_type */
    int32_t faces;         /* texture map: index of the first face pattern */
    int32_t child[3];      /* blended / nested / perturbed operands */
    int32_t texture;       /* uv texture: index into frt_scene.textures */
    int32_t width, height; /* uv checker */
    int32_t octaves, seed; /* perturbed */
    double inv[16];        /* inverse pattern transform */
    double color[5][3];    /* a,b (concrete / uv check); main,ul,ur,bl,br (align check) */
    double frequency, scale_factor, persistence;
} frt_pattern;

/* texture: texel (col,row) = canvas_pixel_at(canvas, col, row) pre-evaluated on the host
 * (color-space function and optional 3x3 super-sampling applied), 3 doubles per texel */
typedef struct frt_texture {
    int64_t offset; /* into frt_scene.texels, in doubles */
    int32_t width, height;
} frt_texture;

enum frt_light_type { FRT_AREA_LIGHT = 0, FRT_CIRCLE_LIGHT = 1, FRT_HEMISPHERE_LIGHT = 2, FRT_POINT_LIGHT = 3 };

typedef struct frt_light {
    int32_t type;
    int32_t num_samples; /* points per cache row */
    int32_t rows;        /* cache rows (reference cache_size), 1 for point lights */
    int32_t pad;
    int64_t points;      /* offset into frt_scene.light_points (3 doubles per point, row-major) */
    double intensity[3];
    /* photon emission (reference light.c:14-99, photon_tracer.c:195-233) */
    double normal[3];    /* emission hemisphere axis: area normalize(uvec x vvec), circle / hemisphere normal */
    double position[3];  /* point / hemisphere light position */
    int64_t num_photons; /* photons apportioned to this light by CIE L* (trace_photons) */
} frt_light;

typedef struct frt_camera {
    int64_t hsize, vsize, usteps, vsteps;
    double half_width, half_height, pixel_size, canvas_distance;
    double inv[16];          /* camera transform inverse */
    double aperture_size;
    int32_t aperture_type;   /* enum aperture_type (camera.h:9-19) */
    int32_t jitter;          /* jittered CMJ sub-pixel tables */
    double aperture_args[4];
} frt_camera;

typedef struct frt_config {
    int32_t include_direct, include_ambient, include_diffuse, include_spec_highlight, include_specular;
    int32_t path_length;
    int32_t all_ni_one;      /* every material has Ni == 1.0: n1 = n2 = 1 without the container walk */
    int32_t pad;
    /* global illumination (reference renderer.c:52-71, photon_tracer.c, pm.c) */
    int32_t use_gi;                 /* include_global || debug_visualize_photon_map */
    int32_t visualize_photon_map;
    int32_t include_caustics;       /* gi.include_caustics */
    int32_t include_final_gather;   /* gi.include_final_gather */
    int32_t gi_usteps, gi_vsteps;   /* final-gather hemisphere grid */
    int32_t irradiance_num;         /* k of the k-nearest-photon estimate */
    int32_t gi_path_length;         /* photon bounces */
    int32_t trace_caustic_map;      /* trace_photons(populate_caustic_map, ...) */
    int32_t trace_global_map;       /* trace_photons(..., populate_global_map) */
    int64_t photon_count;           /* photons per map (gi.photon_count); 0: no maps */
    double irradiance_radius;
    double cone_filter_k;
} frt_config;

typedef struct frt_scene {
    uint32_t abi_version;
    int32_t num_nodes;
    const frt_node *nodes;
    int32_t num_roots;       /* world shapes (generated main() has one: the divided world group) */
    int32_t pad0;
    const int32_t *roots;    /* pre-order index of each world shape */
    int32_t num_xforms;
    int32_t pad1;
    const double *xforms;    /* 16 doubles per transform (the inverse matrix, row-major) */
    int64_t prim_len;
    const double *prim_data;
    int32_t num_materials;
    int32_t num_patterns;
    const frt_material *materials;
    const frt_pattern *patterns;
    int32_t num_textures;
    int32_t pad2;
    const frt_texture *textures;
    int64_t texel_len;       /* doubles */
    const double *texels;
    int32_t num_lights;
    int32_t pad3;
    const frt_light *lights;
    int64_t light_point_len; /* doubles */
    const double *light_points;
    frt_camera camera;
    const double *sample_table; /* usteps*vsteps*2: the non-jittered CMJ table (sampler.c:401-510) */
    frt_config config;
} frt_scene;

typedef struct frt_scene_handle frt_scene_handle;

typedef struct frt_frame_params {
    int64_t row_begin, row_end; /* rows of the frame to render */
    int64_t row_stride;         /* render rows row_begin, row_begin+stride, ... (1 = contiguous) */
    uint64_t seed;              /* counter-RNG seed for stochastic rows (area-light cache rows, jitter) */
    int64_t batch_samples;      /* camera samples per wavefront batch (0 = engine default) */
    int32_t count_reference_rays; /* 1: also count the rays the reference would cast (slower) */
    int32_t precision;          /* enum frt_precision (the former padding word: 0 in every older caller) */
} frt_frame_params;

/*
 * Shading precision of a frame. Parity (the default) computes everything in binary64 and matches the reference.
 * Fast32 computes lighting_microfacet's light-point loop (reference renderer.c:895-979) in binary32 (k_shade_lit32,
 * fast_ray_tracer_amd/csrc/frt_shade32.hpp); geometry, visibility, recursion and every per-node term stay binary64,
 * so a fast frame differs from a parity frame only in the value of lit nodes' diffuse and specular sums
 * (DESIGN.md "Fast shading mode": the error model and the measured mismatch). FRT_PRECISION_DEFAULT leaves the
 * choice to the environment, read at every frame: FRT_PRECISION=fast32 | parity, else parity. A non-zero value
 * here wins over the environment. Any other value, or a fast frame with FRT_SHADE_SPLIT=0, makes frt_render_rows*
 * fail ("precision N is not supported"); nothing falls back silently.
 */
enum frt_precision { FRT_PRECISION_DEFAULT = 0, FRT_PRECISION_PARITY = 1, FRT_PRECISION_FAST32 = 2 };

typedef struct frt_frame_stats {
    uint64_t primary_rays;
    uint64_t secondary_rays;      /* reflection / refraction rays actually traced */
    uint64_t shadow_rays;         /* shadow rays actually traced */
    uint64_t pruned_secondary;    /* zero-weight secondary rays not traced */
    uint64_t hits;                /* path nodes shaded */
    uint64_t errors;              /* capacity / depth overflows (non-zero = result invalid) */
    double render_ms;             /* wall time of the device work (events) */
    double kernel_ms[8];          /* per-kernel accumulated time: trace, shadow, shade, combine, resolve, trace (level 0), prepare, gi */
    uint64_t kernel_launches[8];
    double shadow_kernel_bytes;   /* algorithmic bytes moved by the shadow kernel (DESIGN.md byte model) */
    uint64_t gather_rays;         /* final-gather rays traced (global illumination) */
    uint64_t photons[2];          /* photons in the caustic / global map used by this frame */
    double photon_ms;             /* photon tracing + map build of this frame (0 when the maps were reused) */
    int32_t shadow_jit;           /* 1: the scene-specialised shadow kernel ran (frt_jit.hip), 0: the generic walk */
    int32_t photon_pass;          /* 1: this frame traced its photon maps (a new seed), 0: maps reused / no GI */
    /* kernels inside the slots above (HIP events around each launch on the engine stream):
       0 frt_jit_beam / frt_jit_beam_list (node pair kernel), 1 frt_jit_shadow (per-ray kernel), 2 k_gather_est,
       3 k_gather_hit, 4 frt_jit_tile (tile pair kernel), 5 frt_jit_sub (sub-part pair kernel), 6 frt_jit_subtile
       (sub-tile pair kernel), 7 k_shade_lit (the shading of the path nodes some light reaches; 0 in a fast32 frame), 8 k_lit_scan +
       k_lit_scatter (the lit list in light-row order, multi-row lights), 9 k_shade_lit32 (k_shade_lit's place in a
       fast32 frame; 0 in a parity frame), 10 k_feature_resolve (the features pass, frt_render_features*; 0 in a colour
       frame), 11 frt_jit_split (the tiles of the (super-tile, sample) pairs left mixed; 0 without super-tiles);
       12-15 unused */
    double sub_ms[16];
    uint64_t sub_launches[16];
    uint64_t shadow_rays_walked;  /* shadow rays walked one by one; the rest of shadow_rays were resolved
                                     (exactly, for every ray) per (node, light part) by frt_jit_beam */
    /* the scene-specialised pair kernels' work this frame (0 without them) */
    uint64_t shadow_tile_pairs;   /* (tile of consecutive path nodes, light part) beams frt_jit_tile tested */
    uint64_t shadow_tile_mixed;   /* of those, the ones it could not decide (their nodes go to frt_jit_beam_list) */
    uint64_t shadow_pairs;        /* (path node, light part) beams tested by frt_jit_beam / frt_jit_beam_list */
    uint64_t shadow_pairs_mixed;  /* of those, the ones left mixed */
    uint64_t shadow_sub_pairs;    /* (tile, light sub-part) beams of the mixed tile pairs tested by frt_jit_sub */
    uint64_t shadow_sub_mixed;    /* of those, the ones left mixed */
    uint64_t shadow_subtile_pairs; /* (sub-tile, light sub-part) beams of those tested by frt_jit_subtile */
    uint64_t shadow_subtile_mixed; /* of those, the ones whose nodes frt_jit_beam_list tested */
    uint64_t lit_nodes;           /* path nodes some light sample reaches (k_shade_lit's lanes); counted per frame
                                     when stats are asked for */
    uint64_t prepare_uniform_waves; /* k_prepare waves whose lanes all hit one leaf and took the scalar path
                                       (FRT_PREPARE_UNIFORM); counted in statistics frames only */
} frt_frame_stats;

/* The shadow pass's per-stage counters of the handle's last frame (frt_shadow_stages): the beam stages in their
 * order. With super-tiles (FRT_JIT_SUPERTILE) the first two stages test runs of `supertile` nodes at the levels that
 * use them, and frt_jit_split the tiles of the pairs they leave; without, split_* are 0. split_ms and
 * split_launches are filled by frames rendered with statistics (HIP events), like frt_frame_stats.sub_ms. */
typedef struct frt_shadow_stage_stats {
    uint64_t supertile;        /* path nodes per super-tile of the handle's kernels, 0: none (or switched off) */
    uint64_t tile_pairs;       /* (run, light part) beams tested by frt_jit_tile */
    uint64_t tile_mixed;
    uint64_t sub_pairs;        /* (run, light sample) beams tested by frt_jit_sub */
    uint64_t sub_mixed;
    uint64_t split_pairs;      /* (tile, light sample) beams tested by frt_jit_split */
    uint64_t split_mixed;
    uint64_t subtile_pairs;    /* (sub-tile, light sample) beams tested by frt_jit_subtile */
    uint64_t subtile_mixed;
    uint64_t rays_walked;      /* shadow rays walked one by one (frt_frame_stats.shadow_rays_walked) */
    uint64_t split_launches;
    double split_ms;
} frt_shadow_stage_stats;

/* number of HIP devices visible (0 when no GPU) */
int frt_device_count(void);

/* create the HIP runtime's context on `device` ahead of use (render_multi runs it on a thread of its own per device
 * while it flattens the scene); returns 0, or -1 when the device cannot be set */
int frt_device_warmup(int device);

/* page-locked host memory (hipHostMalloc) for render_multi's canvas array, which the device then writes by DMA
 * instead of through the runtime's staging copies into pageable memory (the reference's canvas_alloc mallocs it,
 * src/libs/canvas/canvas.c:21-24; canvas_free hands it back, canvas.c:54); NULL when it cannot be allocated.
 * frt_host_pinned_free releases it (NULL: nothing) */
void *frt_host_pinned_alloc(size_t bytes);
void frt_host_pinned_free(void *p);

/* sizeof(frt_frame_stats) as this library was built: a caller's mirror of the struct (runtime.py FrameStats)
 * checks its size against it before passing one in (no device needed) */
size_t frt_frame_stats_size(void);

/* sizeof(frt_frame_params) as this library was built, for the same check (runtime.py FrameParams) */
size_t frt_frame_params_size(void);

/* the last frame's per-stage shadow counters of `scene` (zeros before its first frame); returns
 * sizeof(frt_shadow_stage_stats) */
size_t frt_shadow_stages(const frt_scene_handle *scene, frt_shadow_stage_stats *out);

/* message of the last failing call on this thread */
const char *frt_last_error(void);

/* copy a flattened scene into HBM on `device`; the host scene may be freed afterwards */
int frt_scene_upload(const frt_scene *scene, int device, frt_scene_handle **out);

/*
 * Replace the handle's camera; later frames render cam's hsize x vsize. Nothing on the device but the camera depends
 * on it (it enters through camera_ray alone, csrc/frt_camera.hpp), so the scene buffers, the loaded kernels, the
 * level state (which grows on demand, as ever) and the photon maps stay: with global illumination a frame after
 * this call with an unchanged seed reports photon_pass == 0. sample_table holds 2 * usteps * vsteps doubles, as
 * frt_scene.sample_table does, and is uploaded again only when its size or contents differ from the handle's.
 * Returns 0, or -1 with the reason in frt_last_error for a null pointer, a size or step count <= 0, more than
 * 2^31 - 1 samples per pixel or more than 2^52 samples per frame (the engine's 32-bit sample-in-pixel and 64-bit
 * path-node key); after a failure the handle keeps its old camera and stays usable.
 */
int frt_scene_set_camera(frt_scene_handle *h, const frt_camera *cam, const double *sample_table);

/* render rows into a host buffer (rows x hsize x 4 doubles, rows in the order rendered) */
int frt_render_rows(frt_scene_handle *h, const frt_frame_params *params, double *host_rgba,
                    frt_frame_stats *stats);

/* same, writing into device memory on the handle's device (e.g. a torch tensor's storage) */
int frt_render_rows_device(frt_scene_handle *h, const frt_frame_params *params, double *device_rgba,
                           frt_frame_stats *stats);

/*
 * Render nviews cameras over the handle's scene in one frame: a strip. The views share hsize, vsize, usteps, vsteps
 * and jitter (and the steps are the handle's own, whose sample table they use: frt_scene_set_camera one of them
 * first otherwise); they may differ in transform, field-of-view scalars and aperture. Anything else is refused with
 * the reason in frt_last_error. params' row range and stride apply inside each view, and the output is view-major:
 * nviews x rows x hsize x 4 doubles. View k is, bit for bit, what frt_scene_set_camera(cams[k]) followed by
 * frt_render_rows* with the same params (seed included) renders; the levels' launches and count read-backs are
 * paid once for the strip instead of once per view. The handle's own camera is unchanged afterwards.
 */
int frt_render_views_host(frt_scene_handle *h, const frt_camera *cams, int32_t nviews, const frt_frame_params *params,
                          double *host_rgba, frt_frame_stats *stats);
int frt_render_views_device(frt_scene_handle *h, const frt_camera *cams, int32_t nviews,
                            const frt_frame_params *params, double *device_rgba, frt_frame_stats *stats);

/*
 * First-hit feature buffers: what level 0 knows about each pixel, without shading it. The pass runs the closest hit
 * and prepare_computations of the camera samples a colour frame with the same params traces (rows, stride, seed,
 * batch, jitter and aperture alike: sample `sub` of pixel `p` is the same camera_ray in both) and nothing else: no
 * shadow, shading, GI or combine kernel, and no photon pass. params' precision and count_reference_rays are ignored.
 * A sample hits when its closest hit has a leaf.
 *
 * geom: 8 doubles per pixel (one 64-byte line), pixels in the colour output's order:
 *   [0]    depth     mean over the hitting samples of the closest hit's t. ray_for_pixel normalises the direction, so
 *                    t is the Euclidean distance from the ray's origin (with an aperture: the lens point)
 *   [1..3] normal    mean over the hitting samples of comps.normalv: world space, turned towards the eye when the hit
 *                    is inside, after a bump map; the mean is not renormalised
 *   [4..6] albedo    mean over the hitting samples of Kd as prepare_computations leaves it: the pattern's colour
 *                    where the material has a map_Kd, else the material's Kd
 *   [7]    coverage  hits / spp (one IEEE division)
 * Each mean is the sum in sub-sample order (sub = v * usteps + u ascending, misses skipped) divided by the hit count
 * with one IEEE division; a pixel without a hit holds eight +0.0. The result is a placement, as the colour frame is:
 * bit-identical for any batch size, row split, strip position or wave schedule.
 * ids: 2 int32 per pixel: the pre-order node index of the leaf and the material index of the pixel's first hitting
 * sample in sub-sample order; -1, -1 without a hit.
 *
 * Either buffer may be NULL (not both). The *_device calls take device memory on the handle's device, the *_host
 * calls host memory. The *_views calls render a strip as frt_render_views* does (same rules for the cameras, the
 * output view-major): view k is, bit for bit, frt_scene_set_camera(cams[k]) + frt_render_features*.
 * stats (may be NULL) receives primary_rays, render_ms, errors, kernel_ms / kernel_launches [5] (trace) and [6]
 * (prepare), and sub_ms / sub_launches [10] (k_feature_resolve); everything else is 0.
 * Returns 0, or -1 with the reason in frt_last_error (a null handle, params or buffers; both buffers NULL; a strip's
 * refusals; device error bits). The handle is left as a colour frame leaves it: its camera, kernels and photon maps
 * stay.
 */
typedef struct frt_feature_buffers {
    double *geom;  /* 8 doubles per pixel, or NULL */
    int32_t *ids;  /* 2 int32 per pixel, or NULL */
} frt_feature_buffers;

int frt_render_features_device(frt_scene_handle *h, const frt_frame_params *params, const frt_feature_buffers *dev,
                               frt_frame_stats *stats);
int frt_render_features_host(frt_scene_handle *h, const frt_frame_params *params, const frt_feature_buffers *host,
                             frt_frame_stats *stats);
int frt_render_feature_views_device(frt_scene_handle *h, const frt_camera *cams, int32_t nviews,
                                    const frt_frame_params *params, const frt_feature_buffers *dev,
                                    frt_frame_stats *stats);
int frt_render_feature_views_host(frt_scene_handle *h, const frt_camera *cams, int32_t nviews,
                                  const frt_frame_params *params, const frt_feature_buffers *host,
                                  frt_frame_stats *stats);

/* doubles per pixel of frt_feature_buffers.geom (8): a caller's mirror checks it (no device needed) */
size_t frt_feature_geom_words(void);

void frt_scene_release(frt_scene_handle *h);

/* Diagnostics (no device needed): generate the scene-specialised shadow kernel of a flattened
 * scene and compile it for gfx950 with hiprtc, as frt_scene_upload does. Returns 0 compiled,
 * 1 scene not eligible (the generic walk runs), -1 compile error. `log` receives the reason or
 * the compiler log, `src` (may be NULL) the generated HIP source. */
int frt_jit_check(const frt_scene *scene, char *log, size_t log_cap, char *src, size_t src_cap);

/* Diagnostics (no device needed): the meshes frt_scene_upload would search per lane (group subtrees of
 * groups and triangles only, scenes over 512 nodes) and their BVHs, checked: every triangle of a mesh
 * in exactly one leaf, every box containing its triangles' vertices and its children's boxes, every
 * child's smallest pre-order index right. out[0] meshes, out[1] their triangles, out[2] BVH nodes,
 * out[3] deepest level (min(n, 4) written). Returns 0 when sound, else the number of violations. */
int frt_mesh_check(const frt_scene *scene, int64_t *out, int n);

/* Diagnostics (current device): the engine's binary64 sqrt / reciprocal core sequences and normalize
 * (frt_math.hpp) against the compiler's sqrt and division (bit for bit), and the shading's Newton-refined
 * estimates against their 2^-46 relative bound, on n lanes of random vectors; returns the number of
 * failed checks (0: all hold), or -1 on a HIP error. */
int64_t frt_math_selftest(int64_t n, uint64_t seed);

/* Diagnostics (current device): the fast mode's binary32 light-point term against the binary64 term on n lanes of
 * random inputs: unit normal and eye, |over_point|, |light point| <= 8 with |diff| >= 1, Ns from {0, 1, 2.5, 10, 200,
 * 1000, 5000}, a share of lanes with n.l and n.e down to 1e-30 and with n.l slightly negative. Returns the number
 * of lanes whose binary32 result is not finite while the binary64 one is, plus the lanes whose diffuse term l.n is
 * off by more than 32 * 2^-24 (the bound of those input ranges: frt_shade32.hpp), or -1 on a HIP error. For the
 * record, not gated: out[0] the worst deviation of the specular factor relative to its binary64 value over the
 * lanes with l.n >= 2^-16, out[1] the same over their lanes with Ns <= 200, out[2] the worst absolute deviation of
 * l.n, out[3] the number of lanes behind out[0] (min(nout, 4) written; out may be NULL). */
int64_t frt_shade32_selftest(int64_t n, uint64_t seed, double *out, int nout);

/* Counters of the scene-specialised kernels' code-object cache since the library was loaded (no device
 * needed): out[0] hiprtc compiles, out[1] code objects read from the on-disk cache, out[2] code objects
 * written to it, out[3] modules loaded (one per device and scene source), out[4] uploads that found
 * their device's module loaded already. A scene's kernels are compiled once per process (every device
 * and handle shares the code object) and, through the on-disk cache (FRT_JIT_CACHE_DIR, default
 * $XDG_CACHE_HOME/frt_jit or ~/.cache/frt_jit; FRT_JIT_CACHE=0 turns it off), once per machine.
 * Writes min(n, 5) counters; returns 5. */
int frt_jit_cache_stats(int64_t *out, int n);

/* Diagnostics: the phases of this thread's last frt_scene_upload, in ms: out[0] device selection (the
 * process's first HIP call initialises the runtime here), [1] scene buffers to HBM, [2] walk records and
 * mesh BVHs, [3] the scene-specialised kernels' source, [4] their code object (0 when this process had it;
 * an on-disk cache read or a hiprtc compile otherwise), [5] its load into the device's module, [6] the
 * rest (light tables, work buffers, stream), [7] total. Writes min(n, 8); returns 8. */
int frt_upload_phases(double *out, int n);

/* Counters of the photon passes since the library was loaded: out[0] photon passes traced, out[1] passes a
 * handle took from another device's trace of the same scene and seed (render_multi over N devices traces
 * and balances once per process). Writes min(n, 2); returns 2. */
int frt_photon_pass_stats(int64_t *out, int n);

/* Photon map entry points (parity tests; no scene needed).
 * frt_pm_balance replaces pm_balance (reference src/libs/photon_map/pm.c:329-494): the balanced
 * kd-tree of n photons given in the reference's storage order (pos: 3 doubles each); heap_of[i] = the
 * heap index (1..n) of photon i, plane[h] (n + 1 entries) = the split axis of heap node h. Host only.
 * frt_pm_estimate replaces pm_irradiance_estimate (pm.c:91-156, with pm_locate_photons pm.c:163-252)
 * over one map balanced as above: nq queries (pos[3], normal[3] each) on `device`; irrad receives 3
 * doubles per query (before lighting_gi's scaling), found the photons used. pos / power: 3 doubles per
 * photon in storage order, power already scaled (pm_scale_photon_power); theta_phi: the photon's stored
 * direction bytes (Photon.theta, Photon.phi, pm.c:288-300; decoded as pm_photon_dir does). */
int frt_pm_balance(const double *pos, int64_t n, int32_t *heap_of, int8_t *plane);
int frt_pm_estimate(int device, const double *pos, const double *power, const uint8_t *theta_phi, int64_t n,
                    const double *queries, int64_t nq, double radius, int32_t k, double cone_k,
                    double *irrad, int64_t *found);

/*
 * Image encode (fast_ray_tracer_amd/csrc/frt_encode.hip): the 16-bit values of write_ppm_file / write_png
 * (reference src/libs/canvas/canvas.c:150-327, 376-510) computed on the device, byte-identical to the host pass
 * (DESIGN.md "Image encode"). Everything but pow(t, 1/2.4) is plain IEEE arithmetic the device repeats bit for
 * bit; a value whose code the device's pow cannot prove (within FRT_ENCODE_MARGIN of a code boundary or of
 * srgb_max) is left undecided and listed, and the caller (host/frt_canvas.c) recomputes it with the host's own
 * arithmetic.
 */
enum frt_encode_mode {
    FRT_ENCODE_PPM_SCALED = 0,  /* write_ppm_file(c, true, ..)  */
    FRT_ENCODE_PPM_CLAMPED = 1, /* write_ppm_file(c, false, ..) */
    FRT_ENCODE_PNG = 2          /* write_png                    */
};

enum frt_encode_backend { FRT_ENCODE_HOST = 0, FRT_ENCODE_DEVICE = 1, FRT_ENCODE_AUTO = 2 };

/* why the device did not produce the bytes (the host pass did) */
enum frt_encode_decline {
    FRT_ENCODE_TAKEN = 0,        /* the device produced them, or the host backend was asked for */
    FRT_ENCODE_ZERO_MAX = 1,     /* a channel's maximum is 0 (PPM modes: x / rgb_max is not finite) */
    FRT_ENCODE_NON_FINITE = 2,   /* a colour channel of some pixel is NaN or infinite */
    FRT_ENCODE_OVER_CAP = 3,     /* more than 1/64 of the values undecided */
    FRT_ENCODE_NO_DEVICE = 4,    /* no usable GPU, or a HIP call failed (frt_encode_error) */
    FRT_ENCODE_TOO_LARGE = 5     /* 3 * width * height does not fit the 32-bit undecided index */
};

#define FRT_ENCODE_MARGIN 0x1p-40 /* relative distance from a boundary under which a pow-branch value is undecided */

typedef struct frt_encode_stats {
    uint64_t values;     /* 3 * width * height */
    uint64_t undecided;  /* values the device left to the host (patched there) */
    int32_t backend;     /* enum frt_encode_backend: who produced the bytes */
    int32_t decline;     /* enum frt_encode_decline */
    int32_t mode;        /* enum frt_encode_mode */
    int32_t device;      /* the HIP device used, -1 when none */
    double rgb_max[3];   /* construct_ppm's two printed maxima (PNG: rgb_max as measured, srgb_max 1.0) */
    double srgb_max[3];
    double upload_ms;    /* canvas to the device (0 when it was there) */
    double kernel_ms;    /* the maximum and the quantise kernel (HIP events) */
    double readback_ms;  /* the bytes, the undecided list and its pixels to the host */
    double patch_ms;     /* host: recomputing the undecided values */
    double host_ms;      /* the host pass, when it produced the bytes */
} frt_encode_stats;

/*
 * Encode a width x height x 4 binary64 canvas (in host memory, or with rgba_on_device != 0 in device memory on
 * `device`) into out: 6 * width * height bytes, big-endian 16-bit R G B in pixel order. srgb_max / inverse are the
 * quantiser's per-channel constants and code_one the code of an input that is exactly 1.0, all three computed by
 * the caller with the host's arithmetic. The undecided values come back as und_idx[j] = 3 * pixel + channel with
 * (rgba_on_device only) the pixel's four doubles in und_px[4 * j]; both hold values / 64 entries. Returns 0 when
 * the bytes are in out (st->backend FRT_ENCODE_DEVICE, st->undecided entries to patch), 1 when the device
 * declined (st->decline says why; out is unspecified), -1 on a HIP error (frt_encode_error; st->decline
 * FRT_ENCODE_NO_DEVICE).
 */
int frt_encode16_device(const double *rgba, int rgba_on_device, size_t width, size_t height, int mode, int device,
                        const double srgb_max[3], const double inverse[3], const unsigned short code_one[3],
                        unsigned char *out, uint32_t *und_idx, double *und_px, frt_encode_stats *st);

/* copy `bytes` of device memory on `device` to the host (a declined device-resident canvas goes to the host pass) */
int frt_encode_fetch(void *host, const void *device_ptr, size_t bytes, int device);

/* message of this thread's last failing encode call */
const char *frt_encode_error(void);

/* free the encode's device buffers (kept between calls, per device) */
void frt_encode_release(void);

/*
 * Diagnostics (current device): the device's 1.055 * pow(t, 1/2.4) - 0.055 against the host libm's on n values t:
 * log-uniform over [0.0031308, 4], one in eight within 4 ulps of 1.0 and one in eight within 4 ulps of 0.0031308
 * (from it upwards). Returns the number of lanes whose pow or sRGB value deviates from the host's by 2^-44
 * relative or more (or is not finite), -1 on a HIP error. out[0] the worst relative deviation of the sRGB value,
 * out[1] of pow alone, out[2] the lanes whose sRGB value differs at all (min(nout, 3) written; out may be NULL).
 */
int64_t frt_encode_selftest(int64_t n, uint64_t seed, double *out, int nout);

/*
 * Denoise (fast_ray_tracer_amd/csrc/frt_denoise.hip, host/frt_denoise.c; DESIGN.md "Denoise"): an edge-avoiding
 * a-trous filter (Dammertz et al. 2010) over a colour frame, guided by the first-hit feature buffers. The host pass
 * (frt_denoise_host, libfrt_host) is the definition; the device pass repeats it operation for operation in binary64
 * (+ - * / and comparisons only, no fused multiply-add), so the two agree bit for bit.
 *
 * Inputs: nimages images of h x w pixels, stacked view-major. rgba 4 doubles per pixel, geom 8 doubles per pixel
 * (frt_feature_buffers.geom), ids 2 int32 per pixel (frt_feature_buffers.ids).
 * A pixel is valid when ids.node >= 0, depth is finite and > 0, the three colour channels are finite (and its
 * material id is not INT32_MIN, which the guide columns reserve). An invalid pixel is never filtered and never a tap:
 * its output is its input bit for bit. Taps never leave the pixel's own image.
 * Per valid pixel once: a[ch] = albedo[ch] + albedo_eps (demodulate) or 1.0; x[ch] = rgb[ch] / a[ch];
 * nn = (n0*n0 + n1*n1) + n2*n2; inv_nn = nn > 0 ? 1/nn : 0; iz = 1/depth.
 * Iteration i = 0 .. iterations-1 with step s = 2^i: the 5 x 5 taps q = p + s*(dx, dy), dy outside and dx inside,
 * ascending, B3 spline weights hk = K[|dx|] * K[|dy|] with K = {3/8, 1/4, 1/16}. The centre tap weighs hk; another
 * valid tap inside the image is skipped when match_material and the materials differ, or when d = n_p . n_q <= 0;
 * else t = min((d*d) * (inv_nn_p*inv_nn_q), 1.0) squared normal_squarings times, r = z_p - z_q,
 * xz = ((r*r) * kz) * (iz_p*iz_q), xc = |x_p - x_q|^2 * kc_i, u = (1 + xz) * (1 + xc), weight (hk*t) / (u*u), with
 * kz = 1/sigma_depth^2 and kc_i = ldexp(1/sigma_color^2, 2*i). x_{i+1} = sum(weight * x_q) / sum(weight).
 * Output: rgb = x_N * a on valid pixels, alpha copied. out may be rgba itself.
 */
enum frt_denoise_backend { FRT_DENOISE_HOST = 0, FRT_DENOISE_DEVICE = 1, FRT_DENOISE_AUTO = 2 };

#define FRT_DENOISE_MAX_ITERATIONS 8
#define FRT_DENOISE_MAX_SQUARINGS 8

typedef struct frt_denoise_params {
    int32_t iterations;       /* 1..8 (default 5): a-trous passes, steps 1, 2, 4, .. */
    int32_t normal_squarings; /* 0..8 (default 5): the normal term is cos^2 raised to 2^normal_squarings */
    int32_t demodulate;       /* 0 or 1 (default 1): filter rgb / (albedo + albedo_eps) */
    int32_t match_material;   /* 0 or 1 (default 1): taps of another material id weigh 0 */
    double sigma_color;       /* > 0 (default 1.0) */
    double sigma_depth;       /* > 0 (default 0.1): relative depth difference */
    double albedo_eps;        /* > 0 (default 2^-10) */
} frt_denoise_params;

typedef struct frt_denoise_stats {
    uint64_t pixels;        /* w * h * nimages */
    uint64_t valid_pixels;
    int32_t iterations;
    int32_t backend;        /* enum frt_denoise_backend: who produced out */
    int32_t device;         /* the HIP device used, -1 when none */
    int32_t reserved;       /* 0 */
    double upload_ms;       /* the three inputs to the device (0 when they were there) */
    double pack_ms;         /* k_denoise_pack (HIP events) */
    double atrous_ms;       /* the a-trous launches together */
    double atrous_iter_ms[FRT_DENOISE_MAX_ITERATIONS]; /* each launch */
    double readback_ms;     /* out (and the valid counts) to the host */
    double host_ms;         /* the host pass, when it produced out */
} frt_denoise_stats;

size_t frt_denoise_params_size(void);
size_t frt_denoise_stats_size(void);
void frt_denoise_defaults(frt_denoise_params *params);

/*
 * The refusals every denoise entry point shares (no device needed): a null rgba / geom / ids / params / out; w, h or
 * nimages <= 0; more than 2^31 - 1 pixels in total; a parameter outside its range; a sigma or albedo_eps that is not
 * finite. Returns 0, or -1 with the reason in frt_denoise_error().
 */
int frt_denoise_check(const double *rgba, const double *geom, const int32_t *ids, int64_t w, int64_t h,
                      int64_t nimages, const frt_denoise_params *params, const double *out);

/*
 * The device pass. The four buffers are all in host memory (on_device 0: they are uploaded, out read back) or all in
 * device memory on `device`. stats may be NULL. Returns 0, or -1 (a refusal above, no such device, a HIP error:
 * frt_denoise_error); a refusal leaves out untouched. The pass keeps 100 bytes of scratch per pixel on the device
 * between calls (plus 104 for host buffers) until frt_denoise_release().
 */
int frt_denoise_device(const double *rgba, const double *geom, const int32_t *ids, int on_device, int64_t w, int64_t h,
                       int64_t nimages, const frt_denoise_params *params, int device, double *out,
                       frt_denoise_stats *stats);

/* message of this thread's last failing denoise call */
const char *frt_denoise_error(void);
/* (libfrt_host's passes report through the same message) */
void frt_denoise_set_error(const char *message);

/* copy `bytes` of host memory to device memory on `device` (the host pass's result for device-resident buffers) */
int frt_denoise_store(void *device_ptr, const void *host, size_t bytes, int device);

/* free the denoise's device buffers (kept between calls, per device) */
void frt_denoise_release(void);

/* The host pass (frt_denoise_host) and the entry point that picks a backend (frt_denoise) are libfrt_host's:
 * fast_ray_tracer_amd/host/frt_denoise.h. */

/*
 * Accumulator (fast_ray_tracer_amd/csrc/frt_accum.hip, host/frt_accum.c; DESIGN.md "Accumulation and the
 * variance-guided denoise"): the per-pixel running mean and variance of a sequence of frames, Welford's update in
 * binary64 (+ - * / and comparisons only, no fused multiply-add). The host pass (libfrt_host, host/frt_accum.h) is the
 * definition; the device pass repeats it operation for operation, so the two agree bit for bit.
 *
 * State per pixel: n (int32), mean[4] (r, g, b, a), m2[3]; all zero after create and reset.
 * Add one sample x (4 doubles): when any of the four is not finite the pixel skips the sample (counted in
 * frt_accum_stats.skipped). Otherwise n += 1 and for each of the four channels d = x - mean,
 * mean = mean + d / (double)n; for r, g, b also m2 = m2 + d * (x - mean), with the updated mean.
 * Resolve: mean_rgba = mean (zeros where n == 0). var, 4 doubles per pixel: channels 0..2
 * (m2 / (double)(n - 1)) / (double)n, the variance of the mean, 0.0 where n < 2; channel 3 (double)n.
 *
 * The device accumulator keeps its state as columns (7 columns of 8 bytes and one of 4: 60 bytes per pixel), a frame
 * of scratch (32 bytes per pixel; frt_render_rows_accumulate renders into it, host samples are uploaded into it) and,
 * once a resolve into host memory has run, 64 more for its two outputs. Everything is freed by the release.
 */
typedef struct frt_accum_dev frt_accum_dev;

typedef struct frt_accum_stats {
    uint64_t pixels;
    uint64_t frames;     /* adds since the create or the last reset */
    uint64_t skipped;    /* samples skipped since then, over all pixels (a non-finite channel) */
    int32_t device;      /* the HIP device, -1 for a host accumulator */
    int32_t reserved;    /* 0 */
    double add_ms;       /* the last k_accum_add (HIP events; 0 on the host) */
    double resolve_ms;   /* k_accum_resolve (HIP events), or the host's resolve */
} frt_accum_stats;

size_t frt_accum_stats_size(void);

/*
 * Refusals (all return -1 with the reason in frt_accum_error, and leave every output untouched): a null pointer;
 * npixels <= 0 or more than 2^31 - 1 (the columns' index is 32-bit); no such device. A skipped-sample counter is an
 * int32 per wave of 64 pixels: an accumulator takes at most 2^25 - 1 adds between resets (more is refused),
 * so that a wave whose 64 lanes skip every sample stays under 2^31.
 * rgba, mean_rgba and var are all in host memory (on_device 0: uploaded / read back) or all in device memory on the
 * accumulator's device. mean_rgba or var may be NULL (not both). stats may be NULL.
 */
int frt_accum_dev_create(int device, int64_t npixels, frt_accum_dev **out);
int frt_accum_dev_reset(frt_accum_dev *acc);
int frt_accum_dev_add(frt_accum_dev *acc, const double *rgba, int on_device);
int frt_accum_dev_resolve(frt_accum_dev *acc, double *mean_rgba, double *var, int on_device, frt_accum_stats *stats);
void frt_accum_dev_release(frt_accum_dev *acc);
int64_t frt_accum_dev_npixels(const frt_accum_dev *acc);
int frt_accum_dev_device(const frt_accum_dev *acc);
/* the accumulator's scratch frame (npixels x 4 doubles of device memory), allocated on first use; NULL on failure */
double *frt_accum_dev_frame(frt_accum_dev *acc);
/* frt_accum_dev_add of the scratch frame's contents */
int frt_accum_dev_add_frame(frt_accum_dev *acc);

/* message of this thread's last failing accumulator call (libfrt_host's passes report through the same message) */
const char *frt_accum_error(void);
void frt_accum_set_error(const char *message);

/*
 * Render nframes frames of the handle's scene into the accumulator, on the device: frame k (0-based) is exactly what
 * frt_render_rows_device renders with params->seed + k (wrapping uint64) and params otherwise unchanged, into the
 * accumulator's scratch frame, followed by one add. nframes >= 1; the accumulator is on the handle's device and its
 * npixels equals rows x width of params. stats (may be NULL) receives the frames' frt_frame_stats with every uint64
 * counter, every *_ms time, kernel_launches, sub_launches, shadow_kernel_bytes and photon_pass (the frames that
 * traced their photon maps) summed; photons and shadow_jit are the last frame's. Returns 0, or -1 with the reason in
 * frt_last_error; frames added before a failure stay added.
 */
int frt_render_rows_accumulate(frt_scene_handle *h, const frt_frame_params *params, int32_t nframes,
                               frt_accum_dev *acc, frt_frame_stats *stats);

/*
 * Variance-guided denoise (fast_ray_tracer_amd/csrc/frt_denoise_var.hip, host/frt_denoise_var.c; DESIGN.md
 * "Accumulation and the variance-guided denoise"): the spatial filter of SVGF (Schied et al. 2017) without
 * reprojection, on an accumulated mean and the variance of that mean. The host pass (frt_denoise_var_host,
 * libfrt_host) is the definition and the device pass repeats it bit for bit, as for the denoise above, whose
 * definition holds for everything not mentioned here.
 *
 * Inputs: the denoise's three (rgba, geom, ids, stacked over nimages) and var, 4 doubles per pixel as the
 * accumulator resolves it. Outputs: out (may be rgba itself) and out_var (may be var itself, may be NULL).
 * Valid: as above, and additionally var[0..2] finite and >= 0.
 * Pack: as above, plus v[ch] = var[ch] / (a[ch] * a[ch]).
 * Iteration i, step s = 2^i, on this iteration's colour x and variance v:
 *   Guide: vs_q = (v0_q + v1_q) + v2_q; g_p = (sum G * vs_q) / (sum G) over the 3 x 3 taps q = p + (dx, dy) at
 *   distance 1 whatever s is, dy outside and dx inside, ascending, G = {1/2, 1/4}[|dx|] * {1/2, 1/4}[|dy|]; taps outside
 *   the pixel's own image or invalid are skipped; there is no edge-stopping in this pre-filter.
 *   kc_p = kc / (g_p + var_eps) with kc = 1 / sigma_color^2, the same at every iteration (no ldexp tightening: the
 *   shrinking variance does that).
 *   Taps: the 5 x 5 loop above with xc = ((dc0*dc0 + dc1*dc1) + dc2*dc2) * kc_p; next to acc[ch] += w * x_q[ch] and
 *   ws += w it accumulates vacc[ch] += (w * w) * v_q[ch]; the centre weighs hk.
 *   x_{i+1} = acc / ws; v_{i+1}[ch] = vacc[ch] / (ws * ws).
 * Output: on valid pixels rgb = x_N * a and out_var[ch] = v_N[ch] * (a[ch] * a[ch]); alpha and var[3] are copied.
 * Invalid pixels are copied bit for bit in both outputs.
 * A pixel with variance 0 whose neighbours' variance is 0 has kc_p = kc / var_eps: any tap whose colour differs
 * weighs next to nothing, and the pixel is left alone.
 */
typedef struct frt_denoise_var_params {
    int32_t iterations;       /* 1..8 (default 5) */
    int32_t normal_squarings; /* 0..8 (default 5) */
    int32_t demodulate;       /* 0 or 1 (default 1) */
    int32_t match_material;   /* 0 or 1 (default 1) */
    double sigma_color;       /* > 0 (default 2.0): in standard deviations of the pre-filtered variance */
    double sigma_depth;       /* > 0 (default 0.1) */
    double albedo_eps;        /* > 0 (default 2^-10) */
    double var_eps;           /* > 0 (default 2^-40) */
} frt_denoise_var_params;

typedef frt_denoise_stats frt_denoise_var_stats; /* the same fields; pack_ms / atrous_* are the var kernels' */

size_t frt_denoise_var_params_size(void);
void frt_denoise_var_defaults(frt_denoise_var_params *params);

/* the denoise's refusals (frt_denoise_check) with var among the pointers and var_eps among the parameters; out_var
 * may be NULL. Returns 0, or -1 with the reason in frt_denoise_error(). */
int frt_denoise_var_check(const double *rgba, const double *var, const double *geom, const int32_t *ids, int64_t w,
                          int64_t h, int64_t nimages, const frt_denoise_var_params *params, const double *out);

/*
 * The device pass; buffers all in host memory (on_device 0) or all in device memory on `device`, as for
 * frt_denoise_device. It keeps 164 bytes of scratch per pixel on the device between calls (20 columns of 8 bytes, the
 * material column of 4), plus 136 for host buffers, grow-only, until frt_denoise_var_release().
 */
int frt_denoise_var_device(const double *rgba, const double *var, const double *geom, const int32_t *ids,
                           int on_device, int64_t w, int64_t h, int64_t nimages,
                           const frt_denoise_var_params *params, int device, double *out, double *out_var,
                           frt_denoise_var_stats *stats);

/* free the variance-guided denoise's device buffers (kept between calls, per device) */
void frt_denoise_var_release(void);

/* frt_denoise_var_host and frt_denoise_var (backend choice) are libfrt_host's: host/frt_denoise_var.h. */

/*
 * Reprojection (fast_ray_tracer_amd/csrc/frt_accum.hip k_accum_reproject, host/frt_reproject.c; DESIGN.md "Temporal
 * reprojection"): SVGF's reprojection step (Schied et al. 2017). It carries an accumulator's state from the pixels of
 * the camera it was accumulated under (prev) to the pixels of a moved camera (cur), and drops it where the surface a
 * current pixel sees was not visible before. The host pass (frt_reproject_host, libfrt_host) is the definition; the
 * device pass repeats it operation for operation in binary64 (+ - * /, sqrt, floor, comparisons and exact integer
 * conversions only, no fused multiply-add), so the two agree bit for bit.
 *
 * Inputs: a source accumulator src (accumulated under prev) and a destination accumulator dst != src of the same
 * npixels = w x h; the feature buffers of both views as frt_feature_buffers lays them out (prev_geom, prev_ids,
 * cur_geom, cur_ids; of geom only depth [0] and normal [1..3] are read); the two frt_cameras, whose hsize x vsize are
 * both w x h; frt_reproject_params.
 * xf_point(m, p)[r] = ((m[4r]*p[0] + m[4r+1]*p[1]) + m[4r+2]*p[2]) + m[4r+3] for r = 0..2; a.b and |a|^2 of
 * 3-vectors are (a0*b0 + a1*b1) + a2*b2.
 *
 * Setup (frt_reproject_setup, host only, once per call; both passes take its doubles): O_cur = xf_point(cur.inv,
 * (0,0,0)), O_prev likewise (the lens centre when there is an aperture), and prev_fwd, the inverse of prev.inv by the
 * host library's matrix_inverse. It refuses cameras whose sizes differ or are not positive, and a camera matrix,
 * scalar (half_width, half_height, pixel_size, canvas_distance) or inverse that is not finite.
 *
 * Per destination pixel p = (px, py), index py * w + px, with outcome 0 reprojected, 1 current pixel without a hit,
 * 2 no history:
 * 1. Valid: cur_ids.node >= 0 and the current depth d finite and > 0. Otherwise the all-zero state, outcome 1.
 * 2. World point: ray_for_pixel's centre ray with the point aperture: xoff = ((double)px + 0.5) * cur.pixel_size,
 *    yoff likewise with py; P = xf_point(cur.inv, (cur.half_width - xoff, cur.half_height - yoff,
 *    -cur.canvas_distance)); v = P - O_cur; dir = v * (1.0 / sqrt(|v|^2)); W[k] = O_cur[k] + d * dir[k].
 * 3. Into the previous camera: c = xf_point(prev_fwd, W); outcome 2 unless c.z is finite and < 0.
 *    s = -prev.canvas_distance / c.z; fx = (prev.half_width - c.x * s) / prev.pixel_size - 0.5; fy likewise with
 *    half_height and c.y. A coordinate within 2^-20 of a whole pixel is that pixel: rx = floor(fx + 0.5), and
 *    fx = rx where |fx - rx| <= 2^-20; fy likewise. (Under an unmoved camera fx misses px by the rounding of this
 *    chain alone; snapped, the pixel's own tap weighs exactly 1 and the others exactly 0, and the state comes through
 *    unchanged instead of blurred by 2^-50 of its neighbours. A camera move that shifts a surface by less than
 *    2^-20 of a pixel, about 1e-6, is therefore no move for that surface.) Outcome 2 unless fx >= -1.0 &&
 *    fx < (double)w && fy >= -1.0 && fy < (double)h (a NaN fails): the test comes before any conversion to an integer.
 *    x0 = (int)floor(fx), tx = fx - (double)x0; y0, ty likewise.
 * 4. Expected previous depth: e = sqrt(|W - O_prev|^2). (Beyond about 1e154 the square overflows and an infinite e
 *    accepts every previous depth; first-hit depths are nowhere near.)
 * 5. Taps q in the order (x0,y0), (x0+1,y0), (x0,y0+1), (x0+1,y0+1) with weights (1-tx)*(1-ty), tx*(1-ty),
 *    (1-tx)*ty, tx*ty. A tap is accepted when it lies inside the image; src.n_q > 0; prev_ids.node_q == cur_ids.node_p
 *    (and the material ids are equal when match_material); the previous depth z_q is finite and > 0 and
 *    |z_q - e| <= sigma_depth * e; and with dn = n_p . n_q, nn_p = |n_p|^2, nn_q = |n_q|^2: dn > 0 and
 *    dn*dn >= (normal_cos*normal_cos) * (nn_p*nn_q). The state of a tap is read only when it is accepted.
 * 6. Sums over the accepted taps in that order, from 0.0: ws += w; am[ch] += w * mean_q[ch] (4 channels);
 *    av[ch] += w * (m2_q[ch] / (double)n_q) (3 channels); an += w * (double)n_q. Outcome 2 when ws < min_weight.
 * 7. New state: mean[ch] = am[ch] / ws; r = an / ws + 0.5; n = max_history where r >= (double)max_history, else
 *    (int32)r (truncated: an / ws rounded to the nearest count, since the quotient of taps that all hold n samples may
 *    round to just under n), and at least 1; m2[ch] = (av[ch] / ws) * (double)n. Outcome 2 leaves the all-zero state.
 *
 * dst's previous contents are overwritten (a reset, then the fill): its frames become min(src.frames, max_history),
 * its skipped 0, and later adds continue Welford's update from this state unchanged, so a history capped at
 * max_history behaves like an exponential average whose newest frame weighs at least 1 / (max_history + 1).
 */
typedef struct frt_reproject_params {
    int32_t max_history;    /* 1..2^20 (default 32): the count a reprojected pixel keeps at most */
    int32_t match_material; /* 0 or 1 (default 1): taps of another material id are rejected */
    double normal_cos;      /* (0, 1] (default 0.9): smallest cosine between the two normals */
    double sigma_depth;     /* > 0 (default 0.02): relative depth difference a tap may have */
    double min_weight;      /* (0, 1] (default 2^-6): smallest sum of accepted bilinear weights */
} frt_reproject_params;

typedef struct frt_reproject_stats {
    uint64_t pixels;
    uint64_t reprojected; /* outcome 0 */
    uint64_t missed;      /* outcome 1 */
    uint64_t no_history;  /* outcome 2 */
    int32_t device;       /* the HIP device, -1 for host accumulators */
    int32_t reserved;     /* 0 */
    double kernel_ms;     /* k_accum_reproject (HIP events; 0 on the host) */
    double host_ms;       /* the host pass (0 on the device) */
} frt_reproject_stats;

/* what frt_reproject_setup derives from the two cameras */
typedef struct frt_reproject_geometry {
    double o_cur[3], o_prev[3];
    double prev_fwd[16];
} frt_reproject_geometry;

/*
 * The device pass. src and dst are on one device; the four feature buffers are all in host memory (on_device 0: they
 * are uploaded into scratch the destination keeps) or all in device memory on that device. geometry is
 * frt_reproject_setup's (libfrt_host, host/frt_reproject.h). stats may be NULL. Refusals (-1, the reason in
 * frt_accum_error, every output untouched): a null pointer; dst == src; cameras whose sizes differ from w x h, or
 * w * h != npixels of either accumulator; more than 262140 rows (a block is 4 rows, the launch grid 65535 blocks
 * high); accumulators on different devices; a parameter out of range or not finite (the ranges are checked here as
 * in libfrt_host's frt_reproject_params_reason, for callers that come without frt_accum_reproject).
 */
int frt_accum_dev_reproject(frt_accum_dev *dst, const frt_accum_dev *src, const frt_camera *prev_cam,
                            const frt_camera *cur_cam, const frt_reproject_geometry *geometry,
                            const frt_feature_buffers *prev_features, const frt_feature_buffers *cur_features,
                            int64_t w, int64_t h, const frt_reproject_params *params, int on_device,
                            frt_reproject_stats *stats);

/* frt_reproject_defaults, frt_reproject_params_size, frt_reproject_stats_size, frt_reproject_setup,
 * frt_reproject_host and frt_accum_reproject are libfrt_host's: host/frt_reproject.h. */

#ifdef __cplusplus
}
#endif

#endif
