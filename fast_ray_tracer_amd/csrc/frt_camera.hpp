// frt-mi355x camera rays and the ray / hit records of the level queues, shared by the engine
// (frt_engine.hip: k_trace, k_prepare) and the scene-specialised closest-hit kernel (frt_jit.hip
// frt_jit_trace), which generates its level-0 rays in place as k_trace does.
#pragma once

#include "frt_cam_index.hpp"
#include "frt_shadow.hpp"

namespace frt {

// one queued ray of a level (segmented queues: frt_shadow.hpp queue_slot)
struct QueuedRay {
    double o[3];
    double d[3];
    uint64_t key;
    int32_t parent;
    int32_t slot;
};

// a ray's closest hit (k_trace -> k_prepare)
// (the refractive indices either side of a hit, from the containers, go to an array of their own (n12, two per
// ray), written only where a scene has indices other than one: most scenes write and read 16 bytes per hit)
struct HitRec {
    double t;
    int32_t node;  // -1: miss
    int32_t pad;
};

// ---- stochastic camera sampling (counter-based RNG; the reference draws drand48) ----
// Uniform double in [0, 1) for draw d of stream (seed, key): 53 bits of a splitmix64 hash.
__device__ __forceinline__ double rng_uniform(uint64_t seed, uint64_t key, uint64_t d) {
    const uint64_t h = mix64(seed ^ mix64(key * 0x9e3779b97f4a7c15ULL + d * 0xd1b54a32d192ed03ULL + 0x632be59bd9b4e019ULL));
    return (double)(h >> 11) * 0x1.0p-53;
}

// Jittered correlated multi-jittered sub-pixel point (u, v) of one pixel: the
// reference's sampler_reset_2d (sampler.c:411-470: canonical pattern with a
// drand48 jitter per cell, then the x rows and y columns shuffled with
// drand48) evaluated for one cell by tracing the two shuffles backwards.
// Draw numbering: canonical cell (j, i) -> x: 2(jV+i), y: 2(jV+i)+1;
// x-row shuffle step j -> 2UV + j; y-column shuffle step i -> 2UV + V + i.
__device__ inline void cmj_point(uint64_t seed, uint64_t pixel, int U, int V, int u, int v, double* out) {
    const uint64_t base = 2ull * (uint64_t)U * (uint64_t)V;
    // x: rows j < V of length U are permuted (sampler.c:442-450, n = steps[1] = V, m = steps[0] = U)
    int p = v;
    for (int j = V - 1; j >= 0; --j) {
        const int k = (int)(j + rng_uniform(seed, pixel, base + j) * (double)(V - j));
        if (p == j) p = k;
        else if (p == k) p = j;
    }
    {
        const int f = p * U + u;           // flat index of the source cell
        const int jj = f / V, ii = f % V;  // canonical layout idx = j * V + i (sampler.c:419-427)
        const double r = rng_uniform(seed, pixel, 2ull * (uint64_t)f);
        out[0] = (ii + (jj + r) / (double)U) / (double)V;
    }
    // y: columns i < U are permuted (sampler.c:452-460)
    p = u;
    for (int i = U - 1; i >= 0; --i) {
        const int k = (int)(i + rng_uniform(seed, pixel, base + (uint64_t)V + i) * (double)(U - i));
        if (p == i) p = k;
        else if (p == k) p = i;
    }
    {
        const int f = v * U + p;
        const int jj = f / V, ii = f % V;
        const double r = rng_uniform(seed, pixel, 2ull * (uint64_t)f + 1);
        out[1] = (jj + (ii + r) / (double)V) / (double)U;
    }
}

// aperture_fn (camera.c:11-82): rejection sampling on [0,1)^2; point-like types give the centre
__device__ inline void aperture_point(const frt_camera& cam, uint64_t seed, uint64_t sample, double* xy,
                                      unsigned& err) {
    const double* a = cam.aperture_args;
    const int type = cam.aperture_type;
    if (type == 6 || type == 4 || type == 5 || type == 8 || type < 0 || type > 8) {  // point / not-implemented types
        xy[0] = 0.5;
        xy[1] = 0.5;
        return;
    }
    for (int attempt = 0; attempt < 4096; ++attempt) {
        const double x = rng_uniform(seed ^ 0xa5e7u, sample, 2ull * attempt);
        const double y = rng_uniform(seed ^ 0xa5e7u, sample, 2ull * attempt + 1);
        const double u = 2 * x - 1, v = 2 * y - 1;
        bool ok;
        switch (type) {
        case 0: ok = !(u * u + v * v > a[0]); break;                                    // circle r1
        case 1: ok = ((u > a[0]) && (u <= a[1])) || ((v > a[2]) && (v <= a[3])); break;  // cross x1 x2 y1 y2
        case 2:                                                                           // diamond b1..b4
            ok = (u <= 0) ? (-u + a[0] <= v) && (v < u + a[1]) : (0 <= x) ? (u + a[2] <= v) && (v < -u + a[3]) : false;
            break;
        case 3: {  // doughnut r1 r2
            const double mag = u * u + v * v;
            ok = !(mag > a[0] || mag < a[1]);
            break;
        }
        default: ok = true; break;  // square
        }
        if (ok) {
            xy[0] = x;
            xy[1] = y;
            return;
        }
    }
    err |= kErrAperture;  // the reference would loop forever
    xy[0] = 0.5;
    xy[1] = 0.5;
}

// origin0: the origin of a camera without an aperture, computed once per camera (DevScene::cam_origin: this
// function's own expression at ap = (0.5, 0.5)); null: computed here
__device__ __forceinline__ void ray_for_pixel(const frt_camera& cam, double px, double py, const double* jit,
                                              const double* ap, const double* origin0, Ray& r) {
    // renderer.c:95-129; ap = aperture_fn's point in [0,1)^2 (sample_aperture subtracts 0.5, camera.c:85-90)
    double xoff = (px + jit[0]) * cam.pixel_size;
    double yoff = (py + jit[1]) * cam.pixel_size;
    double wx = cam.half_width - xoff, wy = cam.half_height - yoff;
    double p[3] = {wx, wy, -cam.canvas_distance}, pixel[3], origin[3];
    xf_point(cam.inv, p, pixel);
    if (origin0 != nullptr) {
        origin[0] = origin0[0];
        origin[1] = origin0[1];
        origin[2] = origin0[2];
    } else {
        double q[3] = {(ap[0] - 0.5) * cam.aperture_size, (ap[1] - 0.5) * cam.aperture_size, 0.0};
        xf_point(cam.inv, q, origin);
    }
    double v[3] = {pixel[0] - origin[0], pixel[1] - origin[1], pixel[2] - origin[2]};
    r.o[0] = origin[0];
    r.o[1] = origin[1];
    r.o[2] = origin[2];
    normalize3(v, r.d);
}

// global sample index of sample s of a batch's level 0: the pixel's index in the whole frame (the batch's rows may be
// a strided part of it) times spp plus the sub-pixel sample (sub = v * usteps + u). The one place the expression
// lives: camera_ray and camera_key (the level-0 keys that HeadCols does not store) both take it from here.
// B.cam_fast (the host's cam_index_fits32): s and the pixel index are 32-bit values, the two quotients multiply-shift
// (frt_cam_index.hpp), the remainders a multiply-subtract, column and row doubles from 32-bit integers; the products
// of global_pixel and global_sample stay 64-bit. Otherwise two signed 64-bit divisions. The same integers, and the
// same doubles, either way.
struct CameraSample {
    int64_t row, col;
    uint64_t global_pixel, global_sample;
    int sub;
    double px, py;  // col, row
};
__device__ __forceinline__ CameraSample camera_sample(const DevScene& S, const Batch& B, int64_t s) {
    CameraSample c;
    if (B.cam_fast) {
        const uint32_t s32 = (uint32_t)s, spp = (uint32_t)B.spp, hs = (uint32_t)S.cam.hsize;
        const uint32_t sp = magic_div(s32, B.spp_magic, B.spp_shift);
        const uint32_t sub = magic_rem(s32, sp, spp);
        const uint32_t pix = (uint32_t)B.pixel_begin + sp;
        const uint32_t prow = magic_div(pix, B.hs_magic, B.hs_shift);
        const uint32_t col = magic_rem(pix, prow, hs);
        const uint32_t row = (uint32_t)B.row_begin + prow * (uint32_t)B.row_stride;
        c.sub = (int)sub;
        c.row = (int64_t)row;
        c.col = (int64_t)col;
        c.global_pixel = (uint64_t)row * (uint64_t)hs + (uint64_t)col;
        c.global_sample = c.global_pixel * (uint64_t)spp + (uint64_t)sub;
        c.px = (double)col;
        c.py = (double)row;
        return c;
    }
    const int64_t pix = B.pixel_begin + s / B.spp;
    c.sub = (int)(s % B.spp);
    const int64_t hs = S.cam.hsize;
    c.row = B.row_begin + (pix / hs) * B.row_stride;
    c.col = pix % hs;
    c.global_pixel = (uint64_t)(c.row * hs + c.col);
    c.global_sample = c.global_pixel * (uint64_t)B.spp + (uint64_t)c.sub;
    c.px = (double)c.col;
    c.py = (double)c.row;
    return c;
}

// a level-0 path node's key: (global sample << 12) | heap code 1 (the root of the sample's path tree)
__device__ __forceinline__ uint64_t camera_key(const DevScene& S, const Batch& B, int64_t s) {
    return (camera_sample(S, B, s).global_sample << 12) | 1ull;
}

// camera ray of sample s of a batch (k_trace level 0 and k_prepare level 0)
__device__ __forceinline__ void camera_ray(const DevScene& S, const Batch& B, int64_t s, Ray& r, uint64_t& key,
                                           unsigned& err) {
    const CameraSample c = camera_sample(S, B, s);
    const int sub = c.sub;
    double jit[2], ap[2] = {0.5, 0.5};
    if (S.cam.jitter) {
        const int U = (int)S.cam.usteps, V = (int)S.cam.vsteps;
        cmj_point(B.seed, c.global_pixel, U, V, sub % U, sub / U, jit);
    } else {
        jit[0] = S.sample_table[2 * sub];
        jit[1] = S.sample_table[2 * sub + 1];
    }
    if (S.cam.aperture_size != 0.0) aperture_point(S.cam, B.seed, c.global_sample, ap, err);
    // (cam_origin_set only where aperture_size == 0: ap is then the centre the stored origin was computed at)
    ray_for_pixel(S.cam, c.px, c.py, jit, ap, S.cam_origin_set ? S.cam_origin : nullptr, r);
    key = (c.global_sample << 12) | 1ull;
}

}  // namespace frt
