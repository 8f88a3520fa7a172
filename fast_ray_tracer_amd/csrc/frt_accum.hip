// frt-mi355x: the accumulator on the device (include/frt_device.h "Accumulator", DESIGN.md "Accumulation and the
// variance-guided denoise").
//
// host/frt_accum.c is the definition: Welford's running mean and sum of squared deviations per pixel, built from
// + - * / and comparisons only. This file repeats it step for step (ac_add, ac_resolve as there) and is compiled with
// -ffp-contract=off like the host, so every value is the host's bit for bit.
//   k_accum_add      one pixel per lane: one 32-byte sample into the pixel's state
//   k_accum_resolve  one pixel per lane: the mean and the variance of the mean, as two 32-byte records
// The state is kept as columns (frt_cols.hpp): the lanes of a wave handle consecutive pixels, so each of the seven
// words they load and store is one contiguous 512-byte run. No atomics and no LDS: a wave counts the samples it
// skipped with a ballot and adds them to a word of its own, which the host sums at the resolve.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "frt_cols.hpp"
#include "frt_device.h"

namespace {

constexpr int kBlock = 256;
constexpr uint64_t kMaxFrames = (1ull << 25) - 1;  // (64 skipped samples per wave and add stay under 2^31 in an int32)

// a pixel's state but its count (a column of int32 beside these)
struct AccRec {
    double mean[4];
    double m2[3];
};

using AccCols = frt::Cols<AccRec>;

__device__ __forceinline__ bool ac_finite(const double x[4]) {
    return __builtin_isfinite(x[0]) && __builtin_isfinite(x[1]) && __builtin_isfinite(x[2]) &&
           __builtin_isfinite(x[3]);
}

// host: ac_add
__device__ __forceinline__ void ac_add(const double x[4], int n, AccRec& r) {
    const double dn = (double)n;
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
        const double d = x[ch] - r.mean[ch];
        r.mean[ch] = r.mean[ch] + d / dn;
        if (ch < 3) r.m2[ch] = r.m2[ch] + d * (x[ch] - r.mean[ch]);
    }
}

// skipped[wave] grows by the wave's skipped samples (one writer per word; launches on one stream are ordered)
__global__ __launch_bounds__(kBlock) void k_accum_add(const double* __restrict__ rgba, int npx, AccCols S,
                                                      int32_t* __restrict__ count, int32_t* __restrict__ skipped) {
    const int i = (int)(blockIdx.x * kBlock + threadIdx.x);  // (npx + 255 < 2^32, and i < npx below)
    bool skip = false;
    if ((unsigned)i < (unsigned)npx) {
        double x[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = rgba[4 * (size_t)i + k];
        skip = !ac_finite(x);
        if (!skip) {
            AccRec r = S.load(i);
            const int n = count[i] + 1;
            ac_add(x, n, r);
            S.store(i, r);
            count[i] = n;
        }
    }
    const unsigned long long m = __ballot(skip);
    if ((threadIdx.x & 63) == 0) {
        const unsigned wave = (blockIdx.x * kBlock + threadIdx.x) >> 6;
        skipped[wave] = skipped[wave] + (int32_t)__popcll(m);
    }
}

// host: ac_resolve; either output may be null
__global__ __launch_bounds__(kBlock) void k_accum_resolve(int npx, AccCols S, const int32_t* __restrict__ count,
                                                          double* __restrict__ mean_rgba, double* __restrict__ var) {
    const int i = (int)(blockIdx.x * kBlock + threadIdx.x);
    if ((unsigned)i >= (unsigned)npx) return;
    const AccRec r = S.load(i);
    const int n = count[i];
    if (mean_rgba != nullptr) {
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) mean_rgba[4 * (size_t)i + ch] = n == 0 ? 0.0 : r.mean[ch];
    }
    if (var != nullptr) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            var[4 * (size_t)i + ch] = n < 2 ? 0.0 : (r.m2[ch] / (double)(n - 1)) / (double)n;
        var[4 * (size_t)i + 3] = (double)n;
    }
}

thread_local std::string t_error;

int refuse(const std::string& what) {
    t_error = what;
    return -1;
}

int fail(const char* what, hipError_t e) {
    t_error = std::string(what) + ": " + hipGetErrorString(e);
    (void)hipGetLastError();
    return -1;
}

#define AC_HIP(call)                                  \
    do {                                              \
        const hipError_t e_ = (call);                 \
        if (e_ != hipSuccess) return fail(#call, e_); \
    } while (0)

size_t round256(size_t n) { return (n + 255) & ~(size_t)255; }

}  // namespace

struct frt_accum_dev {
    int device = 0;
    int64_t npixels = 0;
    int64_t cap = 0;        // pixels per column (npixels rounded up to 32: every column starts on 256 bytes)
    char* state = nullptr;  // 7 columns of doubles, the counts, the per-wave skipped words
    size_t state_bytes = 0;
    double* frame = nullptr;  // the scratch frame
    double* outs = nullptr;   // mean_rgba and var for a resolve into host memory
    hipEvent_t ev[4] = {};    // around the last add, around the resolve
    uint64_t frames = 0;
    bool add_timed = false;
    // the reprojection into this accumulator (frt_accum_dev_reproject): its per-wave counters, the feature buffers of
    // a call with host buffers, the events around k_accum_reproject
    int32_t* rp_words = nullptr;
    size_t rp_words_cap = 0;
    char* rp_feat = nullptr;
    hipEvent_t rp_ev[2] = {};
};

namespace {

AccCols cols_of(const frt_accum_dev* a) {
    AccCols S;
    S.w = reinterpret_cast<uint64_t*>(a->state);
    S.cap = a->cap;
    return S;
}

int32_t* count_of(const frt_accum_dev* a) { return reinterpret_cast<int32_t*>(a->state + AccCols::bytes(a->cap)); }

unsigned blocks_of(const frt_accum_dev* a) { return (unsigned)((a->npixels + kBlock - 1) / kBlock); }

int32_t* skipped_of(const frt_accum_dev* a) {
    return reinterpret_cast<int32_t*>(a->state + AccCols::bytes(a->cap) + round256((size_t)a->cap * sizeof(int32_t)));
}

int add_device_frame(frt_accum_dev* a, const double* d_rgba) {
    if (a->frames >= kMaxFrames) return refuse("frt_accum_add: more than 2^25 - 1 adds since the last reset");
    AC_HIP(hipEventRecord(a->ev[0], 0));
    hipLaunchKernelGGL(k_accum_add, dim3(blocks_of(a)), dim3(kBlock), 0, 0, d_rgba, (int)a->npixels, cols_of(a),
                       count_of(a), skipped_of(a));
    AC_HIP(hipGetLastError());
    AC_HIP(hipEventRecord(a->ev[1], 0));
    a->add_timed = true;
    a->frames += 1;
    return 0;
}

}  // namespace

extern "C" {

const char* frt_accum_error(void) { return t_error.c_str(); }

void frt_accum_set_error(const char* message) { t_error = message != nullptr ? message : ""; }

size_t frt_accum_stats_size(void) { return sizeof(frt_accum_stats); }

int frt_accum_dev_create(int device, int64_t npixels, frt_accum_dev** out) {
    if (out == nullptr) return refuse("frt_accum_create: a null pointer");
    if (npixels <= 0 || npixels > 0x7fffffffll)
        return refuse("frt_accum_create: npixels must be 1 .. 2^31 - 1 (the columns' index is 32-bit)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
        (void)hipGetLastError();
        return refuse("frt_accum_create: no such HIP device");
    }
    AC_HIP(hipSetDevice(device));
    frt_accum_dev* a = new frt_accum_dev();
    a->device = device;
    a->npixels = npixels;
    a->cap = (npixels + 31) & ~(int64_t)31;
    const size_t words = (size_t)blocks_of(a) * (kBlock / 64);
    a->state_bytes = AccCols::bytes(a->cap) + round256((size_t)a->cap * sizeof(int32_t)) + words * sizeof(int32_t);
    hipError_t e = hipMalloc((void**)&a->state, a->state_bytes);
    if (e == hipSuccess) e = hipMemset(a->state, 0, a->state_bytes);
    for (auto& ev : a->ev) {
        if (e == hipSuccess) e = hipEventCreate(&ev);
    }
    if (e != hipSuccess) {
        frt_accum_dev_release(a);
        return fail("frt_accum_create", e);
    }
    *out = a;
    return 0;
}

int frt_accum_dev_reset(frt_accum_dev* a) {
    if (a == nullptr) return refuse("frt_accum_reset: a null pointer");
    AC_HIP(hipSetDevice(a->device));
    AC_HIP(hipMemset(a->state, 0, a->state_bytes));
    a->frames = 0;
    a->add_timed = false;
    return 0;
}

int64_t frt_accum_dev_npixels(const frt_accum_dev* a) { return a != nullptr ? a->npixels : 0; }

int frt_accum_dev_device(const frt_accum_dev* a) { return a != nullptr ? a->device : -1; }

double* frt_accum_dev_frame(frt_accum_dev* a) {
    if (a == nullptr) return nullptr;
    if (a->frame == nullptr) {
        if (hipSetDevice(a->device) != hipSuccess ||
            hipMalloc((void**)&a->frame, (size_t)a->npixels * 4 * sizeof(double)) != hipSuccess) {
            (void)hipGetLastError();
            a->frame = nullptr;
            t_error = "frt_accum: the scratch frame could not be allocated";
        }
    }
    return a->frame;
}

int frt_accum_dev_add(frt_accum_dev* a, const double* rgba, int on_device) {
    if (a == nullptr || rgba == nullptr) return refuse("frt_accum_add: a null pointer");
    AC_HIP(hipSetDevice(a->device));
    if (on_device) {
        AC_HIP(hipDeviceSynchronize());  // (the frame may still be in flight on another stream)
        return add_device_frame(a, rgba);
    }
    double* frame = frt_accum_dev_frame(a);
    if (frame == nullptr) return -1;
    AC_HIP(hipMemcpy(frame, rgba, (size_t)a->npixels * 4 * sizeof(double), hipMemcpyHostToDevice));
    return add_device_frame(a, frame);
}

int frt_accum_dev_add_frame(frt_accum_dev* a) {
    if (a == nullptr || a->frame == nullptr) return refuse("frt_accum_add: no scratch frame");
    return frt_accum_dev_add(a, a->frame, 1);
}

int frt_accum_dev_resolve(frt_accum_dev* a, double* mean_rgba, double* var, int on_device, frt_accum_stats* st) {
    if (a == nullptr || (mean_rgba == nullptr && var == nullptr))
        return refuse("frt_accum_resolve: a null pointer (the accumulator and one of mean_rgba, var are needed)");
    AC_HIP(hipSetDevice(a->device));
    const size_t bytes = (size_t)a->npixels * 4 * sizeof(double);
    double *d_mean = mean_rgba, *d_var = var;
    if (!on_device) {
        if (a->outs == nullptr) AC_HIP(hipMalloc((void**)&a->outs, 2 * round256(bytes)));
        d_mean = mean_rgba != nullptr ? a->outs : nullptr;
        d_var = var != nullptr ? a->outs + round256(bytes) / sizeof(double) : nullptr;
    }
    AC_HIP(hipEventRecord(a->ev[2], 0));
    hipLaunchKernelGGL(k_accum_resolve, dim3(blocks_of(a)), dim3(kBlock), 0, 0, (int)a->npixels, cols_of(a),
                       count_of(a), d_mean, d_var);
    AC_HIP(hipGetLastError());
    AC_HIP(hipEventRecord(a->ev[3], 0));
    AC_HIP(hipEventSynchronize(a->ev[3]));
    if (!on_device) {
        if (mean_rgba != nullptr) AC_HIP(hipMemcpy(mean_rgba, d_mean, bytes, hipMemcpyDeviceToHost));
        if (var != nullptr) AC_HIP(hipMemcpy(var, d_var, bytes, hipMemcpyDeviceToHost));
    }
    if (st != nullptr) {
        std::memset(st, 0, sizeof(*st));
        st->pixels = (uint64_t)a->npixels;
        st->frames = a->frames;
        st->device = a->device;
        const size_t nwaves = (size_t)((a->npixels + 63) / 64);
        std::vector<int32_t> words(nwaves);
        AC_HIP(hipMemcpy(words.data(), skipped_of(a), nwaves * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (const int32_t n : words) st->skipped += (uint64_t)n;
        float ms = 0.0f;
        if (a->add_timed) {
            AC_HIP(hipEventElapsedTime(&ms, a->ev[0], a->ev[1]));
            st->add_ms = ms;
        }
        AC_HIP(hipEventElapsedTime(&ms, a->ev[2], a->ev[3]));
        st->resolve_ms = ms;
    }
    return 0;
}

void frt_accum_dev_release(frt_accum_dev* a) {
    if (a == nullptr) return;
    if (hipSetDevice(a->device) == hipSuccess) {
        (void)hipFree(a->state);
        (void)hipFree(a->frame);
        (void)hipFree(a->outs);
        (void)hipFree(a->rp_words);
        (void)hipFree(a->rp_feat);
        for (auto& ev : a->ev) {
            if (ev != nullptr) (void)hipEventDestroy(ev);
        }
        for (auto& ev : a->rp_ev) {
            if (ev != nullptr) (void)hipEventDestroy(ev);
        }
    }
    (void)hipGetLastError();
    delete a;
}

}  // extern "C"

// ---- reprojection (include/frt_device.h "Reprojection"; host: host/frt_reproject.c rp_pixel) ----
//   k_accum_reproject  one destination pixel per lane, blocks of 64 x 4: a wave is 64 consecutive pixels of one row.
// The current features and the eight destination columns are contiguous per wave; the four taps are gathers from the
// previous feature buffers and the source's columns. A tap is tested on ids, depth, normal and count first and its
// seven state words are loaded only where it is accepted; the sums run tap by tap. No LDS and no atomics: a wave
// counts its three outcomes by ballot into three words of its own, which the host sums.
namespace {

constexpr int kRpW = 64, kRpH = 4;

struct RpConsts {
    double c_inv[12], c_hw, c_hh, c_pix, c_cd;  // the current camera
    double p_fwd[12], p_hw, p_hh, p_pix, p_cd;  // the previous camera, prev_fwd in its inverse's place
    double oc[3], op[3];
    double cos2, sigma_depth, min_weight;
    int32_t max_history, match_material, w, h;
};

__device__ __forceinline__ void rp_xf_point(const double* m, const double* p, double* r) {
    const double x = ((m[0] * p[0] + m[1] * p[1]) + m[2] * p[2]) + m[3];
    const double y = ((m[4] * p[0] + m[5] * p[1]) + m[6] * p[2]) + m[7];
    const double z = ((m[8] * p[0] + m[9] * p[1]) + m[10] * p[2]) + m[11];
    r[0] = x;
    r[1] = y;
    r[2] = z;
}

__device__ __forceinline__ double rp_dot3(const double* a, const double* b) {
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

// host: rp_pixel; r and n arrive all zero
__device__ __forceinline__ int rp_pixel(const RpConsts& c, int px, int py, const AccCols& S,
                                        const int32_t* __restrict__ sn, const double* __restrict__ pgeom,
                                        const int32_t* __restrict__ pids, const double* __restrict__ cgeom,
                                        const int32_t* __restrict__ cids, AccRec& r, int32_t& n) {
    const int i = py * c.w + px;
    // 1
    const int2 id = *reinterpret_cast<const int2*>(cids + 2 * (size_t)i);
    const int node = id.x, mat = id.y;
    const double* cg = cgeom + 8 * (size_t)i;
    const double d = cg[0];
    const double np_[3] = {cg[1], cg[2], cg[3]};
    if (!(node >= 0 && __builtin_isfinite(d) && d > 0.0)) return 1;
    // 2
    const double xoff = ((double)px + 0.5) * c.c_pix;
    const double yoff = ((double)py + 0.5) * c.c_pix;
    const double cp[3] = {c.c_hw - xoff, c.c_hh - yoff, -c.c_cd};
    double P[3];
    rp_xf_point(c.c_inv, cp, P);
    const double vv[3] = {P[0] - c.oc[0], P[1] - c.oc[1], P[2] - c.oc[2]};
    const double inv = 1.0 / sqrt(rp_dot3(vv, vv));
    double W[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double dir = vv[k] * inv;
        const double t = d * dir;
        W[k] = c.oc[k] + t;
    }
    // 3
    double q3[3];
    rp_xf_point(c.p_fwd, W, q3);
    if (!(__builtin_isfinite(q3[2]) && q3[2] < 0.0)) return 2;
    const double s = -c.p_cd / q3[2];
    double fx = (c.p_hw - q3[0] * s) / c.p_pix - 0.5;
    double fy = (c.p_hh - q3[1] * s) / c.p_pix - 0.5;
    const double rx = __builtin_floor(fx + 0.5), ry = __builtin_floor(fy + 0.5);
    if (__builtin_fabs(fx - rx) <= 0x1p-20) fx = rx;
    if (__builtin_fabs(fy - ry) <= 0x1p-20) fy = ry;
    // (before the conversions: past this line x0 and y0 are in [-1, w - 1] and [-1, h - 1])
    if (!(fx >= -1.0 && fx < (double)c.w && fy >= -1.0 && fy < (double)c.h)) return 2;
    const double flx = __builtin_floor(fx), fly = __builtin_floor(fy);
    const int x0 = (int)flx, y0 = (int)fly;
    const double tx = fx - flx, ty = fy - fly;
    // 4
    const double u[3] = {W[0] - c.op[0], W[1] - c.op[1], W[2] - c.op[2]};
    const double e = sqrt(rp_dot3(u, u));
    const double tol = c.sigma_depth * e;
    const double nnp = rp_dot3(np_, np_);
    // 5, 6
    const double ux = 1.0 - tx, uy = 1.0 - ty;
    const double wt[4] = {ux * uy, tx * uy, ux * ty, tx * ty};
    double ws = 0.0, an = 0.0, am[4] = {0.0, 0.0, 0.0, 0.0}, av[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int qx = x0 + (t & 1), qy = y0 + (t >> 1);
        if ((unsigned)qx >= (unsigned)c.w || (unsigned)qy >= (unsigned)c.h) continue;  // (the gathers stay inside)
        const int q = qy * c.w + qx;
        const int nq = sn[q];
        if (!(nq > 0)) continue;
        const int2 qid = *reinterpret_cast<const int2*>(pids + 2 * (size_t)q);
        if (qid.x != node || (c.match_material && qid.y != mat)) continue;
        const double* qg = pgeom + 8 * (size_t)q;
        const double zq = qg[0];
        if (!(__builtin_isfinite(zq) && zq > 0.0)) continue;
        if (!(__builtin_fabs(zq - e) <= tol)) continue;
        const double nq3[3] = {qg[1], qg[2], qg[3]};
        const double dn = rp_dot3(np_, nq3);
        const double nnq = rp_dot3(nq3, nq3);
        if (!(dn > 0.0 && dn * dn >= c.cos2 * (nnp * nnq))) continue;
        const AccRec sq = S.load(q);
        const double w = wt[t], dq = (double)nq;
        ws = ws + w;
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) am[ch] = am[ch] + w * sq.mean[ch];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) av[ch] = av[ch] + w * (sq.m2[ch] / dq);
        an = an + w * dq;
    }
    if (!(ws >= c.min_weight)) return 2;
    // 7
    const double rr = an / ws + 0.5;
    int nn = rr >= (double)c.max_history ? c.max_history : (int)rr;
    if (nn < 1) nn = 1;
    n = nn;
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) r.mean[ch] = am[ch] / ws;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) r.m2[ch] = (av[ch] / ws) * (double)nn;
    return 0;
}

// words: three per wave (reprojected, missed, no history), wave = row * gridDim.x + column block
__global__ __launch_bounds__(kRpW* kRpH) void k_accum_reproject(RpConsts c, AccCols S, const int32_t* __restrict__ sn,
                                                               AccCols D, int32_t* __restrict__ dn,
                                                               const double* __restrict__ pgeom,
                                                               const int32_t* __restrict__ pids,
                                                               const double* __restrict__ cgeom,
                                                               const int32_t* __restrict__ cids,
                                                               int32_t* __restrict__ words) {
    const int py = __builtin_amdgcn_readfirstlane((int)(blockIdx.y * kRpH + threadIdx.y));  // (a wave is one row)
    if (py >= c.h) return;  // (the whole wave)
    const int px = (int)(blockIdx.x * kRpW + threadIdx.x);
    int outcome = -1;
    if (px < c.w) {
        AccRec r = {};
        int32_t n = 0;
        outcome = rp_pixel(c, px, py, S, sn, pgeom, pids, cgeom, cids, r, n);
        const int i = py * c.w + px;
        D.store(i, r);
        dn[i] = n;
    }
    const unsigned long long m0 = __ballot(outcome == 0), m1 = __ballot(outcome == 1), m2 = __ballot(outcome == 2);
    if (threadIdx.x == 0) {
        const size_t wave = (size_t)py * gridDim.x + blockIdx.x;
        words[3 * wave + 0] = (int32_t)__popcll(m0);
        words[3 * wave + 1] = (int32_t)__popcll(m1);
        words[3 * wave + 2] = (int32_t)__popcll(m2);
    }
}

// (frt_reproject_params_reason of libfrt_host, which this library cannot call: frt_accum_dev_reproject is public, and a
// caller that comes here without frt_accum_reproject gets the same refusals)
const char* rp_params_reason(const frt_reproject_params* p) {
    if (p->max_history < 1 || p->max_history > (1 << 20)) return "frt_reproject: max_history must be 1 .. 2^20";
    if (p->match_material != 0 && p->match_material != 1) return "frt_reproject: match_material must be 0 or 1";
    if (!(std::isfinite(p->normal_cos) && p->normal_cos > 0.0 && p->normal_cos <= 1.0))
        return "frt_reproject: normal_cos must be in (0, 1]";
    if (!(std::isfinite(p->sigma_depth) && p->sigma_depth > 0.0))
        return "frt_reproject: sigma_depth must be finite and > 0";
    if (!(std::isfinite(p->min_weight) && p->min_weight > 0.0 && p->min_weight <= 1.0))
        return "frt_reproject: min_weight must be in (0, 1]";
    return nullptr;
}

}  // namespace

extern "C" {

int frt_accum_dev_reproject(frt_accum_dev* dst, const frt_accum_dev* src, const frt_camera* prev,
                            const frt_camera* cur, const frt_reproject_geometry* g, const frt_feature_buffers* pf,
                            const frt_feature_buffers* cf, int64_t w, int64_t h, const frt_reproject_params* p,
                            int on_device, frt_reproject_stats* st) {
    if (dst == nullptr || src == nullptr || prev == nullptr || cur == nullptr || g == nullptr || pf == nullptr ||
        cf == nullptr || p == nullptr || pf->geom == nullptr || pf->ids == nullptr || cf->geom == nullptr ||
        cf->ids == nullptr)
        return refuse("frt_accum_reproject: a null pointer (both buffers of both views are needed)");
    if (dst == src) return refuse("frt_accum_reproject: the destination is the source");
    if (dst->device != src->device) return refuse("frt_accum_reproject: the accumulators are on different devices");
    if (w <= 0 || h <= 0 || w > 0x7fffffffll || h > 0x7fffffffll || w * h != dst->npixels || w * h != src->npixels)
        return refuse("frt_accum_reproject: w * h is not the accumulators' npixels");
    if (h > (int64_t)kRpH * 65535)
        return refuse("frt_accum_reproject: more than 262140 rows (the launch grid's y extent)");
    if (prev->hsize != w || prev->vsize != h || cur->hsize != w || cur->vsize != h)
        return refuse("frt_reproject: the two cameras must both be w x h");
    if (const char* why = rp_params_reason(p)) return refuse(why);
    for (int k = 0; k < 16; ++k) {
        if (!std::isfinite(g->prev_fwd[k]) || !std::isfinite(cur->inv[k]))
            return refuse("frt_accum_reproject: a camera's matrix is not finite");
    }

    AC_HIP(hipSetDevice(dst->device));
    const size_t npx = (size_t)dst->npixels;
    const size_t geom_bytes = round256(npx * 8 * sizeof(double)), ids_bytes = round256(npx * 2 * sizeof(int32_t));
    const double *d_pgeom = pf->geom, *d_cgeom = cf->geom;
    const int32_t *d_pids = pf->ids, *d_cids = cf->ids;
    if (on_device) {
        AC_HIP(hipDeviceSynchronize());  // (the buffers may still be in flight on another stream)
    } else {
        if (dst->rp_feat == nullptr) AC_HIP(hipMalloc((void**)&dst->rp_feat, 2 * (geom_bytes + ids_bytes)));
        char* base = dst->rp_feat;
        AC_HIP(hipMemcpy(base, pf->geom, npx * 8 * sizeof(double), hipMemcpyHostToDevice));
        AC_HIP(hipMemcpy(base + geom_bytes, cf->geom, npx * 8 * sizeof(double), hipMemcpyHostToDevice));
        AC_HIP(hipMemcpy(base + 2 * geom_bytes, pf->ids, npx * 2 * sizeof(int32_t), hipMemcpyHostToDevice));
        AC_HIP(hipMemcpy(base + 2 * geom_bytes + ids_bytes, cf->ids, npx * 2 * sizeof(int32_t),
                         hipMemcpyHostToDevice));
        d_pgeom = reinterpret_cast<const double*>(base);
        d_cgeom = reinterpret_cast<const double*>(base + geom_bytes);
        d_pids = reinterpret_cast<const int32_t*>(base + 2 * geom_bytes);
        d_cids = reinterpret_cast<const int32_t*>(base + 2 * geom_bytes + ids_bytes);
    }
    const dim3 grid((unsigned)((w + kRpW - 1) / kRpW), (unsigned)((h + kRpH - 1) / kRpH));
    const size_t nwords = 3 * (size_t)grid.x * (size_t)h;
    if (dst->rp_words_cap < nwords) {
        (void)hipFree(dst->rp_words);
        dst->rp_words = nullptr;
        dst->rp_words_cap = 0;
        AC_HIP(hipMalloc((void**)&dst->rp_words, nwords * sizeof(int32_t)));
        dst->rp_words_cap = nwords;
    }
    for (auto& ev : dst->rp_ev) {
        if (ev == nullptr) AC_HIP(hipEventCreate(&ev));
    }

    RpConsts c;
    for (int k = 0; k < 12; ++k) {
        c.c_inv[k] = cur->inv[k];
        c.p_fwd[k] = g->prev_fwd[k];
    }
    c.c_hw = cur->half_width, c.c_hh = cur->half_height, c.c_pix = cur->pixel_size, c.c_cd = cur->canvas_distance;
    c.p_hw = prev->half_width, c.p_hh = prev->half_height, c.p_pix = prev->pixel_size, c.p_cd = prev->canvas_distance;
    for (int k = 0; k < 3; ++k) {
        c.oc[k] = g->o_cur[k];
        c.op[k] = g->o_prev[k];
    }
    c.cos2 = p->normal_cos * p->normal_cos;
    c.sigma_depth = p->sigma_depth;
    c.min_weight = p->min_weight;
    c.max_history = p->max_history;
    c.match_material = p->match_material;
    c.w = (int32_t)w;
    c.h = (int32_t)h;

    // the reset: the kernel writes every pixel's eight words; the skipped words start over
    AC_HIP(hipMemsetAsync(skipped_of(dst), 0, (size_t)blocks_of(dst) * (kBlock / 64) * sizeof(int32_t), 0));
    AC_HIP(hipEventRecord(dst->rp_ev[0], 0));
    hipLaunchKernelGGL(k_accum_reproject, grid, dim3(kRpW, kRpH), 0, 0, c, cols_of(src), count_of(src), cols_of(dst),
                       count_of(dst), d_pgeom, d_pids, d_cgeom, d_cids, dst->rp_words);
    AC_HIP(hipGetLastError());
    AC_HIP(hipEventRecord(dst->rp_ev[1], 0));
    AC_HIP(hipEventSynchronize(dst->rp_ev[1]));
    dst->frames = src->frames < (uint64_t)p->max_history ? src->frames : (uint64_t)p->max_history;
    dst->add_timed = false;
    if (st != nullptr) {
        std::vector<int32_t> words(nwords);
        AC_HIP(hipMemcpy(words.data(), dst->rp_words, nwords * sizeof(int32_t), hipMemcpyDeviceToHost));
        std::memset(st, 0, sizeof(*st));
        st->pixels = (uint64_t)npx;
        for (size_t k = 0; k < nwords; k += 3) {
            st->reprojected += (uint64_t)words[k];
            st->missed += (uint64_t)words[k + 1];
            st->no_history += (uint64_t)words[k + 2];
        }
        st->device = dst->device;
        float ms = 0.0f;
        AC_HIP(hipEventElapsedTime(&ms, dst->rp_ev[0], dst->rp_ev[1]));
        st->kernel_ms = ms;
    }
    return 0;
}

}  // extern "C"
