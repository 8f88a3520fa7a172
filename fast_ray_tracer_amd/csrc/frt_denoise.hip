// frt-mi355x: the denoise on the device (include/frt_device.h "Denoise", DESIGN.md "Denoise").
//
// host/frt_denoise.c is the definition: an edge-avoiding a-trous filter guided by the first-hit feature buffers, built
// from + - * / and comparisons only. This file repeats it step for step (dn_valid, dn_albedo and the pack as there;
// dn_tap is dn_weight with its accumulation, dn_finish the division and dn_unpack) and is compiled with
// -ffp-contract=off like the host, so every value is the host's bit for bit.
//   k_denoise_pack       one pixel per lane: validity, the guides and the demodulated colour, written as columns
//   k_denoise_atrous<>   one launch per iteration, ping-ponging the colour columns; the last one writes the image
// No atomics and no LDS: a pixel's 25 taps are gathered straight from the columns. A wave is 64 consecutive pixels of
// one row, so a tap's load of a column is one contiguous 512-byte run at any step (dx * s is wave-uniform), and a tap
// row outside the image is skipped under scalar control. (Staging the tile and its halo through LDS for the steps 1
// and 2 was measured and not kept: DESIGN.md "Denoise", profiles/denoise_lds_experiment.json.)
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "frt_device.h"

namespace {

constexpr int kInvalid = INT32_MIN;  // the material column's value of an invalid pixel (host: DN_INVALID)
constexpr int kPackBlock = 256;
constexpr int kTileW = 64, kTileH = 4;  // k_denoise_atrous: a wave per row of the tile
constexpr int kMaxIter = FRT_DENOISE_MAX_ITERATIONS;

// the columns of all images (index: image * h * w + y * w + x, 32-bit), carved out of one allocation
struct DnCols {
    double *n0, *n1, *n2, *inv_nn, *iz, *z;
    int32_t* mat;
    double* x[2][3];  // ping-pong
};  // 100 bytes per pixel

struct DnConsts {
    double kz, kc, eps;
    int squarings, demodulate, match_material;
};

__device__ __forceinline__ bool dn_valid(const double* rgba, const double* geom, const int32_t* ids) {
    return ids[0] >= 0 && ids[1] != kInvalid && __builtin_isfinite(geom[0]) && geom[0] > 0 &&
           __builtin_isfinite(rgba[0]) && __builtin_isfinite(rgba[1]) && __builtin_isfinite(rgba[2]);
}

__device__ __forceinline__ double dn_albedo(const double* geom, int ch, const DnConsts& c) {
    return c.demodulate ? geom[4 + ch] + c.eps : 1.0;
}

// counts[wave]: the wave's valid pixels (summed on the host: no atomics)
__global__ __launch_bounds__(kPackBlock) void k_denoise_pack(const double* __restrict__ rgba,
                                                             const double* __restrict__ geom,
                                                             const int32_t* __restrict__ ids, int npx, DnConsts c,
                                                             DnCols P, int32_t* __restrict__ counts) {
    const int i = (int)(blockIdx.x * kPackBlock + threadIdx.x);  // (npx + 255 < 2^32, and i < npx below)
    bool valid = false;
    if ((unsigned)i < (unsigned)npx) {
        double px[4], g[8];
        int32_t id[2];
#pragma unroll
        for (int k = 0; k < 4; ++k) px[k] = rgba[4 * (size_t)i + k];
#pragma unroll
        for (int k = 0; k < 8; ++k) g[k] = geom[8 * (size_t)i + k];
        id[0] = ids[2 * (size_t)i];
        id[1] = ids[2 * (size_t)i + 1];
        valid = dn_valid(px, g, id);
        if (valid) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) P.x[0][ch][i] = px[ch] / dn_albedo(g, ch, c);
            const double n0 = g[1], n1 = g[2], n2 = g[3];
            const double nn = (n0 * n0 + n1 * n1) + n2 * n2;
            P.n0[i] = n0;
            P.n1[i] = n1;
            P.n2[i] = n2;
            P.inv_nn[i] = nn > 0 ? 1.0 / nn : 0.0;
            P.z[i] = g[0];
            P.iz[i] = 1.0 / g[0];
            P.mat[i] = id[1];
        } else {
            P.mat[i] = kInvalid;
        }
    }
    const unsigned long long m = __ballot(valid);
    if ((threadIdx.x & 63) == 0) counts[(blockIdx.x * kPackBlock + threadIdx.x) >> 6] = (int32_t)__popcll(m);
}

// host: K[|d|]
__device__ __forceinline__ constexpr double dn_k(int d) {
    return d == 0 ? 3.0 / 8.0 : (d == 1 || d == -1) ? 1.0 / 4.0 : 1.0 / 16.0;
}

// a pixel's guides and colour, in registers
struct DnPix {
    double n0, n1, n2, inv_nn, iz, z;
    double x[3];
    int mat;
};

// host: dn_weight and the accumulation of dn_atrous_pixel for one tap q != p; `usable`: q is inside p's image and
// valid (an unusable q's words are whatever was loaded, and are dropped)
__device__ __forceinline__ void dn_tap(const DnPix& p, const DnPix& q, bool usable, double hk, const DnConsts& c,
                                       double acc[3], double& ws) {
    const double d = (p.n0 * q.n0 + p.n1 * q.n1) + p.n2 * q.n2;
    const double m = (d * d) * (p.inv_nn * q.inv_nn);
    double t = m < 1.0 ? m : 1.0;
    for (int k = 0; k < c.squarings; ++k) t = t * t;
    const double r = p.z - q.z;
    const double xz = ((r * r) * c.kz) * (p.iz * q.iz);
    const double dc0 = p.x[0] - q.x[0], dc1 = p.x[1] - q.x[1], dc2 = p.x[2] - q.x[2];
    const double xc = ((dc0 * dc0 + dc1 * dc1) + dc2 * dc2) * c.kc;
    const double u = (1.0 + xz) * (1.0 + xc);
    const double wgt = (hk * t) / (u * u);
    const bool skip = !usable || (c.match_material && q.mat != p.mat) || d <= 0 || wgt < 0;
    if (!skip) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) acc[ch] += wgt * q.x[ch];
        ws += wgt;
    }
}

// the centre tap: wgt = hk
__device__ __forceinline__ void dn_centre(const DnPix& p, double hk, double acc[3], double& ws) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) acc[ch] += hk * p.x[ch];
    ws += hk;
}

__device__ __forceinline__ DnPix dn_load(const DnCols& P, int cur, int i) {
    DnPix v;
    v.mat = P.mat[i];
    v.n0 = P.n0[i];
    v.n1 = P.n1[i];
    v.n2 = P.n2[i];
    v.inv_nn = P.inv_nn[i];
    v.iz = P.iz[i];
    v.z = P.z[i];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) v.x[ch] = P.x[cur][ch][i];
    return v;
}

// x_{i+1} = acc / ws into x[cur ^ 1], or (kLast) rgb = x_{i+1} * a and the alpha into out
template <bool kLast>
__device__ __forceinline__ void dn_finish(const DnCols& P, int cur, int p, const double acc[3], double ws,
                                          const DnConsts& c, const double* rgba, const double* __restrict__ geom,
                                          double* out) {
    double y[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) y[ch] = acc[ch] / ws;
    if (kLast) {
        const double alpha = rgba[4 * (size_t)p + 3];
        double g[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (c.demodulate) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) g[4 + ch] = geom[8 * (size_t)p + 4 + ch];
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) out[4 * (size_t)p + ch] = y[ch] * dn_albedo(g, ch, c);
        out[4 * (size_t)p + 3] = alpha;
    } else {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) P.x[cur ^ 1][ch][p] = y[ch];
    }
}

// an invalid pixel's output is its input (out may be rgba: a lane reads and writes its own pixel only)
__device__ __forceinline__ void dn_copy(int p, const double* rgba, double* out) {
#pragma unroll
    for (int k = 0; k < 4; ++k) out[4 * (size_t)p + k] = rgba[4 * (size_t)p + k];
}

// One iteration, step s, from x[cur] to x[cur ^ 1]; kLast writes the image instead.
// blockIdx.x = (image * rowblocks + rowblock) * colblocks + colblock.
template <bool kLast>
__global__ __launch_bounds__(kTileW* kTileH) void k_denoise_atrous(DnCols P, int cur, int w, int h, int colblocks,
                                                                   int rowblocks, int s, DnConsts c,
                                                                   const double* rgba, const double* __restrict__ geom,
                                                                   double* out) {
    const int b = (int)blockIdx.x;
    const int cb = b % colblocks, rest = b / colblocks;
    const int rb = rest % rowblocks, img = rest / rowblocks;
    const int py = __builtin_amdgcn_readfirstlane(rb * kTileH + (int)threadIdx.y);  // (a wave is one row)
    const int px = cb * kTileW + (int)threadIdx.x;
    if (py >= h) return;  // (the whole wave)
    if (px >= w) return;
    const int row0 = img * (h * w);  // (< 2^31: the entry point refuses more pixels)
    const int p = row0 + py * w + px;
    if (P.mat[p] == kInvalid) {
        if (kLast) dn_copy(p, rgba, out);
        return;
    }
    const DnPix vp = dn_load(P, cur, p);
    double acc[3] = {0.0, 0.0, 0.0}, ws = 0.0;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = py + s * dy;
        if ((unsigned)qy >= (unsigned)h) continue;  // (scalar: py and s are wave-uniform)
        const int qrow = row0 + qy * w;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const double hk = dn_k(dx) * dn_k(dy);
            if (dx == 0 && dy == 0) {
                dn_centre(vp, hk, acc, ws);
                continue;
            }
            const int qx = px + s * dx;
            const bool inside = (unsigned)qx < (unsigned)w;
            // a lane whose tap is outside loads its own column instead and drops the tap: the loads stay
            // unconditional (an invalid pixel's guide words are never written, only read and dropped)
            const DnPix vq = dn_load(P, cur, qrow + (inside ? qx : px));
            dn_tap(vp, vq, inside && vq.mat != kInvalid, hk, c, acc, ws);
        }
    }
    dn_finish<kLast>(P, cur, p, acc, ws, c, rgba, geom, out);
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

#define DN_HIP(call)                                  \
    do {                                              \
        const hipError_t e_ = (call);                 \
        if (e_ != hipSuccess) return fail(#call, e_); \
    } while (0)

// a device's buffers, kept between calls (grow only); used under g_mu
struct Scratch {
    char* cols = nullptr;  // the columns, then the pack's per-wave counts
    size_t cols_bytes = 0;
    char* in = nullptr;  // host buffers' copies: rgba (filtered in place), geom, ids
    size_t in_bytes = 0;
    hipEvent_t ev[kMaxIter + 2] = {};
    bool used = false;
};

std::mutex g_mu;
Scratch g_scratch[64];

int ensure(char** p, size_t& have, size_t need) {
    if (need <= have) return 0;
    if (*p != nullptr) DN_HIP(hipFree(*p));
    *p = nullptr;
    have = 0;
    DN_HIP(hipMalloc((void**)p, need));
    have = need;
    return 0;
}

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

size_t round256(size_t n) { return (n + 255) & ~(size_t)255; }

// one a-trous launch on the null stream
int launch_atrous(bool last, unsigned blocks, const DnCols& P, int cur, int w, int h, int colblocks, int rowblocks, int s,
                  const DnConsts& c, const double* rgba, const double* geom, double* out) {
    const dim3 block(kTileW, kTileH);
    if (last) {
        hipLaunchKernelGGL(k_denoise_atrous<true>, dim3(blocks), block, 0, 0, P, cur, w, h, colblocks, rowblocks, s, c,
                           rgba, geom, out);
    } else {
        hipLaunchKernelGGL(k_denoise_atrous<false>, dim3(blocks), block, 0, 0, P, cur, w, h, colblocks, rowblocks, s, c,
                           rgba, geom, out);
    }
    DN_HIP(hipGetLastError());
    return 0;
}

int denoise_locked(Scratch& S, const double* rgba, const double* geom, const int32_t* ids, int on_device, int w, int h,
                   int nimages, const frt_denoise_params& prm, int device, double* out, frt_denoise_stats* st) {
    const size_t npx = (size_t)w * h * nimages;
    const size_t plane = round256(npx * sizeof(double));
    const unsigned nwaves = (unsigned)((npx + 63) / 64), pack_blocks = (unsigned)((npx + kPackBlock - 1) / kPackBlock);
    const size_t count_words = (size_t)pack_blocks * (kPackBlock / 64);
    DN_HIP(hipSetDevice(device));
    S.used = true;
    for (auto& e : S.ev) {
        if (e == nullptr) DN_HIP(hipEventCreate(&e));
    }
    if (ensure(&S.cols, S.cols_bytes, 12 * plane + round256(npx * sizeof(int32_t)) + count_words * sizeof(int32_t)))
        return -1;
    DnCols P;
    double* base = reinterpret_cast<double*>(S.cols);
    const size_t pw = plane / sizeof(double);
    P.n0 = base;
    P.n1 = base + pw;
    P.n2 = base + 2 * pw;
    P.inv_nn = base + 3 * pw;
    P.iz = base + 4 * pw;
    P.z = base + 5 * pw;
    for (int k = 0; k < 6; ++k) P.x[k / 3][k % 3] = base + (size_t)(6 + k) * pw;
    P.mat = reinterpret_cast<int32_t*>(S.cols + 12 * plane);
    int32_t* counts = reinterpret_cast<int32_t*>(S.cols + 12 * plane + round256(npx * sizeof(int32_t)));

    const double *d_rgba = rgba, *d_geom = geom;
    const int32_t* d_ids = ids;
    double* d_out = out;
    if (on_device) {
        DN_HIP(hipDeviceSynchronize());  // (the frame may still be in flight on the engine's stream)
    } else {
        const size_t b_rgba = round256(npx * 4 * sizeof(double)), b_geom = round256(npx * 8 * sizeof(double));
        if (ensure(&S.in, S.in_bytes, b_rgba + b_geom + npx * 2 * sizeof(int32_t))) return -1;
        const auto t0 = std::chrono::steady_clock::now();
        DN_HIP(hipMemcpy(S.in, rgba, npx * 4 * sizeof(double), hipMemcpyHostToDevice));
        DN_HIP(hipMemcpy(S.in + b_rgba, geom, npx * 8 * sizeof(double), hipMemcpyHostToDevice));
        DN_HIP(hipMemcpy(S.in + b_rgba + b_geom, ids, npx * 2 * sizeof(int32_t), hipMemcpyHostToDevice));
        st->upload_ms = ms_since(t0);
        d_rgba = reinterpret_cast<const double*>(S.in);
        d_geom = reinterpret_cast<const double*>(S.in + b_rgba);
        d_ids = reinterpret_cast<const int32_t*>(S.in + b_rgba + b_geom);
        d_out = reinterpret_cast<double*>(S.in);
    }

    // the host's dn_make_consts
    DnConsts c;
    c.kz = 1.0 / (prm.sigma_depth * prm.sigma_depth);
    const double kc0 = 1.0 / (prm.sigma_color * prm.sigma_color);
    c.kc = kc0;
    c.eps = prm.albedo_eps;
    c.squarings = prm.normal_squarings;
    c.demodulate = prm.demodulate;
    c.match_material = prm.match_material;

    DN_HIP(hipEventRecord(S.ev[0], 0));
    hipLaunchKernelGGL(k_denoise_pack, dim3(pack_blocks), dim3(kPackBlock), 0, 0, d_rgba, d_geom, d_ids, (int)npx, c, P,
                       counts);
    DN_HIP(hipGetLastError());
    DN_HIP(hipEventRecord(S.ev[1], 0));
    const int colblocks = (w + kTileW - 1) / kTileW, rowblocks = (h + kTileH - 1) / kTileH;
    const uint64_t blocks = (uint64_t)colblocks * rowblocks * nimages;
    if (blocks > 0x7fffffffull) return refuse("frt_denoise_device: too many tiles for one launch");
    int cur = 0;
    for (int it = 0; it < prm.iterations; ++it) {
        c.kc = std::ldexp(kc0, 2 * it);
        const int s = 1 << it;
        if (launch_atrous(it + 1 == prm.iterations, (unsigned)blocks, P, cur, w, h, colblocks, rowblocks, s, c, d_rgba,
                          d_geom, d_out))
            return -1;
        DN_HIP(hipGetLastError());
        DN_HIP(hipEventRecord(S.ev[it + 2], 0));
        cur ^= 1;
    }
    DN_HIP(hipEventSynchronize(S.ev[prm.iterations + 1]));
    float ms = 0.0f;
    DN_HIP(hipEventElapsedTime(&ms, S.ev[0], S.ev[1]));
    st->pack_ms = ms;
    for (int it = 0; it < prm.iterations; ++it) {
        DN_HIP(hipEventElapsedTime(&ms, S.ev[it + 1], S.ev[it + 2]));
        st->atrous_iter_ms[it] = ms;
        st->atrous_ms += ms;
    }
    const auto t1 = std::chrono::steady_clock::now();
    std::vector<int32_t> host_counts(nwaves);
    DN_HIP(hipMemcpy(host_counts.data(), counts, (size_t)nwaves * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (const int32_t n : host_counts) st->valid_pixels += (uint64_t)n;
    if (!on_device) DN_HIP(hipMemcpy(out, d_out, npx * 4 * sizeof(double), hipMemcpyDeviceToHost));
    st->readback_ms = ms_since(t1);
    st->backend = FRT_DENOISE_DEVICE;
    st->device = device;
    return 0;
}

bool finite_pos(double v) { return std::isfinite(v) && v > 0; }

}  // namespace

extern "C" {

const char* frt_denoise_error(void) { return t_error.c_str(); }

void frt_denoise_set_error(const char* message) { t_error = message != nullptr ? message : ""; }

size_t frt_denoise_params_size(void) { return sizeof(frt_denoise_params); }

size_t frt_denoise_stats_size(void) { return sizeof(frt_denoise_stats); }

void frt_denoise_defaults(frt_denoise_params* p) {
    if (p == nullptr) return;
    p->iterations = 5;
    p->normal_squarings = 5;
    p->demodulate = 1;
    p->match_material = 1;
    p->sigma_color = 1.0;
    p->sigma_depth = 0.1;
    p->albedo_eps = 0x1p-10;
}

int frt_denoise_check(const double* rgba, const double* geom, const int32_t* ids, int64_t w, int64_t h,
                      int64_t nimages, const frt_denoise_params* p, const double* out) {
    if (rgba == nullptr || geom == nullptr || ids == nullptr || p == nullptr || out == nullptr)
        return refuse("frt_denoise: a null pointer (rgba, geom, ids, params and out are all needed)");
    if (w <= 0 || h <= 0 || nimages <= 0) return refuse("frt_denoise: width, height and image count must be positive");
    const int64_t lim = 0x7fffffffll;
    if (w > lim || h > lim || nimages > lim || w * h > lim || w * h * nimages > lim)
        return refuse("frt_denoise: more than 2^31 - 1 pixels (the columns' index is 32-bit)");
    if (p->iterations < 1 || p->iterations > FRT_DENOISE_MAX_ITERATIONS)
        return refuse("frt_denoise: iterations must be 1..8");
    if (p->normal_squarings < 0 || p->normal_squarings > FRT_DENOISE_MAX_SQUARINGS)
        return refuse("frt_denoise: normal_squarings must be 0..8");
    if ((p->demodulate != 0 && p->demodulate != 1) || (p->match_material != 0 && p->match_material != 1))
        return refuse("frt_denoise: demodulate and match_material must be 0 or 1");
    if (!finite_pos(p->sigma_color) || !finite_pos(p->sigma_depth) || !finite_pos(p->albedo_eps))
        return refuse("frt_denoise: sigma_color, sigma_depth and albedo_eps must be finite and > 0");
    return 0;
}

int frt_denoise_device(const double* rgba, const double* geom, const int32_t* ids, int on_device, int64_t w, int64_t h,
                       int64_t nimages, const frt_denoise_params* params, int device, double* out,
                       frt_denoise_stats* st) {
    if (frt_denoise_check(rgba, geom, ids, w, h, nimages, params, out) != 0) return -1;
    frt_denoise_stats local;
    if (st == nullptr) st = &local;
    std::memset(st, 0, sizeof(*st));
    st->pixels = (uint64_t)(w * h * nimages);
    st->iterations = params->iterations;
    st->backend = FRT_DENOISE_HOST;
    st->device = -1;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev || device >= 64) {
        (void)hipGetLastError();
        return refuse("frt_denoise_device: no such HIP device");
    }
    std::lock_guard<std::mutex> lock(g_mu);
    return denoise_locked(g_scratch[device], rgba, geom, ids, on_device, (int)w, (int)h, (int)nimages, *params, device,
                          out, st);
}

int frt_denoise_store(void* device_ptr, const void* host, size_t bytes, int device) {
    DN_HIP(hipSetDevice(device));
    DN_HIP(hipMemcpy(device_ptr, host, bytes, hipMemcpyHostToDevice));
    return 0;
}

void frt_denoise_release(void) {
    std::lock_guard<std::mutex> lock(g_mu);
    for (int d = 0; d < 64; ++d) {
        Scratch& S = g_scratch[d];
        if (!S.used) continue;  // (never used: no HIP call for it)
        if (hipSetDevice(d) != hipSuccess) {
            (void)hipGetLastError();
            continue;
        }
        (void)hipFree(S.cols);
        (void)hipFree(S.in);
        for (auto& e : S.ev) {
            if (e != nullptr) (void)hipEventDestroy(e);
        }
        S = Scratch();
    }
}

}  // extern "C"
