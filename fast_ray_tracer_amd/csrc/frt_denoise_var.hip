// frt-mi355x: the variance-guided denoise on the device (include/frt_device.h "Variance-guided denoise", DESIGN.md
// "Accumulation and the variance-guided denoise").
//
// host/frt_denoise_var.c is the definition: the a-trous filter of frt_denoise.hip with its colour term scaled by the
// pre-filtered variance of the mean, and the variance filtered alongside the colour. This file repeats it step for
// step (dv_valid, dv_albedo, the pack and dv_guide as there; dv_tap is dv_weight with its accumulation, dv_finish the
// divisions and dv_unpack) and is compiled with -ffp-contract=off like the host, so every value is the host's.
//   k_denoise_var_pack       one pixel per lane: validity, the guides, the demodulated colour and its variance
//   k_denoise_var_atrous<>   one launch per iteration, ping-ponging the colour and variance columns; the last one
//                            writes the two images
// The shape is k_denoise_atrous's: a block is 64 x 4 pixels, a wave 64 consecutive pixels of one row with the row
// wave-uniform, so every column load of a tap is one contiguous 512-byte run; tap rows outside the image are skipped
// under scalar control, tap columns outside it load their own column and drop the tap. No atomics and no LDS.
// The summed variance vs = (v0 + v1) + v2 is a column of its own, written by the pack and by every iteration but the
// last beside v: the guide's nine taps load one column, not three (the sum's bits are the host's, which adds the three
// at the tap).
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

constexpr int kInvalid = INT32_MIN;  // the material column's value of an invalid pixel (host: DV_INVALID)
constexpr int kPackBlock = 256;
constexpr int kTileW = 64, kTileH = 4;  // k_denoise_var_atrous: a wave per row of the tile
constexpr int kMaxIter = FRT_DENOISE_MAX_ITERATIONS;
constexpr int kPlanes = 20;

// the columns of all images (index: image * h * w + y * w + x, 32-bit), carved out of one allocation
struct DvCols {
    double *n0, *n1, *n2, *inv_nn, *iz, *z;
    int32_t* mat;
    double* x[2][3];  // ping-pong
    double* v[2][3];
    double* vs[2];
};  // 164 bytes per pixel

struct DvConsts {
    double kz, kc, eps, var_eps;
    int squarings, demodulate, match_material;
};

__device__ __forceinline__ bool dv_valid(const double* rgba, const double* var, const double* geom,
                                         const int32_t* ids) {
    return ids[0] >= 0 && ids[1] != kInvalid && __builtin_isfinite(geom[0]) && geom[0] > 0 &&
           __builtin_isfinite(rgba[0]) && __builtin_isfinite(rgba[1]) && __builtin_isfinite(rgba[2]) &&
           __builtin_isfinite(var[0]) && var[0] >= 0 && __builtin_isfinite(var[1]) && var[1] >= 0 &&
           __builtin_isfinite(var[2]) && var[2] >= 0;
}

__device__ __forceinline__ double dv_albedo(const double* geom, int ch, const DvConsts& c) {
    return c.demodulate ? geom[4 + ch] + c.eps : 1.0;
}

// counts[wave]: the wave's valid pixels (summed on the host: no atomics)
__global__ __launch_bounds__(kPackBlock) void k_denoise_var_pack(const double* __restrict__ rgba,
                                                                 const double* __restrict__ var,
                                                                 const double* __restrict__ geom,
                                                                 const int32_t* __restrict__ ids, int npx, DvConsts c,
                                                                 DvCols P, int32_t* __restrict__ counts) {
    const int i = (int)(blockIdx.x * kPackBlock + threadIdx.x);  // (npx + 255 < 2^32, and i < npx below)
    bool valid = false;
    if ((unsigned)i < (unsigned)npx) {
        double px[4], vr[3], g[8];
        int32_t id[2];
#pragma unroll
        for (int k = 0; k < 4; ++k) px[k] = rgba[4 * (size_t)i + k];
#pragma unroll
        for (int k = 0; k < 3; ++k) vr[k] = var[4 * (size_t)i + k];
#pragma unroll
        for (int k = 0; k < 8; ++k) g[k] = geom[8 * (size_t)i + k];
        id[0] = ids[2 * (size_t)i];
        id[1] = ids[2 * (size_t)i + 1];
        valid = dv_valid(px, vr, g, id);
        if (valid) {
            double v[3];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const double a = dv_albedo(g, ch, c);
                P.x[0][ch][i] = px[ch] / a;
                v[ch] = vr[ch] / (a * a);
                P.v[0][ch][i] = v[ch];
            }
            P.vs[0][i] = (v[0] + v[1]) + v[2];
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
__device__ __forceinline__ constexpr double dv_k(int d) {
    return d == 0 ? 3.0 / 8.0 : (d == 1 || d == -1) ? 1.0 / 4.0 : 1.0 / 16.0;
}

// host: G[|d|]
__device__ __forceinline__ constexpr double dv_g(int d) { return d == 0 ? 1.0 / 2.0 : 1.0 / 4.0; }

// a pixel's guides, colour and variance, in registers
struct DvPix {
    double n0, n1, n2, inv_nn, iz, z;
    double x[3], v[3];
    int mat;
};

// host: dv_weight and the accumulation of dv_atrous_pixel for one tap q != p; `usable`: q is inside p's image and
// valid (an unusable q's words are whatever was loaded, and are dropped)
__device__ __forceinline__ void dv_tap(const DvPix& p, const DvPix& q, bool usable, double hk, double kc_p,
                                       const DvConsts& c, double acc[3], double vacc[3], double& ws) {
    const double d = (p.n0 * q.n0 + p.n1 * q.n1) + p.n2 * q.n2;
    const double m = (d * d) * (p.inv_nn * q.inv_nn);
    double t = m < 1.0 ? m : 1.0;
    for (int k = 0; k < c.squarings; ++k) t = t * t;
    const double r = p.z - q.z;
    const double xz = ((r * r) * c.kz) * (p.iz * q.iz);
    const double dc0 = p.x[0] - q.x[0], dc1 = p.x[1] - q.x[1], dc2 = p.x[2] - q.x[2];
    const double xc = ((dc0 * dc0 + dc1 * dc1) + dc2 * dc2) * kc_p;
    const double u = (1.0 + xz) * (1.0 + xc);
    const double wgt = (hk * t) / (u * u);
    const bool skip = !usable || (c.match_material && q.mat != p.mat) || d <= 0 || wgt < 0;
    if (!skip) {
        const double w2 = wgt * wgt;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            acc[ch] += wgt * q.x[ch];
            vacc[ch] += w2 * q.v[ch];
        }
        ws += wgt;
    }
}

// the centre tap: wgt = hk
__device__ __forceinline__ void dv_centre(const DvPix& p, double hk, double acc[3], double vacc[3], double& ws) {
    const double w2 = hk * hk;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        acc[ch] += hk * p.x[ch];
        vacc[ch] += w2 * p.v[ch];
    }
    ws += hk;
}

__device__ __forceinline__ DvPix dv_load(const DvCols& P, int cur, int i) {
    DvPix v;
    v.mat = P.mat[i];
    v.n0 = P.n0[i];
    v.n1 = P.n1[i];
    v.n2 = P.n2[i];
    v.inv_nn = P.inv_nn[i];
    v.iz = P.iz[i];
    v.z = P.z[i];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) v.x[ch] = P.x[cur][ch][i];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) v.v[ch] = P.v[cur][ch][i];
    return v;
}

// host: dv_guide. py is wave-uniform; row0 the image's first pixel
__device__ __forceinline__ double dv_guide(const DvCols& P, int cur, int row0, int w, int h, int px, int py) {
    double sum = 0.0, sg = 0.0;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const int qy = py + dy;
        if ((unsigned)qy >= (unsigned)h) continue;  // (scalar)
        const int qrow = row0 + qy * w;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = px + dx;
            const bool inside = (unsigned)qx < (unsigned)w;
            const int q = qrow + (inside ? qx : px);
            const double vs = P.vs[cur][q];
            const bool use = inside && P.mat[q] != kInvalid;
            const double g = dv_g(dx) * dv_g(dy);
            if (use) {
                sum += g * vs;
                sg += g;
            }
        }
    }
    return sum / sg;
}

// x_{i+1} = acc / ws, v_{i+1} = vacc / (ws * ws) into the columns of cur ^ 1, or (kLast) rgb = x_{i+1} * a,
// out_var = v_{i+1} * (a * a), the alpha and var[3] into the images
template <bool kLast>
__device__ __forceinline__ void dv_finish(const DvCols& P, int cur, int p, const double acc[3], const double vacc[3],
                                          double ws, const DvConsts& c, const double* rgba, const double* var,
                                          const double* __restrict__ geom, double* out, double* out_var) {
    double y[3], vy[3];
    const double ws2 = ws * ws;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        y[ch] = acc[ch] / ws;
        vy[ch] = vacc[ch] / ws2;
    }
    if (kLast) {
        const double alpha = rgba[4 * (size_t)p + 3];
        double g[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (c.demodulate) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) g[4 + ch] = geom[8 * (size_t)p + 4 + ch];
        }
        double a[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) a[ch] = dv_albedo(g, ch, c);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) out[4 * (size_t)p + ch] = y[ch] * a[ch];
        out[4 * (size_t)p + 3] = alpha;
        if (out_var != nullptr) {
            const double count = var[4 * (size_t)p + 3];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) out_var[4 * (size_t)p + ch] = vy[ch] * (a[ch] * a[ch]);
            out_var[4 * (size_t)p + 3] = count;
        }
    } else {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            P.x[cur ^ 1][ch][p] = y[ch];
            P.v[cur ^ 1][ch][p] = vy[ch];
        }
        P.vs[cur ^ 1][p] = (vy[0] + vy[1]) + vy[2];
    }
}

// an invalid pixel's outputs are its inputs (out may be rgba, out_var var: a lane reads and writes its own pixel only)
__device__ __forceinline__ void dv_copy(int p, const double* rgba, const double* var, double* out, double* out_var) {
#pragma unroll
    for (int k = 0; k < 4; ++k) out[4 * (size_t)p + k] = rgba[4 * (size_t)p + k];
    if (out_var != nullptr) {
#pragma unroll
        for (int k = 0; k < 4; ++k) out_var[4 * (size_t)p + k] = var[4 * (size_t)p + k];
    }
}

// One iteration, step s, from the columns of cur to those of cur ^ 1; kLast writes the images instead.
// blockIdx.x = (image * rowblocks + rowblock) * colblocks + colblock.
template <bool kLast>
__global__ __launch_bounds__(kTileW* kTileH) void k_denoise_var_atrous(DvCols P, int cur, int w, int h, int colblocks,
                                                                       int rowblocks, int s, DvConsts c,
                                                                       const double* rgba, const double* var,
                                                                       const double* __restrict__ geom, double* out,
                                                                       double* out_var) {
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
        if (kLast) dv_copy(p, rgba, var, out, out_var);
        return;
    }
    const double kc_p = c.kc / (dv_guide(P, cur, row0, w, h, px, py) + c.var_eps);
    const DvPix vp = dv_load(P, cur, p);
    double acc[3] = {0.0, 0.0, 0.0}, vacc[3] = {0.0, 0.0, 0.0}, ws = 0.0;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = py + s * dy;
        if ((unsigned)qy >= (unsigned)h) continue;  // (scalar: py and s are wave-uniform)
        const int qrow = row0 + qy * w;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const double hk = dv_k(dx) * dv_k(dy);
            if (dx == 0 && dy == 0) {
                dv_centre(vp, hk, acc, vacc, ws);
                continue;
            }
            const int qx = px + s * dx;
            const bool inside = (unsigned)qx < (unsigned)w;
            // a lane whose tap is outside loads its own column instead and drops the tap: the loads stay
            // unconditional (an invalid pixel's guide words are never written, only read and dropped)
            const DvPix vq = dv_load(P, cur, qrow + (inside ? qx : px));
            dv_tap(vp, vq, inside && vq.mat != kInvalid, hk, kc_p, c, acc, vacc, ws);
        }
    }
    dv_finish<kLast>(P, cur, p, acc, vacc, ws, c, rgba, var, geom, out, out_var);
}

int refuse(const std::string& what) {
    frt_denoise_set_error(what.c_str());
    return -1;
}

int fail(const char* what, hipError_t e) {
    frt_denoise_set_error((std::string(what) + ": " + hipGetErrorString(e)).c_str());
    (void)hipGetLastError();
    return -1;
}

#define DV_HIP(call)                                  \
    do {                                              \
        const hipError_t e_ = (call);                 \
        if (e_ != hipSuccess) return fail(#call, e_); \
    } while (0)

// a device's buffers, kept between calls (grow only); used under g_mu
struct Scratch {
    char* cols = nullptr;  // the columns, then the pack's per-wave counts
    size_t cols_bytes = 0;
    char* in = nullptr;  // host buffers' copies: rgba and var (filtered in place), geom, ids
    size_t in_bytes = 0;
    hipEvent_t ev[kMaxIter + 2] = {};
    bool used = false;
};

std::mutex g_mu;
Scratch g_scratch[64];

int ensure(char** p, size_t& have, size_t need) {
    if (need <= have) return 0;
    if (*p != nullptr) DV_HIP(hipFree(*p));
    *p = nullptr;
    have = 0;
    DV_HIP(hipMalloc((void**)p, need));
    have = need;
    return 0;
}

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

size_t round256(size_t n) { return (n + 255) & ~(size_t)255; }

// one a-trous launch on the null stream
int launch_atrous(bool last, unsigned blocks, const DvCols& P, int cur, int w, int h, int colblocks, int rowblocks, int s,
                  const DvConsts& c, const double* rgba, const double* var, const double* geom, double* out,
                  double* out_var) {
    const dim3 block(kTileW, kTileH);
    if (last) {
        hipLaunchKernelGGL(k_denoise_var_atrous<true>, dim3(blocks), block, 0, 0, P, cur, w, h, colblocks, rowblocks, s,
                           c, rgba, var, geom, out, out_var);
    } else {
        hipLaunchKernelGGL(k_denoise_var_atrous<false>, dim3(blocks), block, 0, 0, P, cur, w, h, colblocks, rowblocks,
                           s, c, rgba, var, geom, out, out_var);
    }
    DV_HIP(hipGetLastError());
    return 0;
}

int denoise_locked(Scratch& S, const double* rgba, const double* var, const double* geom, const int32_t* ids,
                   int on_device, int w, int h, int nimages, const frt_denoise_var_params& prm, int device, double* out,
                   double* out_var, frt_denoise_var_stats* st) {
    const size_t npx = (size_t)w * h * nimages;
    const size_t plane = round256(npx * sizeof(double));
    const unsigned nwaves = (unsigned)((npx + 63) / 64), pack_blocks = (unsigned)((npx + kPackBlock - 1) / kPackBlock);
    const size_t count_words = (size_t)pack_blocks * (kPackBlock / 64);
    DV_HIP(hipSetDevice(device));
    S.used = true;
    for (auto& e : S.ev) {
        if (e == nullptr) DV_HIP(hipEventCreate(&e));
    }
    if (ensure(&S.cols, S.cols_bytes,
               kPlanes * plane + round256(npx * sizeof(int32_t)) + count_words * sizeof(int32_t)))
        return -1;
    DvCols P;
    double* base = reinterpret_cast<double*>(S.cols);
    const size_t pw = plane / sizeof(double);
    P.n0 = base;
    P.n1 = base + pw;
    P.n2 = base + 2 * pw;
    P.inv_nn = base + 3 * pw;
    P.iz = base + 4 * pw;
    P.z = base + 5 * pw;
    for (int k = 0; k < 6; ++k) {
        P.x[k / 3][k % 3] = base + (size_t)(6 + k) * pw;
        P.v[k / 3][k % 3] = base + (size_t)(12 + k) * pw;
    }
    P.vs[0] = base + 18 * pw;
    P.vs[1] = base + 19 * pw;
    P.mat = reinterpret_cast<int32_t*>(S.cols + kPlanes * plane);
    int32_t* counts = reinterpret_cast<int32_t*>(S.cols + kPlanes * plane + round256(npx * sizeof(int32_t)));

    const double *d_rgba = rgba, *d_var = var, *d_geom = geom;
    const int32_t* d_ids = ids;
    double *d_out = out, *d_out_var = out_var;
    const size_t b_rgba = round256(npx * 4 * sizeof(double)), b_geom = round256(npx * 8 * sizeof(double));
    if (on_device) {
        DV_HIP(hipDeviceSynchronize());  // (the frame may still be in flight on the engine's stream)
    } else {
        if (ensure(&S.in, S.in_bytes, 2 * b_rgba + b_geom + npx * 2 * sizeof(int32_t))) return -1;
        const auto t0 = std::chrono::steady_clock::now();
        DV_HIP(hipMemcpy(S.in, rgba, npx * 4 * sizeof(double), hipMemcpyHostToDevice));
        DV_HIP(hipMemcpy(S.in + b_rgba, var, npx * 4 * sizeof(double), hipMemcpyHostToDevice));
        DV_HIP(hipMemcpy(S.in + 2 * b_rgba, geom, npx * 8 * sizeof(double), hipMemcpyHostToDevice));
        DV_HIP(hipMemcpy(S.in + 2 * b_rgba + b_geom, ids, npx * 2 * sizeof(int32_t), hipMemcpyHostToDevice));
        st->upload_ms = ms_since(t0);
        d_rgba = reinterpret_cast<const double*>(S.in);
        d_var = reinterpret_cast<const double*>(S.in + b_rgba);
        d_geom = reinterpret_cast<const double*>(S.in + 2 * b_rgba);
        d_ids = reinterpret_cast<const int32_t*>(S.in + 2 * b_rgba + b_geom);
        d_out = reinterpret_cast<double*>(S.in);
        d_out_var = out_var != nullptr ? reinterpret_cast<double*>(S.in + b_rgba) : nullptr;
    }

    // the host's dv_make_consts
    DvConsts c;
    c.kz = 1.0 / (prm.sigma_depth * prm.sigma_depth);
    c.kc = 1.0 / (prm.sigma_color * prm.sigma_color);
    c.eps = prm.albedo_eps;
    c.var_eps = prm.var_eps;
    c.squarings = prm.normal_squarings;
    c.demodulate = prm.demodulate;
    c.match_material = prm.match_material;

    DV_HIP(hipEventRecord(S.ev[0], 0));
    hipLaunchKernelGGL(k_denoise_var_pack, dim3(pack_blocks), dim3(kPackBlock), 0, 0, d_rgba, d_var, d_geom, d_ids,
                       (int)npx, c, P, counts);
    DV_HIP(hipGetLastError());
    DV_HIP(hipEventRecord(S.ev[1], 0));
    const int colblocks = (w + kTileW - 1) / kTileW, rowblocks = (h + kTileH - 1) / kTileH;
    const uint64_t blocks = (uint64_t)colblocks * rowblocks * nimages;
    if (blocks > 0x7fffffffull) return refuse("frt_denoise_var_device: too many tiles for one launch");
    int cur = 0;
    for (int it = 0; it < prm.iterations; ++it) {
        const int s = 1 << it;
        if (launch_atrous(it + 1 == prm.iterations, (unsigned)blocks, P, cur, w, h, colblocks, rowblocks, s, c, d_rgba,
                          d_var, d_geom, d_out, d_out_var))
            return -1;
        DV_HIP(hipEventRecord(S.ev[it + 2], 0));
        cur ^= 1;
    }
    DV_HIP(hipEventSynchronize(S.ev[prm.iterations + 1]));
    float ms = 0.0f;
    DV_HIP(hipEventElapsedTime(&ms, S.ev[0], S.ev[1]));
    st->pack_ms = ms;
    for (int it = 0; it < prm.iterations; ++it) {
        DV_HIP(hipEventElapsedTime(&ms, S.ev[it + 1], S.ev[it + 2]));
        st->atrous_iter_ms[it] = ms;
        st->atrous_ms += ms;
    }
    const auto t1 = std::chrono::steady_clock::now();
    std::vector<int32_t> host_counts(nwaves);
    DV_HIP(hipMemcpy(host_counts.data(), counts, (size_t)nwaves * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (const int32_t n : host_counts) st->valid_pixels += (uint64_t)n;
    if (!on_device) {
        DV_HIP(hipMemcpy(out, d_out, npx * 4 * sizeof(double), hipMemcpyDeviceToHost));
        if (out_var != nullptr) DV_HIP(hipMemcpy(out_var, d_out_var, npx * 4 * sizeof(double), hipMemcpyDeviceToHost));
    }
    st->readback_ms = ms_since(t1);
    st->backend = FRT_DENOISE_DEVICE;
    st->device = device;
    return 0;
}

bool finite_pos(double v) { return std::isfinite(v) && v > 0; }

}  // namespace

extern "C" {

size_t frt_denoise_var_params_size(void) { return sizeof(frt_denoise_var_params); }

void frt_denoise_var_defaults(frt_denoise_var_params* p) {
    if (p == nullptr) return;
    p->iterations = 5;
    p->normal_squarings = 5;
    p->demodulate = 1;
    p->match_material = 1;
    p->sigma_color = 2.0;
    p->sigma_depth = 0.1;
    p->albedo_eps = 0x1p-10;
    p->var_eps = 0x1p-40;
}

int frt_denoise_var_check(const double* rgba, const double* var, const double* geom, const int32_t* ids, int64_t w,
                          int64_t h, int64_t nimages, const frt_denoise_var_params* p, const double* out) {
    if (rgba == nullptr || var == nullptr || geom == nullptr || ids == nullptr || p == nullptr || out == nullptr)
        return refuse("frt_denoise_var: a null pointer (rgba, var, geom, ids, params and out are all needed)");
    if (w <= 0 || h <= 0 || nimages <= 0)
        return refuse("frt_denoise_var: width, height and image count must be positive");
    const int64_t lim = 0x7fffffffll;
    if (w > lim || h > lim || nimages > lim || w * h > lim || w * h * nimages > lim)
        return refuse("frt_denoise_var: more than 2^31 - 1 pixels (the columns' index is 32-bit)");
    if (p->iterations < 1 || p->iterations > FRT_DENOISE_MAX_ITERATIONS)
        return refuse("frt_denoise_var: iterations must be 1..8");
    if (p->normal_squarings < 0 || p->normal_squarings > FRT_DENOISE_MAX_SQUARINGS)
        return refuse("frt_denoise_var: normal_squarings must be 0..8");
    if ((p->demodulate != 0 && p->demodulate != 1) || (p->match_material != 0 && p->match_material != 1))
        return refuse("frt_denoise_var: demodulate and match_material must be 0 or 1");
    if (!finite_pos(p->sigma_color) || !finite_pos(p->sigma_depth) || !finite_pos(p->albedo_eps) ||
        !finite_pos(p->var_eps))
        return refuse("frt_denoise_var: sigma_color, sigma_depth, albedo_eps and var_eps must be finite and > 0");
    return 0;
}

int frt_denoise_var_device(const double* rgba, const double* var, const double* geom, const int32_t* ids, int on_device,
                           int64_t w, int64_t h, int64_t nimages, const frt_denoise_var_params* params, int device,
                           double* out, double* out_var, frt_denoise_var_stats* st) {
    if (frt_denoise_var_check(rgba, var, geom, ids, w, h, nimages, params, out) != 0) return -1;
    frt_denoise_var_stats local;
    if (st == nullptr) st = &local;
    std::memset(st, 0, sizeof(*st));
    st->pixels = (uint64_t)(w * h * nimages);
    st->iterations = params->iterations;
    st->backend = FRT_DENOISE_HOST;
    st->device = -1;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev || device >= 64) {
        (void)hipGetLastError();
        return refuse("frt_denoise_var_device: no such HIP device");
    }
    std::lock_guard<std::mutex> lock(g_mu);
    return denoise_locked(g_scratch[device], rgba, var, geom, ids, on_device, (int)w, (int)h, (int)nimages, *params,
                          device, out, out_var, st);
}

void frt_denoise_var_release(void) {
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
