// frt-mi355x: the 16-bit image encode on the device (include/frt_device.h "Image encode", DESIGN.md "Image encode").
//
// write_ppm_file / write_png turn the binary64 canvas into big-endian 16-bit codes in three single-threaded host
// passes with one libm pow per channel (host/frt_canvas.c). Here the same codes come from two kernels:
//   k_encode_max  per-channel maximum with the host's semantics (from 0, update on x > max) and a non-finite flag
//   k_encode      scaling / clamp, the sRGB curve and floor(s * inverse), one pixel per lane
// Every operation but pow is an IEEE operation the host performs too (this file is compiled with
// -ffp-contract=off like the host), so its result is the host's bit for bit. The pow branch is decided only where
// the device's value is further than FRT_ENCODE_MARGIN (2^-40 relative) from every boundary the host's value is
// compared against; the rest goes to the undecided list, which host/frt_canvas.c recomputes with its own code.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "frt_device.h"

namespace {

constexpr int kBlock = 256;                 // pixels per block of k_encode (one per lane)
constexpr int kBlockWords = kBlock * 6 / 4; // a block's output: 1536 bytes, whole dwords
constexpr int kSegs = 8;                    // undecided list segments, one counter each on a line of its own
constexpr int kSegStride = 32;              // counters' distance in words (128 bytes)
constexpr double kSqrt3 = 1.7320508075688772;  // host/frt_canvas.c FRT_SQRT3

struct EncConsts {
    double srgb_max[3];
    double inverse[3];
    int code_one[3];
    int mode;
};

__device__ __forceinline__ double srgb_curve(double t) { return 1.055 * pow(t, 1.0 / 2.4) - 0.055; }

// The code of one channel value t (after scaling / clamping), or -1 when the device cannot prove it.
// rgb_to_srgb and quantize of the host, statement for statement; only srgb_curve is approximate.
__device__ __forceinline__ int decide(double t, double smax, double inverse, int code_one) {
    if (t < 0.0031308) {
        const double s = t * 12.92;
        if (s > smax) return 65535;
        if (s < 0) return 0;
        return (int)(unsigned short)floor(s * inverse);
    }
    if (t == 1.0) return code_one;
    const double s = srgb_curve(t);
    if (!(fabs(s - smax) > FRT_ENCODE_MARGIN * smax)) return -1;  // (a NaN lands here too)
    if (s > smax) return 65535;
    const double q = s * inverse, f = floor(q), m = FRT_ENCODE_MARGIN * q;
    if (!(q - f > m && (f + 1.0) - q > m)) return -1;
    return (int)f;
}

// res[0..2]: bit patterns of the channel maxima (non-negative doubles order as their bits), res[3]: non-finite flag
__global__ __launch_bounds__(kBlock) void k_encode_max(const double* __restrict__ rgba, long long npx,
                                                       unsigned long long* res) {
    __shared__ double part[kBlock / 64][3];
    __shared__ int part_bad[kBlock / 64];
    double m[3] = {0.0, 0.0, 0.0};
    int bad = 0;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < npx; i += stride) {
        const double2 a = reinterpret_cast<const double2*>(rgba)[2 * i];
        const double b = rgba[4 * i + 2];
        const double t[3] = {a.x, a.y, b};
        for (int k = 0; k < 3; ++k) {
            if (t[k] > m[k]) m[k] = t[k];
            bad |= !__builtin_isfinite(t[k]);
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        for (int k = 0; k < 3; ++k) {
            const double o = __shfl_xor(m[k], off);
            if (o > m[k]) m[k] = o;
        }
    }
    bad = __any(bad);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        for (int k = 0; k < 3; ++k) part[wave][k] = m[k];
        part_bad[wave] = bad;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        double v = part[0][threadIdx.x];
        for (int w = 1; w < kBlock / 64; ++w)
            if (part[w][threadIdx.x] > v) v = part[w][threadIdx.x];
        if (v > 0.0) atomicMax(res + threadIdx.x, (unsigned long long)__double_as_longlong(v));
    } else if (threadIdx.x == 3) {
        int any = 0;
        for (int w = 0; w < kBlock / 64; ++w) any |= part_bad[w];
        if (any) atomicOr(res + 3, 1ull);
    }
}

// One pixel per lane: a wave reads 2 KB of contiguous canvas; a block's 256 pixels are 1536 output bytes, staged in
// LDS and stored as 384 whole dwords (out_words holds whole blocks: the last block's tail lanes store zeros into the
// padding). Undecided values: one ballot per channel and one counter update per wave that has any, into the block's
// list segment; an entry past the segment's capacity is counted but not stored (the image is declined then).
__global__ __launch_bounds__(kBlock) void k_encode(const double* __restrict__ rgba, long long npx, EncConsts C,
                                                   uint32_t* __restrict__ out_words, uint32_t* __restrict__ list,
                                                   unsigned* counters, unsigned seg_cap) {
    __shared__ unsigned short codes[kBlock * 3];
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    int q[3] = {0, 0, 0};
    if (i < npx) {
        const double2 a = reinterpret_cast<const double2*>(rgba)[2 * i];
        const double b = rgba[4 * i + 2];
        double t[3] = {a.x, a.y, b};
        if (C.mode == FRT_ENCODE_PPM_SCALED) {
            const double len = t[0] + t[1] + t[2];
            if (len > kSqrt3) {
                const double r = 1.0 / len;
                for (int k = 0; k < 3; ++k) t[k] *= r;
                for (int k = 0; k < 3; ++k) t[k] *= kSqrt3;
            }
        } else {
            for (int k = 0; k < 3; ++k) {
                if (t[k] > 1.0) {
                    t[k] = 1.0;
                } else if (t[k] < 0) {
                    t[k] = 0.0;
                }
            }
        }
        for (int k = 0; k < 3; ++k) q[k] = decide(t[k], C.srgb_max[k], C.inverse[k], C.code_one[k]);
    }
    for (int k = 0; k < 3; ++k) {
        const unsigned v = q[k] < 0 ? 0u : (unsigned)q[k];
        codes[threadIdx.x * 3 + k] = (unsigned short)(((v & 0xffu) << 8) | (v >> 8));  // big-endian in memory
    }
    const unsigned long long m0 = __ballot(q[0] < 0), m1 = __ballot(q[1] < 0), m2 = __ballot(q[2] < 0);
    if ((m0 | m1 | m2) != 0ull) {  // (wave-uniform)
        const int lane = threadIdx.x & 63;
        const unsigned seg = blockIdx.x % kSegs;
        const unsigned n0 = (unsigned)__popcll(m0), n1 = (unsigned)__popcll(m1), n2 = (unsigned)__popcll(m2);
        unsigned base = 0;
        if (lane == 0) base = atomicAdd(counters + seg * kSegStride, n0 + n1 + n2);
        base = __shfl(base, 0);
        const unsigned long long below = (1ull << lane) - 1ull;
        const unsigned at[3] = {base + (unsigned)__popcll(m0 & below), base + n0 + (unsigned)__popcll(m1 & below),
                                base + n0 + n1 + (unsigned)__popcll(m2 & below)};
        for (int k = 0; k < 3; ++k) {
            if (q[k] < 0 && at[k] < seg_cap) list[(size_t)seg * seg_cap + at[k]] = (uint32_t)(i * 3 + k);
        }
    }
    __syncthreads();
    const uint32_t* words = reinterpret_cast<const uint32_t*>(codes);
    uint32_t* dst = out_words + (size_t)blockIdx.x * kBlockWords;
    dst[threadIdx.x] = words[threadIdx.x];
    if (threadIdx.x < kBlockWords - kBlock) dst[kBlock + threadIdx.x] = words[kBlock + threadIdx.x];
}

// the canvas pixels of n undecided values (a device-resident canvas: the host patches from these)
__global__ void k_encode_gather(const double* __restrict__ rgba, const uint32_t* __restrict__ idx, unsigned n,
                                double* __restrict__ px) {
    const unsigned j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const size_t p = idx[j] / 3u;
    for (int k = 0; k < 4; ++k) px[4 * (size_t)j + k] = rgba[4 * p + k];
}

__global__ void k_encode_selftest(const double* __restrict__ t, long long n, double* __restrict__ p,
                                  double* __restrict__ s) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    p[i] = pow(t[i], 1.0 / 2.4);
    s[i] = srgb_curve(t[i]);
}

thread_local std::string t_error;

int fail(const char* what, hipError_t e) {
    t_error = std::string(what) + ": " + hipGetErrorString(e);
    (void)hipGetLastError();
    return -1;
}

#define ENC_HIP(call)                                   \
    do {                                                \
        const hipError_t e_ = (call);                   \
        if (e_ != hipSuccess) return fail(#call, e_);   \
    } while (0)

// a device's buffers, kept between calls (grow only); used under g_mu
struct Scratch {
    double* canvas = nullptr;
    size_t canvas_bytes = 0;
    uint32_t* out = nullptr;
    size_t out_bytes = 0;
    uint32_t* list = nullptr;
    size_t list_bytes = 0;
    double* px = nullptr;
    size_t px_bytes = 0;
    unsigned long long* res = nullptr;  // 4 words of k_encode_max, then the counters' lines
    hipEvent_t ev[2] = {nullptr, nullptr};
};

std::mutex g_mu;
Scratch g_scratch[64];

template <typename T>
int ensure(T** p, size_t& have, size_t need) {
    if (need <= have) return 0;
    if (*p != nullptr) ENC_HIP(hipFree(*p));
    *p = nullptr;
    have = 0;
    ENC_HIP(hipMalloc((void**)p, need));
    have = need;
    return 0;
}

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

constexpr size_t kResBytes = 4 * sizeof(unsigned long long) + (size_t)kSegs * kSegStride * sizeof(unsigned);

int encode_locked(Scratch& S, const double* rgba, int on_device, size_t width, size_t height, int mode, int device,
                  const EncConsts& C, unsigned char* out, uint32_t* und_idx, double* und_px, frt_encode_stats* st) {
    const size_t npx = width * height, values = 3 * npx;
    const unsigned cap = (unsigned)(values / 64);
    const unsigned nblocks = (unsigned)((npx + kBlock - 1) / kBlock);
    ENC_HIP(hipSetDevice(device));
    if (S.ev[0] == nullptr) {
        ENC_HIP(hipEventCreate(&S.ev[0]));
        ENC_HIP(hipEventCreate(&S.ev[1]));
    }
    if (S.res == nullptr) ENC_HIP(hipMalloc((void**)&S.res, kResBytes));
    if (ensure(&S.out, S.out_bytes, (size_t)nblocks * kBlockWords * 4)) return -1;
    if (ensure(&S.list, S.list_bytes, ((size_t)kSegs * cap + 1) * sizeof(uint32_t))) return -1;
    const double* src = rgba;
    if (on_device) {
        ENC_HIP(hipDeviceSynchronize());  // (the frame may still be in flight on the engine's stream)
    } else {
        if (ensure(&S.canvas, S.canvas_bytes, npx * 4 * sizeof(double))) return -1;
        const auto t0 = std::chrono::steady_clock::now();
        ENC_HIP(hipMemcpy(S.canvas, rgba, npx * 4 * sizeof(double), hipMemcpyHostToDevice));
        st->upload_ms = ms_since(t0);
        src = S.canvas;
    }
    unsigned* counters = reinterpret_cast<unsigned*>(S.res + 4);
    float ms = 0.0f;

    ENC_HIP(hipMemsetAsync(S.res, 0, kResBytes, 0));
    ENC_HIP(hipEventRecord(S.ev[0], 0));
    const unsigned max_blocks = (unsigned)std::min<size_t>(nblocks, 2048);
    hipLaunchKernelGGL(k_encode_max, dim3(max_blocks), dim3(kBlock), 0, 0, src, (long long)npx, S.res);
    ENC_HIP(hipGetLastError());
    ENC_HIP(hipEventRecord(S.ev[1], 0));
    unsigned long long res[4];
    ENC_HIP(hipMemcpy(res, S.res, sizeof(res), hipMemcpyDeviceToHost));
    ENC_HIP(hipEventElapsedTime(&ms, S.ev[0], S.ev[1]));
    st->kernel_ms = ms;
    for (int k = 0; k < 3; ++k) std::memcpy(&st->rgb_max[k], &res[k], sizeof(double));
    if (res[3] != 0) {
        st->decline = FRT_ENCODE_NON_FINITE;
        return 1;
    }
    if (mode != FRT_ENCODE_PNG && (st->rgb_max[0] == 0.0 || st->rgb_max[1] == 0.0 || st->rgb_max[2] == 0.0)) {
        st->decline = FRT_ENCODE_ZERO_MAX;
        return 1;
    }

    ENC_HIP(hipEventRecord(S.ev[0], 0));
    hipLaunchKernelGGL(k_encode, dim3(nblocks), dim3(kBlock), 0, 0, src, (long long)npx, C, S.out, S.list, counters,
                       cap);
    ENC_HIP(hipGetLastError());
    ENC_HIP(hipEventRecord(S.ev[1], 0));
    unsigned count[kSegs * kSegStride];
    const auto t1 = std::chrono::steady_clock::now();
    ENC_HIP(hipMemcpy(count, counters, sizeof(count), hipMemcpyDeviceToHost));
    ENC_HIP(hipEventElapsedTime(&ms, S.ev[0], S.ev[1]));
    st->kernel_ms += ms;
    uint64_t total = 0;
    for (int s = 0; s < kSegs; ++s) total += count[s * kSegStride];
    st->undecided = total;
    if (total > cap) {
        st->decline = FRT_ENCODE_OVER_CAP;
        return 1;
    }
    const auto t2 = std::chrono::steady_clock::now();  // (the counters' wait above is the kernel's, not read-back)
    (void)t1;
    ENC_HIP(hipMemcpy(out, S.out, npx * 6, hipMemcpyDeviceToHost));
    size_t n = 0;
    for (int s = 0; s < kSegs; ++s) {
        const unsigned c = count[s * kSegStride];  // (<= total <= cap: every entry was stored)
        if (c == 0) continue;
        ENC_HIP(hipMemcpy(und_idx + n, S.list + (size_t)s * cap, c * sizeof(uint32_t), hipMemcpyDeviceToHost));
        n += c;
    }
    if (on_device && n > 0) {
        if (ensure(&S.px, S.px_bytes, (size_t)cap * 4 * sizeof(double))) return -1;
        // (the compacted list goes back into the first segment, which holds cap entries)
        ENC_HIP(hipMemcpy(S.list, und_idx, n * sizeof(uint32_t), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_encode_gather, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, src, S.list,
                           (unsigned)n, S.px);
        ENC_HIP(hipGetLastError());
        ENC_HIP(hipMemcpy(und_px, S.px, n * 4 * sizeof(double), hipMemcpyDeviceToHost));
    }
    st->readback_ms = ms_since(t2);
    st->backend = FRT_ENCODE_DEVICE;
    return 0;
}

}  // namespace

extern "C" {

const char* frt_encode_error(void) { return t_error.c_str(); }

int frt_encode16_device(const double* rgba, int rgba_on_device, size_t width, size_t height, int mode, int device,
                        const double srgb_max[3], const double inverse[3], const unsigned short code_one[3],
                        unsigned char* out, uint32_t* und_idx, double* und_px, frt_encode_stats* st) {
    frt_encode_stats local;
    if (st == nullptr) st = &local;
    std::memset(st, 0, sizeof(*st));
    const size_t npx = width * height;
    st->values = 3 * (uint64_t)npx;
    st->backend = FRT_ENCODE_HOST;
    st->mode = mode;
    st->device = -1;
    for (int k = 0; k < 3; ++k) st->srgb_max[k] = srgb_max[k];
    st->decline = FRT_ENCODE_NO_DEVICE;
    if (npx == 0 || rgba == nullptr || out == nullptr || mode < 0 || mode > FRT_ENCODE_PNG) {
        t_error = "frt_encode16_device: empty canvas or unknown mode";
        return -1;
    }
    if (3 * (uint64_t)npx >= (1ull << 32)) {
        st->decline = FRT_ENCODE_TOO_LARGE;
        return 1;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev || device >= 64) {
        (void)hipGetLastError();
        t_error = "frt_encode16_device: no such HIP device";
        return -1;
    }
    EncConsts C;
    for (int k = 0; k < 3; ++k) {
        C.srgb_max[k] = srgb_max[k];
        C.inverse[k] = inverse[k];
        C.code_one[k] = code_one[k];
    }
    C.mode = mode;
    st->device = device;
    st->decline = FRT_ENCODE_TAKEN;
    std::lock_guard<std::mutex> lock(g_mu);
    const int rc = encode_locked(g_scratch[device], rgba, rgba_on_device, width, height, mode, device, C, out,
                                 und_idx, und_px, st);
    if (rc < 0) st->decline = FRT_ENCODE_NO_DEVICE;
    return rc;
}

int frt_encode_fetch(void* host, const void* device_ptr, size_t bytes, int device) {
    ENC_HIP(hipSetDevice(device));
    ENC_HIP(hipDeviceSynchronize());
    ENC_HIP(hipMemcpy(host, device_ptr, bytes, hipMemcpyDeviceToHost));
    return 0;
}

void frt_encode_release(void) {
    std::lock_guard<std::mutex> lock(g_mu);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess) {
        (void)hipGetLastError();
        return;
    }
    for (int d = 0; d < ndev && d < 64; ++d) {
        Scratch& S = g_scratch[d];
        if (S.res == nullptr) continue;  // (never used)
        if (hipSetDevice(d) != hipSuccess) continue;
        (void)hipFree(S.canvas);
        (void)hipFree(S.out);
        (void)hipFree(S.list);
        (void)hipFree(S.px);
        (void)hipFree(S.res);
        if (S.ev[0]) (void)hipEventDestroy(S.ev[0]);
        if (S.ev[1]) (void)hipEventDestroy(S.ev[1]);
        S = Scratch();
    }
}

int64_t frt_encode_selftest(int64_t n, uint64_t seed, double* out, int nout) {
    if (n < 1) n = 1;
    auto mix = [](uint64_t z) {
        z += 0x9e3779b97f4a7c15ULL;
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
        return z ^ (z >> 31);
    };
    std::vector<double> t((size_t)n), p((size_t)n), s((size_t)n);
    const double lo = std::log(0.0031308), hi = std::log(4.0);
    for (int64_t i = 0; i < n; ++i) {
        const uint64_t h = mix(seed ^ mix((uint64_t)i));
        const double u = (double)(h >> 11) * 0x1.0p-53;
        double v;
        if ((i & 7) == 0) {  // within 4 ulps of 1.0, both sides
            v = 1.0;
            const int steps = (int)(mix(h) % 9) - 4;
            for (int q = 0; q < (steps < 0 ? -steps : steps); ++q) v = std::nextafter(v, steps < 0 ? 0.0 : 2.0);
        } else if ((i & 7) == 1) {  // the threshold and the 4 doubles above it (below it the curve is linear)
            v = 0.0031308;
            const int steps = (int)(mix(h) % 5);
            for (int q = 0; q < steps; ++q) v = std::nextafter(v, 1.0);
        } else {
            v = std::exp(lo + u * (hi - lo));
            if (v < 0.0031308) v = 0.0031308;
        }
        t[(size_t)i] = v;
    }
    double *dt = nullptr, *dp = nullptr, *ds = nullptr;
    const size_t bytes = (size_t)n * sizeof(double);
    bool ok = hipMalloc((void**)&dt, bytes) == hipSuccess && hipMalloc((void**)&dp, bytes) == hipSuccess &&
              hipMalloc((void**)&ds, bytes) == hipSuccess &&
              hipMemcpy(dt, t.data(), bytes, hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(k_encode_selftest, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, dt, (long long)n, dp,
                           ds);
        ok = hipGetLastError() == hipSuccess && hipMemcpy(p.data(), dp, bytes, hipMemcpyDeviceToHost) == hipSuccess &&
             hipMemcpy(s.data(), ds, bytes, hipMemcpyDeviceToHost) == hipSuccess;
    }
    (void)hipFree(dt);
    (void)hipFree(dp);
    (void)hipFree(ds);
    if (!ok) {
        (void)hipGetLastError();
        return -1;
    }
    double worst_s = 0.0, worst_p = 0.0;
    int64_t failed = 0, differ = 0;
    for (int64_t i = 0; i < n; ++i) {
        const double hp = std::pow(t[(size_t)i], 1.0 / 2.4), hs = 1.055 * hp - 0.055;
        const double dp_ = std::fabs(p[(size_t)i] - hp) / hp, ds_ = std::fabs(s[(size_t)i] - hs) / hs;
        if (!(dp_ < 0x1p-44) || !(ds_ < 0x1p-44)) ++failed;  // (a NaN fails)
        if (dp_ > worst_p) worst_p = dp_;
        if (ds_ > worst_s) worst_s = ds_;
        differ += s[(size_t)i] != hs;
    }
    const double res[3] = {worst_s, worst_p, (double)differ};
    for (int k = 0; k < nout && k < 3 && out != nullptr; ++k) out[k] = res[k];
    return failed;
}

}  // extern "C"
