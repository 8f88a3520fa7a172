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
        for (auto& ev : a->ev) {
            if (ev != nullptr) (void)hipEventDestroy(ev);
        }
    }
    (void)hipGetLastError();
    delete a;
}

}  // extern "C"
