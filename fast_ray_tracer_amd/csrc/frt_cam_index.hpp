// frt-mi355x: the 32-bit index arithmetic of a batch's level 0 (frt_camera.hpp camera_sample): division by a
// run-time constant as a multiply and shifts, the constants' host-side derivation, and the rule that says when a
// batch may use them. Plain C++ with no HIP in it, so that a host program can include it on its own
// (tests/test_cam_index.py does); the engine and the hiprtc source of frt_jit_trace read the same text.
#pragma once

#ifndef __HIPCC_RTC__
#include <stdint.h>
#endif

#if defined(__HIPCC__) || defined(__HIPCC_RTC__)
#define FRT_CAM_HD __host__ __device__
#else
#define FRT_CAM_HD
#endif

namespace frt {

// n / d for every 32-bit n and a divisor 1 <= d < 2^32 known on the host: with shift = ceil(log2 d) and
// M = ceil(2^(32 + shift) / d), floor(n * M / 2^(32 + shift)) == n / d exactly (the shadow kernels' rule,
// frt_jit_rt.hpp; Granlund & Montgomery 1994, theorem 4.2 with N = 32). M has 33 bits, bit 32 always set: magic
// holds the low 32, and the quotient is taken as (t + n) >> shift with t = mulhi(magic, n), the 33-bit sum formed
// as t + ((n - t) >> 1) so that it stays in 32 bits (shift 0, d == 1: no halving).
struct DivMagic {
    uint32_t magic, shift;
};

FRT_CAM_HD inline DivMagic div_magic(uint32_t d) {
    uint32_t shift = 0;
    while (shift < 32 && ((uint64_t)1 << shift) < (uint64_t)d) ++shift;
    // M - 2^32 = floor(2^32 * (2^shift - d) / d) + 1: the ceiling where d is no power of two (the quotient is then
    // no integer); for d == 2^shift it gives 1 where the ceiling is 0, and mulhi(1, n) == mulhi(0, n) == 0
    const uint64_t m = (((((uint64_t)1 << shift) - (uint64_t)d) << 32) / (uint64_t)d) + 1;
    return DivMagic{(uint32_t)m, shift};
}

FRT_CAM_HD inline uint32_t magic_div(uint32_t n, uint32_t magic, uint32_t shift) {
    const uint32_t t = (uint32_t)(((uint64_t)magic * (uint64_t)n) >> 32);
    const uint32_t s1 = (shift + 31u) >> 5;  // min(shift, 1) for shift <= 32, in scalar arithmetic on the device
    return (t + ((n - t) >> s1)) >> (shift - s1);
}

// n % d from the quotient: one 32-bit multiply-subtract
FRT_CAM_HD inline uint32_t magic_rem(uint32_t n, uint32_t q, uint32_t d) { return n - q * d; }

// Whether a batch's camera_sample may index in 32 bits: its samples (the dividend of / spp) and its pixels, in
// render order from pixel_begin on (the dividend of / hsize), fit 32 bits unsigned, spp and hsize are below 2^31,
// and so is the frame row of its last pixel (column and row become doubles from 32-bit values).
FRT_CAM_HD inline bool cam_index_fits32(int64_t num_samples, int64_t pixel_begin, int64_t pixels, int64_t spp,
                                        int64_t hsize, int64_t row_begin, int64_t row_stride) {
    const int64_t u32 = 0xFFFFFFFFll, i31 = 0x7FFFFFFFll;
    if (num_samples < 0 || num_samples > u32) return false;
    if (pixel_begin < 0 || pixel_begin > u32 || pixels < 1 || pixels > u32 || pixel_begin + pixels > u32) return false;
    if (spp < 1 || spp > i31 || hsize < 1 || hsize > i31) return false;
    if (row_begin < 0 || row_begin > i31 || row_stride < 1 || row_stride > i31) return false;
    return row_begin + ((pixel_begin + pixels - 1) / hsize) * row_stride <= i31;
}

}  // namespace frt
