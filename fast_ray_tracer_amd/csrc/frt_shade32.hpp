// frt-mi355x fast shading mode (FRT_PRECISION=fast32): one light point's terms of lighting_microfacet
// (renderer.c:895-979) in binary32, and the same terms in binary64 for the lanes that leave binary32's safe range.
//
// What is binary32: per light point, diff = (c - over_point) + offset (c: the light's centroid; c - over_point is
// formed in binary64 once per node and light and rounded; the offsets are the light's points minus c, rounded at
// upload), m2 = diff.diff, 1 / |diff|, l.n, l.e, the half vector's terms n.h, e.h, l.h, (n.h)^Ns, the Fresnel
// factor (1 - l.h)^5 and the BRDF quotient. What is not: the three running sums (each term is converted and added
// in binary64: 64 binary32 additions would cost more accuracy than all of the above together) and everything per
// node (shade_node32, frt_engine.hip).
//
// Accuracy assumed of the hardware estimates (u = 2^-24): v_rsq_f32, v_rcp_f32, v_log_f32, v_exp_f32 are each
// within 2 ulp (the ISA documents 1 ulp) for normal operands and results; none of them sees a denormal operand on
// the binary32 path (the range checks below), and nothing depends on whether denormal results are flushed.
//
// Error model for |c - over_point| <= 16, |diff| >= 1:
//   diff     each component within 16u / |diff| of |diff| (the rounding of c - over_point, of the offset, of the sum)
//   l.n      32u absolute: the cancellation above, 4u for the dot product, a few ulps for the reciprocal root
//            (frt_shade32_selftest gates this bound)
//   (n.h)^Ns exp2(Ns log2(n.h)). The quotient n.h = (l.n + n.e) / |l + e| carries ~8u relative, which the exponent
//            would multiply by 1.44 Ns (1e-3 of a highlight at Ns = 2000: measured on the goldens). Where the power
//            matters n.h is near 1, so for n.h >= 0.9 the logarithm comes from the sine instead of the cosine:
//            (n.h)^2 = n.n - s2, s2 = |n x (l + e)|^2 / |l + e|^2 (Lagrange's identity; n.n: the rounded normal's own
//            squared length). The cross product's components are differences of rounded products: s2 is within
//            ~8u sin(t) + 4u s2 absolute (t: the angle between n and the half vector), and n.n - s2 rounds to u / 2, so
//            log2(n.h) = log2(n.n - s2) / 2 is within 0.72 (8u sin(t) + 4u s2 + u) absolute. A highlight's points have
//            Ns sin(t)^2 / 2 of order 10 at most, so the power is within about Ns 0.5 (6 sqrt(20 / Ns) + 1) u relative:
//            4e-5 at Ns = 200, 1e-4 at Ns = 2000 (instead of 1e-4 and 1e-3).
//   quotient a few ulps
//
// A lane takes the binary64 evaluation of a point (point_term64: the arithmetic of shade_node's term(), shared-term
// vectors and factored sums, without the tail skip, on the point c + offset) when
//   m2 outside [2^-40, 2^40]          the reciprocal root or m2 r r would leave the normal range (NaN included)
//   |l.n| < 2^-17                     the sign of l.n decides whether the point contributes at all (renderer.c:931) and
//                                     the binary32 value is good to 32u = 2^-19: decided in binary64; this also bounds
//                                     the BRDF denominator 4 (n.l)(n.e)(e.h) away from underflow
//   n.e outside [2^-20, 4], e.e or n.n outside [1/4, 4], Ns outside [0, 2^20] or not finite   (per node: spec_ok)
//   |l + e|^2 outside [2^-6, 8]       the half vector cancels (l = -e)
// behind a wave ballot; each lane's decision and value are its own (no value depends on the other lanes of the wave).
// Within those ranges every binary32 intermediate is a normal number or an exact zero below 2^63, and above 2^-64
// except the power, whose underflow to zero is the correct rounding of a term below 2^-126.
#pragma once

#include "frt_math.hpp"

namespace frt {

struct ShadeSums {
    double ldn, b, fb;  // sum of l.n, of the BRDF factor b, of F b (binary64 in both modes)
};

// a (node, light) pair's constants of the point loop
struct Point64 {
    double base[3];  // c - over_point
    double n[3], e[3];
    double ned, ee, ns, cdist;  // n.e, e.e, Ns, (Ns + 2) / 2 pi
};
struct Point32 {
    float base[3], n[3], e[3];
    float ned, ee, ns, cdist;
    float nn;       // the rounded normal's squared length (n[] . n[], formed in binary64)
    float skip_c;   // the specular tail test's constant (shade_node); +inf: never skipped
    bool spec_ok;   // the node's n.e, e.e and Ns are inside the binary32 ranges above
    bool diffuse, spec;  // include_diffuse, include_spec_highlight
};

constexpr float kLdnMin32 = 0x1p-17f;

__device__ __forceinline__ double fma3(const double* a, const double* b) {
    return __builtin_fma(a[0], b[0], __builtin_fma(a[1], b[1], a[2] * b[2]));
}
__device__ __forceinline__ float fma3f(const float* a, const float* b) {
    return __builtin_fmaf(a[0], b[0], __builtin_fmaf(a[1], b[1], a[2] * b[2]));
}

__device__ __forceinline__ Point32 point32_of(const Point64& Q, float skip_c, bool diffuse, bool spec) {
    Point32 P;
    for (int k = 0; k < 3; ++k) {
        P.base[k] = (float)Q.base[k];
        P.n[k] = (float)Q.n[k];
        P.e[k] = (float)Q.e[k];
    }
    P.ned = (float)Q.ned;
    P.ee = (float)Q.ee;
    P.ns = (float)Q.ns;
    P.cdist = (float)Q.cdist;
    P.nn = (float)((double)P.n[0] * P.n[0] + (double)P.n[1] * P.n[1] + (double)P.n[2] * P.n[2]);
    P.skip_c = skip_c;
    P.spec_ok = Q.ned >= 0x1p-20 && Q.ned <= 4.0 && Q.ee >= 0.25 && Q.ee <= 4.0 && P.nn >= 0.25f && P.nn <= 4.0f &&
                Q.ns >= 0.0 && Q.ns <= 0x1p20;
    P.diffuse = diffuse;
    P.spec = spec;
    return P;
}

// one light point in binary64 (off: the point minus the light's centroid)
__device__ __forceinline__ void point_term64(const Point64& Q, const double* off, bool diffuse, bool spec,
                                             ShadeSums& s) {
    const double diff[3] = {Q.base[0] + off[0], Q.base[1] + off[1], Q.base[2] + off[2]};
    const double m2 = fma3(diff, diff);
    const double rl = rsqrt_shade(m2);
    const double ldn = fma3(diff, Q.n) * rl;
    if (!(ldn >= 0.0)) return;
    if (diffuse) s.ldn += ldn;
    if (!spec) return;
    const double el = fma3(diff, Q.e) * rl, ll = (m2 * rl) * rl;
    const double rh = rsqrt_shade(ll + 2.0 * el + Q.ee);
    const double ndh = fmax(0.0, (ldn + Q.ned) * rh);
    const double edh = fmax(0.0, (el + Q.ee) * rh);
    const double ldh = (ll + el) * rh;
    const double dist_term = pow_ns(ndh, Q.ns) * Q.cdist;
    const double om = 1.0 - ldh, om2 = om * om;
    const double factor = om2 * om2 * om;
    const double brdf = brdf_shade(dist_term, ndh, edh, ldn, Q.ned);
    s.b += brdf;
    s.fb += factor * brdf;
}

// one light point in binary32 (Q: the same constants in binary64 for the lanes out of range)
__device__ __forceinline__ void point_term32(const Point32& P, const Point64& Q, const float* off, ShadeSums& s) {
    const float d[3] = {P.base[0] + off[0], P.base[1] + off[1], P.base[2] + off[2]};
    const float m2 = fma3f(d, d);
    const float rl = __builtin_amdgcn_rsqf(m2);
    const float ldn = fma3f(d, P.n) * rl;
    // (comparisons written so that a NaN lands on the binary64 side)
    bool slow = !(m2 >= 0x1p-40f && m2 <= 0x1p40f && __builtin_fabsf(ldn) >= kLdnMin32);
    const bool front = ldn > 0.0f;
    float lg = 0.0f, ndh = 0.0f, edh = 0.0f, ldh = 0.0f;
    bool tail = false;
    if (P.spec) {
        const float el = fma3f(d, P.e) * rl, ll = (m2 * rl) * rl;
        const float h2 = __builtin_fmaf(2.0f, el, ll) + P.ee;
        const float rh = __builtin_amdgcn_rsqf(h2);
        slow = slow || (front && !(P.spec_ok && h2 >= 0x1p-6f && h2 <= 8.0f));
        ndh = __builtin_fmaxf(0.0f, (ldn + P.ned) * rh);
        edh = __builtin_fmaxf(0.0f, (el + P.ee) * rh);
        ldh = (ll + el) * rh;
        lg = __builtin_amdgcn_logf(ndh);
        // shade_node's specular tail test (the point's specular terms below 2^-62 of its diffuse one)
        tail = front && P.ns * lg - 2.0f * __builtin_amdgcn_logf(ldn) + P.skip_c < 0.0f;
    }
    const bool lit = front && !slow;
    if (P.diffuse && lit) s.ldn += (double)ldn;
    const bool shine = P.spec && lit && !tail;
    if (__ballot(shine) != 0ull) {  // (skipped where no lane needs it; a lane's value is its own)
        // log2(n.h) from the sine where n.h is near 1 (the error model above): s2 = |n x (l + e)|^2 / |l + e|^2
        const float l[3] = {d[0] * rl, d[1] * rl, d[2] * rl};
        const float v[3] = {l[0] + P.e[0], l[1] + P.e[1], l[2] + P.e[2]};
        const float c[3] = {__builtin_fmaf(P.n[1], v[2], -(P.n[2] * v[1])), __builtin_fmaf(P.n[2], v[0], -(P.n[0] * v[2])),
                            __builtin_fmaf(P.n[0], v[1], -(P.n[1] * v[0]))};
        const float s2 = fma3f(c, c) * __builtin_amdgcn_rcpf(fma3f(v, v));
        const float lgs = 0.5f * __builtin_amdgcn_logf(P.nn - s2);
        const float dist_term = __builtin_amdgcn_exp2f(P.ns * (ndh >= 0.9f ? lgs : lg)) * P.cdist;
        const float om = 1.0f - ldh, om2 = om * om;
        const float factor = om2 * om2 * om;
        const float g2 = 2.0f * ndh;
        const float a = dist_term * __builtin_fminf(edh, __builtin_fminf(g2 * P.ned, g2 * ldn));
        const float q = a * __builtin_amdgcn_rcpf(edh * (4.0f * ldn * P.ned));
        if (shine) {
            s.b += (double)q;
            s.fb += (double)(factor * q);
        }
    }
    if (__builtin_expect(__ballot(slow) != 0ull, 0)) {
        if (slow) {
            const double o64[3] = {(double)off[0], (double)off[1], (double)off[2]};
            point_term64(Q, o64, P.diffuse, P.spec, s);
        }
    }
}

}  // namespace frt
