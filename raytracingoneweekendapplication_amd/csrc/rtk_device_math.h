// rtk_device_math.h -- the few device helpers the traversal (rtk_trace.hip) and the frame-assembly kernels
// (rtk_frame.hip) both use: the three-component vector and the byte conversion of the reference's image writer -- and the
// f64 square root and reciprocal without their range scaling, with the guard that admits an operand to them.
#ifndef RTK_DEVICE_MATH_H
#define RTK_DEVICE_MATH_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rtk {

template <typename real>
struct V3 {
    real x, y, z;
};
#define RTK_DEV __device__ __forceinline__

template <typename real> RTK_DEV V3<real> mk(real a, real b, real c) { return V3<real>{a, b, c}; }
template <typename real> RTK_DEV V3<real> operator+(V3<real> a, V3<real> b) { return V3<real>{a.x + b.x, a.y + b.y, a.z + b.z}; }
template <typename real> RTK_DEV V3<real> scale(real t, V3<real> a) { return V3<real>{t * a.x, t * a.y, t * a.z}; }

// ---- f64 square root and reciprocal without the range scaling ---------------------------------------------------------
// The compiler expands __builtin_sqrt(double) and 1.0 / x into a hardware seed, a fixed refinement and instructions that
// only serve operands at the ends of the exponent range.  The two functions below are those expansions, read from the ISA
// of the lean MIXED f64 render kernel, with exactly those instructions left out; every remaining operation is the same
// one on the same operands, so wherever the dropped instructions do nothing the result is the same bits.
//
// sqrt, as compiled (18 instructions):
//     v_cmp_gt_f64 2^-767, x ; v_cndmask k, 0, 256 ; v_ldexp_f64 X, x, k          X = x * 2^256 when x < 2^-767, else x
//     v_rsq_f64 y, X
//     g = X * y ; h = y * 0.5 ; r = fma(-h, g, 0.5) ; g = fma(g, r, g) ; d = fma(-g, g, X) ; h = fma(h, r, h)
//     g = fma(d, h, g) ; d = fma(-g, g, X) ; g = fma(d, h, g)
//     v_cndmask k, 0, -128 ; v_ldexp_f64 g, g, k                                   g * 2^-128 when X was scaled
//     v_cmp_class_f64 X, {+-0, +inf} ; 2 x v_cndmask                               X itself when it is +-0 or +inf
// Inert for 2^-767 <= x < +inf: k = 0 both times (ldexp by 0 returns its operand) and the class test fails.
RTK_DEV double sqrt_inrange(double x) {
    const double y = __builtin_amdgcn_rsq(x);
    double g = x * y;
    double h = y * 0.5;
    const double r = __builtin_fma(-h, g, 0.5);
    g = __builtin_fma(g, r, g);
    double d = __builtin_fma(-g, g, x);
    h = __builtin_fma(h, r, h);
    g = __builtin_fma(d, h, g);
    d = __builtin_fma(-g, g, x);
    return __builtin_fma(d, h, g);
}
// 1.0 / x, as compiled (11 instructions):
//     v_div_scale_f64 D, x, x, 1.0 ; v_rcp_f64 y, D
//     e = fma(-D, y, 1.0) ; y = fma(y, e, y) ; e = fma(-D, y, 1.0) ; y = fma(y, e, y)
//     v_div_scale_f64 N, vcc, 1.0, x, 1.0 ; q = N * y ; r = fma(-D, q, N)
//     v_div_fmas_f64 q, r, y, q                                                    fma(r, y, q), times 2^64 when vcc
//     v_div_fixup_f64 q, q, x, 1.0
// The ISA manual's V_DIV_SCALE_F64 (S0 = the operand returned, S1 = denominator, S2 = numerator) leaves S0 as it is and vcc
// clear unless one of these holds: S1 or S2 is zero; exponent(S2) - exponent(S1) >= 768; S1 is denormal; 1 / S1 is denormal;
// S2 / S1 is denormal; exponent(S2) <= 53.  With S2 = 1.0 that is: unscaled for every normal x with 2^-767 <= |x| <= 2^1022.
// V_DIV_FIXUP_F64 replaces the quotient only for a NaN, infinite or zero numerator or denominator and for a quotient below the
// denormal range (exponent(S2) - exponent(S1) < -1075); otherwise it returns |S0| with the sign of S1 xor S2, which S0
// already has.  So inside that range D = x, N = 1.0, q = 1.0 * y = y (exact) and the two
// last instructions return fma(r, y, q).
RTK_DEV double rcp_inrange(double x) {
    double y = __builtin_amdgcn_rcp(x);
    double e = __builtin_fma(-x, y, 1.0);
    y = __builtin_fma(y, e, y);
    e = __builtin_fma(-x, y, 1.0);
    y = __builtin_fma(y, e, y);
    const double r = __builtin_fma(-x, y, 1.0);
    return __builtin_fma(r, y, y);
}
// The range both short forms are admitted on: 2^-510 <= x < 2^510 -- positive, normal, finite, far inside both ranges above,
// and closed under what the sites do next (the square root of an admitted x is admitted, so unit_vector needs one test for
// its sqrt and its 1/t).  One unsigned compare on the high word: the biased exponents 513 .. 1532 with a clear sign bit;
// zeros, denormals, negatives, infinities and NaNs all land outside.
RTK_DEV bool inrange_f64(double x) {
    const uint32_t hi = uint32_t(__builtin_bit_cast(unsigned long long, x) >> 32);
    return hi - 0x20100000u < 0x3FC00000u;
}
// The guard of a site: every ACTIVE lane's operand is admitted (a scalar branch; the wave takes the full expansion together
// when any lane is out of range, so the fast path carries no per-lane select).
RTK_DEV bool wave_all_inrange(double x) { return __builtin_amdgcn_ballot_w64(!inrange_f64(x)) == 0ull; }
// The full expansions a failed guard falls back to.  In the product they are inlined into a cold block behind the scalar branch
// (a call would cost the kernels scratch); the instruction-cost probes (tools/isa_costs.py) count what a step EXECUTES, so
// there the fall-backs are real functions outside the probe's body.
#ifdef RTK_ISA_PROBES
#define RTK_COLD __device__ __attribute__((noinline))
#else
#define RTK_COLD RTK_DEV
#endif
RTK_COLD double sqrt_full(double x) { return __builtin_sqrt(x); }
RTK_COLD double rcp_full(double x) { return 1.0 / x; }
RTK_COLD double rcp_sqrt_full(double x) { return 1.0 / __builtin_sqrt(x); }
// A site's square root / reciprocal.  SHORT: the lean MIXED f64 render kernel and the f64 lane-per-ray kernels (through
// which the known-answer tests reach these functions); everything else, and float, compiles to today's expansion.
template <bool SHORT>
RTK_DEV double sqrt_site(double x) {
    if constexpr (SHORT) {
        if (__builtin_expect(wave_all_inrange(x), 1)) return sqrt_inrange(x);
        return sqrt_full(x);
    }
    return __builtin_sqrt(x);
}
template <bool SHORT> RTK_DEV float sqrt_site(float x) { return __builtin_sqrtf(x); }
template <bool SHORT>
RTK_DEV double rcp_site(double x) {
    if constexpr (SHORT) {
        if (__builtin_expect(wave_all_inrange(x), 1)) return rcp_inrange(x);
        return rcp_full(x);
    }
    return 1.0 / x;
}
template <bool SHORT> RTK_DEV float rcp_site(float x) { return 1.0f / x; }
// 1 / sqrt(x) as vec3.h's unit_vector and random_unit_vector compute it (a square root, then a division of 1 by it).
template <bool SHORT>
RTK_DEV double rcp_sqrt_site(double x) {
    if constexpr (SHORT) {
        if (__builtin_expect(wave_all_inrange(x), 1)) return rcp_inrange(sqrt_inrange(x));  // 2^-255 <= sqrt(x) < 2^255: admitted
        return rcp_sqrt_full(x);
    }
    return 1.0 / __builtin_sqrt(x);
}
template <bool SHORT> RTK_DEV float rcp_sqrt_site(float x) { return 1.0f / __builtin_sqrtf(x); }

RTK_DEV uint8_t to_byte(double x) {  // Camera.txt:29-34,77-83
    double g = x > 0 ? __builtin_sqrt(x) : 0.0;
    g = g < 0.000 ? 0.000 : (g > 0.999 ? 0.999 : g);
    return uint8_t(int(255.999 * g));
}

}  // namespace rtk

#endif  // RTK_DEVICE_MATH_H
