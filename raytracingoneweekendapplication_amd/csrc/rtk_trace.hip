// rtk_trace.hip -- the per-pixel sample loop of camera::render() as one CDNA4
// (gfx950) kernel family.  Hand-written HIP, wave64, no MFMA (branchy traversal,
// not a contraction), no CUDA idioms.
//
// Replaces, on the device:
//   render_rows λ   Camera.txt:65-93     rtk_render_kernel (one lane = one pixel of an 8x8 tile = one wave)
//   get_ray         Camera.txt:177-200   make_primary_ray
//   ray_color       Camera.txt:203-238   the bounce loop in trace_sample (iterative: radiance = Σ throughput·emission)
//   world.hit       bvh.h:64-72 &c.      closest_hit: executes the linear traversal program (rtk_device_layout.h)
//   *.hit           sphere.h:32-58, quad.h:29-73, triangle.h:65-122, constant_medium.h:20-53
//   scatter/emitted material.h           shade
//   texture::value  texture.h, perlin.h  texture_value, perlin_noise
//
// Parity rules kept in this file (the CPU oracle is compared bit-for-bit where the
// maths allows): same operation order as the reference inside every formula,
// v/t computed as (1/t)*v (vec3.h:91-93), no FMA contraction (the file is built
// with -ffp-contract=off), RNG draws in the reference's order including g++'s
// right-to-left argument evaluation, and the reference's visiting order in the
// BVH (left then right, both always).  The hit record is DEFERRED: traversal
// keeps only (t, winning op); position, normal and uv are computed once per
// segment from the winning primitive, which gives the same values because they
// are pure functions of (ray, t, primitive).
//
// Frame assembly -- partial sums -> images and progressive-session state -- is rtk_frame.hip; the two files share
// rtk_device_math.h (V3, mk, operator+, scale, to_byte) and nothing else.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "rtk.h"
#include "rtk_device_layout.h"
#include "rtk_device_math.h"
#include "rtk_gather_rule.h"
#include "rtk_image_pass.h"
#include "rtk_grid_plan.h"
#include "rtk_kernel_choice.h"
#include "rtk_lds_plan.h"
#include "rtk_trace.h"

namespace rtk {

// ------------------------------------------------------------------ math -----
// (V3, RTK_DEV, mk, operator+ and scale: rtk_device_math.h)
template <typename real> RTK_DEV V3<real> ld3(const real* p) { return V3<real>{p[0], p[1], p[2]}; }
template <typename real> RTK_DEV V3<real> operator-(V3<real> a) { return V3<real>{-a.x, -a.y, -a.z}; }
template <typename real> RTK_DEV V3<real> operator-(V3<real> a, V3<real> b) { return V3<real>{a.x - b.x, a.y - b.y, a.z - b.z}; }
template <typename real> RTK_DEV V3<real> operator*(V3<real> a, V3<real> b) { return V3<real>{a.x * b.x, a.y * b.y, a.z * b.z}; }
template <typename real> RTK_DEV V3<real> divide(V3<real> a, real t) { return scale(real(1) / t, a); }  // vec3.h:91-93
template <typename real> RTK_DEV real dot(V3<real> a, V3<real> b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
template <typename real> RTK_DEV V3<real> cross(V3<real> a, V3<real> b) {
    return V3<real>{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
template <typename real> RTK_DEV real length_squared(V3<real> a) { return a.x * a.x + a.y * a.y + a.z * a.z; }

RTK_DEV double rt_sqrt(double x) { return __builtin_sqrt(x); }
RTK_DEV float rt_sqrt(float x) { return __builtin_sqrtf(x); }
RTK_DEV double rt_fabs(double x) { return __builtin_fabs(x); }
RTK_DEV float rt_fabs(float x) { return __builtin_fabsf(x); }
RTK_DEV double rt_fmin(double a, double b) { return __builtin_fmin(a, b); }
RTK_DEV float rt_fmin(float a, float b) { return __builtin_fminf(a, b); }
RTK_DEV double rt_fmax(double a, double b) { return __builtin_fmax(a, b); }
RTK_DEV float rt_fmax(float a, float b) { return __builtin_fmaxf(a, b); }
RTK_DEV double rt_floor(double x) { return __builtin_floor(x); }
RTK_DEV float rt_floor(float x) { return __builtin_floorf(x); }
RTK_DEV double rt_round(double x) { return __builtin_round(x); }
RTK_DEV float rt_round(float x) { return __builtin_roundf(x); }
RTK_DEV double rt_pow(double x, double y) { return pow(x, y); }
RTK_DEV float rt_pow(float x, float y) { return powf(x, y); }
RTK_DEV double rt_log(double x) { return log(x); }
RTK_DEV float rt_log(float x) { return logf(x); }
RTK_DEV double rt_sin(double x) { return sin(x); }
RTK_DEV float rt_sin(float x) { return sinf(x); }
RTK_DEV double rt_acos(double x) { return acos(x); }
RTK_DEV float rt_acos(float x) { return acosf(x); }
RTK_DEV double rt_atan2(double y, double x) { return atan2(y, x); }
RTK_DEV float rt_atan2(float y, float x) { return atan2f(y, x); }

template <typename real> RTK_DEV real real_inf() { return real(__builtin_huge_val()); }
// Round 3: libm-heavy f64 code kept OUT OF LINE (see sphere_uv below for the reasoning and the first two).
// Measured and left inline: perlin::noise (43.7 vs 34.0 ms) and texture::value as a whole (864 B of scratch).
#define RTK_NOINLINE __device__ __attribute__((noinline))
// pow (the specular material): C5 38.87 -> 38.25 ms at 32 spp
template <typename real> RTK_NOINLINE real call_pow(real x, real y) { return rt_pow(x, y); }
// log (constant_medium's scatter distance, twice per segment in book 2): 38.87 -> 35.72; both: 33.98
template <typename real> RTK_NOINLINE real call_log(real x) { return rt_log(x); }

// v_min/v_max as single instructions.  __builtin_fmin/fmax are IEEE minnum/maxnum, for which the
// compiler first canonicalises every operand it cannot prove quiet (an extra v_max x,x per use).
// Operands here are results of arithmetic or interval ends, never signalling NaNs; a quiet NaN
// operand is dropped exactly as minnum/maxnum drop it.
RTK_DEV double raw_min(double a, double b) { double r; asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
RTK_DEV double raw_max(double a, double b) { double r; asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
RTK_DEV float raw_min(float a, float b) { float r; asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
RTK_DEV float raw_max(float a, float b) { float r; asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
RTK_DEV float raw_max3(float a, float b, float c) { float r; asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
RTK_DEV float raw_min3(float a, float b, float c) { float r; asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
// (SHORT: see rtk_device_math.h sqrt_site; one guard on |a|^2 serves the square root and the division)
template <bool SHORT = false, typename real> RTK_DEV V3<real> unit_vector(V3<real> a) { return scale(rcp_sqrt_site<SHORT>(length_squared(a)), a); }
template <typename real> RTK_DEV bool near_zero(V3<real> a) {
    const real s = real(1e-8);
    return rt_fabs(a.x) < s && rt_fabs(a.y) < s && rt_fabs(a.z) < s;
}
// x^5 for Schlick's approximation (material.h:73: pow((1 - cosine), 5)).  double: the correctly rounded value, from products
// carried as (value, rounding error) pairs -- x^2 = x2 + e2 exactly (one fused multiply-add recovers the error), x^4 = x4 + e4,
// x^5 = x5 + e5 to ~2^-100, so the final sum rounds like the exact power (0 mismatches against exact rational arithmetic in
// 2e5 arguments, tests/test_schlick_power.py).  float (statistical parity only): three plain products.
RTK_DEV double pow5(double x) {
    const double x2 = x * x, e2 = __builtin_fma(x, x, -x2);
    const double x4 = x2 * x2, e4 = __builtin_fma(x2, x2, -x4) + 2.0 * (x2 * e2);
    const double x5 = x4 * x, e5 = __builtin_fma(x4, x, -x5) + e4 * x;
    return x5 + e5;
}
RTK_DEV float pow5(float x) {
    const float x2 = x * x;
    return x2 * x2 * x;
}
template <typename real> RTK_DEV V3<real> reflect(V3<real> v, V3<real> n) { return v - scale(real(2) * dot(v, n), n); }  // vec3.h:125-127
template <bool SHORT = false, typename real> RTK_DEV V3<real> refract(V3<real> uv, V3<real> n, real eta) {             // vec3.h:128-133
    real cos_theta = rt_fmin(dot(-uv, n), real(1));
    V3<real> perp = scale(eta, uv + scale(cos_theta, n));
    // (SHORT: |1 - |perp|^2| is exactly 0 at the critical angle and can be NaN -- guarded)
    V3<real> par = scale(-sqrt_site<SHORT>(rt_fabs(real(1) - length_squared(perp))), n);
    return perp + par;
}

// ------------------------------------------------------------------ counters --
template <bool COUNT>
struct Counters {
    uint32_t c[C_COUNT];
    RTK_DEV void clear() {
#pragma unroll
        for (int k = 0; k < C_COUNT; k++) c[k] = 0;
    }
    RTK_DEV void inc(int slot, uint32_t n = 1) { c[slot] += n; }
};
template <>
struct Counters<false> {
    RTK_DEV void clear() {}
    RTK_DEV void inc(int, uint32_t = 1) {}
};

// ------------------------------------------------------------------ RNG -------
// Per-lane PCG-RXS-M-XS-32: 32-bit state, one v_mul_lo_u32 for the LCG step and
// one for the output permutation, no 64-bit multiply (gfx950 has no fast one).
// The stream of a sample is seeded by hashing (seed, sample, pixel), so it does
// not depend on lane, tile, launch geometry or GPU count.
RTK_DEV uint32_t pcg_hash(uint32_t v) {
    uint32_t st = v * 747796405u + 2891336453u;
    uint32_t w = ((st >> ((st >> 28u) + 4u)) ^ st) * 277803737u;
    return (w >> 22u) ^ w;
}
template <typename real, bool COUNT>
RTK_DEV real rnd(uint32_t& s, Counters<COUNT>& cnt) {
    uint32_t old = s;
    s = old * 747796405u + 2891336453u;
    uint32_t w = ((old >> ((old >> 28u) + 4u)) ^ old) * 277803737u;
    cnt.inc(C_RNG);
    return real(((w >> 22u) ^ w) >> 8) * real(1.0 / 16777216.0);
}
// random_double(-1, 1) = -1 + 2 * random_double() (rtweekend.h) of the next draw, without a rounding anywhere: a draw is
// v * 2^-24 with v a 24-bit integer, so 2 * draw and -1 + 2 * draw are exact (multiples of 2^-23 in [-1, 1)), and the same
// number is (v - 2^23) * 2^-23 -- an integer subtraction, a conversion and one exact scaling instead of a conversion and
// three floating-point operations.  Same bits in double and in float (24 significant bits suffice), zero included (+0).
template <typename real, bool COUNT>
RTK_DEV real rnd_pm1(uint32_t& s, Counters<COUNT>& cnt) {
    uint32_t old = s;
    s = old * 747796405u + 2891336453u;
    uint32_t w = ((old >> ((old >> 28u) + 4u)) ^ old) * 277803737u;
    cnt.inc(C_RNG);
    return real(int32_t(((w >> 22u) ^ w) >> 8) - 8388608) * real(1.0 / 8388608.0);
}
// vec3.h:107-115 -- always accepts; components drawn z, y, x.
// (SHORT: the components are multiples of 2^-23 in [-1, 1), so |p|^2 is 0 or within 2^-46 .. 3 -- admitted unless the draw is
// (0, 0, 0), which must still give the reference's 0 * (1 / 0); the guard sends that wave to the full expansion.  With this
// generator it never does: of the 2^32 states 256 draw a zero next and none draws two in a row.)
template <typename real, bool SHORT = false, bool COUNT>
RTK_DEV V3<real> random_unit_vector(uint32_t& s, Counters<COUNT>& cnt) {
    real c = rnd_pm1<real>(s, cnt);
    real b = rnd_pm1<real>(s, cnt);
    real a = rnd_pm1<real>(s, cnt);
    V3<real> p = mk(a, b, c);
    return scale(rcp_sqrt_site<SHORT>(length_squared(p)), p);
}

// ------------------------------------------------------------------ rays ------
// Object-space ray for a chain of instance transforms (hittable.h:46-49,101-116).
template <uint32_t FEAT>
constexpr bool kChainPrefetch = (FEAT & ~uint32_t(F_FMA_BOX | F_F32_BOX | F_LDS_BOXES)) == kFeatAll || (FEAT & ~uint32_t(F_FMA_BOX | F_F32_BOX | F_MATTE)) == kFeatQuadBox;
// The constants of the first two steps of a chain are requested together, in front of the branches that pick them: walking
// the record step by step costs a dependent read per branch (count, is_rotate[k], that step's constants), and a chain
// switch is nothing but those reads and two dozen operations.  Longer chains (kMaxChain = 4) finish in the loop.
// PREFETCH: the full-feature kernels (C5 44.4 -> 43.6 ms) and, since round 3, the quad/box kernels: with the deep hierarchy of
// round 2 the 36 B of scratch it costs them outweighed it (C3 26.2 -> 26.5 ms at 100 spp); on the flattened programs a chain
// switch is a larger share of the frame and it pays (21.70 -> 21.25 ms).  (Reading the staged chains through a pointer typed
// as LDS -- ds_read instead of the flat loads a generic pointer compiles to, 3.6 per Cornell sample -- was measured in round 3
// as well: 21.51 without the prefetch, 21.70 with it, C5 29.46 -> 29.80 ms: the register allocator's answer costs more than
// the cheaper loads save; removed.)
template <bool PREFETCH = false, typename real>
RTK_DEV void apply_chain(const ChainRec<real>* __restrict__ chains, uint32_t chain, V3<real> wo, V3<real> wd, V3<real>& o, V3<real>& d) {
    o = wo;
    d = wd;
    if (chain == 0) return;
    const ChainRec<real>& ch = chains[chain];
    const int n = ch.count;
    auto step = [&](int rotate, real a, real b, real c) {
        if (rotate) {
            const real sn = a, cs = b;
            o = mk((cs * o.x) - (sn * o.z), o.y, (sn * o.x) + (cs * o.z));
            d = mk((cs * d.x) - (sn * d.z), d.y, (sn * d.x) + (cs * d.z));
        } else {
            o = o - mk(a, b, c);
        }
    };
    int first = 0;
    if constexpr (PREFETCH) {
        const int r0 = ch.is_rotate[0], r1 = ch.is_rotate[1];
        const real a0 = ch.a[0], b0 = ch.b[0], c0 = ch.c[0], a1 = ch.a[1], b1 = ch.b[1], c1 = ch.c[1];
        if (n > 0) step(r0, a0, b0, c0);
        if (n > 1) step(r1, a1, b1, c1);
        first = 2;
    }
    for (int k = first; k < n; k++) step(ch.is_rotate[k], ch.a[k], ch.b[k], ch.c[k]);
}
// Hit point and normal back to world space (hittable.h:55,122-134), innermost first.
template <bool PREFETCH = false, typename real>
RTK_DEV void unapply_chain(const ChainRec<real>* __restrict__ chains, uint32_t chain, V3<real>& p, V3<real>& n) {
    if (chain == 0) return;
    const ChainRec<real>& ch = chains[chain];
    const int count = ch.count;
    auto step = [&](int rotate, real a, real b, real c) {
        if (rotate) {
            const real sn = a, cs = b;
            p = mk((cs * p.x) + (sn * p.z), p.y, (-sn * p.x) + (cs * p.z));
            n = mk((cs * n.x) + (sn * n.z), n.y, (-sn * n.x) + (cs * n.z));
        } else {
            p = p + mk(a, b, c);
        }
    };
    if constexpr (PREFETCH) {
        const int r0 = ch.is_rotate[0], r1 = ch.is_rotate[1];
        const real a0 = ch.a[0], b0 = ch.b[0], c0 = ch.c[0], a1 = ch.a[1], b1 = ch.b[1], c1 = ch.c[1];
        for (int k = count - 1; k >= 2; k--) step(ch.is_rotate[k], ch.a[k], ch.b[k], ch.c[k]);
        if (count > 1) step(r1, a1, b1, c1);
        if (count > 0) step(r0, a0, b0, c0);
    } else {
        for (int k = count - 1; k >= 0; k--) step(ch.is_rotate[k], ch.a[k], ch.b[k], ch.c[k]);
    }
}

// ------------------------------------------------------------------ traversal --
// aabb::hit (aabb.h:61-85).  The reference's per-axis early-outs reduce to one
// final comparison because tmin only grows and tmax only shrinks.
//
// EXACT_NAN = true is the literal form: per axis `t0 < t1` selects near/far (a NaN
// from 0*inf makes the comparison false, i.e. the reference's else-branch), and
// max/min then drop a NaN operand exactly as its `>`/`<` updates do.
// EXACT_NAN = false is for rays whose 1/d is finite and non-zero on every axis
// (Lane::box_kind == OP_BOX): then t0 and t1 cannot be NaN (bounds and origin are finite), and
// near = min(t0,t1), far = max(t0,t1) are the same values as the select -- five
// instructions fewer per axis.  Rays with a zero or infinite direction component
// take the exact form (the aabb known-answer vectors exercise them).
RTK_DEV double rt_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
RTK_DEV float rt_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
// Conservative-culling form, only for hierarchies whose boxes were grown by rtk_scene_optimize (F_FMA_BOX kernels,
// rtk_scene_upload_fast): t = b*inv - o*inv with one fused multiply-add per plane (o*inv hoisted per segment),
// 18 instead of 24 f64 operations per box.  Against (b - o)*inv the result moves by at most ~2^-52 |o*inv|, i.e.
// the plane by ~2^-52 |o| -- far inside the 2^-40 x scene-extent margin those boxes carry, so every box the exact
// test enters is entered here too and the closest hit (computed by the unchanged primitive tests) is the same.
// Rays with a zero or infinite direction component never come here (they take the literal form).
template <typename real>
RTK_DEV bool slab_test_fma(const Slot<real>& b, V3<real> oi, V3<real> inv, real tmin, real tmax) {
    const real t0x = rt_fma(b.v[0], inv.x, -oi.x), t1x = rt_fma(b.v[1], inv.x, -oi.x);
    const real t0y = rt_fma(b.v[2], inv.y, -oi.y), t1y = rt_fma(b.v[3], inv.y, -oi.y);
    const real t0z = rt_fma(b.v[4], inv.z, -oi.z), t1z = rt_fma(b.v[5], inv.z, -oi.z);
    const real nx = raw_min(t0x, t1x), fx = raw_max(t0x, t1x);
    const real ny = raw_min(t0y, t1y), fy = raw_max(t0y, t1y);
    const real nz = raw_min(t0z, t1z), fz = raw_max(t0z, t1z);
    tmin = raw_max(nz, raw_max(ny, raw_max(nx, tmin)));
    tmax = raw_min(fz, raw_min(fy, raw_min(fx, tmax)));
    return tmax > tmin;
}

template <bool EXACT_NAN, typename real>
RTK_DEV bool slab_test(const Slot<real>& b, V3<real> o, V3<real> inv, real tmin, real tmax) {
    const real t0x = (b.v[0] - o.x) * inv.x, t1x = (b.v[1] - o.x) * inv.x;
    const real t0y = (b.v[2] - o.y) * inv.y, t1y = (b.v[3] - o.y) * inv.y;
    const real t0z = (b.v[4] - o.z) * inv.z, t1z = (b.v[5] - o.z) * inv.z;
    real nx, fx, ny, fy, nz, fz;
    if constexpr (EXACT_NAN) {
        const bool lx = t0x < t1x, ly = t0y < t1y, lz = t0z < t1z;
        nx = lx ? t0x : t1x; fx = lx ? t1x : t0x;
        ny = ly ? t0y : t1y; fy = ly ? t1y : t0y;
        nz = lz ? t0z : t1z; fz = lz ? t1z : t0z;
    } else {
        nx = raw_min(t0x, t1x); fx = raw_max(t0x, t1x);
        ny = raw_min(t0y, t1y); fy = raw_max(t0y, t1y);
        nz = raw_min(t0z, t1z); fz = raw_max(t0z, t1z);
    }
    tmin = raw_max(nz, raw_max(ny, raw_max(nx, tmin)));
    tmax = raw_min(fz, raw_min(fy, raw_min(fx, tmax)));
    return tmax > tmin;
}

// Element e of a primitive whose reals are packed over consecutive slots ...
template <typename real, int E>
RTK_DEV real packed(const Slot<real>* rec) {
    return rec[E / Slot<real>::kReals].v[E % Slot<real>::kReals];
}
// ... or over the 16-byte units of a COMPACT record: elements 0..2 in the head, the header at bytes 24..31, element
// e >= 3 at byte 32 + 8 (e - 3) (rtk_device_layout.h).
template <typename real, int E>
RTK_DEV real packed(const Unit16* rec) {
    return real(reinterpret_cast<const double*>(rec)[E < 3 ? E : E + 1]);
}
// ... or over a quad record already in registers (COLD kernels: the whole 144-byte record is requested from memory at
// once, ahead of quad::hit's early-outs -- read field by field behind them it costs a second round trip to L2).
struct QuadRegs {
    double q[18];  // the record's nine units as doubles; q[3] holds the header's bits
};
template <typename real, int E>
RTK_DEV real packed(const QuadRegs* rec) {
    return real(rec->q[E < 3 ? E : E + 1]);
}
template <typename real, int E, typename Rec>
RTK_DEV V3<real> packed3(const Rec* rec) {
    return V3<real>{packed<real, E>(rec), packed<real, E + 1>(rec), packed<real, E + 2>(rec)};
}
// Header words, record length and the few fields whose position differs between the two layouts.
template <typename real> RTK_DEV uint32_t rec_kind_payload(const Slot<real>* rec) { return rec->kind_payload; }
template <typename real> RTK_DEV uint32_t rec_kind_payload(const Unit16* rec) { return rec[1].w[2]; }
template <typename real> RTK_DEV uint32_t rec_aux(const Slot<real>* rec) { return rec->aux; }
template <typename real> RTK_DEV uint32_t rec_aux(const Unit16* rec) { return rec[1].w[3]; }
template <typename real> RTK_DEV uint32_t rec_units(const Slot<real>*, uint32_t kind) { return uint32_t(slots_of<real>(kind)); }
template <typename real> RTK_DEV uint32_t rec_units(const Unit16*, uint32_t kind) { return uint32_t(compact_units(kind)); }
template <typename real> RTK_DEV V3<real> moving_dir(const Slot<real>* rec) { return mk(rec[1].v[0], rec[1].v[1], rec[1].v[2]); }   // centre2 - centre1 of a moving sphere
template <typename real> RTK_DEV V3<real> moving_dir(const Unit16* rec) { return packed3<real, 5>(rec); }

// n / a, correctly rounded, from y = RN(1/a) (computed once per segment by a true division): q0 = RN(n*y) is within
// one ulp of the quotient, r = n - a*q0 is exact in one fused multiply-add, and q0 + r*y rounds to RN(n/a)
// (Markstein's division step, the same correction the hardware division expansion ends with) -- three instructions
// instead of the ~25 of a full f64 division.  tests/test_division_identity.py checks the identity against `/` on
// 4e8 random operand pairs including all-ones significands.  (If q0 underflows the result is a denormal on either
// path and fails the `tmin < root` test below either way.)
template <typename real>
RTK_DEV real divide_by(real n, real a, real inv_a) {
    const real q0 = n * inv_a;
    const real r = rt_fma(-a, q0, n);
    return rt_fma(r, inv_a, q0);
}

// ---- exact ties (fast-order kernels) ---------------------------------------------------------------------------------
// Two primitives hit at EXACTLY the same distance: the reference resolves it by its visiting order -- a sphere accepts a
// root only strictly inside (tmin, closest so far) (sphere.h:44-48), so of two spheres the EARLIER one stays; a quad or a
// triangle accepts t == closest so far (quad.h:39, triangle.h:91), so the LATER one replaces whatever was there.  In a
// re-grouped hierarchy the visiting order is another one; the records carry their rank in the reference's order
// (SceneView::tie_rank, from rtk_node.c) and the same outcome is reproduced from the ranks: a quad/triangle beats a sphere,
// the higher rank wins among quads/triangles, the lower rank among spheres.  The tables are touched only when a tie
// actually occurs.  Unknown ranks (0, or no table) leave the decision to the visiting order, as before.
RTK_DEV bool is_strict_kind(uint32_t k) { return k == OP_SPHERE || k == OP_SPHERE_MOVING; }
RTK_DEV bool is_inclusive_kind(uint32_t k) { return k == OP_QUAD || k == OP_TRI; }
// a sphere's root equals the closest distance so far: does the sphere take the hit over?
RTK_DEV bool tie_sphere_wins(const uint32_t* __restrict__ ranks, uint32_t pc, uint32_t best_pc, uint32_t best_kind) {
    if (!ranks || best_pc == kNoHit || !is_strict_kind(best_kind)) return false;
    const uint32_t mine = ranks[pc], theirs = ranks[best_pc];
    return mine != 0 && theirs != 0 && mine < theirs;
}
// a quad's / triangle's t equals the closest distance so far (which its inclusive test admits): does it take the hit over?
RTK_DEV bool tie_inclusive_wins(const uint32_t* __restrict__ ranks, uint32_t pc, uint32_t best_pc, uint32_t best_kind) {
    if (!ranks || best_pc == kNoHit || !is_inclusive_kind(best_kind)) return true;
    const uint32_t mine = ranks[pc], theirs = ranks[best_pc];
    return mine == 0 || theirs == 0 || mine > theirs;
}

// sphere::hit up to the accepted root (sphere.h:32-49); cc = center.at(r.time()); a = d.d, inv_a = 1/a.
// TIE kernels: the interval test admits r == tmax as well -- the same two comparisons -- and only a root that was admitted
// is then checked for being that tie, which `wins_tie()` (tie_sphere_wins on the lane's state) decides; a tie that loses is
// a miss, exactly as in the reference, whose second root then lies beyond tmax.  The common path costs nothing extra.
// radius2 = radius * radius (sphere.h:37), either formed by the caller or -- lean MIXED program -- the same product stored at
// upload.  SHORT (rtk_device_math.h sqrt_site): the discriminant can be exactly 0 (a tangent ray) and nothing bounds it from
// below after the cancellation, so the site is guarded.
template <bool TIE = false, bool SHORT = false, typename real, typename F>
RTK_DEV bool sphere_root(V3<real> cc, real radius2, V3<real> o, V3<real> d, real a, real inv_a, real tmin, real tmax, real& root, F&& wins_tie) {
    V3<real> oc = cc - o;
    real h = dot(d, oc);
    real c = length_squared(oc) - radius2;
    real disc = h * h - a * c;
    if (disc < real(0)) return false;
    real sq = sqrt_site<SHORT>(disc);
    real r = divide_by(h - sq, a, inv_a);
    if constexpr (TIE) {
        if (!(tmin < r && r <= tmax)) {
            r = divide_by(h + sq, a, inv_a);
            if (!(tmin < r && r <= tmax)) return false;
        }
        if (r == tmax && !wins_tie()) return false;
    } else {
        if (!(tmin < r && r < tmax)) {
            r = divide_by(h + sq, a, inv_a);
            if (!(tmin < r && r < tmax)) return false;
        }
    }
    root = r;
    return true;
}
template <typename real>
RTK_DEV bool sphere_root(V3<real> cc, real radius, V3<real> o, V3<real> d, real a, real inv_a, real tmin, real tmax, real& root) {
    return sphere_root<false>(cc, radius * radius, o, d, a, inv_a, tmin, tmax, root, [] { return false; });
}

// quad::hit (quad.h:29-73) on the packed record n(3),D,Q(3),w(3),v(3),u(3).
template <typename real, typename Rec>
RTK_DEV bool quad_test(const Rec* rec, V3<real> o, V3<real> d, real tmin, real tmax, real& t_out, real& alpha, real& beta) {
    V3<real> n = packed3<real, 0>(rec);
    real denom = dot(n, d);
    if (rt_fabs(denom) < real(1e-8)) return false;
    real t = (packed<real, 3>(rec) - dot(n, o)) / denom;
    if (!(tmin <= t && t <= tmax)) return false;
    V3<real> P = o + scale(t, d);
    V3<real> planar = P - packed3<real, 4>(rec);
    V3<real> w = packed3<real, 7>(rec);
    alpha = dot(w, cross(planar, packed3<real, 10>(rec)));
    beta = dot(w, cross(packed3<real, 13>(rec), planar));
    if (!(real(0) <= alpha && alpha <= real(1)) || !(real(0) <= beta && beta <= real(1))) return false;
    t_out = t;
    return true;
}

// triangle::hit (triangle.h:65-122): Moeller-Trumbore with the reference's float
// determinant (triangle.h:72,77) and float barycentrics (triangle.h:96-98), on
// the packed record e2(3),e1(3),p0(3).
template <typename real, typename Rec>
RTK_DEV bool tri_test(const Rec* rec, V3<real> o, V3<real> d, real tmin, real tmax, real& t_out, float& fa, float& fb, float& fg) {
    V3<real> e2 = packed3<real, 0>(rec), e1 = packed3<real, 3>(rec);
    V3<real> pvec = cross(d, e2);
    float det = float(dot(e1, pvec));
    if (__builtin_fabsf(det) < real(1e-8)) return false;
    float inv_det = 1.0f / det;
    V3<real> tvec = o - packed3<real, 6>(rec);
    real u = dot(tvec, pvec) * real(inv_det);
    if (u < real(0) || u > real(1)) return false;
    V3<real> qvec = cross(tvec, e1);
    real v = dot(d, qvec) * real(inv_det);
    if (v < real(0) || u + v > real(1)) return false;
    real t = dot(e2, qvec) * real(inv_det);
    if (t < tmin || t > tmax) return false;
    fa = float(real(1) - u - v);
    fb = float(u);
    fg = float(v);
    real da = real(fa), db = real(fb);
    if (!(real(0) <= da && da <= real(1)) || !(real(0) <= db && db <= real(1))) return false;
    t_out = t;
    return true;
}

// ------------------------------------------------------------------ lane state --
// Everything a lane carries between scheduler iterations.  One lane = one pixel;
// it walks that pixel's samples in order, each sample's segments in order, and
// each segment's traversal program in order -- the same sequence of arithmetic as
// the reference's recursion for that pixel, merely interleaved with other lanes.
template <typename real>
struct Lane {
    V3<real> ro, rd;         // world-space ray of the current segment (ray_color's `r`)
    V3<real> o, d, inv;      // the ray in the current chain's object space, and 1/d (aabb.h:67, hoisted: same value per box)
    V3<real> oi;             // o * inv, for the fused slab test of F_FMA_BOX kernels (dead, hence free, in the others)
    // F_F32_BOX kernels: the ray as the f32 culling boxes see it -- 1/d and o/d in float, the query interval rounded
    // outward.  inv and oi above are dead there.
    V3<float> inv32, oi32;
    V3<float> oi32_lo;  // oi32 holds the UPPER bracket of o/d, this the lower one (see begin_culling32)
    float tmin32, tmax32;
    V3<float> inv32s, oi32s; // lean MIXED kernel: inv32 and oi32 times 1 / (end of the current interval), see rescale32
    float m2slack32;         // COMPACT kernels with centre / half-extent boxes: -2 x the ray's slack (slab_test32_che)
    real a, inv_a, tm;       // d.d (sphere.h:35, hoisted likewise) and 1/(d.d) for divide_by; ray time
    real tmin, best_t;       // current query interval: (tmin, closest so far)
    real sv_tmin, sv_best_t, rec1_t;  // constant_medium::hit nests two closest-hit queries of its boundary
                                      // (constant_medium.h:23,26); the outer query is parked here meanwhile
    V3<real> throughput, radiance, sum;
    uint32_t pc, kind, best_pc, sv_best_pc, rng;  // kind = record kind at pc (kept in a register so the vote needs no LDS read)
    int depth, s;
    uint32_t segs;           // segments traced for the current (pixel, chunk): the tile-cost estimate
    uint32_t box_kind;       // OP_BOX when 1/d is finite and non-zero on all three axes (slab tests cannot produce NaNs: the lane
                             // joins the box loop); kIrregularBox otherwise (its boxes go through step_other's literal slab test)
};

constexpr uint32_t kIrregularBox = 0xFFu;  // matches no record kind

template <typename real>
RTK_DEV bool regular_direction(V3<real> inv) {
    const real inf = real_inf<real>();
    return rt_fabs(inv.x) > real(0) && rt_fabs(inv.x) < inf && rt_fabs(inv.y) > real(0) && rt_fabs(inv.y) < inf && rt_fabs(inv.z) > real(0) &&
           rt_fabs(inv.z) < inf;
}

// The ray the records are tested against: the object-space ray when the scene has instance transforms, else the
// world-space ray itself (no second copy is kept in registers).
template <bool XF, typename real> RTK_DEV const V3<real>& ray_o(const Lane<real>& L) { if constexpr (XF) return L.o; else return L.ro; }
template <bool XF, typename real> RTK_DEV const V3<real>& ray_d(const Lane<real>& L) { if constexpr (XF) return L.d; else return L.rd; }

// The f64 query interval (tmin, best_t) as the f32 slab test uses it: rounded outward, so nothing the exact interval
// admits is rejected.  A float conversion rounds to nearest (error <= 2^-24 relative); scaling by 1 -/+ 2^-22 moves
// the bound safely past the exact value; infinities stay infinities.
RTK_DEV float below(double x) { const float f = float(x); return f - __builtin_fabsf(f) * 2.3841858e-07f; }
RTK_DEV float above(double x) { const float f = float(x); return f + __builtin_fabsf(f) * 2.3841858e-07f; }
RTK_DEV float below(float x) { return x; }
RTK_DEV float above(float x) { return x; }

template <typename real>
RTK_DEV void sync_interval32(Lane<real>& L) {
    L.tmin32 = below(L.tmin);
    L.tmax32 = above(L.best_t);
}

// F_F32_BOX: 1/d and o/d in float for the culling boxes (one v_rcp_f32 per axis instead of an f64 division), and
// whether the f32 test may be used at all: direction components neither zero nor beyond float range, origin inside
// the coordinate bound the box margin was sized for (rtk_api.cpp build_mixed_program).
template <int CH = 0, typename real>
RTK_DEV void begin_culling32(Lane<real>& L, V3<real> o, V3<real> d, float extent) {
    const V3<float> d32 = V3<float>{float(d.x), float(d.y), float(d.z)};
    L.inv32 = V3<float>{__builtin_amdgcn_rcpf(d32.x), __builtin_amdgcn_rcpf(d32.y), __builtin_amdgcn_rcpf(d32.z)};
    L.oi32 = V3<float>{float(o.x) * L.inv32.x, float(o.y) * L.inv32.y, float(o.z) * L.inv32.z};
    if constexpr (CH >= 2) {
        // centre / half-extent boxes that carry only their own share: the origin's -- o/d off by < (2.5 + 1) 2^-23 |o/d| per
        // axis, the two final roundings of the test included -- becomes ONE slack for all axes, 2^-20 of the largest |o/d|
        const float big_oi = raw_max3(__builtin_fabsf(L.oi32.x), __builtin_fabsf(L.oi32.y), __builtin_fabsf(L.oi32.z));
        L.m2slack32 = -2.0f * (big_oi * (CH == 3 ? 1.9073486e-06f : 9.5367432e-07f));  // (3: oi32 becomes the bracket's upper end below -- twice the slack covers that)
    }
    if constexpr (CH == 0 || CH == 3)  // (centre / half-extent boxes: no bracket; 3 = a counting kernel that serves both record forms)
    // The origin's share of the float error travels with the RAY: o/d is bracketed, oi32_lo <= o/d <= oi32 -- the float
    // product is off by < 2^-21.9 relative (float(o) 2^-24, v_rcp_f32 1 ulp on float(d) 2^-24, the product 2^-24), and the
    // slab test's own final rounding adds 2^-24 of it -- so the boxes only have to carry their OWN share, 2^-21 of their own
    // coordinates (rtk_api.cpp), not 2^-19 of the largest coordinate in the scene.
    {
        const float k = 4.7683716e-07f;  // 2^-21
        const V3<float> e = V3<float>{__builtin_fabsf(L.oi32.x) * k, __builtin_fabsf(L.oi32.y) * k, __builtin_fabsf(L.oi32.z) * k};
        L.oi32_lo = V3<float>{L.oi32.x - e.x, L.oi32.y - e.y, L.oi32.z - e.z};
        L.oi32 = V3<float>{L.oi32.x + e.x, L.oi32.y + e.y, L.oi32.z + e.z};
    }
    // (lean MIXED kernel: the constants are multiplied once more by 1 / (end of the interval) <= 1, down to
    // 2^-42 / extent -- direction components within 2^-40 .. 2^40 keep every product a normal float; anything else takes
    // the exact path like a zero component does)
    const float big = CH == 1 ? 1.0e12f : 3.0e38f, tiny = CH == 1 ? 1.0e-12f : 1.0e-30f;
    const bool ok = __builtin_fabsf(L.inv32.x) < big && __builtin_fabsf(L.inv32.y) < big && __builtin_fabsf(L.inv32.z) < big &&
                    __builtin_fabsf(d32.x) < big && __builtin_fabsf(d32.y) < big && __builtin_fabsf(d32.z) < big &&
                    __builtin_fabsf(d32.x) > tiny && __builtin_fabsf(d32.y) > tiny && __builtin_fabsf(d32.z) > tiny &&
                    __builtin_fabsf(float(o.x)) <= extent && __builtin_fabsf(float(o.y)) <= extent && __builtin_fabsf(float(o.z)) <= extent;
    L.box_kind = ok ? uint32_t(OP_BOX) : kIrregularBox;
}

// world.hit(r, interval(0.001, inf), rec) (Camera.txt:211) starts here.
template <bool XF, bool MIXED = false, int CH = 0, typename real, bool COUNT>
RTK_DEV void begin_segment(Lane<real>& L, Counters<COUNT>& cnt, float extent = 0.0f) {
    cnt.inc(C_SEGMENTS);
    L.segs += 1;
    if constexpr (XF) {
        L.o = L.ro;
        L.d = L.rd;
    }
    L.a = length_squared(L.rd);
    // (lean MIXED kernel, CH == 1: the guarded short reciprocal of rtk_device_math.h -- a = |d|^2 of a ray anyone may hand in)
    L.inv_a = rcp_site<MIXED && CH == 1>(L.a);
    L.tmin = real(0.001);
    L.best_t = real_inf<real>();
    if constexpr (MIXED) {
        begin_culling32<CH>(L, L.ro, L.rd, extent);
        sync_interval32(L);
        if constexpr (CH == 1) rescale32(L, extent);
    } else {
        L.inv = mk(real(1) / L.rd.x, real(1) / L.rd.y, real(1) / L.rd.z);
        L.box_kind = regular_direction(L.inv) ? uint32_t(OP_BOX) : kIrregularBox;
        L.oi = L.ro * L.inv;
    }
    L.best_pc = kNoHit;
    L.pc = 0;
}

// What a primitive test needs to resolve an exact tie (see "exact ties" above): the rank table of the program the kernel
// executes and a way to learn the kind of the record at a pc (the current winner's).  TieCtx<false, ...> compiles to nothing.
template <bool TIE, typename KindOf>
struct TieCtx {
    static constexpr bool enabled = TIE;
    const uint32_t* ranks;
    KindOf kind_of;
    uint32_t shift = 0;  // a pc is (rank index << shift): 5 in the lean MIXED kernel, whose pcs count bytes
    RTK_DEV uint32_t at(uint32_t pc) const { return pc == kNoHit ? kNoHit : pc >> shift; }
    RTK_DEV bool sphere_wins(uint32_t pc, uint32_t best_pc) const { return tie_sphere_wins(ranks, at(pc), at(best_pc), best_pc == kNoHit ? 0u : kind_of(best_pc)); }
    RTK_DEV bool inclusive_wins(uint32_t pc, uint32_t best_pc) const { return tie_inclusive_wins(ranks, at(pc), at(best_pc), best_pc == kNoHit ? 0u : kind_of(best_pc)); }
};
struct NoTie {
    static constexpr bool enabled = false;
    RTK_DEV bool sphere_wins(uint32_t, uint32_t) const { return false; }
    RTK_DEV bool inclusive_wins(uint32_t, uint32_t) const { return true; }
};

// The lean MIXED kernel's box test works in t' = t * s with s = 1 / (end of the current interval), so that
// the interval is [~0, 1] and its two clamps are the output clamp of v_max3 / v_min3.  The end is tmax32 or, while there is
// no hit yet, a bound no hit can exceed: origin and every box lie in [-extent, extent]^3, so a hit has
// t <= 2 sqrt(3) extent / |d| <= 4 extent |1/d_x|.  s is rounded DOWN (v_rcp_f32 is good to an ulp; times 1 - 2^-22), so 1
// maps to a t at or beyond the end; the lower clamp sits at t = 0 instead of tmin = 0.001 -- both on the permissive side.
// The two extra roundings (inv * s, oi * s: 2^-24 each) are inside the margins the half-extents carry (rtk_api.cpp:
// 3 x 2^-23 of the 4 x 2^-23 budgeted for the box's own share, 4.5 x 2^-23 of the 8 x 2^-23 for the origin's).
template <typename real>
RTK_DEV void rescale32(Lane<real>& L, float extent) {
    const float bound = 4.0f * extent * __builtin_fabsf(L.inv32.x);
    const float end = raw_min(L.tmax32, bound);
    const float s = __builtin_amdgcn_rcpf(end) * 0.99999976f;
    L.inv32s = V3<float>{L.inv32.x * s, L.inv32.y * s, L.inv32.z * s};
    L.oi32s = V3<float>{L.oi32.x * s, L.oi32.y * s, L.oi32.z * s};
}
// A primitive test accepted t: it is the closest hit so far (hittable_list.h:27-31 / bvh.h:69 shrink the interval).
template <bool MIXED, bool SCALED = false, typename real>
RTK_DEV void take_hit(Lane<real>& L, real t, float extent = 0.0f) {
    L.best_t = t;
    L.best_pc = L.pc;
    if constexpr (MIXED) L.tmax32 = above(t);
    if constexpr (SCALED) rescale32(L, extent);
}
// The three primitive tests against the lane's current ray and interval, shared by every program layout: `units` is the
// record's length in that layout; MIXED kernels keep the float copy of the interval in step.
template <bool XF, bool MIXED, bool SCALED = false, bool SHORT = false, typename real, bool COUNT, typename Tie>
RTK_DEV void hit_sphere(Lane<real>& L, V3<real> cc, real radius2, uint32_t units, Counters<COUNT>& cnt, const Tie& tie, float extent = 0.0f) {
    cnt.inc(C_SPHERE);
    real r;
    if (sphere_root<Tie::enabled, SHORT>(cc, radius2, ray_o<XF>(L), ray_d<XF>(L), L.a, L.inv_a, L.tmin, L.best_t, r, [&] { return tie.sphere_wins(L.pc, L.best_pc); }))
        take_hit<MIXED, SCALED>(L, r, extent);
    L.pc += units;
}
template <bool XF, bool MIXED, typename real, bool COUNT, typename Rec, typename Tie>
RTK_DEV void hit_quad(Lane<real>& L, const Rec* __restrict__ rec, uint32_t units, Counters<COUNT>& cnt, const Tie& tie) {
    cnt.inc(C_QUAD);
    real t, al, be;
    if (quad_test(rec, ray_o<XF>(L), ray_d<XF>(L), L.tmin, L.best_t, t, al, be)) {
        bool ok = true;
        if constexpr (Tie::enabled) {
            if (t == L.best_t) ok = tie.inclusive_wins(L.pc, L.best_pc);
        }
        if (ok) take_hit<MIXED>(L, t);
    }
    L.pc += units;
}
template <bool XF, bool MIXED, typename real, bool COUNT, typename Rec, typename Tie>
RTK_DEV void hit_tri(Lane<real>& L, const Rec* __restrict__ rec, uint32_t units, Counters<COUNT>& cnt, const Tie& tie) {
    cnt.inc(C_TRI);
    real t;
    float fa, fb, fg;
    if (tri_test(rec, ray_o<XF>(L), ray_d<XF>(L), L.tmin, L.best_t, t, fa, fb, fg)) {
        bool ok = true;
        if constexpr (Tie::enabled) {
            if (t == L.best_t) ok = tie.inclusive_wins(L.pc, L.best_pc);
        }
        if (ok) take_hit<MIXED>(L, t);
    }
    L.pc += units;
}

// ---- F_F32_BOX: the steps on the MIXED / COMPACT programs (rtk_device_layout.h) -------------------------------
// Conservative slab tests in float, on bounds that were rounded outward and grown for exactly this arithmetic; v_max3 / v_min3
// fold the reduction and a tie is let through (>=).
// UNITS = length of a box record: 1 in the MIXED program (32-byte units), 2 in the COMPACT one (16-byte units)
// The sign-selected form: which bound of an axis is the near plane depends only on the sign of that direction component,
// known per ray -- three wave-level masks (SGPR pairs, taken once at the loop's entry: no lane changes its ray inside it)
// pick it with six v_cndmask instead of six min/max, so near and far planes can use the two ends of the o/d bracket:
// near = b_near/d - (o/d)_upper, far = b_far/d - (o/d)_lower.  Same instruction count as slab_test32.
struct SignMasks {
    unsigned long long x, y, z;  // bit l: lane l's direction component is negative
};
RTK_DEV float pick(float a, float b, unsigned long long mask) {  // lane-wise: mask bit set ? b : a
    float r;
    asm("v_cndmask_b32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(mask));
    return r;
}
RTK_DEV bool slab_test32_signed(const MixedHead& b, V3<float> oi_hi, V3<float> oi_lo, V3<float> inv, float tmin, float tmax, const SignMasks& m) {
    const float nx = __builtin_fmaf(pick(b.f(0), b.f(1), m.x), inv.x, -oi_hi.x), fx = __builtin_fmaf(pick(b.f(1), b.f(0), m.x), inv.x, -oi_lo.x);
    const float ny = __builtin_fmaf(pick(b.f(2), b.f(3), m.y), inv.y, -oi_hi.y), fy = __builtin_fmaf(pick(b.f(3), b.f(2), m.y), inv.y, -oi_lo.y);
    const float nz = __builtin_fmaf(pick(b.f(4), b.f(5), m.z), inv.z, -oi_hi.z), fz = __builtin_fmaf(pick(b.f(5), b.f(4), m.z), inv.z, -oi_lo.z);
    const float near = raw_max(raw_max3(nx, ny, nz), tmin);
    const float far = raw_min(raw_min3(fx, fy, fz), tmax);
    return far >= near;
}
template <uint32_t UNITS = 1, typename real, bool COUNT>
RTK_DEV void step_box32(Lane<real>& L, const MixedHead& rec, Counters<COUNT>& cnt, const SignMasks& m) {
    cnt.inc(C_BOX);
    const bool hit = slab_test32_signed(rec, L.oi32, L.oi32_lo, L.inv32, L.tmin32, L.tmax32, m);
    L.pc = hit ? L.pc + UNITS : rec.aux;
}
// The lean MIXED kernel's program counters count BYTES (a unit is 32 of them) when its boxes are centre / half-extent
// records: the box step then needs no shift to turn its pc into an LDS address -- box step 19 -> 18 instructions.
constexpr uint32_t kChPcUnit = 32u;
// MIXED program: the box as centre c = f[0..2] and half-extent h = f[3..5]; per axis
// tc = c/d - o/d, near = tc - h/|d|, far = tc + h/|d| -- which plane is the near one never has to be asked.  The
// half-extent was grown for exactly this arithmetic (rtk_api.cpp build_mixed_program), so the test is conservative.
// (|1/d| is a source modifier: no instructions.)
// ... with the ray's slack (COMPACT programs): the planes may each be off by `slack` = -m2slack / 2 in t, so the box is
// passed when min(far, tmax) - max(near, tmin) >= -2 slack -- at the interval's ends a touch more permissive than
// clamping the widened planes, never less.
RTK_DEV bool slab_test32_che(const MixedHead& b, V3<float> oi, V3<float> inv, float tmin, float tmax, float m2slack) {
    const float tcx = __builtin_fmaf(b.f(0), inv.x, -oi.x), tcy = __builtin_fmaf(b.f(1), inv.y, -oi.y), tcz = __builtin_fmaf(b.f(2), inv.z, -oi.z);
    const float ax = __builtin_fabsf(inv.x), ay = __builtin_fabsf(inv.y), az = __builtin_fabsf(inv.z);
    const float nx = __builtin_fmaf(-b.f(3), ax, tcx), fx = __builtin_fmaf(b.f(3), ax, tcx);
    const float ny = __builtin_fmaf(-b.f(4), ay, tcy), fy = __builtin_fmaf(b.f(4), ay, tcy);
    const float nz = __builtin_fmaf(-b.f(5), az, tcz), fz = __builtin_fmaf(b.f(5), az, tcz);
    const float near = raw_max(raw_max3(nx, ny, nz), tmin);
    const float far = raw_min(raw_min3(fx, fy, fz), tmax);
    return far - near >= m2slack;
}
template <typename real, bool COUNT>
RTK_DEV void step_box32_che(Lane<real>& L, const MixedHead& rec, Counters<COUNT>& cnt) {
    cnt.inc(C_BOX);
    const bool hit = slab_test32_che(rec, L.oi32, L.inv32, L.tmin32, L.tmax32, L.m2slack32);
    L.pc = hit ? L.pc + 2u : rec.aux;
}
// ... in the ray parameter scaled by rescale32: the interval is [0, 1], its clamps are output modifiers.  Strict compare: a
// box has a positive extent along the ray (far' - near' = 2 h |inv'| > 0), so far' == near' after clamping means both were
// clamped to the same end -- the box lies wholly before 0 or wholly beyond 1.
RTK_DEV float max3_clamp01(float a, float b, float c) { float r; asm("v_max3_f32 %0, %1, %2, %3 clamp" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
RTK_DEV float min3_clamp01(float a, float b, float c) { float r; asm("v_min3_f32 %0, %1, %2, %3 clamp" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
// (Packed f32 arithmetic for this test was measured in round 3 and removed: five v_pk_fma_f32 with op_sel / neg modifiers
// (inline asm on aligned register pairs: no moves) instead of nine v_fma_f32 -- 12 instead of 16 VALU instructions per box
// step in the ISA, same bits, same image -- ran C2 at 19.35 instead of 18.50 ms: the packed instruction issues at 0.24 per
// cycle per SIMD against 0.45 for v_fma_f32 (csrc/rtk_microbench.hip, aggregate rates: two operations per lane at half the
// rate -- five packed cost what ten plain ones do) and lengthens the step's dependent chain.  Left to the compiler
// (ext_vector_type(2) fma) the same test cost 9-19 extra moves per step: 22.6 ms.)
RTK_DEV bool slab_test32_chs(const MixedHead& b, V3<float> oi, V3<float> inv) {
    const float tcx = __builtin_fmaf(b.f(0), inv.x, -oi.x), tcy = __builtin_fmaf(b.f(1), inv.y, -oi.y), tcz = __builtin_fmaf(b.f(2), inv.z, -oi.z);
    const float ax = __builtin_fabsf(inv.x), ay = __builtin_fabsf(inv.y), az = __builtin_fabsf(inv.z);
    const float nx = __builtin_fmaf(-b.f(3), ax, tcx), fx = __builtin_fmaf(b.f(3), ax, tcx);
    const float ny = __builtin_fmaf(-b.f(4), ay, tcy), fy = __builtin_fmaf(b.f(4), ay, tcy);
    const float nz = __builtin_fmaf(-b.f(5), az, tcz), fz = __builtin_fmaf(b.f(5), az, tcz);
    return min3_clamp01(fx, fy, fz) > max3_clamp01(nx, ny, nz);
}
template <typename real, bool COUNT>
RTK_DEV void step_box32_ch(Lane<real>& L, const MixedHead& rec, Counters<COUNT>& cnt) {
    cnt.inc(C_BOX);
    const bool hit = slab_test32_chs(rec, L.oi32s, L.inv32s);
    L.pc = hit ? L.pc + kChPcUnit : rec.aux;  // (pcs of this kernel count bytes, and so does the link)
}
// The same step on the program's LDS image (rtk_device_layout.h MixedImg): `a` = the first 16 bytes of the record (centre,
// link), `b` = the second (half-extent).  The arithmetic is slab_test32_chs's, on the same values.
typedef uint32_t rtk_u32x4 __attribute__((ext_vector_type(4)));  // 16 bytes of an LDS record as one ds_read_b128 returns them
template <typename real, bool COUNT>
RTK_DEV void step_box_img(Lane<real>& L, rtk_u32x4 a, rtk_u32x4 b, Counters<COUNT>& cnt) {
    cnt.inc(C_BOX);
    // (vector elements are copied to scalars first: __builtin_bit_cast applied to the element expression itself reads element 0
    // every time with the compiler in use)
    const uint32_t a0 = a.x, a1 = a.y, a2 = a.z, b0 = b.x, b1 = b.y, b2 = b.z;
    MixedHead rec;
    rec.w[0] = a0, rec.w[1] = a1, rec.w[2] = a2, rec.w[3] = b0, rec.w[4] = b1, rec.w[5] = b2;
    const bool hit = slab_test32_chs(rec, L.oi32s, L.inv32s);
    L.pc = hit ? L.pc + kChPcUnit : a.w;  // (a box's word 3 is its link as stored: byte pcs, kind nibble 0)
}
// A box of those programs for a ray the float test must not judge (zero / out-of-range direction component, origin
// outside the sized bound): aabb::hit's literal form in f64 on the (outward-rounded, hence still enclosing) bounds.
template <bool XF = false, uint32_t UNITS = 1, uint32_t PCU = 1, typename real, bool COUNT>
RTK_DEV void step_box_mixed_exact(Lane<real>& L, const MixedHead& rec, Counters<COUNT>& cnt, bool compact_ch = false) {
    cnt.inc(C_BOX);
    Slot<real> b;
    if (UNITS == 1 || (UNITS == 2 && compact_ch)) {  // centre / half-extent records (the MIXED program; COMPACT programs of the mesh family)
        for (int k = 0; k < 3; k++) {
            b.v[2 * k] = real(rec.f(k)) - real(rec.f(3 + k));
            b.v[2 * k + 1] = real(rec.f(k)) + real(rec.f(3 + k));
        }
    } else {
        for (int k = 0; k < 6; k++) b.v[k] = real(rec.f(k));
    }
    const V3<real> d = ray_d<XF>(L);
    const V3<real> inv = mk(real(1) / d.x, real(1) / d.y, real(1) / d.z);
    const bool hit = slab_test<true>(b, ray_o<XF>(L), inv, L.tmin, L.best_t);
    L.pc = hit ? L.pc + UNITS * PCU : rec.aux;
}
// sphere::hit on a MIXED record: centre in the head unit, radius in the next one.
template <uint32_t PCU = 1, typename real, bool COUNT, typename Tie, typename Rec>
RTK_DEV void step_sphere_mixed(Lane<real>& L, const Rec& head, const Rec* __restrict__ rec, Counters<COUNT>& cnt, const Tie& tie, float extent) {
    const double radius2 = reinterpret_cast<const double*>(rec + 1)[2];  // radius * radius from the upload: the same product, once
    hit_sphere<false, true, true, true>(L, mk(real(head.d(0)), real(head.d(1)), real(head.d(2))), real(radius2), 2u * PCU, cnt, tie, extent);
}
// ... with the head of a MixedImg record as the box loop holds it: its first 16 bytes `a` (centre x) and its second `b` (y, z)
template <uint32_t PCU = 1, typename real, bool COUNT, typename Tie>
RTK_DEV void step_sphere_img(Lane<real>& L, rtk_u32x4 a, rtk_u32x4 b, const MixedImg* __restrict__ rec, Counters<COUNT>& cnt, const Tie& tie, float extent) {
    const double radius2 = reinterpret_cast<const double*>(rec + 1)[2];
    const unsigned long long xw = (unsigned long long)(a.x) | ((unsigned long long)(a.y) << 32);
    const unsigned long long yw = (unsigned long long)(b.x) | ((unsigned long long)(b.y) << 32);
    const unsigned long long zw = (unsigned long long)(b.z) | ((unsigned long long)(b.w) << 32);
    const double cx = __builtin_bit_cast(double, xw), cy = __builtin_bit_cast(double, yw), cz = __builtin_bit_cast(double, zw);
    hit_sphere<false, true, true, true>(L, mk(real(cx), real(cy), real(cz)), real(radius2), 2u * PCU, cnt, tie, extent);
}
// ... and on a COMPACT record (3 units): the head (centre) is usually in registers already, the radius follows it.
template <bool XF, typename real, bool COUNT, typename Tie>
RTK_DEV void step_sphere_compact(Lane<real>& L, const MixedHead& head, const Unit16* __restrict__ rec, Counters<COUNT>& cnt, const Tie& tie) {
    hit_sphere<XF, true>(L, mk(real(head.d(0)), real(head.d(1)), real(head.d(2))), packed<real, 3>(rec) * packed<real, 3>(rec), 3u, cnt, tie);
}
// The remaining record kinds of a sphere-only program: a moving sphere, or a box for an irregular ray.
template <uint32_t PCU = 1, typename real, bool COUNT, typename Tie, typename Rec>
RTK_DEV void step_other_mixed(Lane<real>& L, const Rec* __restrict__ rec, Counters<COUNT>& cnt, const Tie& tie, float extent) {
    const uint32_t kind = rec->kind();
    if (kind == OP_BOX) {
        if constexpr (std::is_same_v<Rec, MixedImg>) {
            MixedHead box;  // the record's six values and its link, as step_box_mixed_exact reads them
            for (int k = 0; k < 6; k++) box.w[k] = __builtin_bit_cast(uint32_t, rec->f(k));
            box.aux = rec->link();
            step_box_mixed_exact<false, 1, PCU>(L, box, cnt);
        } else {
            step_box_mixed_exact<false, 1, PCU>(L, *rec, cnt);
        }
    } else if (kind == OP_SPHERE_MOVING) {
        const double* cont = reinterpret_cast<const double*>(rec + 1);
        const V3<real> cc = mk(real(rec->d(0)), real(rec->d(1)), real(rec->d(2))) + scale(L.tm, mk(real(cont[2]), real(cont[3]), real(cont[4])));
        hit_sphere<false, true, true, true>(L, cc, real(cont[5]), 3u * PCU, cnt, tie, extent);  // cont[5] = radius * radius
    } else {
        L.pc += uint32_t(mixed_units(kind)) * PCU;  // unreachable for a validated sphere-only program
    }
}
// bvh_node::hit's box test (bvh.h:65): on a miss skip the whole subtree.
template <bool EXACT_NAN, bool XF, bool FMA = false, typename real, bool COUNT>
RTK_DEV void step_box(Lane<real>& L, const Slot<real>& rec, Counters<COUNT>& cnt) {
    cnt.inc(C_BOX);
    bool hit;
    if constexpr (FMA && !EXACT_NAN) hit = slab_test_fma(rec, L.oi, L.inv, L.tmin, L.best_t);
    else hit = slab_test<EXACT_NAN>(rec, ray_o<XF>(L), L.inv, L.tmin, L.best_t);
    L.pc = hit ? L.pc + 1 : rec.aux;
}

// sphere::hit of a stationary sphere.
template <bool XF, bool SHORT = false, typename real, bool COUNT, typename Tie>
RTK_DEV void step_sphere(Lane<real>& L, const Slot<real>& rec, Counters<COUNT>& cnt, const Tie& tie) {
    hit_sphere<XF, false, false, SHORT>(L, mk(rec.v[0], rec.v[1], rec.v[2]), rec.v[3] * rec.v[3], 1u, cnt, tie);
}

// Which COMPACT programs hold centre / half-extent box records: those of the mesh family -- the same rule
// in rtk_api.cpp, which also sets SceneView::compact_ch for the counting kernel, the one kernel that serves every family.
// (Measured: C4 62.3 -> 59.7 ms; the Cornell box and book 2, thin axis-aligned quads at coordinates in the hundreds
// and thousands, lose 2-4 % to the all-axes slack and keep the sign-selected test with its per-axis bracket.)
template <uint32_t FEAT>
constexpr bool kCompactChStatic = (FEAT & F_F32_BOX) != 0 && (FEAT & ~uint32_t(F_FMA_BOX | F_F32_BOX | F_MATTE | F_LDS_BOXES)) == kFeatMesh;
template <uint32_t FEAT, bool COUNT, typename real>
RTK_DEV bool compact_ch_records(const SceneView<real>& sc) {
    if constexpr (kCompactChStatic<FEAT>) return true;
    else if constexpr (COUNT) return sc.compact_ch != 0;
    else return false;
}
// Every other record kind (moving sphere, quad, triangle, chain switch, the three medium ops, a box met by a ray the
// box loop does not take).  `rec` points at the record in the program (LDS or global), in the slot layout (Slot<real>)
// or -- F_F32_BOX kernels of the non-lean families -- the COMPACT one (Unit16).
template <typename real, uint32_t FEAT, bool BRACKET = true, bool COUNT, typename Rec, typename Tie>
RTK_DEV void step_other(Lane<real>& L, const Rec* __restrict__ rec, const SceneView<real>& sc, Counters<COUNT>& cnt, const Tie& tie, float extent = 0.0f) {
    constexpr bool XF = (FEAT & F_XFORM) != 0;
    constexpr bool MIXED = (FEAT & F_F32_BOX) != 0;  // here: the COMPACT program (f32 culling boxes; the float interval follows every change)
    const uint32_t kp = rec_kind_payload<real>(rec);
    const uint32_t aux = rec_aux<real>(rec);
    const uint32_t kind = kp & 15u;
    if (kind == OP_BOX) {  // only for rays with a zero or infinite direction component: the literal, NaN-exact slab test
        if constexpr (MIXED) step_box_mixed_exact<XF, 2>(L, *reinterpret_cast<const MixedHead*>(rec), cnt, compact_ch_records<FEAT, COUNT>(sc));
        else step_box<true, XF>(L, *reinterpret_cast<const Slot<real>*>(rec), cnt);
    } else if (kind == OP_SPHERE_MOVING) {
        const V3<real> cc = packed3<real, 0>(rec) + scale(L.tm, moving_dir<real>(rec));
        hit_sphere<XF, MIXED>(L, cc, packed<real, 3>(rec) * packed<real, 3>(rec), rec_units<real>(rec, kind), cnt, tie);
    } else if ((FEAT & F_QUAD) && kind == OP_QUAD) {
        hit_quad<XF, MIXED>(L, rec, rec_units<real>(rec, kind), cnt, tie);
    } else if ((FEAT & F_TRI) && kind == OP_TRI) {
        hit_tri<XF, MIXED>(L, rec, rec_units<real>(rec, kind), cnt, tie);
    } else if ((FEAT & F_XFORM) && kind == OP_CHAIN) {
        cnt.inc(C_XFORM, aux);
        apply_chain<kChainPrefetch<FEAT>>(sc.chains, kp >> 4, L.ro, L.rd, L.o, L.d);
        L.a = length_squared(L.d);
        L.inv_a = real(1) / L.a;
        if constexpr (MIXED) {
            begin_culling32(L, L.o, L.d, extent);  // (programs with instance chains keep the sign-selected test) 1/d, o/d in float for the boxes of this space; the interval (a ray parameter) is unchanged
        } else {
            L.inv = mk(real(1) / L.d.x, real(1) / L.d.y, real(1) / L.d.z);
            L.box_kind = regular_direction(L.inv) ? uint32_t(OP_BOX) : kIrregularBox;
            L.oi = L.o * L.inv;
        }
        L.pc += rec_units<real>(rec, kind);
    } else if ((FEAT & F_MEDIA) && kind == OP_MED_SPHERE) {
        // constant_medium::hit (constant_medium.h:20-53) with a stationary sphere as the boundary, in one step: the two
        // boundary->hit calls (universe, then (t1 + 0.0001, inf)) are two sphere::hit calls on the same sphere and ray, then the
        // clamp to the ray's interval, one random_double() and the scatter distance.  The lane's own interval and closest hit
        // are only touched by the final acceptance, so nothing is parked meanwhile.
        cnt.inc(C_MEDIUM);
        const V3<real> cc = packed3<real, 0>(rec);
        const real radius = packed<real, 3>(rec);
        real r1, r2;
        cnt.inc(C_SPHERE);
        if (sphere_root(cc, radius, ray_o<XF>(L), ray_d<XF>(L), L.a, L.inv_a, -real_inf<real>(), real_inf<real>(), r1)) {  // constant_medium.h:23
            cnt.inc(C_SPHERE);
            if (sphere_root(cc, radius, ray_o<XF>(L), ray_d<XF>(L), L.a, L.inv_a, r1 + real(0.0001), real_inf<real>(), r2)) {  // constant_medium.h:26
                if (r1 < L.tmin) r1 = L.tmin;
                if (r2 > L.best_t) r2 = L.best_t;
                if (r1 < r2) {
                    if (r1 < real(0)) r1 = real(0);
                    const real ray_length = rt_sqrt(L.a);
                    const real inside = (r2 - r1) * ray_length;
                    const real hit_distance = packed<real, 4>(rec) * call_log(rnd<real>(L.rng, cnt));
                    if (!(hit_distance > inside)) take_hit<MIXED>(L, r1 + hit_distance / ray_length);
                }
            }
        }
        L.pc += rec_units<real>(rec, kind);
    } else if ((FEAT & F_MEDIA) && BRACKET && kind == OP_MED_BEGIN) {
        cnt.inc(C_MEDIUM);
        L.sv_tmin = L.tmin;
        L.sv_best_t = L.best_t;
        L.sv_best_pc = L.best_pc;
        L.tmin = -real_inf<real>();
        L.best_t = real_inf<real>();
        L.best_pc = kNoHit;
        L.pc += rec_units<real>(rec, kind);
        if constexpr (MIXED) sync_interval32(L);
    } else if ((FEAT & F_MEDIA) && BRACKET && kind == OP_MED_MID) {
        if (L.best_pc == kNoHit) {  // constant_medium.h:23-24
            L.tmin = L.sv_tmin;
            L.best_t = L.sv_best_t;
            L.best_pc = L.sv_best_pc;
            L.pc = aux;
        } else {
            L.rec1_t = L.best_t;
            L.tmin = L.rec1_t + real(0.0001);  // constant_medium.h:26
            L.best_t = real_inf<real>();
            L.best_pc = kNoHit;
            L.pc += rec_units<real>(rec, kind);
        }
        if constexpr (MIXED) sync_interval32(L);
    } else if ((FEAT & F_MEDIA) && BRACKET && kind == OP_MED_END) {
        const bool hit2 = L.best_pc != kNoHit;
        real r2 = L.best_t;
        L.tmin = L.sv_tmin;
        L.best_t = L.sv_best_t;
        L.best_pc = L.sv_best_pc;
        if (hit2) {  // constant_medium.h:29-50
            real r1 = L.rec1_t;
            if (r1 < L.tmin) r1 = L.tmin;
            if (r2 > L.best_t) r2 = L.best_t;
            if (r1 < r2) {
                if (r1 < real(0)) r1 = real(0);
                const real ray_length = rt_sqrt(L.a);
                const real inside = (r2 - r1) * ray_length;
                const real hit_distance = packed<real, 0>(rec) * call_log(rnd<real>(L.rng, cnt));
                if (!(hit_distance > inside)) {
                    L.best_t = r1 + hit_distance / ray_length;
                    L.best_pc = L.pc;
                }
            }
        }
        L.pc += rec_units<real>(rec, kind);
        if constexpr (MIXED) sync_interval32(L);
    } else {
        L.pc += rec_units<real>(rec, kind);  // unreachable for a validated program
    }
}

// ------------------------------------------------------------------ textures --
// perlin::noise (perlin.h:14-37,72-89).
template <typename real, bool COUNT>
RTK_DEV real perlin_noise(const PerlinRec<real>& pn, V3<real> p, Counters<COUNT>& cnt) {
    cnt.inc(C_NOISE);
    const real fx = rt_floor(p.x), fy = rt_floor(p.y), fz = rt_floor(p.z);
    const real u = p.x - fx, v = p.y - fy, w = p.z - fz;
    const int i = int(fx), j = int(fy), k = int(fz);
    const real uu = u * u * (real(3) - real(2) * u);
    const real vv = v * v * (real(3) - real(2) * v);
    const real ww = w * w * (real(3) - real(2) * w);
    real accum = real(0);
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int c = 0; c < 2; c++) {
                const int idx = pn.perm_x[(i + a) & 255] ^ pn.perm_y[(j + b) & 255] ^ pn.perm_z[(k + c) & 255];
                const V3<real> g = ld3(pn.randvec[idx]);
                const V3<real> wv = mk(u - real(a), v - real(b), w - real(c));
                accum += (real(a) * uu + real(1 - a) * (real(1) - uu)) * (real(b) * vv + real(1 - b) * (real(1) - vv)) *
                         (real(c) * ww + real(1 - c) * (real(1) - ww)) * dot(g, wv);
            }
    return accum;
}

// get_sphere_uv (sphere.h:67-73) and noise_texture::value's tail (texture.h:114-116: 1 + sin(...)) are libm-heavy f64 code
// (acos, atan2, sin: long polynomial expansions) that few lanes ever reach; inlined into the shade step they sit on top of
// everything live there and account for most of the full-feature kernel's scratch (compile-only ablation,
// tools/kernel_resources.py: without the two 248 VGPRs and no scratch at the 2-wave bound, with them 256 + 292 B).  Kept OUT
// OF LINE a call saves and restores around itself on the cold path only: 248 VGPRs + 32 B at
// two waves per SIMD, 168 + 352 B at three (it was 168 + 640 B) -- and three waves then win: C5 at 32 spp 42.05 ms (inline,
// 2 waves) -> 40.5 (out of line, 2 waves) -> 38.85 (out of line, 3 waves); out of line at 3 waves with only the uv function
// moved: 47.3.  Same image.  (Moving more -- pow, perlin::turb, the image lookup, get_lighting, the media's log -- was
// measured too and lost: 43.0-46.7 ms at three waves.)
template <typename real>
RTK_NOINLINE void sphere_uv(real ox, real oy, real oz, real* __restrict__ uv) {  // sphere.h:67-73 on the outward unit normal
    const real pi = real(3.1415926535897932385);
    const real theta = rt_acos(-oy);
    const real phi = rt_atan2(-oz, ox) + pi;
    uv[0] = phi / (real(2) * pi);
    uv[1] = theta / pi;
}
template <typename real>
RTK_NOINLINE real noise_tail(real arg) { return real(1) + rt_sin(arg); }  // texture.h:115: 1 + sin(scale * p.z + 10 * turb)

// texture::value (texture.h:20-120); checker nesting is followed iteratively.
template <typename real, bool COUNT>
RTK_DEV V3<real> texture_value(const SceneView<real>& sc, int tex, real u, real v, V3<real> p, Counters<COUNT>& cnt) {
    for (;;) {
        const TextureRec<real>& t = sc.textures[tex];
        if (t.kind == RTK_TEX_SOLID) return ld3(t.color);
        if (t.kind == RTK_TEX_CHECKER) {  // texture.h:42-50
            const int xi = int(rt_floor(t.param * p.x));
            const int yi = int(rt_floor(t.param * p.y));
            const int zi = int(rt_floor(t.param * p.z));
            tex = ((xi + yi + zi) % 2 == 0) ? t.even : t.odd;
            continue;
        }
        if (t.kind == RTK_TEX_CHECKER_TRI) {  // texture.h:66-76
            v = real(1) - v;
            const int ui = int(rt_round(t.param * u * real(10)));
            const int vi = int(rt_round(t.param * v * real(10)));
            tex = ((ui + vi) % 2 == 0) ? t.even : t.odd;
            continue;
        }
        if (t.kind == RTK_TEX_IMAGE) {  // texture.h:90-104, rtw_stb_image.h:71-81
            const ImageRec im = sc.images[t.image];
            if (im.width <= 0 || im.height <= 0) return mk(real(0), real(1), real(1));
            u = u < real(0) ? real(0) : (u > real(1) ? real(1) : u);
            const real vc = v < real(0) ? real(0) : (v > real(1) ? real(1) : v);
            v = real(1) - vc;
            int i = int(u * real(im.width));
            int j = int(v * real(im.height));
            i = i < 0 ? 0 : (i < im.width ? i : im.width - 1);
            j = j < 0 ? 0 : (j < im.height ? j : im.height - 1);
            cnt.inc(C_TEXEL);
            const uint8_t* px = sc.texels + im.texel_offset + (int64_t(j) * im.width + i) * 3;
            const real cs = real(1) / real(255);
            return mk(cs * real(px[0]), cs * real(px[1]), cs * real(px[2]));
        }
        // noise_texture (texture.h:114-116) with perlin::turb(p, 7) (perlin.h:38-50)
        const PerlinRec<real>& pn = sc.perlins[t.image];
        real accum = real(0), weight = real(1);
        V3<real> q = p;
        for (int k = 0; k < 7; k++) {
            accum += weight * perlin_noise(pn, q, cnt);
            weight *= real(0.5);
            q = mk(q.x * real(2), q.y * real(2), q.z * real(2));
        }
        const real s = noise_tail(t.param * p.z + real(10) * rt_fabs(accum));
        return mk(s * real(0.5), s * real(0.5), s * real(0.5));
    }
}

template <typename real, uint32_t FEAT, bool COUNT>
RTK_DEV V3<real> material_color(const SceneView<real>& sc, const MaterialRec<real>& m, real u, real v, V3<real> p, Counters<COUNT>& cnt) {
    if (!(FEAT & F_TEXTURE) || m.tex < 0) return ld3(m.albedo);  // solid colours are folded into the material at upload
    return texture_value(sc, m.tex, u, v, p, cnt);
}

#ifdef RTK_PROFILE
// Profile build: shade's sub-phases, accumulated per wave (flushed to counters[kShadeProfBase + 2 k] cycles / [.. + 1]
// calls: k = 0 the deferred hit record, 1 materials and textures, 2 the miss path in front of them, 3 the scattered ray).
struct ShadeProf {
    unsigned long long t[4] = {0, 0, 0, 0}, n[4] = {0, 0, 0, 0};
};
constexpr int kShadeProfBase = 32 + 4 * 4096;
#define RTK_SHADE_PROF_PARAM , ShadeProf& sprof
#define RTK_SHADE_PROF_ARG , sprof
#define RTK_SHADE_PROF_BEGIN unsigned long long sp_prev_ = __builtin_amdgcn_s_memtime();
#define RTK_SHADE_PROF(k)                                             \
    {                                                                 \
        const unsigned long long now_ = __builtin_amdgcn_s_memtime(); \
        sprof.t[k] += now_ - sp_prev_;                                \
        sprof.n[k] += 1;                                              \
        sp_prev_ = now_;                                              \
    }
#else
#define RTK_SHADE_PROF_PARAM
#define RTK_SHADE_PROF_ARG
#define RTK_SHADE_PROF_BEGIN
#define RTK_SHADE_PROF(k)
#endif

// ------------------------------------------------------------------ shading ---
template <typename real>
struct Surface {  // hit_record (hittable.h:11-27)
    V3<real> p, normal;
    real u, v;
    int material;
    bool front_face;
};

// The deferred hit record of a MIXED program's winner (sphere.h:50-56; solid colours only: no uv).
template <typename real, typename Rec>
RTK_DEV void make_surface_mixed(const Rec* __restrict__ prog, uint32_t best_pc, real t, V3<real> wo, V3<real> wd, real tm, Surface<real>& sf) {
    const Rec* rec = prog + best_pc;
    const uint32_t kind = rec->kind();
    const double* cont = reinterpret_cast<const double*>(rec + 1);
    sf.material = int(rec->aux_word() >> 8);
    sf.p = wo + scale(t, wd);
    sf.u = real(0);
    sf.v = real(0);
    V3<real> cc = mk(real(rec->d(0)), real(rec->d(1)), real(rec->d(2)));
    if (kind == OP_SPHERE_MOVING) cc = cc + scale(tm, mk(real(cont[2]), real(cont[3]), real(cont[4])));
    const V3<real> outward = scale(real(cont[1]), sf.p - cc);
    sf.front_face = dot(wd, outward) < real(0);
    sf.normal = sf.front_face ? outward : -outward;
}


// The barycentrics of the winning triangle for its UVs (triangle.h:96-110): triangle::hit once more on the winner, with an
// open interval.  Inline (keeping it out of line was tried on the mesh kernels at four waves per SIMD and not kept).
template <typename real, typename Rec>
RTK_DEV void tri_barycentrics(const Rec* __restrict__ rec, real ox, real oy, real oz, real dx, real dy, real dz, float* fa, float* fb, float* fg) {
    real tt;
    float a = 0, b = 0, g = 0;
    tri_test(rec, mk(ox, oy, oz), mk(dx, dy, dz), -real_inf<real>(), real_inf<real>(), tt, a, b, g);
    *fa = a;
    *fb = b;
    *fg = g;
}

// Build the hit record of the winning record (the deferred half of *.hit).  Sphere
// and quad geometry is read from the program record itself (LDS when staged); only
// triangles go to their side record for the normal and the UVs.  `prog` is the slot
// program or the COMPACT one (same payload element numbering in both).
template <typename real, uint32_t FEAT, typename Rec>
RTK_DEV void make_surface(const Rec* __restrict__ prog, const SceneView<real>& sc, const MaterialRec<real>* __restrict__ mats, uint32_t best_pc, real t,
                          V3<real> wo, V3<real> wd, real tm, Surface<real>& sf, bool force_uv = false) {
    const Rec* rec = prog + best_pc;
    const uint32_t kp = rec_kind_payload<real>(rec), aux = rec_aux<real>(rec);
    const uint32_t kind = kp & 15u;
    const uint32_t idx = kp >> 4;
    const uint32_t chain = (FEAT & F_XFORM) ? (aux & 255u) : 0u;
    sf.material = int(aux >> 8);
    V3<real> o = wo, d = wd;
    if (FEAT & F_XFORM) apply_chain<kChainPrefetch<FEAT>>(sc.chains, chain, wo, wd, o, d);
    sf.p = o + scale(t, d);
    sf.u = real(0);
    sf.v = real(0);
    V3<real> outward;
    bool face_from_ray = true;
    if (kind == OP_SPHERE || kind == OP_SPHERE_MOVING) {  // sphere.h:50-56,67-73
        V3<real> cc = packed3<real, 0>(rec);
        if (kind == OP_SPHERE_MOVING) cc = cc + scale(tm, moving_dir<real>(rec));
        outward = scale(packed<real, 4>(rec), sf.p - cc);  // (p - center) / radius = (1/radius) * (p - center) (vec3.h:91-93); element 4 = 1/radius from the upload
        if ((FEAT & F_TEXTURE) && (force_uv || mats[sf.material].needs_uv)) {
            real uv[2];
            sphere_uv(outward.x, outward.y, outward.z, uv);
            sf.u = uv[0];
            sf.v = uv[1];
        }
    } else if ((FEAT & F_QUAD) && kind == OP_QUAD) {  // quad.h:44-57; record = n(3),D,Q(3),w(3),v(3),u(3)
        V3<real> planar = sf.p - packed3<real, 4>(rec);
        V3<real> w = packed3<real, 7>(rec);
        sf.u = dot(w, cross(planar, packed3<real, 10>(rec)));
        sf.v = dot(w, cross(packed3<real, 13>(rec), planar));
        outward = packed3<real, 0>(rec);
    } else if ((FEAT & F_TRI) && kind == OP_TRI) {  // triangle.h:96-110
        const TriRec<real>& tr = sc.tris[idx];
        real tt;
        float fa = 0, fb = 0, fg = 0;
        tri_barycentrics(rec, o.x, o.y, o.z, d.x, d.y, d.z, &fa, &fb, &fg);
        sf.u = real(fa * tr.uv0[0] + fb * tr.uv1[0] + fg * tr.uv2[0]);
        sf.v = real(fa * tr.uv0[1] + fb * tr.uv1[1] + fg * tr.uv2[1]);
        outward = ld3(tr.n);
    } else {  // OP_MED_END: constant_medium.h:45-50
        outward = mk(real(1), real(0), real(0));
        face_from_ray = false;
    }
    if (face_from_ray) {  // hittable.h:23-26
        sf.front_face = dot(d, outward) < real(0);
        sf.normal = sf.front_face ? outward : -outward;
    } else {
        sf.front_face = true;
        sf.normal = outward;
    }
    if (FEAT & F_XFORM) unapply_chain<kChainPrefetch<FEAT>>(sc.chains, chain, sf.p, sf.normal);
}

// get_lighting (Camera.txt:240-272).
template <typename real>
RTK_DEV V3<real> point_lighting(const SceneView<real>& sc, V3<real> p, V3<real> normal) {
    V3<real> result = mk(real(0), real(0), real(0));
    for (int i = 0; i < sc.n_lights; i++) {
        const LightRec<real>& L = sc.lights[i];
        V3<real> dir = ld3(L.position) - p;
        real dist2 = length_squared(dir);
        dir = unit_vector(dir);
        real dn = dot(normal, dir);
        real diffuse = dn > real(0) ? dn : real(0);
        real radius_effect = L.size * real(0.1);
        if (dist2 <= L.size * L.size) {
            result = result + scale(diffuse, ld3(L.intensity));
        } else {
            real att = real(1) / (dist2 + radius_effect);
            result = result + scale(diffuse, scale(att, ld3(L.intensity)));
        }
    }
    return result;
}

// get_ray (Camera.txt:177-200) for sample L.s of pixel (i, j): seeds the sample's
// RNG stream, draws sample_square (y then x, g++ order), the lens, then the time.
template <typename real, bool COUNT>
RTK_DEV void begin_sample(Lane<real>& L, const CameraRec<real>& cam, int i, int j, uint32_t seed_hash, Counters<COUNT>& cnt) {
    cnt.inc(C_SAMPLES);
    L.rng = pcg_hash(uint32_t(j * cam.width + i) + pcg_hash(uint32_t(L.s) + seed_hash));
    const real oy = rnd<real>(L.rng, cnt) - real(0.5);
    const real ox = rnd<real>(L.rng, cnt) - real(0.5);
    const V3<real> pixel_sample = ld3(cam.pixel00) + scale(real(i) + ox, ld3(cam.du)) + scale(real(j) + oy, ld3(cam.dv));
    V3<real> ro = ld3(cam.center);
    if (cam.defocus_angle > real(0)) {  // vec3.h:135-142
        real px, py;
        for (;;) {
            py = rnd_pm1<real>(L.rng, cnt);
            px = rnd_pm1<real>(L.rng, cnt);
            if (px * px + py * py < real(1)) break;  // (the reference adds z * z = 0 * 0: x + 0 == x for x >= +0)
        }
        ro = ld3(cam.center) + scale(px, ld3(cam.disk_u)) + scale(py, ld3(cam.disk_v));
    }
    L.ro = ro;
    L.rd = pixel_sample - ro;
    L.tm = rnd<real>(L.rng, cnt);
    L.radiance = mk(real(0), real(0), real(0));
    L.throughput = mk(real(1), real(1), real(1));
    L.depth = cam.max_depth;
}

// Kernels without point lights and emissive materials: a path gathers radiance only at the miss that ends it, so
// `radiance` is +0 until then and `pixel_color += radiance` (Camera.txt:72) adds either +0 (sum + 0 == sum: the sum is
// never -0) or 0 + throughput * background == throughput * background.  Those kernels keep no radiance registers
// (lean MIXED kernel: 119 -> 113 VGPRs, C2 20.95 -> 20.84 ms, same framebuffer).
// (round 3) The same holds with emissive materials as long as there are no point lights: a diffuse_light ends the path it
// emits into (material.h:99-101,116-118), so `radiance` is +0 until then as well and 0 + throughput * emitted == throughput *
// emitted.  Only get_lighting (Camera.txt:228) adds radiance in the middle of a path.  The quad/box and mesh families (area
// lights, no point lights) drop six registers of lane state with it: C3's kernel 128 VGPRs + 16 B -> 125 + 0, C4's 128 + 44 B
// -> 126 + 0 (53.0 -> 51.8 ms).
template <uint32_t FEAT>
constexpr bool kNoRadianceState = (FEAT & F_LIGHTS) == 0;

// material::scatter / emitted on a finished hit record (material.h:22-172) and the rest of ray_color's body
// (Camera.txt:216-237): what shade() runs after it has built the record -- and what the known-answer entry point
// rtk_debug_scatter runs on caller-supplied records.  Returns true when the sample's path has ended.
// SHORT: the square roots and 1/t of the branches below take the guarded short forms of rtk_device_math.h -- by default in
// the lean MIXED f64 kernel alone; rtk_debug_scatter's kernel asks for them too, so that the known-answer tests reach them.
template <typename real, uint32_t FEAT>
constexpr bool kShortMath = sizeof(real) == 8 && (FEAT & ~uint32_t(F_MATTE)) == (kFeatLean | uint32_t(F_F32_BOX));
template <typename real, uint32_t FEAT, int FORCE_KIND = -1, bool SHORT = kShortMath<real, FEAT>, bool COUNT>
RTK_DEV bool shade_surface(Lane<real>& L, const Surface<real>& sf, const SceneView<real>& sc, const MaterialRec<real>* __restrict__ mats,
                           Counters<COUNT>& cnt RTK_SHADE_PROF_PARAM) {
    RTK_SHADE_PROF_BEGIN
    const MaterialRec<real>& m = mats[sf.material];
    const int mkind = FORCE_KIND >= 0 ? FORCE_KIND : m.kind;  // (FORCE_KIND: the instruction-cost probes compile one material's path alone, tools/isa_costs.py)
    const V3<real> rd = L.rd;

    V3<real> attenuation, next_d;
    bool scattered = true;
    // Code shared between material branches is hoisted in front of them, so that a wave whose lanes hold different
    // materials executes it once instead of once per branch:
    //  - lambertian and metal both start by drawing random_unit_vector() (material.h:30,84): three draws, a square
    //    root, a division;
    //  - metal normalises the reflected direction (material.h:83), dielectric and specular the incoming one
    //    (material.h:52,146): a square root and a division.
    // The hoisted values stay live across the branches; the kernels with instance transforms are already short of
    // registers (they spill), so those keep one copy per branch (kHoist = false).
    constexpr bool kHoist = (FEAT & F_XFORM) == 0;
    V3<real> ruv = mk(real(0), real(0), real(0)), unit_in = rd;
    if constexpr (kHoist) {
        if (mkind == RTK_MAT_LAMBERTIAN || mkind == RTK_MAT_METAL) ruv = random_unit_vector<real, SHORT>(L.rng, cnt);
        if (mkind == RTK_MAT_METAL) unit_in = reflect(rd, sf.normal);
        // (SHORT: the direction of a ray anyone may hand in, 1e-150 or 1e150 long -- guarded on its squared length)
        if (mkind == RTK_MAT_METAL || mkind == RTK_MAT_DIELECTRIC || ((FEAT & F_EXOTIC_MAT) && mkind == RTK_MAT_SPECULAR)) unit_in = unit_vector<SHORT>(unit_in);
    }
    if (mkind == RTK_MAT_LAMBERTIAN) {  // material.h:29-38
        if constexpr (!kHoist) ruv = random_unit_vector<real, SHORT>(L.rng, cnt);
        V3<real> dir = sf.normal + ruv;
        if (near_zero(dir)) dir = sf.normal;
        next_d = dir;
        attenuation = material_color<real, FEAT>(sc, m, sf.u, sf.v, sf.p, cnt);
    } else if (!(FEAT & F_MATTE) && mkind == RTK_MAT_METAL) {  // material.h:82-88
        if constexpr (!kHoist) {
            ruv = random_unit_vector<real, SHORT>(L.rng, cnt);
            unit_in = unit_vector<SHORT>(reflect(rd, sf.normal));
        }
        V3<real> fuzz = scale(m.param, ruv);
        next_d = unit_in + fuzz;
        attenuation = ld3(m.albedo);
        scattered = dot(next_d, sf.normal) > real(0);
    } else if (!(FEAT & F_MATTE) && mkind == RTK_MAT_DIELECTRIC) {  // material.h:47-65
        attenuation = mk(real(1), real(1), real(1));
        // 1/refraction_index and Schlick's r0^2 for both faces are per-material constants: computed once at upload,
        // in double, by the same expressions (material.h:50,71-72)
        const real ri = sf.front_face ? m.albedo[0] : m.param;
        if constexpr (!kHoist) unit_in = unit_vector<SHORT>(rd);
        const V3<real> unit_d = unit_in;
        const real cos_theta = rt_fmin(dot(-unit_d, sf.normal), real(1));
        const real sin_theta = sqrt_site<SHORT>(real(1) - cos_theta * cos_theta);  // (SHORT: exactly 0 at normal incidence -- guarded)
        bool reflect_it = ri * sin_theta > real(1);
        if (!reflect_it) {  // Schlick (material.h:69-74); the draw is skipped on total internal reflection
            const real r0 = sf.front_face ? m.albedo[1] : m.albedo[2];
            // Schlick's (1 - cos)^5 (material.h:73 calls pow) by multiplication, ~200 instructions less than pow in the
            // dielectric branch -- in f64 CORRECTLY ROUNDED (pow5: the products carried with their rounding errors), which is
            // what glibc's pow returns in 99.92 % of cases (tests/test_schlick_power.py; the plain ((x^2)^2)*x of rounds 1-2
            // agreed with it in 49 %).  The value only feeds the comparison with a 24-bit uniform below: a different outcome
            // needs pow's own misrounding AND the reflectance within an ulp of a multiple of 2^-24 -- ~1e-12 per dielectric
            // interaction, i.e. ~1e-4 per full C2 frame (it was ~1e-9 and 0.1-1 per frame).
            const real omc = real(1) - cos_theta;
            const real refl = r0 + (real(1) - r0) * pow5(omc);
            reflect_it = refl > rnd<real>(L.rng, cnt);
        }
        next_d = reflect_it ? reflect(unit_d, sf.normal) : refract<SHORT>(unit_d, sf.normal, ri);
    } else if ((FEAT & F_EXOTIC_MAT) && !(FEAT & F_MATTE) && mkind == RTK_MAT_ISOTROPIC) {  // material.h:129-134
        next_d = random_unit_vector<real>(L.rng, cnt);
        attenuation = material_color<real, FEAT>(sc, m, sf.u, sf.v, sf.p, cnt);
    } else if ((FEAT & F_EXOTIC_MAT) && !(FEAT & F_MATTE) && mkind == RTK_MAT_SPECULAR) {  // material.h:145-167
        if constexpr (!kHoist) unit_in = unit_vector(rd);
        const V3<real> unit_d = unit_in;
        const V3<real> refl = reflect(unit_d, sf.normal);
        V3<real> diffuse = random_unit_vector<real>(L.rng, cnt);  // random_on_hemisphere, vec3.h:116-124
        if (!(dot(diffuse, sf.normal) > real(0))) diffuse = -diffuse;
        const real f = call_pow(real(1) - dot(refl, unit_d), m.param);
        V3<real> dir = scale(f, refl) + scale(real(1) - f, diffuse);
        if (near_zero(dir)) dir = sf.normal;
        next_d = dir;
        attenuation = ld3(m.albedo);
    } else {  // diffuse_light / emissive_light: emits, never scatters (material.h:99-101,116-118)
        if (FEAT & F_EXOTIC_MAT) {
            V3<real> emitted = material_color<real, FEAT>(sc, m, sf.u, sf.v, sf.p, cnt);
            if constexpr (kNoRadianceState<FEAT>) L.sum = L.sum + L.throughput * emitted;  // = sum + (0 + throughput * emitted), the same bits
            else L.radiance = L.radiance + L.throughput * emitted;
        }
        return true;
    }
    RTK_SHADE_PROF(1)
    if (!scattered) return true;  // Camera.txt:223-225 (emission of a scattering material is zero)
    if ((FEAT & F_LIGHTS) && sc.n_lights > 0) {  // Camera.txt:228
        V3<real> lighting = attenuation * point_lighting(sc, sf.p, sf.normal);
        L.radiance = L.radiance + L.throughput * lighting;
    }
    L.throughput = L.throughput * attenuation;
    L.ro = sf.p;
    L.rd = next_d;
    L.depth -= 1;
    RTK_SHADE_PROF(3)
    return L.depth <= 0;  // Camera.txt:205-206: the next ray_color call returns black
}

// The traversal program ran to OP_END: the body of ray_color after world.hit
// (Camera.txt:211-237), iteratively (radiance = sum of throughput * emission).
// Returns true when the sample's path has ended.
// `hit_rec` = the record of the closest hit (program + L.best_pc; anything when there is none).
template <typename real, uint32_t FEAT, bool COUNT, typename ProgT>
RTK_DEV bool shade(Lane<real>& L, const ProgT* __restrict__ hit_rec, const SceneView<real>& sc, const MaterialRec<real>* __restrict__ mats,
                   const CameraRec<real>& cam, Counters<COUNT>& cnt RTK_SHADE_PROF_PARAM) {
    RTK_SHADE_PROF_BEGIN
    if (L.best_pc == kNoHit) {  // Camera.txt:211-213
        if constexpr (kNoRadianceState<FEAT>) L.sum = L.sum + L.throughput * ld3(cam.background);  // = sum + (0 + throughput * background), the same bits
        else L.radiance = L.radiance + L.throughput * ld3(cam.background);
        return true;
    }
    cnt.inc(C_SURFACE);
    RTK_SHADE_PROF(2)
    Surface<real> sf;
    if constexpr (std::is_same_v<ProgT, MixedHead> || std::is_same_v<ProgT, MixedImg>) make_surface_mixed(hit_rec, 0u, L.best_t, L.ro, L.rd, L.tm, sf);  // lean MIXED program
    else make_surface<real, FEAT>(hit_rec, sc, mats, 0u, L.best_t, L.ro, L.rd, L.tm, sf);                             // slot or COMPACT program
    RTK_SHADE_PROF(0)
    return shade_surface<real, FEAT>(L, sf, sc, mats, cnt RTK_SHADE_PROF_ARG);
}

// ------------------------------------------------------------------ kernel ----
// Persistent waves + a wave-level ballot scheduler.
//
// Each workgroup first stages the traversal program from HBM into LDS with
// coalesced 16-byte loads (when IN_LDS: the host checked it fits); then every
// wave repeatedly pulls the next work item -- an 8x8 tile of this rank x a chunk of
// 8 samples -- from an atomic counter.  A lane owns one pixel of the item and walks
// that chunk's samples in order; the resolve kernel adds a pixel's chunks in index
// order.  The sum is therefore a fixed function of (scene, camera, seed, pixel) --
// the image does not depend on which wave, workgroup or GPU rendered what -- but it
// is NOT the reference's left-to-right sum over all samples (Camera.txt:70-73): with
// chunked partial sums and the iterative throughput product the linear image agrees
// with the reference to ~1e-17 (asserted < 1e-12), and only the u8 bytes are equal.
//
// Paths have 1..max_depth segments and rays visit 1..100+ program records, so a
// lock-step "all lanes trace, then all lanes shade" loop leaves ~90 % of the
// lanes idle.  Instead each lane is a small state machine (Lane<real>) and in
// every iteration the wave VOTES (v_cmp + s_bcnt1 on the 64-bit ballots) on which
// kind of work has the most lanes ready -- box test, sphere test, another record
// kind, or shade/regenerate -- and runs only that, under a wave-uniform branch.
// Lanes waiting for a different kind keep their state and join a later vote; a
// lane whose path ends starts its next sample in the same shade step, so nobody
// waits for the longest path in the wave.  Scheduling changes only the
// interleaving between lanes, never a lane's own arithmetic, so the image is
// bit-identical to a lock-step execution.
enum Want : int { W_DONE = 0, W_BOX = 1, W_SPHERE = 2, W_OTHER = 3, W_SHADE = 4, W_QUAD = 5, W_TRI = 6 };

// Lane count of a ballot as a 32-bit scalar, one s_bcnt1_i32_b64.  With __builtin_popcountll the compiler
// carries the count as i64 and performs the vote's comparisons on the vector unit (v_cmp_lt_u64).
// A wave-uniform condition as a scalar branch: the compiler cannot always prove uniformity and would otherwise turn
// the branch into exec-mask bookkeeping.
RTK_DEV bool uniform(bool c) { return __builtin_amdgcn_readfirstlane(int(c)) != 0; }

RTK_DEV int popcount64(unsigned long long m) {
    int n;
    asm("s_bcnt1_i32_b64 %0, %1" : "=s"(n) : "s"(m) : "scc");
    return n;
}

// Diagnostic build only (tools/profile_phases.py compiles this file with -DRTK_PROFILE into a separate
// library): s_memtime stamps at the scheduler's phase boundaries; per phase the wave adds its cycles,
// step count and active-lane count to counters[3*phase .. 3*phase+2].  The product build has none of it.
#ifdef RTK_PROFILE
#define RTK_PROF_DECL unsigned long long prof_t[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, prof_n[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, prof_l[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; \
    unsigned long long prof_prev = __builtin_amdgcn_s_memtime();                                                                       \
    const unsigned long long prof_wall0 = wall_clock64();                                                                              \
    unsigned long long prof_wall_empty = 0, prof_chunk_t0 = 0;                                                                         \
    ShadeProf sprof;
#define RTK_PROF_CHUNK_BEGIN prof_chunk_t0 = wall_clock64();
#define RTK_PROF_CHUNK_END /* (pixel, chunk)s that ended after the work queue ran dry and took over 300 us: [31] count, then {begin, duration, segments, slot << 8 | pixel} from [32] on */ \
    {                                                                                                                                  \
        const unsigned long long dur_ = wall_clock64() - prof_chunk_t0;                                                                \
        if (prof_wall_empty != 0 && dur_ > 30000ull) {                                                                                                       \
            const unsigned long long i_ = atomicAdd(&counters[31], 1ull);                                                              \
            if (i_ < 4096ull) {                                                                                                        \
                counters[32 + 4 * i_] = prof_chunk_t0;                                                                                 \
                counters[33 + 4 * i_] = dur_;                                                                                          \
                counters[34 + 4 * i_] = (unsigned long long)(L.segs);                                                                  \
                counters[35 + 4 * i_] = ((unsigned long long)(my_slot) << 8) | (unsigned long long)(my_pix);                           \
            }                                                                                                                          \
        }                                                                                                                              \
    }
#define RTK_PROF_QUEUE_EMPTY \
    if (prof_wall_empty == 0) prof_wall_empty = wall_clock64();
#define RTK_PROF_MARK(phase, steps, lanes)                           \
    {                                                                \
        const unsigned long long now_ = __builtin_amdgcn_s_memtime(); \
        prof_t[phase] += now_ - prof_prev;                           \
        prof_n[phase] += (steps);                                    \
        prof_l[phase] += (lanes);                                    \
        prof_prev = now_;                                            \
    }
#define RTK_PROF_FLUSH                                                        \
    if (lane == 0)                                                            \
        for (int k_ = 0; k_ < 4; k_++) {                                      \
            atomicAdd(&counters[kShadeProfBase + 2 * k_], sprof.t[k_]);       \
            atomicAdd(&counters[kShadeProfBase + 2 * k_ + 1], sprof.n[k_]);   \
        }                                                                     \
    if (lane == 0)                                                            \
        for (int ph_ = 0; ph_ < 10; ph_++) { /* phases 6, 7 (parts of the shade step) live at [25..30], 8 and 9 behind the shade sub-phases */ \
            const int at_ = ph_ < 6 ? 3 * ph_ : (ph_ < 8 ? 25 + 3 * (ph_ - 6) : kShadeProfBase + 8 + 3 * (ph_ - 8)); \
            atomicAdd(&counters[at_], prof_t[ph_]);                           \
            atomicAdd(&counters[at_ + 1], prof_n[ph_]);                       \
            atomicAdd(&counters[at_ + 2], prof_l[ph_]);                       \
        }                                                                     \
    if (lane == 0) { /* wave lifetimes on the 100 MHz wall clock: [18] sum, [19] max, [20] sum of the time after the queue ran dry, [21] its max, [22] waves, [23] 2^62 - first start, [24] last end */ \
        const unsigned long long end_ = wall_clock64();                       \
        if (prof_wall_empty == 0) prof_wall_empty = end_;                     \
        atomicAdd(&counters[18], end_ - prof_wall0);                          \
        atomicMax(&counters[19], end_ - prof_wall0);                          \
        atomicAdd(&counters[20], end_ - prof_wall_empty);                     \
        atomicMax(&counters[21], end_ - prof_wall_empty);                     \
        atomicAdd(&counters[22], 1ull);                                       \
        atomicMax(&counters[23], (1ull << 62) - prof_wall0);                  \
        atomicMax(&counters[24], end_);                                       \
    }
#else
#define RTK_PROF_DECL
#define RTK_PROF_QUEUE_EMPTY
#define RTK_PROF_CHUNK_BEGIN
#define RTK_PROF_CHUNK_END
#define RTK_PROF_MARK(phase, steps, lanes)
#define RTK_PROF_FLUSH
#endif

// A finished (pixel, chunk): its sum of ray_color values goes to partial[item][3][64].
template <typename real>
RTK_DEV void store_partial(real* __restrict__ partial, int item, int pix, V3<real> sum) {
    real* base = partial + size_t(item) * 192 + pix;
    base[0] = sum.x;
    base[64] = sum.y;
    base[128] = sum.z;
}

// Wave priorities (s_setprio) by scheduler phase.  The SIMD's instruction arbiter serves the higher priority first (then the
// older wave); waves inside a traversal loop -- short dependent chains, an LDS round trip per step -- lose issue slots to
// waves that are in a shade step (long independent runs of arithmetic) exactly when a stall costs them most.  Measured on
// C2 (tools/ab, same box): no priorities 21.93-22.09 ms; box loop 1 / 2 / 3: 21.55 / 21.53 / 21.52; box 2 + sphere loop 1:
// 21.45-21.49 (kept); raising the shade step instead: 22.5.
constexpr int kBoxLoopPrio = 2, kSphereLoopPrio = 1, kPrimLoopPrio = 1;  // (prim: the quad and triangle loops)
// Box steps per trip around the box loop's scalar checks.  Measured per kernel (tools/ab): the MIXED sphere kernel
// (long runs of cheap box steps) 27.8 / 26.3 / 25.5 / 24.8 / 24.6 ms at 1 / 2 / 4 / 6 / 8; the reference-order
// kernels lose with any unrolling (C2 53.2 -> 54.8 at 4; C4 62.6 -> 64.2), the full-feature kernel gains 1 % at 2;
// the fused-slab sphere kernels (f32 mode, f64 fallback) behave like the MIXED one (f32: 20.6 -> 18.8 ms at 8).
constexpr int kUnrollMixed = 8;
// the boxes-in-LDS kernels: C4 49.9 / 48.2 / 47.8 / 49.7 ms at 1 / 2 / 4 / 8 (64 spp), C5 +0.8 % at 4
constexpr int kUnrollSplit = 4;
// the subset kernels, now that their primitive tests ride inside the loop: quad/box (C3) 30.5 / 29.4 / 30.7 ms at
// 1 / 2 / 4; mesh with the program in LDS (C4 f32) 28.8 / 25.5 / 25.3
constexpr int kUnrollQuadBox = 2, kUnrollMesh = 4, kUnrollCompactQuadBox = 2, kUnrollCompactMesh = 4;
// the lean kernel with the exact slab test (sphere scenes in the reference order): C2 50.7 / 50.0 / 52.0 ms at 1 / 2 / 4
constexpr int kUnrollLean = 2;
constexpr int kUnrollCold = 4;  // the hot/cold full-feature kernel: C5 45.8 / 42.9 / 42.2 / 42.5 / 42.8 ms at 1 / 2 / 4 / 6 / 8
// Lanes of a wave that must sit on a triangle / quad record for those tests to ride along inside the box loop (the
// measurements are beside the two blocks).
constexpr int kTriRide = 16, kQuadRide = 16;
#ifndef RTK_DEV_MASK_OFF
#define RTK_DEV_MASK_OFF 0u   // register-pressure experiments (tools/kernel_resources.py): feature bits compiled out of every kernel
#endif

// The render kernel's body is rtk_render_body.inc: the view kernel below runs the same text.
template <typename real, uint32_t FEAT_ALL, bool COUNT, bool IN_LDS>
__global__ __launch_bounds__(kernel_choice::max_threads(sizeof(real), FEAT_ALL, IN_LDS)) void rtk_render_kernel(SceneView<real> sc, const CameraRec<real>* __restrict__ cam_ptr, TileMap tmap, uint32_t seed,
                                                          real* __restrict__ partial, unsigned long long* __restrict__ counters,
                                                          unsigned int* __restrict__ tile_counter, const int32_t* __restrict__ tile_order,
                                                          unsigned int* __restrict__ tile_cost, uint32_t diag) {
#define RTK_BODY_VIEWS 0
#include "rtk_render_body.inc"
#undef RTK_BODY_VIEWS
}

// View batches (include/rtk.h "View batches"): the same body over work items (view, tile, chunk) of n_views frames of one size.
// tmap.tiles_x / tiles_y are a view's grid, tmap.n_tiles_local = n_views * tiles (rank 0 of 1), so a partial sum lands in
// partial[chunk][view * tiles + tile][3][64]; no tile order, no tile cost, no counters (a counting batch is rendered view by
// view with the plain kernel).  No static LDS here either: the lean MIXED form uses byte pcs as LDS addresses.
template <typename real, uint32_t FEAT_ALL, bool IN_LDS>
__global__ __launch_bounds__(kernel_choice::max_threads(sizeof(real), FEAT_ALL, IN_LDS)) void rtk_view_batch_kernel(SceneView<real> sc, const ViewRec<real>* __restrict__ views, TileMap tmap,
                                                                                                   real* __restrict__ partial, unsigned int* __restrict__ tile_counter,
                                                                                                   uint32_t diag) {
    constexpr bool COUNT = sizeof(real) == 0;  // false, and dependent: the body's `if constexpr (COUNT)` branches are not instantiated
    [[maybe_unused]] unsigned long long* const counters = nullptr;
    [[maybe_unused]] const int32_t* const tile_order = nullptr;
    [[maybe_unused]] unsigned int* const tile_cost = nullptr;
    [[maybe_unused]] const uint32_t seed = 0u;
#define RTK_BODY_VIEWS 1
#include "rtk_render_body.inc"
#undef RTK_BODY_VIEWS
}

// hittable::hit of the scene root on the query interval L.tmin .. L.best_t (set up by begin_segment<true>): the slot program
// walked one lane at a time, with every record kind and the tie table (inert for reference-order uploads).  L.best_pc /
// L.best_t hold the winner.  The known-answer entry point and the AOV pass share it.
// ANY_HIT (rtk_query_occluded, programs without media only): the walk stops at the first accepted hit -- without a medium
// bracket nothing ever takes a winner back, so whether there is one is settled then.
template <bool ANY_HIT = false, typename real, bool COUNT>
RTK_DEV void closest_hit_slots(Lane<real>& L, const SceneView<real>& sc, Counters<COUNT>& cnt) {
    const Slot<real>* prog = sc.program;
    auto kind_of = [&](uint32_t pc) -> uint32_t { return prog[pc].kind_payload & 15u; };
    const TieCtx<true, decltype(kind_of)> tie{sc.tie_rank_slot, kind_of};  // inert (null table) for reference-order uploads
    for (;;) {
        if constexpr (ANY_HIT)
            if (L.best_pc != kNoHit) break;
        const Slot<real>* rec = prog + L.pc;
        const uint32_t kind = rec->kind_payload & 15u;
        if (kind == OP_END) break;
        if (kind == OP_BOX) {
            if (L.box_kind == OP_BOX) step_box<false, true>(L, *rec, cnt);
            else step_box<true, true>(L, *rec, cnt);
        } else if (kind == OP_SPHERE) {
            step_sphere<true, sizeof(real) == 8>(L, *rec, cnt, tie);  // f64: the guarded short square root (rtk_device_math.h), which the known-answer tests reach here
        } else {
            step_other<real, kFeatAll>(L, rec, sc, cnt, tie);
        }
    }
}

// ------------------------------------------------------------------ lane-per-ray kernels --
// One lane per ray or pixel, next to the persistent render kernel: the known-answer (rtk_debug_*), AOV / guide and ray-query
// kernels.  What they share (DESIGN.md "What a lane-per-ray kernel is made of"):

// The stream of keys (seed, pixel, sample), the keying of the render's samples: seed_hash = pcg_hash(seed).
RTK_DEV uint32_t stream_key(uint32_t seed_hash, uint32_t pixel, uint32_t sample) { return pcg_hash(pixel + pcg_hash(sample + seed_hash)); }
// keys[3] = seed, pixel, sample of one known-answer case
RTK_DEV uint32_t stream_key(const uint32_t* __restrict__ keys) { return stream_key(pcg_hash(keys[0]), keys[1], keys[2]); }

// r[7] = origin, direction, time -> the lane's world-space ray.
template <typename real>
RTK_DEV void load_ray(Lane<real>& L, const double* __restrict__ r) {
    L.ro = mk(real(r[0]), real(r[1]), real(r[2]));
    L.rd = mk(real(r[3]), real(r[4]), real(r[5]));
    L.tm = real(r[6]);
}

// No outer query of a constant medium is parked (Lane::sv_*): the state a path starts in.
template <typename real>
RTK_DEV void clear_parked(Lane<real>& L) {
    L.sv_tmin = L.sv_best_t = L.rec1_t = real(0);
    L.sv_best_pc = kNoHit;
}

// ... and world.hit(r, interval(0.001, inf), rec) of L.ro / L.rd begins: closest_hit_slots comes next.
template <typename real, bool COUNT>
RTK_DEV void begin_walk(Lane<real>& L, Counters<COUNT>& cnt) {
    clear_parked(L);
    begin_segment<true>(L, cnt);
}

// Lens models (include/rtk.h "Lens models"): the primary ray of sample `sample` of pixel (i, j) through another projection than
// get_ray's.  The rule of the three film models: three draws from the sample's stream, then double arithmetic in both real
// modes, contraction off whatever the flags of the kernel it lands in, nothing renormalised.
struct LensLocal { double x, y, z; };
#ifndef RTK_LENS_INLINE
#define RTK_LENS_LOCAL RTK_NOINLINE   // (tools/kernel_resources.py -DRTK_LENS_INLINE: the inlined form DESIGN.md compares it with)
#else
#define RTK_LENS_LOCAL RTK_DEV
#endif
// The local direction at film coordinates (x, y) of EQUIRECT and FISHEYE; aspect = double(H) / double(W).  Out of line, on
// scalars alone and returned in registers: the double sin / cos carry a large-argument path that the path-loop kernels would
// otherwise pay for in registers (DESIGN.md "lens models" has the counts), as the render kernels keep acos / atan2 / sin out.
RTK_LENS_LOCAL LensLocal lens_local(int model, double half_h, double half_v, double aspect, double x, double y) {
#pragma clang fp contract(off)
    LensLocal l{0.0, 0.0, -1.0};
    if (model == RTK_LENS_EQUIRECT) {
        const double lon = x * half_h, lat = y * half_v, c = cos(lat);
        l.x = c * sin(lon);
        l.y = sin(lat);
        l.z = -(c * cos(lon));
    } else {  // RTK_LENS_FISHEYE
        const double yy = y * aspect;
        const double rr = rt_sqrt(x * x + yy * yy);
        if (rr != 0.0) {
            const double theta = rr * half_h, st = sin(theta);
            l.x = st * (x / rr);
            l.y = st * (yy / rr);
            l.z = -cos(theta);
        }
    }
    return l;
}

// r[7] = origin, direction, time of the film models; rng = the sample's stream, left three draws on.
RTK_DEV void lens_film_ray(const LensRec& lens, int width, int height, int i, int j, uint32_t& rng, double* __restrict__ r) {
#pragma clang fp contract(off)
    Counters<false> cnt;
    const double oy = rnd<double>(rng, cnt) - 0.5;
    const double ox = rnd<double>(rng, cnt) - 0.5;
    r[6] = rnd<double>(rng, cnt);
    const double x = 2.0 * ((double(i) + ox) + 0.5) / double(width) - 1.0;
    const double y = 1.0 - 2.0 * ((double(j) + oy) + 0.5) / double(height);
    LensLocal l{0.0, 0.0, -1.0};
    r[0] = lens.center[0]; r[1] = lens.center[1]; r[2] = lens.center[2];
    if (lens.model == RTK_LENS_ORTHOGRAPHIC) {
        const double ax = x * lens.half_h, ay = y * lens.half_v;
        for (int k = 0; k < 3; k++) r[k] = (lens.center[k] + ax * lens.u[k]) + ay * lens.v[k];
    } else {
        l = lens_local(lens.model, lens.half_h, lens.half_v, double(height) / double(width), x, y);
    }
    for (int k = 0; k < 3; k++) r[3 + k] = (l.x * lens.u[k] + l.y * lens.v[k]) + l.z * lens.w[k];
}

// The one function behind rtk_lens_rays, rtk_lens_render and the lens forms of the AOV / guide kernel: the lane's ray, its
// stream where ray generation left it, and the start of a path (radiance, throughput, depth, as begin_sample leaves them); the
// record's reals in double in r[7]; returns the record's skip.  PERSPECTIVE is begin_sample itself, in `real`, and the record its
// values widened; the film models compute the record and the lane takes it rounded to `real`, as load_query_ray would.
template <typename real>
RTK_DEV uint32_t lens_begin(Lane<real>& L, const LensRec& lens, const CameraRec<real>& cam, int i, int j, uint32_t sample, uint32_t seed_hash,
                            double* __restrict__ r) {
    L.s = int(sample);
    if (lens.model == RTK_LENS_PERSPECTIVE) {
        Counters<true> cnt;
        cnt.clear();
        begin_sample(L, cam, i, j, seed_hash, cnt);
        r[0] = double(L.ro.x); r[1] = double(L.ro.y); r[2] = double(L.ro.z);
        r[3] = double(L.rd.x); r[4] = double(L.rd.y); r[5] = double(L.rd.z);
        r[6] = double(L.tm);
        return cnt.c[C_RNG];
    }
    L.rng = stream_key(seed_hash, uint32_t(j * cam.width + i), sample);
    lens_film_ray(lens, cam.width, cam.height, i, j, L.rng, r);
    load_ray(L, r);
    L.radiance = mk(real(0), real(0), real(0));
    L.throughput = mk(real(1), real(1), real(1));
    L.depth = cam.max_depth;
    return 3u;
}

// The sample generators of rtk_guide_kernel: sample L.s of pixel (i, j) from the render's camera, or through a lens.
struct CameraSamples {
    template <typename real, bool COUNT>
    RTK_DEV void begin(Lane<real>& L, const CameraRec<real>& cam, int i, int j, uint32_t seed_hash, Counters<COUNT>& cnt) const {
        begin_sample(L, cam, i, j, seed_hash, cnt);
    }
};
struct LensSamples {
    LensRec lens;
    template <typename real, bool COUNT>
    RTK_DEV void begin(Lane<real>& L, const CameraRec<real>& cam, int i, int j, uint32_t seed_hash, Counters<COUNT>&) const {
        double r[7];
        (void)lens_begin(L, lens, cam, i, j, uint32_t(L.s), seed_hash, r);
    }
};

// hittable::hit(r, interval(tmin, tmax), rec) of the scene root for r[9] = origin, direction, time, tmin, tmax: the one walk
// behind rtk_debug_closest_hit, rtk_query_hits and rtk_query_occluded.  The lane holds the ray (load_ray) and L.rng, the stream
// a constant medium draws from; L.best_pc / L.best_t hold the winner afterwards, cnt.c[C_RNG] the draws.
template <bool ANY_HIT = false, typename real>
RTK_DEV void query_closest(Lane<real>& L, const double* r, const SceneView<real>& sc, Counters<true>& cnt) {
    cnt.clear();
    L.segs = 0;
    begin_walk(L, cnt);
    L.tmin = real(r[7]);
    L.best_t = real(r[8]);
    closest_hit_slots<ANY_HIT>(L, sc, cnt);
}

// The hit_record of the walk's winner (L.best_pc != kNoHit), u and v included.
template <typename real>
RTK_DEV Surface<real> hit_surface(const Lane<real>& L, const SceneView<real>& sc) {
    Surface<real> sf;
    make_surface<real, kFeatAll>(sc.program, sc, sc.materials, L.best_pc, L.best_t, L.ro, L.rd, L.tm, sf, true);
    return sf;
}

// Known-answer entry point (tests): hittable::hit(r, interval(tmin, tmax), rec) of the uploaded scene's root for
// caller-supplied rays with a stream of keys each -- query_closest, as rtk_query_hits_kernel runs it for one seed and a skip.
// out[12] = hit, t, p(3), normal(3), front_face, u, v, material.
template <typename real>
__global__ __launch_bounds__(256) void rtk_debug_hit_kernel(SceneView<real> sc, int n, const double* __restrict__ rays, const uint32_t* __restrict__ keys,
                                                             double* __restrict__ out, unsigned long long* __restrict__ draws) {
    const int gid = blockIdx.x * 256 + threadIdx.x;
    if (gid >= n) return;
    Counters<true> cnt;
    Lane<real> L;
    const double* r = rays + size_t(gid) * 9;
    load_ray(L, r);
    L.rng = stream_key(keys + gid * 3);
    query_closest(L, r, sc, cnt);
    double* o = out + size_t(gid) * 12;
    for (int k = 0; k < 12; k++) o[k] = 0.0;
    o[11] = -1.0;
    if (L.best_pc != kNoHit) {
        const Surface<real> sf = hit_surface(L, sc);
        o[0] = 1.0;
        o[1] = double(L.best_t);
        o[2] = double(sf.p.x); o[3] = double(sf.p.y); o[4] = double(sf.p.z);
        o[5] = double(sf.normal.x); o[6] = double(sf.normal.y); o[7] = double(sf.normal.z);
        o[8] = sf.front_face ? 1.0 : 0.0;
        o[9] = double(sf.u); o[10] = double(sf.v);
        o[11] = double(sf.material);
    }
    draws[gid] = cnt.c[C_RNG];
}

// Known-answer entry points for the shading side (tests): the very device functions the render kernel executes --
// shade_surface (material::scatter / emitted, material.h:22-172), texture_value (texture.h:20-120, perlin.h:14-50) and
// begin_sample (get_ray, Camera.txt:177-200) -- on caller-supplied inputs, one lane per case.
//   scatter: mat[n]; ray[n][7] = origin, direction, time; rec[n][11] = t, p(3), normal(3), front_face, u, v, -;
//            out[n][14] = scattered?, scattered ray origin(3) direction(3), attenuation(3), time, emitted(3)
template <typename real>
__global__ __launch_bounds__(256) void rtk_debug_scatter_kernel(SceneView<real> sc, int n, const int32_t* __restrict__ mat, const double* __restrict__ ray,
                                                                 const double* __restrict__ rec, const uint32_t* __restrict__ keys, double* __restrict__ out,
                                                                 unsigned long long* __restrict__ draws) {
    const int gid = blockIdx.x * 256 + threadIdx.x;
    if (gid >= n) return;
    sc.n_lights = 0;  // get_lighting (Camera.txt:228) belongs to ray_color, not to scatter()
    Counters<true> cnt;
    cnt.clear();
    const double* h = rec + size_t(gid) * 11;
    Lane<real> L;
    load_ray(L, ray + size_t(gid) * 7);
    L.rng = stream_key(keys + gid * 3);
    L.throughput = mk(real(1), real(1), real(1));
    L.radiance = mk(real(0), real(0), real(0));
    L.sum = mk(real(0), real(0), real(0));
    L.depth = 1 << 20;
    Surface<real> sf;
    sf.p = mk(real(h[1]), real(h[2]), real(h[3]));
    sf.normal = mk(real(h[4]), real(h[5]), real(h[6]));
    sf.front_face = h[7] != 0.0;
    sf.u = real(h[8]);
    sf.v = real(h[9]);
    sf.material = mat[gid];
#ifdef RTK_PROFILE
    ShadeProf sprof;  // (the profile build's shade functions take their sub-phase accumulators)
#endif
    const bool ended = shade_surface<real, kFeatAll, -1, sizeof(real) == 8>(L, sf, sc, sc.materials, cnt RTK_SHADE_PROF_ARG);  // f64: with the short forms
    double* o = out + size_t(gid) * 14;
    o[0] = ended ? 0.0 : 1.0;
    o[1] = double(L.ro.x); o[2] = double(L.ro.y); o[3] = double(L.ro.z);
    o[4] = double(L.rd.x); o[5] = double(L.rd.y); o[6] = double(L.rd.z);
    o[7] = double(L.throughput.x); o[8] = double(L.throughput.y); o[9] = double(L.throughput.z);
    o[10] = double(L.tm);
    o[11] = double(L.radiance.x); o[12] = double(L.radiance.y); o[13] = double(L.radiance.z);
    draws[gid] = cnt.c[C_RNG];
}
//   texture: tex[n]; uvp[n][5] = u, v, p(3); out[n][3] = texture::value(u, v, p); work[n][2] = perlin::noise calls, texel fetches
template <typename real>
__global__ __launch_bounds__(256) void rtk_debug_texture_kernel(SceneView<real> sc, int n, const int32_t* __restrict__ tex, const double* __restrict__ uvp,
                                                                 double* __restrict__ out, unsigned long long* __restrict__ work) {
    const int gid = blockIdx.x * 256 + threadIdx.x;
    if (gid >= n) return;
    Counters<true> cnt;
    cnt.clear();
    const double* q = uvp + size_t(gid) * 5;
    const V3<real> c = texture_value(sc, tex[gid], real(q[0]), real(q[1]), mk(real(q[2]), real(q[3]), real(q[4])), cnt);
    out[size_t(gid) * 3] = double(c.x);
    out[size_t(gid) * 3 + 1] = double(c.y);
    out[size_t(gid) * 3 + 2] = double(c.z);
    work[size_t(gid) * 2] = cnt.c[C_NOISE];
    work[size_t(gid) * 2 + 1] = cnt.c[C_TEXEL];
}
//   get_ray: ijs[n][3] = pixel i, j, sample; out[n][7] = origin, direction, time
template <typename real>
__global__ __launch_bounds__(256) void rtk_debug_get_ray_kernel(CameraRec<real> cam, uint32_t seed, int n, const int32_t* __restrict__ ijs, double* __restrict__ out,
                                                                 unsigned long long* __restrict__ draws) {
    const int gid = blockIdx.x * 256 + threadIdx.x;
    if (gid >= n) return;
    Counters<true> cnt;
    cnt.clear();
    Lane<real> L;
    L.s = ijs[gid * 3 + 2];
    begin_sample(L, cam, ijs[gid * 3], ijs[gid * 3 + 1], pcg_hash(seed), cnt);
    double* o = out + size_t(gid) * 7;
    o[0] = double(L.ro.x); o[1] = double(L.ro.y); o[2] = double(L.ro.z);
    o[3] = double(L.rd.x); o[4] = double(L.rd.y); o[5] = double(L.rd.z);
    o[6] = double(L.tm);
    draws[gid] = cnt.c[C_RNG];
}

// ------------------------------------------------------------------ guide buffers --
// First-hit guide buffers (AOVs) of the denoiser and their mirror-following form (include/rtk.h, rtk_render_aovs and
// rtk_render_guides): one kernel body, rtk_guide_kernel<real, CHAIN>, one lane per pixel on the image passes' tile grid
// (rtk_image_pass.h).  Sample s of pixel (i, j) takes the render's primary ray -- begin_sample with the render's seed, bit for
// bit.  Segment b of the sample (CHAIN = false: b = 0 alone) re-seeds its stream with keys (seed, pixel, 2^31 + (2b << 20) + s),
// as rtk_debug_closest_hit does, so a constant medium never draws the render's numbers, and finds world.hit(r, interval(0.001,
// inf)) (Camera.txt:211) with the known-answer traversal.  Sums run in `real` in sample order and are divided by their count
// once.  What b = 0 finds is the first-hit record, out[px][0..7], the same instructions in both instantiations:
//   [0..2] albedo: miss -> background clamped to [0, 1]; lambertian / isotropic -> texture::value; metal / specular ->
//          albedo; dielectric -> 1; diffuse_light -> min(1, texture::value)    (mean over n)
//   [3]    hits / n (medium hits count)
//   [4..6] sum over hits of the record's normal (isotropic hits add 0) / n
//   [7]    mean over hits of t * |rd| (0 without hits)
// CHAIN adds the surface a chain of followed specular hits ends on, out[px][8..15].  A followed hit (a mirror or glass, by
// `follow`) with b < max_bounces runs material::scatter on the stream of keys (seed, pixel, 2^31 + ((2b + 1) << 20) + s) --
// shade_surface without point lights as rtk_debug_scatter runs it, compiled for the two followed kinds alone (FORCE_KIND: no
// texture code in the chain); L.throughput carries T.  A hit that is not followed, or does not scatter, ends the chain:
//   [8..10]  seen albedo: T * (albedo rule of the end hit, or the clamped background), mean over n
//   [11]     end hits / n
//   [12..14] sum over end hits of the record's normal (isotropic: 0) / n
//   [15]     mean over end hits of the path length sum_b t_b |rd_b| (0 without end hits)
template <typename real>
RTK_DEV real clamp01(real x) { return x < real(0) ? real(0) : (x > real(1) ? real(1) : x); }

template <typename real>
RTK_DEV V3<real> clamped_background(const CameraRec<real>& cam) {
    return mk(clamp01(cam.background[0]), clamp01(cam.background[1]), clamp01(cam.background[2]));
}

// The albedo rule of a hit on material m.
template <typename real, bool COUNT>
RTK_DEV V3<real> first_hit_albedo(const SceneView<real>& sc, const MaterialRec<real>& m, const Surface<real>& sf, Counters<COUNT>& cnt) {
    const int kind = m.kind;
    V3<real> a = mk(real(1), real(1), real(1));  // dielectric
    if (kind == RTK_MAT_LAMBERTIAN || kind == RTK_MAT_ISOTROPIC || kind == RTK_MAT_DIFFUSE_LIGHT) {
        a = material_color<real, kFeatAll>(sc, m, sf.u, sf.v, sf.p, cnt);
        if (kind == RTK_MAT_DIFFUSE_LIGHT) a = mk(a.x > real(1) ? real(1) : a.x, a.y > real(1) ? real(1) : a.y, a.z > real(1) ? real(1) : a.z);
    } else if (kind == RTK_MAT_METAL || kind == RTK_MAT_SPECULAR) {
        a = ld3(m.albedo);
    }
    return a;
}

// One record of eight: the sums over a pixel's samples and their two float4.
template <typename real>
struct HitSums {
    V3<real> albedo = mk(real(0), real(0), real(0)), normal = mk(real(0), real(0), real(0));
    real hits = real(0), len = real(0);
    RTK_DEV void miss(V3<real> colour) { albedo = albedo + colour; }
    RTK_DEV void hit(V3<real> colour, V3<real> nrm, real length) {
        albedo = albedo + colour;
        hits = hits + real(1);
        normal = normal + nrm;
        len = len + length;
    }
    RTK_DEV void write(float4* __restrict__ o, real n) const {
        o[0] = make_float4(float(albedo.x / n), float(albedo.y / n), float(albedo.z / n), float(hits / n));
        o[1] = make_float4(float(normal.x / n), float(normal.y / n), float(normal.z / n), hits > real(0) ? float(len / hits) : 0.0f);
    }
};

// follow / max_bounces: read by CHAIN alone.  out holds two float4 per pixel, four with CHAIN.  gen makes the primary ray of
// sample L.s: CameraSamples (begin_sample: rtk_render_aovs / _guides) or LensSamples (rtk_lens_aovs / _guides).
template <typename real, bool CHAIN, typename Gen>
__global__ __launch_bounds__(256) void rtk_guide_kernel(TileGrid grid, SceneView<real> sc, CameraRec<real> cam, uint32_t seed, int n_samples, int follow,
                                                         int max_bounces, float4* __restrict__ out, Gen gen) {
    int i, j;
    if (!lane_pixel(grid, i, j)) return;
    if constexpr (CHAIN) sc.n_lights = 0;  // get_lighting (Camera.txt:228) belongs to ray_color, not to scatter()
    Counters<false> cnt;
    const uint32_t seed_hash = pcg_hash(seed);
    const uint32_t pixel = uint32_t(j * cam.width + i);
    HitSums<real> first, end;
#ifdef RTK_PROFILE
    ShadeProf sprof;  // (the profile build's shade functions take their sub-phase accumulators)
#endif
    for (int s = 0; s < n_samples; s++) {
        Lane<real> L;
        L.s = s;
        L.segs = 0;
        gen.begin(L, cam, i, j, seed_hash, cnt);
        if constexpr (CHAIN) L.depth = 1 << 20;  // (the chain is capped by max_bounces, not by the camera's max_depth)
        [[maybe_unused]] real len = real(0);
        for (int b = 0;; b++) {
            const uint32_t key = 0x80000000u + (uint32_t(2 * b) << 20) + uint32_t(s);
            L.rng = stream_key(seed_hash, pixel, key);
            begin_walk(L, cnt);
            closest_hit_slots(L, sc, cnt);
            if (L.best_pc == kNoHit) {
                const V3<real> bg = clamped_background(cam);
                if (b == 0) first.miss(bg);
                if constexpr (CHAIN) end.miss(L.throughput * bg);
                break;
            }
            const Surface<real> sf = hit_surface(L, sc);
            const MaterialRec<real>& m = sc.materials[sf.material];
            const int mkind = m.kind;
            const real seg = L.best_t * rt_sqrt(length_squared(L.rd));
            if constexpr (CHAIN) len = len + seg;
            const V3<real> a = first_hit_albedo(sc, m, sf, cnt);
            const V3<real> nrm = mkind != RTK_MAT_ISOTROPIC ? sf.normal : mk(real(0), real(0), real(0));
            if (b == 0) first.hit(a, nrm, seg);
            if constexpr (CHAIN) {
                const bool mirror = (follow & RTK_GUIDE_FOLLOW_MIRROR) && mkind == RTK_MAT_METAL && m.param == real(0);
                const bool glass = (follow & RTK_GUIDE_FOLLOW_DIELECTRIC) && mkind == RTK_MAT_DIELECTRIC;
                if ((mirror || glass) && b < max_bounces) {
                    L.rng = stream_key(seed_hash, pixel, key + (1u << 20));
                    const bool ended = mirror ? shade_surface<real, kFeatAll, RTK_MAT_METAL>(L, sf, sc, sc.materials, cnt RTK_SHADE_PROF_ARG)
                                              : shade_surface<real, kFeatAll, RTK_MAT_DIELECTRIC>(L, sf, sc, sc.materials, cnt RTK_SHADE_PROF_ARG);
                    if (!ended) continue;  // L.ro / L.rd = the scattered ray, L.throughput = T * attenuation, L.tm kept
                }
                end.hit(L.throughput * a, nrm, len);
            }
            break;
        }
    }
    const real n = real(n_samples);
    float4* o = out + (size_t(j) * cam.width + i) * (CHAIN ? 4 : 2);
    first.write(o, n);
    if constexpr (CHAIN) end.write(o + 2, n);
}

// ------------------------------------------------------------------ ray queries --
// Hits, occlusion and radiance for rays the caller chooses (include/rtk.h "Ray queries"): one lane per ray, on the slot program
// with every record kind, through the functions the known-answer, AOV and guide kernels run.  A ray record (rtk_ray, 88 bytes,
// 8-byte aligned) is read as eleven 8-byte words: origin, direction, time, tmin, tmax, {pixel, sample}, {skip, reserved}.
// Lanes of a wave walk different paths; one whose path has ended idles until its wave is done (no refill).

// The state the generator reaches from `state` after n draws (rnd: s <- a s + c), by squaring the step: at most 32 rounds for
// any n (Brown, "Random number generation with arbitrary strides", 1994).
RTK_DEV uint32_t rng_skip(uint32_t state, uint32_t n) {
    uint32_t mult = 747796405u, plus = 2891336453u, acc_mult = 1u, acc_plus = 0u;
    for (; n != 0u; n >>= 1) {
        if (n & 1u) {
            acc_mult *= mult;
            acc_plus = acc_plus * mult + plus;
        }
        plus = (mult + 1u) * plus;
        mult *= mult;
    }
    return acc_mult * state + acc_plus;
}

// A ray record -> the lane's ray and its stream: keys (seed, pixel, sample + sample_offset), advanced by skip.  With offset 0
// and skip 0 that is rtk_debug_hit_kernel's stream_key(keys) for keys = {seed, pixel, sample}.
template <typename real>
RTK_DEV void load_query_ray(Lane<real>& L, const double* __restrict__ r, uint32_t seed_hash, uint32_t sample_offset) {
    const uint2 key = *reinterpret_cast<const uint2*>(r + 9), skip = *reinterpret_cast<const uint2*>(r + 10);
    load_ray(L, r);
    L.rng = rng_skip(stream_key(seed_hash, key.x, key.y + sample_offset), skip.x);
}

// hittable::hit(r, interval(tmin, tmax), rec) of the scene root on device buffers.  A hit record (rtk_ray_hit, 96 bytes) is
// written as nine doubles and three pairs of 32-bit integers.
template <typename real>
__global__ __launch_bounds__(256) void rtk_query_hits_kernel(SceneView<real> sc, uint32_t seed, long long n, const double* __restrict__ rays,
                                                              double* __restrict__ hits) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= n) return;
    const double* r = rays + gid * 11;
    Counters<true> cnt;
    Lane<real> L;
    load_query_ray(L, r, pcg_hash(seed), 0u);
    query_closest(L, r, sc, cnt);
    double* o = hits + gid * 12;
    int2* oi = reinterpret_cast<int2*>(o + 9);
    if (L.best_pc == kNoHit) {
        for (int k = 0; k < 9; k++) o[k] = 0.0;
        oi[0] = make_int2(0, 0);
        oi[1] = make_int2(-1, 0);
        oi[2] = make_int2(-1, int(cnt.c[C_RNG]));
        return;
    }
    const Surface<real> sf = hit_surface(L, sc);
    // the winner's record names its primitive: the payload is the index into the description's table of its kind
    const uint32_t kp = sc.program[L.best_pc].kind_payload, kind = kp & 15u;
    const int node_kind = (kind == OP_SPHERE || kind == OP_SPHERE_MOVING) ? RTK_NODE_SPHERE
                          : (kind == OP_QUAD ? RTK_NODE_QUAD : (kind == OP_TRI ? RTK_NODE_TRIANGLE : RTK_NODE_MEDIUM));
    o[0] = double(L.best_t);
    o[1] = double(sf.p.x); o[2] = double(sf.p.y); o[3] = double(sf.p.z);
    o[4] = double(sf.normal.x); o[5] = double(sf.normal.y); o[6] = double(sf.normal.z);
    o[7] = double(sf.u); o[8] = double(sf.v);
    oi[0] = make_int2(1, sf.front_face ? 1 : 0);
    oi[1] = make_int2(sf.material, node_kind);
    oi[2] = make_int2(int(kp >> 4), int(cnt.c[C_RNG]));
}

// The hit flag of rtk_query_hits_kernel for the same ray, keys and skip.  ANY_HIT: the program holds no medium (the launcher
// knows the scene's features), and the walk ends at the first accepted hit.
template <typename real, bool ANY_HIT>
__global__ __launch_bounds__(256) void rtk_query_occluded_kernel(SceneView<real> sc, uint32_t seed, long long n, const double* __restrict__ rays,
                                                                  int32_t* __restrict__ occluded) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= n) return;
    const double* r = rays + gid * 11;
    Counters<true> cnt;
    Lane<real> L;
    load_query_ray(L, r, pcg_hash(seed), 0u);
    query_closest<ANY_HIT>(L, r, sc, cnt);
    occluded[gid] = L.best_pc != kNoHit ? 1 : 0;
}

// ray_color(r, max_depth, world, lights) (Camera.txt:203-238), iteratively, as the render kernels run it: begin_segment,
// world.hit on interval(0.001, inf), shade -- until the path ends.  cam carries background, max_depth and spp = the samples per
// ray; sample s of a ray draws from the stream (seed, pixel, sample + s) advanced by skip.  The sum runs in sample order and
// is divided once.  COUNT: draws[k] = the uniforms the paths of ray k drew.
// The path of the ray and stream a lane holds (L.ro, L.rd, L.tm, L.rng; radiance 0, throughput 1, depth = max_depth), to its end:
// the loop the radiance query, the probe bake and the lens frames share.  L.radiance is ray_color's value afterwards.
template <typename real, bool COUNT>
RTK_DEV void trace_path(Lane<real>& L, const SceneView<real>& sc, const CameraRec<real>& cam, Counters<COUNT>& cnt RTK_SHADE_PROF_PARAM) {
    clear_parked(L);
    L.segs = 0;
    while (L.depth > 0) {
        begin_segment<true>(L, cnt);
        closest_hit_slots(L, sc, cnt);
        const Slot<real>* hit_rec = sc.program + (L.best_pc != kNoHit ? L.best_pc : 0u);
        if (shade<real, kFeatAll, COUNT>(L, hit_rec, sc, sc.materials, cam, cnt RTK_SHADE_PROF_ARG)) break;
    }
}

template <typename real, bool COUNT>
__global__ __launch_bounds__(256) void rtk_query_radiance_kernel(SceneView<real> sc, CameraRec<real> cam, uint32_t seed, long long n,
                                                                  const double* __restrict__ rays, real* __restrict__ radiance, uint32_t* __restrict__ draws) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= n) return;
    const double* r = rays + gid * 11;
    Counters<COUNT> cnt;
    cnt.clear();
#ifdef RTK_PROFILE
    ShadeProf sprof;  // (the profile build's shade functions take their sub-phase accumulators)
#endif
    const uint32_t seed_hash = pcg_hash(seed);
    V3<real> sum = mk(real(0), real(0), real(0));
    for (int s = 0; s < cam.spp; s++) {
        Lane<real> L;
        load_query_ray(L, r, seed_hash, uint32_t(s));
        L.radiance = mk(real(0), real(0), real(0));
        L.throughput = mk(real(1), real(1), real(1));
        L.depth = cam.max_depth;
        trace_path(L, sc, cam, cnt RTK_SHADE_PROF_ARG);
        sum = sum + L.radiance;
    }
    const real ns = real(cam.spp);
    real* o = radiance + gid * 3;
    o[0] = sum.x / ns;
    o[1] = sum.y / ns;
    o[2] = sum.z / ns;
    if constexpr (COUNT) draws[gid] = cnt.c[C_RNG];
}

// ------------------------------------------------------------------ light probes --
// Baked SH radiance (include/rtk.h "Light probes"): the rays of a probe are made where they are used and reduced where they land.

// Direction j of a probe with `rays` rays (a spherical Fibonacci set; the header has the formulas).  In double, not renormalised,
// and with contraction off whatever the flags of the kernel it is inlined into: 1 - z z is the two-rounding form, and the bits
// are the same in rtk_probe_rays_kernel and rtk_probe_bake_kernel.
RTK_DEV void probe_direction(uint32_t j, int rays, double d[3]) {
#pragma clang fp contract(off)
    const double z = 1.0 - double(2u * j + 1u) / double(rays);
    const uint32_t u = j * 2654435769u;                            // the golden ratio in 32-bit fixed point
    const double phi = double(u) * (6.283185307179586476925286766559 * 0x1p-32);
    const double r = rt_sqrt(1.0 - z * z);
    d[0] = r * cos(phi);
    d[1] = r * sin(phi);
    d[2] = z;
}

// The nine real spherical harmonics up to l = 2 of d, in the header's order.
RTK_DEV void probe_basis(const double d[3], double Y[9]) {
#pragma clang fp contract(off)
    const double x = d[0], y = d[1], z = d[2];
    Y[0] = 0.28209479177387814;
    Y[1] = 0.4886025119029199 * y;
    Y[2] = 0.4886025119029199 * z;
    Y[3] = 0.4886025119029199 * x;
    Y[4] = 1.0925484305920792 * (x * y);
    Y[5] = 1.0925484305920792 * (y * z);
    Y[6] = 0.31539156525252005 * (3.0 * (z * z) - 1.0);
    Y[7] = 1.0925484305920792 * (x * z);
    Y[8] = 0.5462742152960396 * (x * x - y * y);
}

// The ray records of n probes, probe-major: lane gid writes ray gid % rays of probe gid / rays as eleven 8-byte words.
__global__ __launch_bounds__(256) void rtk_probe_rays_kernel(long long n_rays, int rays, int spr, uint32_t first_key, double time,
                                                              const double* __restrict__ positions, double* __restrict__ out) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= n_rays) return;
    const long long k = gid / rays;
    const uint32_t j = uint32_t(gid - k * rays);
    double d[3];
    probe_direction(j, rays, d);
    const double* p = positions + k * 3;
    double* o = out + gid * 11;
    o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
    o[3] = d[0]; o[4] = d[1]; o[5] = d[2];
    o[6] = time;
    o[7] = 0.001;
    o[8] = __builtin_inf();
    uint2* keys = reinterpret_cast<uint2*>(o + 9);
    keys[0] = make_uint2(first_key + uint32_t(k), j * uint32_t(spr));
    keys[1] = make_uint2(0u, 0u);
}

// One workgroup of 256 per probe (blockIdx.x = k); lane t takes rays j = t, t + 256, ... (rays is a multiple of 256, so every
// lane makes the same number of passes and reaches the barrier).  Per ray: the direction, the lane's ray as load_query_ray sets
// it from the record rtk_probe_rays_kernel writes, rtk_query_radiance_kernel's sample loop, nine basis values and 27
// products in double.  No accumulator is live across the path loop, whose register count stays the radiance query's: each pass of
// 256 rays is reduced at once.  Reduction, in a fixed order: the 64 products of a wave by a butterfly (offsets 32, 16, .. 1),
// which leaves the sum in every lane; lane c of the wave (c = 0 .. 26) adds sum c to the wave's running sum part[wave][c] in LDS
// -- passes in increasing j; wave-private, so no barrier --; after one barrier lanes 0 .. 26 add the four waves' sums in wave
// order, scale once by 4 pi / rays and store as `real`.
template <typename real>
__global__ __launch_bounds__(256) void rtk_probe_bake_kernel(SceneView<real> sc, CameraRec<real> cam, uint32_t seed, uint32_t first_key, int rays, double time,
                                                              const double* __restrict__ positions, real* __restrict__ sh) {
    __shared__ double part[4][27];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const long long k = blockIdx.x;
    if (lane < 27) part[wave][lane] = 0.0;
    Counters<false> cnt;
    cnt.clear();
#ifdef RTK_PROFILE
    ShadeProf sprof;
#endif
    const uint32_t seed_hash = pcg_hash(seed), pixel = first_key + uint32_t(k);
    const double* p = positions + k * 3;
    const V3<real> origin = mk(real(p[0]), real(p[1]), real(p[2]));
    for (int j = t; j < rays; j += 256) {
        V3<real> rd;
        {
            double d[3];
            probe_direction(uint32_t(j), rays, d);
            rd = mk(real(d[0]), real(d[1]), real(d[2]));
        }
        V3<real> sum = mk(real(0), real(0), real(0));
        for (int s = 0; s < cam.spp; s++) {
            Lane<real> L;
            L.ro = origin;
            L.rd = rd;
            L.tm = real(time);
            L.rng = stream_key(seed_hash, pixel, uint32_t(j) * uint32_t(cam.spp) + uint32_t(s));   // (skip = 0)
            L.radiance = mk(real(0), real(0), real(0));
            L.throughput = mk(real(1), real(1), real(1));
            L.depth = cam.max_depth;
            trace_path(L, sc, cam, cnt RTK_SHADE_PROF_ARG);
            sum = sum + L.radiance;
        }
        const real ns = real(cam.spp);
        const double rgb[3] = {double(sum.x / ns), double(sum.y / ns), double(sum.z / ns)};
        double Y[9];
        {
            // The direction in double is computed again rather than kept in six registers across the path loop (the F32 kernel
            // would drop from three waves per SIMD to two); the empty asm keeps the compiler from merging the two evaluations.
            uint32_t j_again = uint32_t(j);
            asm volatile("" : "+v"(j_again));
            double d[3];
            probe_direction(j_again, rays, d);
            probe_basis(d, Y);
        }
        double mine = 0.0;
        for (int i = 0; i < 9; i++)
            for (int ch = 0; ch < 3; ch++) {
                double v = rgb[ch] * Y[i];
                for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
                if (lane == i * 3 + ch) mine = v;
            }
        if (lane < 27) part[wave][lane] += mine;
    }
    __syncthreads();
    if (t < 27) {
        const double total = ((part[0][t] + part[1][t]) + part[2][t]) + part[3][t];
        sh[k * 27 + t] = real(total * (12.566370614359172953850573533118 / double(rays)));
    }
}

// ------------------------------------------------------------------ surface gathers --
// Irradiance and occlusion at points with normals (include/rtk.h "Surface gathers"), stage 1 of two: one wave per unit
// w = (point k, pass q) = 64 rays j = 64 q .. 64 q + 63 of that point, four consecutive units per workgroup, so that a point's
// passes spread over the chip as the query's workgroups do and no launch is as long as its slowest point.  A wave whose unit
// is past the end leaves whole; no barrier, no LDS.  Each unit's sums go to the workspace as doubles, four words per unit;
// stage 2 (rtk_gather.hip) adds a point's passes in order.  first_key, points and normals are the batch's: k counts from its
// first point.

// Per lane: the direction (rtk_gather_rule.h) through the rounding load_ray applies to a record, the stream of the record
// rtk_gather_rays_kernel writes, rtk_query_radiance_kernel's sample loop restated, then three butterflies (offsets 32 .. 1), which
// leave each sum in every lane; lanes 0 .. 2 store.  Nothing but the unit's index is live across the path loop.
template <typename real>
__global__ __launch_bounds__(256) void rtk_gather_irradiance_kernel(SceneView<real> sc, CameraRec<real> cam, uint32_t seed, uint32_t first_key, int rays,
                                                                     uint32_t rotate, double time, long long units, const double* __restrict__ points,
                                                                     const double* __restrict__ normals, double* __restrict__ partial) {
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= units) return;
    const int passes = rays >> 6;
    const long long k = w / passes;
    const uint32_t j = uint32_t(w - k * passes) * 64u + uint32_t(lane);
    Counters<false> cnt;
    cnt.clear();
#ifdef RTK_PROFILE
    ShadeProf sprof;
#endif
    const uint32_t seed_hash = pcg_hash(seed), pixel = first_key + uint32_t(k);
    const double* p = points + k * 3;
    const V3<real> origin = mk(real(p[0]), real(p[1]), real(p[2]));
    V3<real> rd;
    {
        double d[3];
        gather_direction(j, rays, gather_rotation(rotate, pixel), normals + k * 3, d);
        rd = mk(real(d[0]), real(d[1]), real(d[2]));
    }
    V3<real> sum = mk(real(0), real(0), real(0));
    for (int s = 0; s < cam.spp; s++) {
        Lane<real> L;
        L.ro = origin;
        L.rd = rd;
        L.tm = real(time);
        L.rng = stream_key(seed_hash, pixel, j * uint32_t(cam.spp) + uint32_t(s));   // (skip = 0)
        L.radiance = mk(real(0), real(0), real(0));
        L.throughput = mk(real(1), real(1), real(1));
        L.depth = cam.max_depth;
        trace_path(L, sc, cam, cnt RTK_SHADE_PROF_ARG);
        sum = sum + L.radiance;
    }
    const real ns = real(cam.spp);
    const double rgb[3] = {double(sum.x / ns), double(sum.y / ns), double(sum.z / ns)};
    double mine = 0.0;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        double v = rgb[ch];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if (lane == ch) mine = v;
    }
    if (lane < 3) partial[w * 4 + lane] = mine;
}

// The same units for occlusion: rtk_query_occluded_kernel's walk of the record (tmin 0.001, tmax as given, the stream of sample
// j * spr), then four butterflies -- the open rays as a double and the sum of their directions, the doubles of the record --
// and lanes 0 .. 3 store.
template <typename real, bool ANY_HIT>
__global__ __launch_bounds__(256) void rtk_gather_occlusion_kernel(SceneView<real> sc, uint32_t seed, uint32_t first_key, int rays, int spr, uint32_t rotate,
                                                                    double time, double tmax, long long units, const double* __restrict__ points,
                                                                    const double* __restrict__ normals, double* __restrict__ partial) {
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= units) return;
    const int passes = rays >> 6;
    const long long k = w / passes;
    const uint32_t j = uint32_t(w - k * passes) * 64u + uint32_t(lane);
    const uint32_t pixel = first_key + uint32_t(k);
    const double* p = points + k * 3;
    double r[9] = {p[0], p[1], p[2], 0.0, 0.0, 0.0, time, 0.001, tmax};
    gather_direction(j, rays, gather_rotation(rotate, pixel), normals + k * 3, r + 3);
    Counters<true> cnt;
    Lane<real> L;
    load_ray(L, r);
    L.rng = stream_key(pcg_hash(seed), pixel, j * uint32_t(spr));   // (skip = 0)
    query_closest<ANY_HIT>(L, r, sc, cnt);
    const bool open = L.best_pc == kNoHit;
    double mine = 0.0;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        double v = open ? (c == 0 ? 1.0 : r[2 + c]) : 0.0;
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if (lane == c) mine = v;
    }
    if (lane < 4) partial[w * 4 + lane] = mine;
}

// ------------------------------------------------------------------ lens models --
// Whole frames through a lens (include/rtk.h "Lens models"): lens_begin above makes the sample; these kernels store it or trace it.

// The records of samples first_sample .. first_sample + n_samples - 1 of every pixel, pixel-major, samples inner: lane gid writes
// sample gid % n_samples of pixel gid / n_samples as eleven 8-byte words.
template <typename real>
__global__ __launch_bounds__(256) void rtk_lens_rays_kernel(long long n_rays, LensRec lens, CameraRec<real> cam, uint32_t seed, uint32_t first_sample, int n_samples,
                                                             double* __restrict__ out) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= n_rays) return;
    const uint32_t pixel = uint32_t(gid / n_samples), sample = first_sample + uint32_t(gid - (long long)pixel * n_samples);
    Lane<real> L;
    double r[7];
    const uint32_t skip = lens_begin(L, lens, cam, int(pixel % uint32_t(cam.width)), int(pixel / uint32_t(cam.width)), sample, pcg_hash(seed), r);
    double* o = out + gid * 11;
    for (int k = 0; k < 7; k++) o[k] = r[k];
    o[7] = 0.001;
    o[8] = __builtin_inf();
    uint2* keys = reinterpret_cast<uint2*>(o + 9);
    keys[0] = make_uint2(pixel, sample);
    keys[1] = make_uint2(skip, 0u);
}

// The standard error of a pixel's mean from the sums of y_s and y_s^2 over its n samples (the session estimate's form).
RTK_DEV float lens_se(double s1, double s2, int n) {
    if (n < 2) return 0.0f;
    const double m = s1 / double(n);
    double v = (s2 - double(n) * m * m) / double(n - 1);
    v = v > 0.0 ? v : 0.0;
    return float(__builtin_sqrt(v / double(n)));
}

// The lanes of a lens frame.  G = 1 << group_log2 consecutive lanes share a pixel (G = 1, 2, 4, 8, 16: the largest that does not exceed
// the samples per pixel) and a wave holds the 64 / G pixels of a small tile, 8x8, 8x4, 4x4, 4x2 or 2x2.  Lane `slot` of a pixel
// traces samples slot, slot + G, ...; after each round of G samples every lane of the pixel reads the round's radiance from its
// G lanes IN SAMPLE ORDER and adds it to its own copy of the sums, so the pixel's sums are ((0 + L_0) + L_1) + ... whatever G is:
// no atomics, nothing depends on the launch geometry.  Per sample: the record in registers (no record touches memory), then the
// radiance query's path; the record's doubles die before the path starts, and only the three colour sums and the two noise sums
// live across it.  Why not one lane per pixel with the whole sample loop inside, as the guide kernel has it: a wave then lasts
// the sum over the samples of its longest path, and a frame has G times fewer, G times longer waves -- where the cost sits in a
// few tiles (an equirect view of book1_final: 6.7 ms against 6.0 for rtk_lens_rays + rtk_query_radiance) the tail decides
// (DESIGN.md "lens models").
struct LensLanes {
    int width, height, tiles_x, n_tiles, group_log2;
};
static LensLanes lens_lanes(int width, int height, int spp) {
    int g = 0;
    while (g < 4 && (2 << g) <= spp) g++;
    const int tw = 8 >> (g / 2), th = 8 >> ((g + 1) / 2);
    const int tiles_x = (width + tw - 1) / tw;
    return LensLanes{width, height, tiles_x, tiles_x * ((height + th - 1) / th), g};
}

template <typename real>
__global__ __launch_bounds__(256) void rtk_lens_render_kernel(LensLanes lanes, SceneView<real> sc, CameraRec<real> cam, LensRec lens, uint32_t seed, uint32_t first_sample,
                                                               real* __restrict__ out, float* __restrict__ noise) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const int tile = int(gid >> 6), lane = int(gid & 63), g = lanes.group_log2, group = 1 << g;
    if (tile >= lanes.n_tiles) return;
    const int lw = 3 - g / 2, slot = lane & (group - 1), p = lane >> g;
    const int i = ((tile % lanes.tiles_x) << lw) + (p & ((1 << lw) - 1)), j = (tile / lanes.tiles_x) * (8 >> ((g + 1) / 2)) + (p >> lw);
    if (i >= lanes.width || j >= lanes.height) return;            // (the G lanes of a pixel leave together)
    Counters<false> cnt;
#ifdef RTK_PROFILE
    ShadeProf sprof;  // (the profile build's shade functions take their sub-phase accumulators)
#endif
    const uint32_t seed_hash = pcg_hash(seed);
    V3<real> sum = mk(real(0), real(0), real(0));
    double s1 = 0.0, s2 = 0.0;
    for (int base = 0; base < cam.spp; base += group) {
        V3<real> radiance = mk(real(0), real(0), real(0));
        if (base + slot < cam.spp) {
            Lane<real> L;
            {
                double r[7];
                (void)lens_begin(L, lens, cam, i, j, first_sample + uint32_t(base + slot), seed_hash, r);
            }
            trace_path(L, sc, cam, cnt RTK_SHADE_PROF_ARG);
            radiance = radiance + L.radiance;                     // (what the query returns for samples = 1: 0 + L, never -0)
        }
        const int n = cam.spp - base < group ? cam.spp - base : group;
        for (int k = 0; k < n; k++) {                             // the round's samples in sample order, from the pixel's own lanes
            const V3<real> r = mk(__shfl(radiance.x, k, group), __shfl(radiance.y, k, group), __shfl(radiance.z, k, group));
            sum = sum + r;
            const double y = ((double(r.x) + double(r.y)) + double(r.z)) / 3.0;
            s1 = s1 + y;
            s2 = s2 + y * y;
        }
    }
    if (slot != 0) return;
    const size_t px = size_t(j) * cam.width + i;
    real* o = out + px * 3;
    o[0] = sum.x * cam.samples_scale;
    o[1] = sum.y * cam.samples_scale;
    o[2] = sum.z * cam.samples_scale;
    if (noise) noise[px] = lens_se(s1, s2, cam.spp);
}

// ------------------------------------------------------------------ launchers --

// Geometry of a persistent launch: waves per workgroup and workgroups per CU so
// that (a) the register-limited wave count per CU is reached and (b) every
// resident workgroup's LDS copy of the program fits.  The arithmetic is rtk_grid_plan.h's;
// `cap` = variant bits 5..7 (tests and tools: at most 2^(cap - 1) waves, 0 = no cap).
template <typename Kernel>
static hipError_t plan_launch(Kernel kernel, int kMaxWavesPerBlock, size_t lds_bytes, int n_tiles, int cap, int& blocks, int& threads) {
    int device = 0, cus = 256, waves_per_cu = 0;
    hipError_t e = hipGetDevice(&device);
    if (e != hipSuccess) return e;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
    if (lds_plan::needs_opt_in(lds_bytes)) {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds_bytes));
        if (e != hipSuccess) return e;
    }
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&waves_per_cu, kernel, 64, 0);  // register-limited waves per CU
    if (e != hipSuccess) return e;
    int by_lds = 0;  // (no LDS staged: no limit)
    if (lds_bytes > 0) {
        by_lds = lds_plan::workgroups_per_cu(lds_bytes);
        if (by_lds < 1) return hipErrorInvalidValue;
    }
    const grid_plan::Grid g = grid_plan::plan(cus, waves_per_cu, kMaxWavesPerBlock, by_lds, n_tiles, cap);
    blocks = g.blocks;
    threads = g.threads;
    if (getenv("RTK_DEBUG"))
        fprintf(stderr, "[rtk] launch plan: occupancy API %d waves/CU, %d workgroup(s)/CU x %d waves, grid %d x %d threads, LDS %zu B/workgroup\n",
                g.waves_per_cu, g.blocks_per_cu, g.waves_per_block, blocks, threads, lds_bytes);
    return hipSuccess;
}

// What a workgroup stages in LDS and where: rtk_lds_plan.h decides, from the scene's record counts and the kernel's FEAT word
// (F_F32_BOX selects the MIXED program in the lean family and the COMPACT one in the others).
static_assert(lds_plan::kCapacity == size_t(kLdsBytesPerCU) && lds_plan::kXform == F_XFORM && lds_plan::kTexture == F_TEXTURE && lds_plan::kF32Box == F_F32_BOX &&
              lds_plan::kMatte == F_MATTE && lds_plan::kLdsBoxes == F_LDS_BOXES && lds_plan::kLeanFamily == kFeatLean, "rtk_lds_plan.h restates rtk_device_layout.h");
static_assert(lds_plan::kMixedUnitBytes == sizeof(MixedHead) && lds_plan::kUnit16Bytes == sizeof(Unit16), "rtk_lds_plan.h restates rtk_device_layout.h");
static_assert(kernel_choice::kFmaBox == F_FMA_BOX && kernel_choice::kSphereMediaOnly == F_SPHERE_MEDIA_ONLY && kernel_choice::kMeshFamily == kFeatMesh &&
              kernel_choice::kQuadBoxFamily == kFeatQuadBox && kernel_choice::kFullFamily == kFeatAll, "rtk_kernel_choice.h restates rtk_device_layout.h");
template <typename real>
static constexpr lds_plan::RecordSizes lds_record_sizes() {
    constexpr lds_plan::RecordSizes s = sizeof(real) == 8 ? lds_plan::kSizesF64 : lds_plan::kSizesF32;
    static_assert(s.slot == sizeof(Slot<real>) && s.box == sizeof(BoxRec<real>) && s.material == sizeof(MaterialRec<real>) && s.perlin == sizeof(PerlinRec<real>) &&
                  s.chain == sizeof(ChainRec<real>), "rtk_lds_plan.h restates rtk_device_layout.h");
    return s;
}
template <typename real>
static lds_plan::Counts lds_counts(const SceneView<real>& sc) {
    lds_plan::Counts n;
    n.slots = size_t(sc.n_slots);
    n.units = size_t(sc.n_units);
    n.units16 = size_t(sc.n_units16);
    n.hot_units = size_t(sc.n_hot_units);
    n.cached_boxes = size_t(sc.n_cached_boxes);
    n.kind_words = size_t(sc.n_kind_words);
    n.rank_words = size_t(sc.n_rank_words);
    n.materials = size_t(sc.n_materials);
    n.perlins = size_t(sc.n_perlins);
    n.chains = size_t(sc.n_chains);
    return n;
}
template <typename real, uint32_t FEAT, bool COUNT, bool IN_LDS>
static hipError_t launch_one(const SceneView<real>& sc, const CameraRec<real>* cam, const TileMap& tmap, uint32_t seed, void* partial,
                             unsigned long long* counters, unsigned int* tile_counter, const int32_t* tile_order, unsigned int* tile_cost, uint32_t diag,
                             hipStream_t stream, const ViewRec<real>* views = nullptr) {
    const int n_items = tmap.n_tiles_local * tmap.n_chunks;
    if (n_items <= 0) return hipSuccess;
    if (views != nullptr && !kernel_choice::has_view_kernel(FEAT, COUNT, IN_LDS)) return hipErrorInvalidValue;  // (the caller asks view_kernel_name first)
    auto kernel = rtk_render_kernel<real, FEAT, COUNT, IN_LDS>;
    const lds_plan::Plan plan = lds_plan::plan(lds_counts(sc), lds_record_sizes<real>(), FEAT, IN_LDS, size_t(tmap.n_tiles_local), tile_order != nullptr);
    const size_t lds = plan.total;
    TileMap tm = tmap;
    tm.mats_lds_offset = plan.mats_lds_offset;
    tm.perlin_lds_offset = plan.perlin_lds_offset;
    tm.chains_lds_offset = plan.chains_lds_offset;
    tm.order_in_lds = plan.order_in_lds;
    tm.order_lds_offset = plan.order_lds_offset;
    if (getenv("RTK_DEBUG"))
        fprintf(stderr, "[rtk] lds plan: real %zu FEAT %u IN_LDS %d views %d: total %zu B, mats_lds_offset %d, perlin_lds_offset %d, chains_lds_offset %d, order_in_lds %d, order_lds_offset %d\n",
                sizeof(real), unsigned(FEAT), int(IN_LDS), int(views != nullptr), lds, int(tm.mats_lds_offset), int(tm.perlin_lds_offset), int(tm.chains_lds_offset),
                int(tm.order_in_lds), int(tm.order_lds_offset));
    int blocks = 0, threads = 0;
    if constexpr (kernel_choice::has_view_kernel(FEAT, COUNT, IN_LDS)) {
        if (views != nullptr) {  // the view kernel: the same staging plan, its own occupancy
            auto view_kernel = rtk_view_batch_kernel<real, FEAT, IN_LDS>;
            hipError_t ev = plan_launch(view_kernel, kernel_choice::max_threads(sizeof(real), FEAT, IN_LDS) / 64, lds, n_items, int(diag >> 5) & 7, blocks, threads);
            if (ev != hipSuccess) return ev;
            ev = hipMemsetAsync(tile_counter, 0, sizeof(unsigned int), stream);
            if (ev != hipSuccess) return ev;
            view_kernel<<<dim3(blocks), dim3(threads), lds, stream>>>(sc, views, tm, static_cast<real*>(partial), tile_counter, diag);
            return hipGetLastError();
        }
    }
    hipError_t e = plan_launch(kernel, kernel_choice::max_threads(sizeof(real), FEAT, IN_LDS) / 64, lds, n_items, int(diag >> 5) & 7, blocks, threads);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(tile_counter, 0, sizeof(unsigned int), stream);
    if (e != hipSuccess) return e;
    kernel<<<dim3(blocks), dim3(threads), lds, stream>>>(sc, cam, tm, seed, static_cast<real*>(partial), counters, tile_counter, tile_order, tile_cost, diag);
    return hipGetLastError();
}

// Which kernel a launch runs is rtk_kernel_choice.h's decision: this is the one place that tells it what the upload built.
template <typename real>
static kernel_choice::Choice choose_for_scene(const SceneView<real>& sc, uint32_t features, bool count, bool allow_lds, uint32_t diag) {
    const kernel_choice::Inputs in{sizeof(real), features, count, allow_lds, diag, sc.program_mixed != nullptr, sc.program_compact != nullptr,
                                   sc.program_hot != nullptr, sc.box_cache != nullptr, lds_counts(sc)};
    return kernel_choice::choose(in);
}

#ifndef RTK_DEV_ONLY_ALL
#define RTK_DEV_ONLY_ALL 0   // tools/kernel_resources.py -DRTK_DEV_ONLY_ALL: only the full-feature family (quick register experiments)
#endif

// launch_render (views = null) and launch_view_batch: one decision, then the row of the table that it names -- exactly that
// row, or an error: a choice that is not compiled never runs a neighbouring kernel.
template <typename real>
static hipError_t launch_chosen(const SceneView<real>& sc, const CameraRec<real>* cam, const TileMap& tmap, uint32_t seed, uint32_t features, bool count,
                                bool allow_lds, uint32_t diag, void* partial, unsigned long long* counters, unsigned int* tile_counter,
                                const int32_t* tile_order, unsigned int* tile_cost, hipStream_t stream, const ViewRec<real>* views) {
    const kernel_choice::Choice k = choose_for_scene(sc, features, count, allow_lds, diag);
#define RTK_LAUNCH_ROW(F, C, L)                                                                                        \
    if constexpr (sizeof(real) != 0 && (!RTK_DEV_ONLY_ALL || kernel_choice::family(F) == kernel_choice::kFullFamily)) \
        if (k.feat == F && k.count == C && k.in_lds == L)                                                              \
            return launch_one<real, F, C, L>(sc, cam, tmap, seed, partial, counters, tile_counter, tile_order, tile_cost, diag, stream, views);
    RTK_RENDER_KERNELS_BOTH(RTK_LAUNCH_ROW)
    if constexpr (sizeof(real) == 8) {
        RTK_RENDER_KERNELS_F64(RTK_LAUNCH_ROW)
    }
#undef RTK_LAUNCH_ROW
    return hipErrorInvalidValue;
}
template <typename real>
hipError_t launch_render(const SceneView<real>& sc, const CameraRec<real>* cam, const TileMap& tmap, uint32_t seed, uint32_t features, bool count,
                         bool allow_lds, uint32_t diag, void* partial, unsigned long long* counters, unsigned int* tile_counter,
                         const int32_t* tile_order, unsigned int* tile_cost, hipStream_t stream) {
    return launch_chosen<real>(sc, cam, tmap, seed, features, count, allow_lds, diag, partial, counters, tile_counter, tile_order, tile_cost, stream, nullptr);
}
template hipError_t launch_render<double>(const SceneView<double>&, const CameraRec<double>*, const TileMap&, uint32_t, uint32_t, bool, bool, uint32_t, void*,
                                          unsigned long long*, unsigned int*, const int32_t*, unsigned int*, hipStream_t);
template hipError_t launch_render<float>(const SceneView<float>&, const CameraRec<float>*, const TileMap&, uint32_t, uint32_t, bool, bool, uint32_t, void*,
                                         unsigned long long*, unsigned int*, const int32_t*, unsigned int*, hipStream_t);

template <typename real>
hipError_t launch_view_batch(const SceneView<real>& sc, const ViewRec<real>* d_views, const TileMap& tmap, uint32_t features, bool allow_lds, uint32_t diag,
                             void* partial, unsigned int* tile_counter, hipStream_t stream) {
    if (!d_views) return hipErrorInvalidValue;
    return launch_chosen<real>(sc, nullptr, tmap, 0u, features, false, allow_lds, diag, partial, nullptr, tile_counter, nullptr, nullptr, stream, d_views);
}
template hipError_t launch_view_batch<double>(const SceneView<double>&, const ViewRec<double>*, const TileMap&, uint32_t, bool, uint32_t, void*, unsigned int*, hipStream_t);
template hipError_t launch_view_batch<float>(const SceneView<float>&, const ViewRec<float>*, const TileMap&, uint32_t, bool, uint32_t, void*, unsigned int*, hipStream_t);

template <typename real>
const char* render_kernel_name(const SceneView<real>& sc, uint32_t features, bool count, bool allow_lds, uint32_t diag) {
    static thread_local char name[96];
    kernel_choice::format_name(name, sizeof name, sizeof(real), choose_for_scene(sc, features, count, allow_lds, diag), false);
    return name;
}
template const char* render_kernel_name<double>(const SceneView<double>&, uint32_t, bool, bool, uint32_t);
template const char* render_kernel_name<float>(const SceneView<float>&, uint32_t, bool, bool, uint32_t);

// What a view batch dispatches: the view kernel of the instantiation the choice names, or -- where that one has none (the
// program in global memory) -- the plain kernel, launched once per view.
template <typename real>
const char* view_kernel_name(const SceneView<real>& sc, uint32_t features, bool allow_lds, uint32_t diag, bool* is_view_kernel) {
    static thread_local char name[96];
    const kernel_choice::Choice k = choose_for_scene(sc, features, false, allow_lds, diag);
    const bool view = kernel_choice::has_view_kernel(k.feat, k.count, k.in_lds);
    if (is_view_kernel) *is_view_kernel = view;
    kernel_choice::format_name(name, sizeof name, sizeof(real), k, view);
    return name;
}
template const char* view_kernel_name<double>(const SceneView<double>&, uint32_t, bool, uint32_t, bool*);
template const char* view_kernel_name<float>(const SceneView<float>&, uint32_t, bool, uint32_t, bool*);

// The grid of a lane-per-ray launch: 256-thread blocks over n lanes.
static dim3 lane_grid(long long n) { return dim3((unsigned int)((n + 255) / 256)); }

template <typename real>
hipError_t launch_debug_hit(const SceneView<real>& sc, int n, const double* d_rays, const uint32_t* d_keys, double* d_out, unsigned long long* d_draws,
                            hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    rtk_debug_hit_kernel<real><<<lane_grid(n), dim3(256), 0, stream>>>(sc, n, d_rays, d_keys, d_out, d_draws);
    return hipGetLastError();
}
template hipError_t launch_debug_hit<double>(const SceneView<double>&, int, const double*, const uint32_t*, double*, unsigned long long*, hipStream_t);
template hipError_t launch_debug_hit<float>(const SceneView<float>&, int, const double*, const uint32_t*, double*, unsigned long long*, hipStream_t);

template <typename real>
hipError_t launch_debug_scatter(const SceneView<real>& sc, int n, const int32_t* d_mat, const double* d_ray, const double* d_rec, const uint32_t* d_keys, double* d_out,
                                unsigned long long* d_draws, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    rtk_debug_scatter_kernel<real><<<lane_grid(n), dim3(256), 0, stream>>>(sc, n, d_mat, d_ray, d_rec, d_keys, d_out, d_draws);
    return hipGetLastError();
}
template hipError_t launch_debug_scatter<double>(const SceneView<double>&, int, const int32_t*, const double*, const double*, const uint32_t*, double*, unsigned long long*, hipStream_t);
template hipError_t launch_debug_scatter<float>(const SceneView<float>&, int, const int32_t*, const double*, const double*, const uint32_t*, double*, unsigned long long*, hipStream_t);

template <typename real>
hipError_t launch_debug_texture(const SceneView<real>& sc, int n, const int32_t* d_tex, const double* d_uvp, double* d_out, unsigned long long* d_work, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    rtk_debug_texture_kernel<real><<<lane_grid(n), dim3(256), 0, stream>>>(sc, n, d_tex, d_uvp, d_out, d_work);
    return hipGetLastError();
}
template hipError_t launch_debug_texture<double>(const SceneView<double>&, int, const int32_t*, const double*, double*, unsigned long long*, hipStream_t);
template hipError_t launch_debug_texture<float>(const SceneView<float>&, int, const int32_t*, const double*, double*, unsigned long long*, hipStream_t);

template <typename real>
hipError_t launch_debug_get_ray(const CameraRec<real>& cam, uint32_t seed, int n, const int32_t* d_ijs, double* d_out, unsigned long long* d_draws, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    rtk_debug_get_ray_kernel<real><<<lane_grid(n), dim3(256), 0, stream>>>(cam, seed, n, d_ijs, d_out, d_draws);
    return hipGetLastError();
}
template hipError_t launch_debug_get_ray<double>(const CameraRec<double>&, uint32_t, int, const int32_t*, double*, unsigned long long*, hipStream_t);
template hipError_t launch_debug_get_ray<float>(const CameraRec<float>&, uint32_t, int, const int32_t*, double*, unsigned long long*, hipStream_t);

template <typename real>
hipError_t launch_aov(const SceneView<real>& sc, const CameraRec<real>& cam, uint32_t seed, int n_samples, float* d_aov, hipStream_t stream) {
    const TileGrid grid = tile_grid(cam.width, cam.height);
    rtk_guide_kernel<real, false><<<lane_grid(64ll * grid.n_tiles), dim3(256), 0, stream>>>(grid, sc, cam, seed, n_samples, 0, 0, reinterpret_cast<float4*>(d_aov), CameraSamples{});
    return hipGetLastError();
}
template hipError_t launch_aov<double>(const SceneView<double>&, const CameraRec<double>&, uint32_t, int, float*, hipStream_t);
template hipError_t launch_aov<float>(const SceneView<float>&, const CameraRec<float>&, uint32_t, int, float*, hipStream_t);

template <typename real>
hipError_t launch_guides(const SceneView<real>& sc, const CameraRec<real>& cam, uint32_t seed, int n_samples, int follow, int max_bounces, float* d_guides,
                         hipStream_t stream) {
    const TileGrid grid = tile_grid(cam.width, cam.height);
    rtk_guide_kernel<real, true><<<lane_grid(64ll * grid.n_tiles), dim3(256), 0, stream>>>(grid, sc, cam, seed, n_samples, follow, max_bounces,
                                                                                         reinterpret_cast<float4*>(d_guides), CameraSamples{});
    return hipGetLastError();
}
template hipError_t launch_guides<double>(const SceneView<double>&, const CameraRec<double>&, uint32_t, int, int, int, float*, hipStream_t);
template hipError_t launch_guides<float>(const SceneView<float>&, const CameraRec<float>&, uint32_t, int, int, int, float*, hipStream_t);

template <typename real>
hipError_t launch_query_hits(const SceneView<real>& sc, uint32_t seed, long long n, const void* d_rays, void* d_hits, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    rtk_query_hits_kernel<real><<<lane_grid(n), dim3(256), 0, stream>>>(sc, seed, n, static_cast<const double*>(d_rays), static_cast<double*>(d_hits));
    return hipGetLastError();
}
template hipError_t launch_query_hits<double>(const SceneView<double>&, uint32_t, long long, const void*, void*, hipStream_t);
template hipError_t launch_query_hits<float>(const SceneView<float>&, uint32_t, long long, const void*, void*, hipStream_t);

template <typename real>
hipError_t launch_query_occluded(const SceneView<real>& sc, uint32_t seed, bool any_hit, long long n, const void* d_rays, int32_t* d_occluded, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    const double* rays = static_cast<const double*>(d_rays);
    if (any_hit) rtk_query_occluded_kernel<real, true><<<lane_grid(n), dim3(256), 0, stream>>>(sc, seed, n, rays, d_occluded);
    else rtk_query_occluded_kernel<real, false><<<lane_grid(n), dim3(256), 0, stream>>>(sc, seed, n, rays, d_occluded);
    return hipGetLastError();
}
template hipError_t launch_query_occluded<double>(const SceneView<double>&, uint32_t, bool, long long, const void*, int32_t*, hipStream_t);
template hipError_t launch_query_occluded<float>(const SceneView<float>&, uint32_t, bool, long long, const void*, int32_t*, hipStream_t);

template <typename real>
hipError_t launch_query_radiance(const SceneView<real>& sc, const CameraRec<real>& cam, uint32_t seed, long long n, const void* d_rays, void* d_radiance,
                                 uint32_t* d_draws, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    const double* rays = static_cast<const double*>(d_rays);
    real* out = static_cast<real*>(d_radiance);
    if (d_draws) rtk_query_radiance_kernel<real, true><<<lane_grid(n), dim3(256), 0, stream>>>(sc, cam, seed, n, rays, out, d_draws);
    else rtk_query_radiance_kernel<real, false><<<lane_grid(n), dim3(256), 0, stream>>>(sc, cam, seed, n, rays, out, nullptr);
    return hipGetLastError();
}
template hipError_t launch_query_radiance<double>(const SceneView<double>&, const CameraRec<double>&, uint32_t, long long, const void*, void*, uint32_t*, hipStream_t);
template hipError_t launch_query_radiance<float>(const SceneView<float>&, const CameraRec<float>&, uint32_t, long long, const void*, void*, uint32_t*, hipStream_t);

hipError_t launch_probe_rays(long long n, int rays, int samples, uint32_t first_key, double time, const double* d_positions, void* d_rays, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    rtk_probe_rays_kernel<<<lane_grid(n * rays), dim3(256), 0, stream>>>(n * rays, rays, samples, first_key, time, d_positions, static_cast<double*>(d_rays));
    return hipGetLastError();
}

template <typename real>
hipError_t launch_probe_bake(const SceneView<real>& sc, const CameraRec<real>& cam, uint32_t seed, uint32_t first_key, int rays, double time, long long n,
                             const double* d_positions, void* d_sh, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    rtk_probe_bake_kernel<real><<<dim3((unsigned int)n), dim3(256), 0, stream>>>(sc, cam, seed, first_key, rays, time, d_positions, static_cast<real*>(d_sh));
    return hipGetLastError();
}
template hipError_t launch_probe_bake<double>(const SceneView<double>&, const CameraRec<double>&, uint32_t, uint32_t, int, double, long long, const double*, void*, hipStream_t);
template hipError_t launch_probe_bake<float>(const SceneView<float>&, const CameraRec<float>&, uint32_t, uint32_t, int, double, long long, const double*, void*, hipStream_t);

template <typename real>
hipError_t launch_gather_irradiance(const SceneView<real>& sc, const CameraRec<real>& cam, uint32_t seed, uint32_t first_key, int rays, uint32_t rotate, double time,
                                    long long n, const double* d_points, const double* d_normals, double* d_partial, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    const long long units = n * (rays / 64);
    rtk_gather_irradiance_kernel<real><<<dim3((unsigned int)((units + 3) / 4)), dim3(256), 0, stream>>>(sc, cam, seed, first_key, rays, rotate, time, units, d_points,
                                                                                                         d_normals, d_partial);
    return hipGetLastError();
}
template hipError_t launch_gather_irradiance<double>(const SceneView<double>&, const CameraRec<double>&, uint32_t, uint32_t, int, uint32_t, double, long long, const double*,
                                                     const double*, double*, hipStream_t);
template hipError_t launch_gather_irradiance<float>(const SceneView<float>&, const CameraRec<float>&, uint32_t, uint32_t, int, uint32_t, double, long long, const double*,
                                                    const double*, double*, hipStream_t);

template <typename real>
hipError_t launch_gather_occlusion(const SceneView<real>& sc, uint32_t seed, bool any_hit, uint32_t first_key, int rays, int samples, uint32_t rotate, double time,
                                   double tmax, long long n, const double* d_points, const double* d_normals, double* d_partial, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    const long long units = n * (rays / 64);
    const dim3 grid((unsigned int)((units + 3) / 4));
    if (any_hit) rtk_gather_occlusion_kernel<real, true><<<grid, dim3(256), 0, stream>>>(sc, seed, first_key, rays, samples, rotate, time, tmax, units, d_points, d_normals, d_partial);
    else rtk_gather_occlusion_kernel<real, false><<<grid, dim3(256), 0, stream>>>(sc, seed, first_key, rays, samples, rotate, time, tmax, units, d_points, d_normals, d_partial);
    return hipGetLastError();
}
template hipError_t launch_gather_occlusion<double>(const SceneView<double>&, uint32_t, bool, uint32_t, int, int, uint32_t, double, double, long long, const double*,
                                                    const double*, double*, hipStream_t);
template hipError_t launch_gather_occlusion<float>(const SceneView<float>&, uint32_t, bool, uint32_t, int, int, uint32_t, double, double, long long, const double*,
                                                   const double*, double*, hipStream_t);

template <typename real>
hipError_t launch_lens_rays(const LensRec& lens, const CameraRec<real>& cam, uint32_t seed, uint32_t first_sample, int n_samples, void* d_rays, hipStream_t stream) {
    const long long n = (long long)cam.width * cam.height * n_samples;
    if (n <= 0) return hipSuccess;
    rtk_lens_rays_kernel<real><<<lane_grid(n), dim3(256), 0, stream>>>(n, lens, cam, seed, first_sample, n_samples, static_cast<double*>(d_rays));
    return hipGetLastError();
}
template hipError_t launch_lens_rays<double>(const LensRec&, const CameraRec<double>&, uint32_t, uint32_t, int, void*, hipStream_t);
template hipError_t launch_lens_rays<float>(const LensRec&, const CameraRec<float>&, uint32_t, uint32_t, int, void*, hipStream_t);

template <typename real>
hipError_t launch_lens_render(const SceneView<real>& sc, const LensRec& lens, const CameraRec<real>& cam, uint32_t seed, uint32_t first_sample, void* d_linear,
                              float* d_noise, hipStream_t stream) {
    const LensLanes lanes = lens_lanes(cam.width, cam.height, cam.spp);
    rtk_lens_render_kernel<real><<<lane_grid(64ll * lanes.n_tiles), dim3(256), 0, stream>>>(lanes, sc, cam, lens, seed, first_sample, static_cast<real*>(d_linear), d_noise);
    return hipGetLastError();
}
template hipError_t launch_lens_render<double>(const SceneView<double>&, const LensRec&, const CameraRec<double>&, uint32_t, uint32_t, void*, float*, hipStream_t);
template hipError_t launch_lens_render<float>(const SceneView<float>&, const LensRec&, const CameraRec<float>&, uint32_t, uint32_t, void*, float*, hipStream_t);

template <typename real>
hipError_t launch_lens_aov(const SceneView<real>& sc, const LensRec& lens, const CameraRec<real>& cam, uint32_t seed, int n_samples, float* d_aov, hipStream_t stream) {
    const TileGrid grid = tile_grid(cam.width, cam.height);
    rtk_guide_kernel<real, false><<<lane_grid(64ll * grid.n_tiles), dim3(256), 0, stream>>>(grid, sc, cam, seed, n_samples, 0, 0, reinterpret_cast<float4*>(d_aov),
                                                                                          LensSamples{lens});
    return hipGetLastError();
}
template hipError_t launch_lens_aov<double>(const SceneView<double>&, const LensRec&, const CameraRec<double>&, uint32_t, int, float*, hipStream_t);
template hipError_t launch_lens_aov<float>(const SceneView<float>&, const LensRec&, const CameraRec<float>&, uint32_t, int, float*, hipStream_t);

template <typename real>
hipError_t launch_lens_guides(const SceneView<real>& sc, const LensRec& lens, const CameraRec<real>& cam, uint32_t seed, int n_samples, int follow, int max_bounces,
                              float* d_guides, hipStream_t stream) {
    const TileGrid grid = tile_grid(cam.width, cam.height);
    rtk_guide_kernel<real, true><<<lane_grid(64ll * grid.n_tiles), dim3(256), 0, stream>>>(grid, sc, cam, seed, n_samples, follow, max_bounces,
                                                                                         reinterpret_cast<float4*>(d_guides), LensSamples{lens});
    return hipGetLastError();
}
template hipError_t launch_lens_guides<double>(const SceneView<double>&, const LensRec&, const CameraRec<double>&, uint32_t, int, int, int, float*, hipStream_t);
template hipError_t launch_lens_guides<float>(const SceneView<float>&, const LensRec&, const CameraRec<float>&, uint32_t, int, int, int, float*, hipStream_t);

#ifdef RTK_ISA_PROBES
// Instruction-cost probes (tools/isa_costs.py; never part of the product build): one kernel per unit of work of the lean
// MIXED kernel family (what bench.py times on C2), each loading a lane's state from memory, running ONE step through the
// product's own step function and storing the state back.  The tool counts the VALU instructions of each probe by class in the
// ISA and subtracts the empty probe: what is left is the instruction cost of that unit of work when a whole wave executes it
// once -- the per-unit figures behind bench.py's roofline.work_frac (work counters x these costs / 64 lanes / SIMD-cycles
// available: a fraction that executing MORE instructions cannot raise).
constexpr uint32_t kProbeFeat = kFeatLean | uint32_t(F_F32_BOX);
enum ProbeKind : int { PROBE_EMPTY, PROBE_BOX, PROBE_SPHERE, PROBE_SEGMENT, PROBE_SAMPLE, PROBE_MISS, PROBE_LAMBERTIAN, PROBE_METAL, PROBE_DIELECTRIC, PROBE_PARTIAL };
template <int KIND>
__global__ __launch_bounds__(1024) void rtk_isa_probe(Lane<double>* __restrict__ lanes, const MixedHead* __restrict__ prog, SceneView<double> sc,
                                                       const CameraRec<double>* __restrict__ cam_ptr, double* __restrict__ partial, float extent) {
    const int gid = blockIdx.x * 1024 + threadIdx.x;
    Lane<double> L = lanes[gid];
    Counters<false> cnt;
    const NoTie tie{};
    const MixedHead* rec = reinterpret_cast<const MixedHead*>(reinterpret_cast<const unsigned char*>(prog) + L.pc);
    if constexpr (KIND == PROBE_BOX) {  // one box step: the slab test on the record in registers, then the next record and its kind
        // (on the LDS image's record form, as the timed kernel <double, 256u, false, true> steps it: two 16-byte reads, kind and link in the first)
        const rtk_u32x4* at = reinterpret_cast<const rtk_u32x4*>(rec);
        rtk_u32x4 a = at[0], b = at[1];
        step_box_img(L, a, b, cnt);
        at = reinterpret_cast<const rtk_u32x4*>(reinterpret_cast<const unsigned char*>(prog) + L.pc);
        a = at[0], b = at[1];
        L.kind = a.w & 15u;
        L.oi32_lo.x = __builtin_bit_cast(float, uint32_t(a.x)) + __builtin_bit_cast(float, uint32_t(b.x));  // (keeps the fetched record alive, as the next step's slab test does)
    } else if constexpr (KIND == PROBE_SPHERE) {
        MixedHead cur = *rec;
        step_sphere_mixed<kChPcUnit>(L, cur, rec, cnt, tie, extent);
        cur = *reinterpret_cast<const MixedHead*>(reinterpret_cast<const unsigned char*>(prog) + L.pc);
        L.kind = cur.kind_payload & 15u;
        L.oi32_lo.x = cur.f(0);
    } else if constexpr (KIND == PROBE_SEGMENT) {
        begin_segment<false, true, 1>(L, cnt, extent);
        L.kind = rec->kind_payload & 15u;
    } else if constexpr (KIND == PROBE_SAMPLE) {
        begin_sample(L, *cam_ptr, int(L.segs), L.depth, pcg_hash(L.best_pc), cnt);
    } else if constexpr (KIND == PROBE_MISS) {
        L.sum = L.sum + L.throughput * ld3(cam_ptr->background);
    } else if constexpr (KIND == PROBE_LAMBERTIAN || KIND == PROBE_METAL || KIND == PROBE_DIELECTRIC) {
        Surface<double> sf;
        make_surface_mixed(rec, 0u, L.best_t, L.ro, L.rd, L.tm, sf);
        constexpr int kMat = KIND == PROBE_LAMBERTIAN ? int(RTK_MAT_LAMBERTIAN) : (KIND == PROBE_METAL ? int(RTK_MAT_METAL) : int(RTK_MAT_DIELECTRIC));
#ifdef RTK_PROFILE
        ShadeProf sprof;
#endif
        const bool ended = shade_surface<double, kProbeFeat, kMat>(L, sf, sc, sc.materials, cnt RTK_SHADE_PROF_ARG);
        L.kind = ended ? 1u : 0u;
    } else if constexpr (KIND == PROBE_PARTIAL) {
        store_partial(partial, int(L.segs), L.depth, L.sum);
    }
    lanes[gid] = L;
}
template __global__ void rtk_isa_probe<PROBE_EMPTY>(Lane<double>*, const MixedHead*, SceneView<double>, const CameraRec<double>*, double*, float);
template __global__ void rtk_isa_probe<PROBE_BOX>(Lane<double>*, const MixedHead*, SceneView<double>, const CameraRec<double>*, double*, float);
template __global__ void rtk_isa_probe<PROBE_SPHERE>(Lane<double>*, const MixedHead*, SceneView<double>, const CameraRec<double>*, double*, float);
template __global__ void rtk_isa_probe<PROBE_SEGMENT>(Lane<double>*, const MixedHead*, SceneView<double>, const CameraRec<double>*, double*, float);
template __global__ void rtk_isa_probe<PROBE_SAMPLE>(Lane<double>*, const MixedHead*, SceneView<double>, const CameraRec<double>*, double*, float);
template __global__ void rtk_isa_probe<PROBE_MISS>(Lane<double>*, const MixedHead*, SceneView<double>, const CameraRec<double>*, double*, float);
template __global__ void rtk_isa_probe<PROBE_LAMBERTIAN>(Lane<double>*, const MixedHead*, SceneView<double>, const CameraRec<double>*, double*, float);
template __global__ void rtk_isa_probe<PROBE_METAL>(Lane<double>*, const MixedHead*, SceneView<double>, const CameraRec<double>*, double*, float);
template __global__ void rtk_isa_probe<PROBE_DIELECTRIC>(Lane<double>*, const MixedHead*, SceneView<double>, const CameraRec<double>*, double*, float);
template __global__ void rtk_isa_probe<PROBE_PARTIAL>(Lane<double>*, const MixedHead*, SceneView<double>, const CameraRec<double>*, double*, float);
#endif  // RTK_ISA_PROBES

}  // namespace rtk
