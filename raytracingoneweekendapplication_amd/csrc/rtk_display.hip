// rtk_display.hip -- the display transform (include/rtk.h, "Display transform"): metered exposure, bloom, a tone curve and an
// encoding between a linear frame and its 8-bit pixels.  Hand-written HIP for gfx950, wave64.
//
// Passes per frame, all on the object's stream; the exposure goes from the metering kernel to the kernels that use it
// through device memory, the host never reads it unless asked (rtk_display_exposure):
//   rtk_display_histogram_kernel   luminance histogram, 320 integer bins.  A thread takes four consecutive pixels (three 16-byte
//                                  loads in F32 mode, six in F64 mode).  Each wave of a block keeps its own LDS copy of the bins; a
//                                  pixel is counted with a returnless LDS add, after a ballot pre-count: the lanes whose bin is the
//                                  first lane's are counted by one add of their number (rendered frames put most of a wave into
//                                  one bin, and same-address LDS adds serialise).  One flush per block: integer global adds of the
//                                  non-zero bins.  Integers only: the counts are the same bits in any order of arrival.
//   rtk_display_meter_kernel       one wave: trimmed log-average of the histogram in double (fixed order), target exposure,
//                                  adaptation; copies the histogram out for rtk_display_histogram and clears it for the next frame.
//   rtk_display_set_exposure_kernel  a manual exposure instead of the two above.
//   rtk_display_bloom_down_kernel  bright pass + 2x2 mean (level 1, reading the frame); rtk_display_bloom_halve_kernel: 2x2 mean (levels 2..n);
//   rtk_display_bloom_tent_kernel  (1 2 1)/4 along one axis, launched twice per level;
//   rtk_display_bloom_up_kernel    U_k = T_k + bilinear(U_{k+1}), in place.  The pyramid is float4 texels, allocated on first use.
//   rtk_display_apply_kernel       sanitise, scale, add the bloom, curve, encode; four pixels per thread, 16-byte accesses.
// Without bloom: 3 launches per frame (2 with a manual exposure); with n levels 3 + 3n + (n - 1).
//
// No float atomics, no order-dependent sum: the same inputs give the same bits.
#include <hip/hip_runtime.h>

#include <cmath>

#include "rtk.h"
#include "rtk_image_pass.h"
#include "rtk_internal.h"

namespace rtk {
namespace {

// 1: the histogram pass counts the lanes that share the first lane's bin with one LDS add (the kept form); 0, for tools/display_probe.py
// on a diagnostic build: one add per lane into the wave's own copy ("Display transform", has the measurement).
#ifndef RTK_DISPLAY_PRECOUNT
#define RTK_DISPLAY_PRECOUNT 1
#endif

// The most blocks the histogram pass launches (each then strides over the frame): every block ends with one global add per
// non-zero bin, and adds to one address serialise in L2, so the flush, not the streaming, decides the pass's time when there are
// thousands of blocks (DESIGN.md has the measurement).
#ifndef RTK_DISPLAY_HIST_BLOCKS
#define RTK_DISPLAY_HIST_BLOCKS 2048
#endif

constexpr int kBins = 320;          // 8 per octave, 2^-20 .. 2^20
constexpr int kMaxLevels = 6;

// Step 1 of the rule: NaN and values <= 0 become 0, values above 65504 become 65504.
template <typename real>
RTK_DEV real sanitise(real v) {
    return v > real(0) ? (v > real(65504) ? real(65504) : v) : real(0);
}

// Step 2: the metering luminance in float32, every product and sum rounded on its own.
RTK_DEV float meter_luminance(float r, float g, float b) {
    return __fadd_rn(__fadd_rn(__fmul_rn(0.2126f, r), __fmul_rn(0.7152f, g)), __fmul_rn(0.0722f, b));
}

// Four consecutive pixels (12 reals) starting at pixel p0: 16-byte loads when `vec` (base 16-byte aligned, p0 a multiple of 4, all
// four inside), else scalar loads of the pixels below n_px (the rest 0).
template <typename real>
RTK_DEV void load4(const real* in, size_t p0, size_t n_px, bool vec, real v[12]) {
    if (vec && p0 + 4 <= n_px) {
        if constexpr (sizeof(real) == 4) {
            const float4* q = reinterpret_cast<const float4*>(in + p0 * 3);
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const float4 t = q[k];
                v[4 * k] = t.x, v[4 * k + 1] = t.y, v[4 * k + 2] = t.z, v[4 * k + 3] = t.w;
            }
        } else {
            const double2* q = reinterpret_cast<const double2*>(in + p0 * 3);
#pragma unroll
            for (int k = 0; k < 6; k++) {
                const double2 t = q[k];
                v[2 * k] = t.x, v[2 * k + 1] = t.y;
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < 12; k++) v[k] = p0 * 3 + k < n_px * 3 ? in[p0 * 3 + k] : real(0);
    }
}

// ---------------------------------------------------------------------------------------------------------- metering --
template <typename real>
__global__ __launch_bounds__(256) void rtk_display_histogram_kernel(const real* __restrict__ in, size_t n_px, int vec, unsigned int* __restrict__ hist) {
    __shared__ unsigned int bins[4][kBins];
    for (int k = threadIdx.x; k < 4 * kBins; k += 256) (&bins[0][0])[k] = 0u;
    __syncthreads();
    unsigned int* mine = bins[threadIdx.x >> 6];
    const int lane = threadIdx.x & 63;
    const size_t n_groups = (n_px + 3) / 4, stride = size_t(gridDim.x) * 256;
    for (size_t base = size_t(blockIdx.x) * 256; base < n_groups; base += stride) {   // (base is the same for the whole block)
        const size_t g = base + threadIdx.x;
        real v[12];
        if (g < n_groups) load4(in, g * 4, n_px, vec != 0, v);
#pragma unroll
        for (int p = 0; p < 4; p++) {
            bool counted = false;
            int bin = 0;
            if (g < n_groups && g * 4 + p < n_px) {
                const float y = meter_luminance(float(sanitise(v[3 * p])), float(sanitise(v[3 * p + 1])), float(sanitise(v[3 * p + 2])));
                counted = y >= 0x1p-20f;
                const int code = int(__float_as_uint(y) >> 20);
                bin = (code < 1175 ? code : 1175) - 856;
            }
            if (counted) {
#if RTK_DISPLAY_PRECOUNT
                // the ballot pre-count: the lanes that share the first counted lane's bin cost one add
                const int leader = __builtin_amdgcn_readfirstlane(bin);
                const unsigned long long same = __ballot(bin == leader);
                if (bin != leader)
                    atomicAdd(&mine[bin], 1u);
                else if (lane == __ffsll(same) - 1)
                    atomicAdd(&mine[leader], (unsigned int)__popcll(same));
#else
                atomicAdd(&mine[bin], 1u);
#endif
            }
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < kBins; k += 256) {
        const unsigned int n = bins[0][k] + bins[1][k] + bins[2][k] + bins[3][k];
        if (n) atomicAdd(&hist[k], n);
    }
}

struct MeterParams {
    double key, low, high, min_exposure, max_exposure, adapt;
    double log2_centre[8];   // log2(1 + (m + 0.5) / 8), from the host: no logarithm runs here
    int first;               // the first frame after create / reset: no previous exposure
};

// state[0] = E, state[1] = E_target.  One wave; lane l owns bins 5l .. 5l+4.
__global__ __launch_bounds__(64) void rtk_display_meter_kernel(MeterParams P, unsigned int* hist, unsigned int* __restrict__ last_hist, double* state) {
    __shared__ unsigned long long lane_count[64];
    __shared__ double lane_num[64], lane_den[64];
    const int lane = threadIdx.x;
    unsigned int c[5];
    unsigned long long own = 0;
#pragma unroll
    for (int k = 0; k < 5; k++) {
        c[k] = hist[5 * lane + k];
        last_hist[5 * lane + k] = c[k];
        hist[5 * lane + k] = 0u;   // cleared for the next frame
        own += c[k];
    }
    lane_count[lane] = own;
    __syncthreads();
    unsigned long long before = 0, total = 0;
    for (int l = 0; l < 64; l++) {
        if (l < lane) before += lane_count[l];
        total += lane_count[l];
    }
    const double lo = P.low * double(total), hi = P.high * double(total);
    double num = 0.0, den = 0.0;
    unsigned long long run = before;
#pragma unroll
    for (int k = 0; k < 5; k++) {
        const double c0 = double(run);
        run += c[k];
        const double c1 = double(run);
        const double a = c1 < hi ? c1 : hi, b = c0 > lo ? c0 : lo;
        const double m = a - b > 0.0 ? a - b : 0.0;
        const int bin = 5 * lane + k;
        const double lambda = double((bin >> 3) - 20) + P.log2_centre[bin & 7];
        num += m * lambda;
        den += m;
    }
    lane_num[lane] = num;
    lane_den[lane] = den;
    __syncthreads();
    if (lane == 0) {
        double sn = 0.0, sd = 0.0;
        for (int l = 0; l < 64; l++) {
            sn += lane_num[l];
            sd += lane_den[l];
        }
        const double prev = P.first ? 1.0 : state[0];
        double target = prev;
        if (total != 0 && sd > 0.0) {
            target = P.key / exp2(sn / sd);
            target = target < P.min_exposure ? P.min_exposure : (target > P.max_exposure ? P.max_exposure : target);
        }
        const double e = (P.first || P.adapt == 1.0) ? target : prev * pow(target / prev, P.adapt);
        state[0] = e;
        state[1] = target;
    }
}

__global__ void rtk_display_set_exposure_kernel(double e, double* state) {
    state[0] = e;
    state[1] = e;
}

// -------------------------------------------------------------------------------------------------------------- bloom --
RTK_DEV int clampi(int v, int hi) { return rtk::clampi(v, 0, hi); }

// ((a + b) + (c + d)) / 4 per channel; a, b the upper row.
RTK_DEV float4 mean4(float4 a, float4 b, float4 c, float4 d) {
    return make_float4(((a.x + b.x) + (c.x + d.x)) * 0.25f, ((a.y + b.y) + (c.y + d.y)) * 0.25f, ((a.z + b.z) + (c.z + d.z)) * 0.25f, 0.0f);
}

// Level 1: T_0 = max(E x - threshold, 0) of the frame itself, then the 2x2 mean.
template <typename real>
__global__ __launch_bounds__(256) void rtk_display_bloom_down_kernel(const real* __restrict__ in, int w, int h, const double* __restrict__ state, float threshold,
                                                                      float4* __restrict__ out, int ow, int oh) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= ow * oh) return;
    const int i = idx % ow, j = idx / ow;
    const real e = real(state[0]);
    float4 t[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int x = clampi(2 * i + (k & 1), w - 1), y = clampi(2 * j + (k >> 1), h - 1);
        const real* p = in + (size_t(y) * w + x) * 3;
        const float r = float(e * sanitise(p[0])) - threshold, g = float(e * sanitise(p[1])) - threshold, b = float(e * sanitise(p[2])) - threshold;
        t[k] = make_float4(r > 0.0f ? r : 0.0f, g > 0.0f ? g : 0.0f, b > 0.0f ? b : 0.0f, 0.0f);
    }
    out[idx] = mean4(t[0], t[1], t[2], t[3]);
}

__global__ __launch_bounds__(256) void rtk_display_bloom_halve_kernel(const float4* __restrict__ in, int w, int h, float4* __restrict__ out, int ow, int oh) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= ow * oh) return;
    const int i = idx % ow, j = idx / ow;
    const int x0 = clampi(2 * i, w - 1), x1 = clampi(2 * i + 1, w - 1), y0 = clampi(2 * j, h - 1), y1 = clampi(2 * j + 1, h - 1);
    out[idx] = mean4(in[size_t(y0) * w + x0], in[size_t(y0) * w + x1], in[size_t(y1) * w + x0], in[size_t(y1) * w + x1]);
}

// ((a + 2 b) + c) / 4 along x (VERTICAL = false) or y, edges clamped.
template <bool VERTICAL>
__global__ __launch_bounds__(256) void rtk_display_bloom_tent_kernel(const float4* __restrict__ in, int w, int h, float4* __restrict__ out) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= w * h) return;
    const int i = idx % w, j = idx / w;
    float4 a, c;
    const float4 b = in[idx];
    if constexpr (VERTICAL) {
        a = in[size_t(clampi(j - 1, h - 1)) * w + i];
        c = in[size_t(clampi(j + 1, h - 1)) * w + i];
    } else {
        a = in[size_t(j) * w + clampi(i - 1, w - 1)];
        c = in[size_t(j) * w + clampi(i + 1, w - 1)];
    }
    out[idx] = make_float4(((a.x + 2.0f * b.x) + c.x) * 0.25f, ((a.y + 2.0f * b.y) + c.y) * 0.25f, ((a.z + 2.0f * b.z) + c.z) * 0.25f, 0.0f);
}

// The centred bilinear sample of a half-size level at target texel (i, j): m = 2i - 1, x0 = floor(m / 4), fx = (m - 4 x0) / 4, taps
// x0 and x0 + 1 clamped; the same in y, y outer.
RTK_DEV float4 bilinear_half(const float4* __restrict__ low, int lw, int lh, int i, int j) {
    const int mx = 2 * i - 1, my = 2 * j - 1;
    const int x0 = (mx + 4) / 4 - 1, y0 = (my + 4) / 4 - 1;   // floor, also for m = -1
    const float fx = float(mx - 4 * x0) * 0.25f, fy = float(my - 4 * y0) * 0.25f;
    const int xa = clampi(x0, lw - 1), xb = clampi(x0 + 1, lw - 1), ya = clampi(y0, lh - 1), yb = clampi(y0 + 1, lh - 1);
    const float4 p = low[size_t(ya) * lw + xa], q = low[size_t(ya) * lw + xb], r = low[size_t(yb) * lw + xa], s = low[size_t(yb) * lw + xb];
    const float gx = 1.0f - fx, gy = 1.0f - fy;
    return make_float4(gy * (gx * p.x + fx * q.x) + fy * (gx * r.x + fx * s.x), gy * (gx * p.y + fx * q.y) + fy * (gx * r.y + fx * s.y),
                       gy * (gx * p.z + fx * q.z) + fy * (gx * r.z + fx * s.z), 0.0f);
}

// U_k = T_k + bilinear(U_{k+1}), in place in level k.
__global__ __launch_bounds__(256) void rtk_display_bloom_up_kernel(float4* __restrict__ level, int w, int h, const float4* __restrict__ low, int lw, int lh) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= w * h) return;
    const float4 t = level[idx], u = bilinear_half(low, lw, lh, idx % w, idx / w);
    level[idx] = make_float4(t.x + u.x, t.y + u.y, t.z + u.z, 0.0f);
}

// -------------------------------------------------------------------------------------------------------------- apply --
struct ApplyParams {
    size_t n_px;
    int width, height;
    int vec;                  // 16-byte accesses: every given buffer is 16-byte aligned
    float white;              // REINHARD
    float bloom, inv_levels;  // strength, 1 / n
    int bloom_w, bloom_h;     // level 1
};

// g = t <= 0.0031308 ? 12.92 t : 1.055 t^(1/2.4) - 0.055 in double, clamped to [0, 0.999], quantised like to_byte.
RTK_DEV uint8_t srgb_byte(double t) {
    double g = t <= 0.0031308 ? 12.92 * t : 1.055 * pow(t, 1.0 / 2.4) - 0.055;
    g = g < 0.000 ? 0.000 : (g > 0.999 ? 0.999 : g);
    return uint8_t(int(255.999 * g));
}

template <typename real, int CURVE, int ENCODE, bool BLOOM>
__global__ __launch_bounds__(256) void rtk_display_apply_kernel(ApplyParams P, const real* in, const double* __restrict__ state, const float4* __restrict__ bloom1,
                                                                 real* out_linear, uint8_t* __restrict__ out_rgb8) {  // (out_linear may be in: no __restrict__)
    const size_t g = size_t(blockIdx.x) * 256 + threadIdx.x, p0 = g * 4;
    if (p0 >= P.n_px) return;
    const bool full = P.vec && p0 + 4 <= P.n_px;
    real v[12];
    load4(in, p0, P.n_px, P.vec != 0, v);
    const real e = real(state[0]);
    uint8_t bytes[12];
#pragma unroll
    for (int p = 0; p < 4; p++) {
        real r = e * sanitise(v[3 * p]), gg = e * sanitise(v[3 * p + 1]), b = e * sanitise(v[3 * p + 2]);
        if constexpr (BLOOM) {
            if (p0 + p < P.n_px) {
                const size_t px = p0 + p;
                const float4 u = bilinear_half(bloom1, P.bloom_w, P.bloom_h, int(px % P.width), int(px / P.width));
                r += real(P.bloom * (u.x * P.inv_levels));
                gg += real(P.bloom * (u.y * P.inv_levels));
                b += real(P.bloom * (u.z * P.inv_levels));
            }
        }
        if constexpr (CURVE == RTK_DISPLAY_REINHARD) {
            const real y = (real(0.2126) * r + real(0.7152) * gg) + real(0.0722) * b;
            const real k = (real(1) + y / (real(P.white) * real(P.white))) / (real(1) + y);
            r *= k, gg *= k, b *= k;
        } else if constexpr (CURVE == RTK_DISPLAY_ACES) {
            real* ch[3] = {&r, &gg, &b};
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const real x = *ch[k];
                const real t = (x * (real(2.51) * x + real(0.03))) / (x * (real(2.43) * x + real(0.59)) + real(0.14));
                *ch[k] = t < real(0) ? real(0) : (t > real(1) ? real(1) : t);
            }
        }
        v[3 * p] = r, v[3 * p + 1] = gg, v[3 * p + 2] = b;
        if (out_rgb8) {
#pragma unroll
            for (int k = 0; k < 3; k++) bytes[3 * p + k] = ENCODE == RTK_DISPLAY_SRGB ? srgb_byte(double(v[3 * p + k])) : to_byte(double(v[3 * p + k]));
        }
    }
    if (full) {
        if (out_linear) {
            if constexpr (sizeof(real) == 4) {
                float4* q = reinterpret_cast<float4*>(out_linear + p0 * 3);
#pragma unroll
                for (int k = 0; k < 3; k++) q[k] = make_float4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
            } else {
                double2* q = reinterpret_cast<double2*>(out_linear + p0 * 3);
#pragma unroll
                for (int k = 0; k < 6; k++) q[k] = make_double2(v[2 * k], v[2 * k + 1]);
            }
        }
        if (out_rgb8) {   // 12 bytes at a multiple of 12 from a 16-byte aligned base: three 4-byte stores
            uint32_t* q = reinterpret_cast<uint32_t*>(out_rgb8 + p0 * 3);
#pragma unroll
            for (int k = 0; k < 3; k++)
                q[k] = uint32_t(bytes[4 * k]) | uint32_t(bytes[4 * k + 1]) << 8 | uint32_t(bytes[4 * k + 2]) << 16 | uint32_t(bytes[4 * k + 3]) << 24;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 12; k++) {
            if (p0 * 3 + k < P.n_px * 3) {
                if (out_linear) out_linear[p0 * 3 + k] = v[k];
                if (out_rgb8) out_rgb8[p0 * 3 + k] = bytes[k];
            }
        }
    }
}

template <typename real, int CURVE, int ENCODE, bool BLOOM>
void launch_apply(const ApplyParams& P, const void* in, const double* state, const float4* bloom1, void* out_linear, uint8_t* out_rgb8, hipStream_t stream) {
    const size_t groups = (P.n_px + 3) / 4;
    rtk_display_apply_kernel<real, CURVE, ENCODE, BLOOM><<<dim3((unsigned int)((groups + 255) / 256)), dim3(256), 0, stream>>>(
        P, static_cast<const real*>(in), state, bloom1, static_cast<real*>(out_linear), out_rgb8);
}

using ApplyFn = void (*)(const ApplyParams&, const void*, const double*, const float4*, void*, uint8_t*, hipStream_t);

template <typename real, int CURVE, int ENCODE>
ApplyFn pick_bloom(bool bloom) { return bloom ? launch_apply<real, CURVE, ENCODE, true> : launch_apply<real, CURVE, ENCODE, false>; }
template <typename real, int CURVE>
ApplyFn pick_encode(int encode, bool bloom) {
    return encode == RTK_DISPLAY_SRGB ? pick_bloom<real, CURVE, RTK_DISPLAY_SRGB>(bloom) : pick_bloom<real, CURVE, RTK_DISPLAY_GAMMA2>(bloom);
}
template <typename real>
ApplyFn pick_curve(int curve, int encode, bool bloom) {
    return curve == RTK_DISPLAY_ACES       ? pick_encode<real, RTK_DISPLAY_ACES>(encode, bloom)
           : curve == RTK_DISPLAY_REINHARD ? pick_encode<real, RTK_DISPLAY_REINHARD>(encode, bloom)
                                           : pick_encode<real, RTK_DISPLAY_CLAMP>(encode, bloom);
}

// ------------------------------------------------------------------------------------------------------------ options --
struct DisplayOpts {   // rtk_display_opts with the defaults filled in
    double exposure;   // 0 = metered
    MeterParams meter;
    int curve, encode, levels;
    float white, bloom, threshold;
};

bool finite_f(float v) { return v == v && v <= 3.0e38f && v >= -3.0e38f; }

// RTK_OK, or RTK_ERR_INVALID with the field's name in g_error.
int resolve_display_opts(const rtk_display_opts* in, DisplayOpts& D, const char* who) {
    rtk_display_opts o{};
    if (in) o = *in;
    const struct { const char* name; float v; } fields[] = {{"exposure", o.exposure}, {"key", o.key}, {"meter_low", o.meter_low}, {"meter_high", o.meter_high},
                                                           {"min_exposure", o.min_exposure}, {"max_exposure", o.max_exposure}, {"adapt", o.adapt}, {"white", o.white},
                                                           {"bloom", o.bloom}, {"bloom_threshold", o.bloom_threshold}};
    for (const auto& f : fields)
        if (!finite_f(f.v) || f.v < 0.0f) return fail(RTK_ERR_INVALID, "%s: %s must be finite and >= 0 (0 = default)", who, f.name);
    if (o.reserved != 0) return fail(RTK_ERR_INVALID, "%s: reserved must be 0", who);
    if (o.curve != RTK_DISPLAY_CLAMP && o.curve != RTK_DISPLAY_REINHARD && o.curve != RTK_DISPLAY_ACES) return fail(RTK_ERR_INVALID, "%s: unknown curve %d", who, o.curve);
    if (o.encode != RTK_DISPLAY_GAMMA2 && o.encode != RTK_DISPLAY_SRGB) return fail(RTK_ERR_INVALID, "%s: unknown encode %d", who, o.encode);
    if (o.bloom_levels < 0 || o.bloom_levels > kMaxLevels) return fail(RTK_ERR_INVALID, "%s: bloom_levels %d out of range (1..6, 0 = 4)", who, o.bloom_levels);
    const float low = o.meter_low == 0.0f ? 0.10f : o.meter_low, high = o.meter_high == 0.0f ? 0.90f : o.meter_high;
    if (!(low < high)) return fail(RTK_ERR_INVALID, "%s: meter_low %g must lie below meter_high %g", who, double(low), double(high));
    if (high > 1.0f) return fail(RTK_ERR_INVALID, "%s: meter_high %g above 1", who, double(high));
    const float lo_e = o.min_exposure == 0.0f ? 0x1p-10f : o.min_exposure, hi_e = o.max_exposure == 0.0f ? 0x1p10f : o.max_exposure;
    if (lo_e > hi_e) return fail(RTK_ERR_INVALID, "%s: min_exposure %g above max_exposure %g", who, double(lo_e), double(hi_e));
    if (o.adapt > 1.0f) return fail(RTK_ERR_INVALID, "%s: adapt %g out of range (0 < adapt <= 1, 0 = 1)", who, double(o.adapt));
    D.exposure = double(o.exposure);
    D.meter.key = double(o.key == 0.0f ? 0.18f : o.key);
    D.meter.low = double(low);
    D.meter.high = double(high);
    D.meter.min_exposure = double(lo_e);
    D.meter.max_exposure = double(hi_e);
    D.meter.adapt = double(o.adapt == 0.0f ? 1.0f : o.adapt);
    for (int m = 0; m < 8; m++) D.meter.log2_centre[m] = std::log2(1.0 + (m + 0.5) / 8.0);
    D.curve = o.curve;
    D.encode = o.encode;
    D.white = o.white == 0.0f ? 4.0f : o.white;
    D.bloom = o.bloom;
    D.threshold = o.bloom_threshold == 0.0f ? 1.0f : o.bloom_threshold;
    D.levels = o.bloom_levels == 0 ? 4 : o.bloom_levels;
    return RTK_OK;
}

}  // namespace
}  // namespace rtk

using namespace rtk;

struct rtk_display {
    rtk_ctx* ctx = nullptr;
    int device = 0;
    int width = 0, height = 0, real_mode = 0;
    hipStream_t stream = nullptr;
    void* memory = nullptr;        // state (2 doubles), the running histogram, the last metered histogram
    double* state = nullptr;
    unsigned int *hist = nullptr, *last_hist = nullptr;
    void* pyramid = nullptr;       // bloom: levels 1..6 and one scratch image of level 1's size, float4 texels; allocated on first use
    float4* level[kMaxLevels + 1]{};   // [1..6]
    float4* scratch = nullptr;
    int lw[kMaxLevels + 1]{}, lh[kMaxLevels + 1]{};   // [0] = the frame
    int frames = 0;                // since create / reset; 0: the next frame has no previous exposure
};

namespace {

hipError_t ensure_pyramid(rtk_display* d) {
    if (d->pyramid) return hipSuccess;
    size_t texels = 0;
    for (int k = 1; k <= kMaxLevels; k++) texels += size_t(d->lw[k]) * d->lh[k];
    const size_t scratch = size_t(d->lw[1]) * d->lh[1];
    const hipError_t e = hipMalloc(&d->pyramid, (texels + scratch) * sizeof(float4));
    if (e != hipSuccess) return e;
    float4* p = static_cast<float4*>(d->pyramid);
    for (int k = 1; k <= kMaxLevels; k++) {
        d->level[k] = p;
        p += size_t(d->lw[k]) * d->lh[k];
    }
    d->scratch = p;
    return hipSuccess;
}

template <typename real>
void launch_bloom(rtk_display* d, const void* in, const DisplayOpts& D) {
    const hipStream_t st = d->stream;
    auto blocks = [](int w, int h) { return dim3((unsigned int)((size_t(w) * h + 255) / 256)); };
    for (int k = 1; k <= D.levels; k++) {
        const int w = d->lw[k], h = d->lh[k];
        if (k == 1)
            rtk_display_bloom_down_kernel<real><<<blocks(w, h), dim3(256), 0, st>>>(static_cast<const real*>(in), d->lw[0], d->lh[0], d->state, D.threshold, d->level[1], w, h);
        else
            rtk_display_bloom_halve_kernel<<<blocks(w, h), dim3(256), 0, st>>>(d->level[k - 1], d->lw[k - 1], d->lh[k - 1], d->level[k], w, h);
        rtk_display_bloom_tent_kernel<false><<<blocks(w, h), dim3(256), 0, st>>>(d->level[k], w, h, d->scratch);
        rtk_display_bloom_tent_kernel<true><<<blocks(w, h), dim3(256), 0, st>>>(d->scratch, w, h, d->level[k]);
    }
    for (int k = D.levels - 1; k >= 1; k--)
        rtk_display_bloom_up_kernel<<<blocks(d->lw[k], d->lh[k]), dim3(256), 0, st>>>(d->level[k], d->lw[k], d->lh[k], d->level[k + 1], d->lw[k + 1], d->lh[k + 1]);
}

}  // namespace

extern "C" {

int rtk_display_create(rtk_ctx* ctx, int32_t width, int32_t height, int32_t real_mode, void* stream, rtk_display** out) {
    if (!ctx || !out) return fail(RTK_ERR_INVALID, "rtk_display_create: null argument");
    if (check_image_size("rtk_display_create", width, height) != RTK_OK) return RTK_ERR_INVALID;
    if (size_t(width) * height > (size_t(1) << 31) - 4) return fail(RTK_ERR_INVALID, "rtk_display_create: image %dx%d has more than 2^31 pixels", width, height);
    if (check_real_mode("rtk_display_create", real_mode) != RTK_OK) return RTK_ERR_INVALID;
    hipError_t e = hipSetDevice(ctx_device(ctx));
    if (e != hipSuccess) return fail(RTK_ERR_HIP, "rtk_display_create: %s", hipGetErrorString(e));
    const size_t bytes = 2 * sizeof(double) + 2 * kBins * sizeof(unsigned int);
    void* mem = nullptr;
    e = hipMalloc(&mem, bytes);
    if (e == hipSuccess) {
        e = hipMemsetAsync(mem, 0, bytes, static_cast<hipStream_t>(stream));   // in stream order before the first frame; nothing waits
        if (e != hipSuccess) (void)hipFree(mem);
    }
    if (e != hipSuccess) return fail(RTK_ERR_HIP, "rtk_display_create: %s", hipGetErrorString(e));
    rtk_display* d = new rtk_display;
    d->ctx = ctx;
    d->device = ctx_device(ctx);
    d->width = width;
    d->height = height;
    d->real_mode = real_mode;
    d->stream = static_cast<hipStream_t>(stream);
    d->memory = mem;
    d->state = static_cast<double*>(mem);
    d->hist = reinterpret_cast<unsigned int*>(d->state + 2);
    d->last_hist = d->hist + kBins;
    d->lw[0] = width;
    d->lh[0] = height;
    for (int k = 1; k <= kMaxLevels; k++) {
        d->lw[k] = (d->lw[k - 1] + 1) / 2;
        d->lh[k] = (d->lh[k - 1] + 1) / 2;
    }
    *out = d;
    return RTK_OK;
}

int rtk_display_apply(rtk_display* d, const void* d_linear, const rtk_display_opts* opts, void* d_out_linear, uint8_t* d_out_rgb8) {
    const char* who = "rtk_display_apply";
    DisplayOpts D{};
    if (resolve_display_opts(opts, D, who) != RTK_OK) return RTK_ERR_INVALID;
    if (!d) return fail(RTK_ERR_INVALID, "%s: null object", who);
    if (!d_linear) return fail(RTK_ERR_INVALID, "%s: d_linear is required", who);
    if (!d_out_linear && !d_out_rgb8) return fail(RTK_ERR_INVALID, "%s: no output", who);
    hipError_t e = hipSetDevice(d->device);
    const bool bloom = D.bloom > 0.0f;
    if (e == hipSuccess && bloom) e = ensure_pyramid(d);
    if (e != hipSuccess) return fail(RTK_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    const bool f64 = d->real_mode == RTK_REAL_F64;
    const size_t n_px = size_t(d->width) * d->height;
    const int vec_in = aligned16(d_linear);
    if (D.exposure > 0.0) {
        rtk_display_set_exposure_kernel<<<dim3(1), dim3(1), 0, d->stream>>>(D.exposure, d->state);
    } else {
        const size_t groups = (n_px + 3) / 4, blocks = (groups + 255) / 256;
        const dim3 grid((unsigned int)(blocks < RTK_DISPLAY_HIST_BLOCKS ? blocks : RTK_DISPLAY_HIST_BLOCKS));
        if (f64)
            rtk_display_histogram_kernel<double><<<grid, dim3(256), 0, d->stream>>>(static_cast<const double*>(d_linear), n_px, vec_in, d->hist);
        else
            rtk_display_histogram_kernel<float><<<grid, dim3(256), 0, d->stream>>>(static_cast<const float*>(d_linear), n_px, vec_in, d->hist);
        D.meter.first = d->frames == 0;
        rtk_display_meter_kernel<<<dim3(1), dim3(64), 0, d->stream>>>(D.meter, d->hist, d->last_hist, d->state);
    }
    if (bloom) {
        if (f64)
            launch_bloom<double>(d, d_linear, D);
        else
            launch_bloom<float>(d, d_linear, D);
    }
    ApplyParams P{};
    P.n_px = n_px;
    P.width = d->width;
    P.height = d->height;
    P.vec = vec_in && (!d_out_linear || aligned16(d_out_linear)) && (!d_out_rgb8 || aligned16(d_out_rgb8));
    P.white = D.white;
    P.bloom = D.bloom;
    P.inv_levels = 1.0f / float(D.levels);
    P.bloom_w = d->lw[1];
    P.bloom_h = d->lh[1];
    const ApplyFn apply = f64 ? pick_curve<double>(D.curve, D.encode, bloom) : pick_curve<float>(D.curve, D.encode, bloom);
    apply(P, d_linear, d->state, d->level[1], d_out_linear, d_out_rgb8, d->stream);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(RTK_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    d->frames++;
    return RTK_OK;
}

int rtk_display_apply_host(rtk_display* d, const double* h_linear, const rtk_display_opts* opts, double* h_out_linear, uint8_t* h_out_rgb8) {
    const char* who = "rtk_display_apply_host";
    {
        DisplayOpts D{};
        if (resolve_display_opts(opts, D, who) != RTK_OK) return RTK_ERR_INVALID;
    }
    if (!d) return fail(RTK_ERR_INVALID, "%s: null object", who);
    if (!h_linear) return fail(RTK_ERR_INVALID, "%s: h_linear is required", who);
    if (!h_out_linear && !h_out_rgb8) return fail(RTK_ERR_INVALID, "%s: no output", who);
    hipError_t e = hipSetDevice(d->device);
    if (e != hipSuccess) return fail(RTK_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    const size_t px = size_t(d->width) * d->height;
    HostStaging s(d->real_mode == RTK_REAL_F64);
    const int lin = s.linear(px * 3), rgb8 = s.piece(px * 3, h_out_rgb8 != nullptr);   // linear is in, then out in place
    e = s.alloc();
    if (e == hipSuccess) e = s.upload_linear(lin, h_linear);
    if (e != hipSuccess) return fail(RTK_ERR_HIP, "%s: device buffers: %s", who, hipGetErrorString(e));
    const int rc = rtk_display_apply(d, s.ptr(lin), opts, h_out_linear ? s.ptr(lin) : nullptr, s.ptr<uint8_t>(rgb8));
    if (rc != RTK_OK) return rc;
    e = hipStreamSynchronize(d->stream);
    if (e == hipSuccess) e = s.download_linear(lin, h_out_linear);
    if (e == hipSuccess) e = s.download(rgb8, h_out_rgb8);
    if (e != hipSuccess) return fail(RTK_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    return RTK_OK;
}

int rtk_display_exposure(rtk_display* d, double out[2]) {
    if (!d || !out) return fail(RTK_ERR_INVALID, "rtk_display_exposure: null argument");
    if (d->frames == 0) {   // nothing applied since create / reset
        out[0] = out[1] = 1.0;
        return RTK_OK;
    }
    hipError_t e = hipSetDevice(d->device);
    if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
    if (e == hipSuccess) e = hipMemcpy(out, d->state, 2 * sizeof(double), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(RTK_ERR_HIP, "rtk_display_exposure: %s", hipGetErrorString(e));
    return RTK_OK;
}

int rtk_display_histogram(rtk_display* d, uint32_t out[320]) {
    if (!d || !out) return fail(RTK_ERR_INVALID, "rtk_display_histogram: null argument");
    hipError_t e = hipSetDevice(d->device);
    if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
    if (e == hipSuccess) e = hipMemcpy(out, d->last_hist, kBins * sizeof(unsigned int), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(RTK_ERR_HIP, "rtk_display_histogram: %s", hipGetErrorString(e));
    return RTK_OK;
}

int rtk_display_reset(rtk_display* d) {
    if (!d) return fail(RTK_ERR_INVALID, "rtk_display_reset: null object");
    d->frames = 0;  // the next frame's metering kernel is told that there is no previous exposure: nothing to enqueue
    return RTK_OK;
}

int rtk_display_frames(const rtk_display* d) {
    if (!d) return fail(RTK_ERR_INVALID, "rtk_display_frames: null object");
    return d->frames;
}

int rtk_display_destroy(rtk_display* d) {
    if (!d) return RTK_OK;
    hipError_t e = hipSetDevice(d->device);
    if (e == hipSuccess) e = hipStreamSynchronize(d->stream);  // the last frame may still use the object's memory
    (void)hipFree(d->pyramid);
    (void)hipFree(d->memory);
    delete d;
    if (e != hipSuccess) return fail(RTK_ERR_HIP, "rtk_display_destroy: %s", hipGetErrorString(e));
    return RTK_OK;
}

}  // extern "C"
