// rtk_upsample.hip -- guided upsampling (include/rtk.h, "Guided upsampling"): joint-bilateral upsampling (Kopf et al. 2007) of a
// frame rendered at 1/f of the width and height, steered by the guides of both resolutions, optionally on demodulated
// irradiance.  One kernel per frame: every full-resolution pixel gathers the four low-resolution pixels around it, weighs them
// with the guided filter's own expressions (rtk_guide_weights.h) and writes colour, standard error, bytes and support.
// Hand-written HIP for gfx950, wave64.
//
// Layout.  One lane per full pixel, one wave per 8x8 tile (the render's tile convention), four tiles per 256-thread block.  A
// lane reads its own four guide float4s, the depths of its four neighbours (lines its own tile or the next one loads anyway)
// and four low-resolution taps of 3 reals + se + three float4s + one hit fraction each.  The taps of a wave cover a patch of at
// most (8 / f + 2)^2 low pixels -- 36 at f = 2, 16 at f = 4, each read by up to 4 f^2 lanes of the same wave or its neighbour -- a few
// KB that the vector L1 serves after the first touch.  Nothing is staged in LDS: staging would cost a barrier and a divergent
// fill for data that is read four times per lane and is already one L1 hit away, and most of the pass's memory traffic is the
// full-resolution guide reads and the output writes, not the taps ("Guided upsampling").
//
// Arithmetic.  The tap position is integer arithmetic; everything after it is float32, without atomics and in a fixed tap order
// (b outer, a inner): the same inputs give the same bits.
#include <hip/hip_runtime.h>

#include <cmath>

#include "rtk.h"
#include "rtk_guide_weights.h"
#include "rtk_internal.h"

namespace rtk {
namespace {

struct UpsampleParams {
    TileGrid grid;   // the full image
    int low_width, low_height, factor;
    float sigma_n, sigma_z, sigma_a;
};

// floor(n / d) and the remainder in 0 .. d-1, d > 0, n >= -(d - 1).
__device__ __forceinline__ void floor_div(int n, int d, int& q, int& r) {
    q = (n + d) / d - 1;
    r = n - q * d;
}

template <typename real, bool DEMOD>
__global__ __launch_bounds__(256) void rtk_upsample_kernel(UpsampleParams P, const real* __restrict__ low_linear, const float* __restrict__ low_noise,
                                                            const float4* __restrict__ low_guides, const float4* __restrict__ guides,
                                                            real* __restrict__ out_linear, float* __restrict__ out_noise, uint8_t* __restrict__ out_rgb8,
                                                            float* __restrict__ out_support) {
    int i, j;
    if (!lane_pixel(P.grid, i, j)) return;
    const int W = P.grid.width, H = P.grid.height, LW = P.low_width, LH = P.low_height, f = P.factor;
    const size_t px = size_t(j) * W + i;
    const float hit1_p = guides[px * 4].w;
    const float4 g1p = guides[px * 4 + 1], ap = guides[px * 4 + 2], g2p = guides[px * 4 + 3];  // {normal, depth}, {seen albedo, end hit}, {end normal, length}
    const float grad1 = guide_depth_gradient(guides, 1, i, j, W, H), grad2 = guide_depth_gradient(guides, 3, i, j, W, H);
    const bool n1p_zero = zero3(g1p), n2p_zero = zero3(g2p);
    const float n1p_len = sqrtf(g1p.x * g1p.x + g1p.y * g1p.y + g1p.z * g1p.z), n2p_len = sqrtf(g2p.x * g2p.x + g2p.y * g2p.y + g2p.z * g2p.z);
    int x0, y0, rx, ry;
    floor_div(2 * i - (f - 1), 2 * f, x0, rx);
    floor_div(2 * j - (f - 1), 2 * f, y0, ry);
    const float fx = float(rx) / float(2 * f), fy = float(ry) / float(2 * f);
    float so = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f, s_beta = 0.0f, s_acc = 0.0f;
    for (int tb = 0; tb < 2; tb++) {
        const int tj = y0 + tb;
        if (tj < 0 || tj >= LH) continue;
        for (int ta = 0; ta < 2; ta++) {
            const int ti = x0 + ta;
            if (ti < 0 || ti >= LW) continue;
            const size_t q = size_t(tj) * LW + ti;
            const float hit1_q = low_guides[q * 4].w;
            const float4 g1q = low_guides[q * 4 + 1], aq = low_guides[q * 4 + 2], g2q = low_guides[q * 4 + 3];
            float cr = float(low_linear[q * 3]), cg = float(low_linear[q * 3 + 1]), cb = float(low_linear[q * 3 + 2]);
            const float se = low_noise[q];
            float var = se * se;
            const float beta = (ta ? fx : 1.0f - fx) * (tb ? fy : 1.0f - fy);
            const float wn1 = normal_weight(g1p, n1p_zero, n1p_len, g1q, P.sigma_n), wn2 = normal_weight(g2p, n2p_zero, n2p_len, g2q, P.sigma_n);
            const float wn = wn1 < wn2 ? wn1 : wn2;
            const float ox = fx - float(ta), oy = fy - float(tb);
            const float o = float(f) * sqrtf(ox * ox + oy * oy);
            const float wz1 = depth_weight(hit1_p, hit1_q, g1p.w, g1q.w, grad1, o, P.sigma_z), wz2 = depth_weight(ap.w, aq.w, g2p.w, g2q.w, grad2, o, P.sigma_z);
            const float wz = wz1 < wz2 ? wz1 : wz2;
            float wa = 1.0f;
            if constexpr (DEMOD) {
                const float4 A = demodulation_albedo(aq);
                const float m = (A.x + A.y + A.z) / 3.0f;
                cr /= A.x;
                cg /= A.y;
                cb /= A.z;
                var /= m * m;
            } else {
                const float ex = ap.x - aq.x, ey = ap.y - aq.y, ez = ap.z - aq.z;
                wa = __expf(-sqrtf(ex * ex + ey * ey + ez * ez) / P.sigma_a);
            }
            const float w = wn * wz * wa;
            const float om = beta * (w + 1e-3f);
            so += om;
            sr += om * cr;
            sg += om * cg;
            sb += om * cb;
            sv += om * om * var;
            s_beta += beta;
            s_acc += beta * w;
        }
    }
    float r = sr / so, g = sg / so, b = sb / so, var_out = sv / (so * so);
    if constexpr (DEMOD) {
        const float4 A = demodulation_albedo(ap);
        const float m = (A.x + A.y + A.z) / 3.0f;
        r *= A.x;
        g *= A.y;
        b *= A.z;
        var_out *= m * m;
    }
    if (out_linear) {
        out_linear[px * 3] = real(r);
        out_linear[px * 3 + 1] = real(g);
        out_linear[px * 3 + 2] = real(b);
    }
    if (out_noise) out_noise[px] = sqrtf(var_out);
    if (out_support) out_support[px] = s_acc / s_beta;
    if (out_rgb8) {
        out_rgb8[px * 3] = to_byte(double(r));
        out_rgb8[px * 3 + 1] = to_byte(double(g));
        out_rgb8[px * 3 + 2] = to_byte(double(b));
    }
}

// The options with defaults for 0 fields, written into P; RTK_ERR_INVALID (reason in g_error) when they are out of range.
int resolve_upsample_opts(const rtk_upsample_opts* in, UpsampleParams& P, bool& demodulate, const char* who) {
    rtk_upsample_opts o{};
    if (in) o = *in;
    if (o.flags & ~RTK_UPSAMPLE_DEMODULATE) return fail(RTK_ERR_INVALID, "%s: unknown flags 0x%x", who, unsigned(o.flags));
    if (o.reserved != 0) return fail(RTK_ERR_INVALID, "%s: reserved must be 0", who);
    if (o.factor != 0 && (o.factor < 2 || o.factor > 4)) return fail(RTK_ERR_INVALID, "%s: factor %d out of range (2..4, 0 = 2)", who, o.factor);
    const float s[3] = {o.sigma_n, o.sigma_z, o.sigma_a};
    for (float v : s)
        if (!(v >= 0.0f) || v > 3.0e38f) return fail(RTK_ERR_INVALID, "%s: sigmas must be finite and >= 0 (0 = default)", who);
    P.factor = o.factor == 0 ? 2 : o.factor;
    P.sigma_n = o.sigma_n == 0.0f ? 128.0f : o.sigma_n;
    P.sigma_z = o.sigma_z == 0.0f ? 1.0f : o.sigma_z;
    P.sigma_a = o.sigma_a == 0.0f ? 0.1f : o.sigma_a;
    demodulate = (o.flags & RTK_UPSAMPLE_DEMODULATE) != 0;
    return RTK_OK;
}

// The checks rtk_upsample and rtk_upsample_host share (options first: they need neither context nor device).
int check_upsample_args(const char* who, const rtk_upsample_opts* opts, UpsampleParams& P, bool& demodulate, const rtk_ctx* ctx, const rtk_camera* full,
                        int32_t real_mode, bool inputs, bool outputs) {
    if (resolve_upsample_opts(opts, P, demodulate, who) != RTK_OK) return RTK_ERR_INVALID;
    if (!ctx) return fail(RTK_ERR_INVALID, "%s: null context", who);
    if (!full) return fail(RTK_ERR_INVALID, "%s: null camera", who);
    if (!inputs) return fail(RTK_ERR_INVALID, "%s: the low-resolution colour, noise and guides and the full-resolution guides are required", who);
    if (!outputs) return fail(RTK_ERR_INVALID, "%s: no output", who);
    if (check_image_size(who, full->image_width, full->image_height) != RTK_OK || check_real_mode(who, real_mode) != RTK_OK) return RTK_ERR_INVALID;
    P.grid = tile_grid(full->image_width, full->image_height);
    P.low_width = (P.grid.width + P.factor - 1) / P.factor;
    P.low_height = (P.grid.height + P.factor - 1) / P.factor;
    return RTK_OK;
}

template <typename real, bool DEMOD>
void launch_upsample(const UpsampleParams& P, const void* low_linear, const float* low_noise, const float* low_guides, const float* guides, void* out_linear,
                     float* out_noise, uint8_t* out_rgb8, float* out_support, hipStream_t stream) {
    const dim3 grid((P.grid.n_tiles + 3) / 4), block(256);
    rtk_upsample_kernel<real, DEMOD><<<grid, block, 0, stream>>>(P, static_cast<const real*>(low_linear), low_noise, reinterpret_cast<const float4*>(low_guides),
                                                                 reinterpret_cast<const float4*>(guides), static_cast<real*>(out_linear), out_noise, out_rgb8,
                                                                 out_support);
}

}  // namespace
}  // namespace rtk

using namespace rtk;

extern "C" {

int rtk_upsample_camera(const rtk_camera* full, int32_t factor, rtk_camera* out_low) {
    if (!full || !out_low) return fail(RTK_ERR_INVALID, "rtk_upsample_camera: null argument");
    if (factor < 2 || factor > 4) return fail(RTK_ERR_INVALID, "rtk_upsample_camera: factor %d out of range (2..4)", factor);
    if (full->image_width <= 0 || full->image_height <= 0) return fail(RTK_ERR_INVALID, "rtk_upsample_camera: bad image size %dx%d", full->image_width, full->image_height);
    rtk_camera low = *full;
    low.image_width = (full->image_width + factor - 1) / factor;
    low.image_height = (full->image_height + factor - 1) / factor;
    const double f = double(factor), h = (f - 1.0) / 2.0;
    const rtk_vec3 &du = full->pixel_delta_u, &dv = full->pixel_delta_v;
    low.pixel00_loc = rtk_vec3{full->pixel00_loc.x + h * (du.x + dv.x), full->pixel00_loc.y + h * (du.y + dv.y), full->pixel00_loc.z + h * (du.z + dv.z)};
    low.pixel_delta_u = rtk_vec3{f * du.x, f * du.y, f * du.z};
    low.pixel_delta_v = rtk_vec3{f * dv.x, f * dv.y, f * dv.z};
    *out_low = low;
    return RTK_OK;
}

int rtk_upsample(rtk_ctx* ctx, const rtk_camera* full, int32_t real_mode, const void* d_low_linear, const float* d_low_noise, const float* d_low_guides,
                 const float* d_guides, const rtk_upsample_opts* opts, void* d_out_linear, float* d_out_noise, uint8_t* d_out_rgb8, float* d_out_support,
                 void* stream) {
    const char* who = "rtk_upsample";
    UpsampleParams P{};
    bool demod = false;
    const int rc = check_upsample_args(who, opts, P, demod, ctx, full, real_mode, d_low_linear && d_low_noise && d_low_guides && d_guides,
                                       d_out_linear || d_out_noise || d_out_rgb8 || d_out_support);
    if (rc != RTK_OK) return rc;
    if (check_aligned16(d_low_guides, who, "d_low_guides") != RTK_OK || check_aligned16(d_guides, who, "d_guides") != RTK_OK) return RTK_ERR_INVALID;
    hipError_t e = hipSetDevice(ctx_device(ctx));
    if (e == hipSuccess) {
        const hipStream_t st = static_cast<hipStream_t>(stream);
        e = with_real_demod(real_mode == RTK_REAL_F64, demod, [&](auto real, auto dm) {
            launch_upsample<decltype(real), decltype(dm)::value>(P, d_low_linear, d_low_noise, d_low_guides, d_guides, d_out_linear, d_out_noise, d_out_rgb8,
                                                                 d_out_support, st);
            return hipGetLastError();
        });
    }
    if (e != hipSuccess) return fail(RTK_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    return RTK_OK;
}

int rtk_upsample_host(rtk_ctx* ctx, const rtk_camera* full, int32_t real_mode, const double* h_low_linear, const float* h_low_noise, const float* h_low_guides,
                      const float* h_guides, const rtk_upsample_opts* opts, double* h_out_linear, float* h_out_noise, uint8_t* h_out_rgb8, float* h_out_support) {
    const char* who = "rtk_upsample_host";
    UpsampleParams P{};
    bool demod = false;
    int rc = check_upsample_args(who, opts, P, demod, ctx, full, real_mode, h_low_linear && h_low_noise && h_low_guides && h_guides,
                                 h_out_linear || h_out_noise || h_out_rgb8 || h_out_support);
    if (rc != RTK_OK) return rc;
    hipError_t e = hipSetDevice(ctx_device(ctx));
    if (e != hipSuccess) return fail(RTK_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    const size_t px = size_t(P.grid.width) * P.grid.height, lpx = size_t(P.low_width) * P.low_height;
    HostStaging s(real_mode == RTK_REAL_F64);
    const int guides = s.piece(px * 16 * sizeof(float)), low_guides = s.piece(lpx * 16 * sizeof(float)), low = s.linear(lpx * 3), low_noise = s.piece(lpx * sizeof(float));
    const int out = s.linear(px * 3, h_out_linear != nullptr), noise = s.piece(px * sizeof(float), h_out_noise != nullptr);
    const int support = s.piece(px * sizeof(float), h_out_support != nullptr), rgb8 = s.piece(px * 3, h_out_rgb8 != nullptr);
    e = s.alloc();
    if (e == hipSuccess) e = s.upload_linear(low, h_low_linear);
    if (e == hipSuccess) e = s.upload(guides, h_guides);
    if (e == hipSuccess) e = s.upload(low_guides, h_low_guides);
    if (e == hipSuccess) e = s.upload(low_noise, h_low_noise);
    if (e != hipSuccess) return fail(RTK_ERR_HIP, "%s: device buffers: %s", who, hipGetErrorString(e));
    rc = rtk_upsample(ctx, full, real_mode, s.ptr(low), s.ptr<float>(low_noise), s.ptr<float>(low_guides), s.ptr<float>(guides), opts, s.ptr(out), s.ptr<float>(noise),
                      s.ptr<uint8_t>(rgb8), s.ptr<float>(support), nullptr);
    if (rc != RTK_OK) return rc;
    e = hipStreamSynchronize(nullptr);
    if (e == hipSuccess) e = s.download_linear(out, h_out_linear);
    if (e == hipSuccess) e = s.download(noise, h_out_noise);
    if (e == hipSuccess) e = s.download(support, h_out_support);
    if (e == hipSuccess) e = s.download(rgb8, h_out_rgb8);
    if (e != hipSuccess) return fail(RTK_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    return RTK_OK;
}

}  // extern "C"
