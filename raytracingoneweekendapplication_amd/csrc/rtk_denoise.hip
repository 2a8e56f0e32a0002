// rtk_denoise.hip -- the entry points of the AOV and guide passes (their kernel, rtk_guide_kernel without and with the chain, shares
// the traversal of rtk_trace.hip) and the variance-guided edge-avoiding a-trous filter of include/rtk.h ("Denoiser"): Dammertz et
// al. 2010 with the luminance weight of SVGF (Schied et al. 2017), spatial part only, and its guided form ("Guides that follow
// mirrors": two sets of guides, optional albedo demodulation).  Hand-written HIP for gfx950, wave64.
//
// Layout.  Every pixel carries its colour and variance as one float4 {r, g, b, var} (the context's ping-pong buffers) and its
// guides as the two float4s rtk_render_aovs writes, {albedo, hit fraction} and {mean normal, depth}: a tap is three 16-byte
// loads.  One lane per pixel, one wave per 8x8 tile (the render's tile convention), four tiles per 256-thread block.  The 5x5
// taps of a wave cover at most (8 + 4 * step)^2 pixels, which the vector L1 / L2 serve; nothing is staged in LDS.
//
// Determinism.  No atomics, a fixed tap order (dy outer, dx inner) and f32 arithmetic throughout: the same inputs give the same
// bits on every run.
#include <hip/hip_runtime.h>

#include "rtk.h"
#include "rtk_guide_weights.h"
#include "rtk_internal.h"
#include "rtk_trace.h"

namespace rtk {
namespace {

#define RTK_DN __device__ __forceinline__

struct DenoiseParams {
    TileGrid grid;
    float sigma_l, sigma_n, sigma_z, sigma_a;
};

// {colour, se^2} of the input image, the colour read as `real` and rounded to float.
template <typename real>
__global__ __launch_bounds__(256) void rtk_denoise_pack_kernel(DenoiseParams P, const real* __restrict__ linear, const float* __restrict__ noise,
                                                                float4* __restrict__ cv) {
    int i, j;
    if (!lane_pixel(P.grid, i, j)) return;
    const size_t px = size_t(j) * P.grid.width + i;
    const float se = noise[px];
    cv[px] = make_float4(float(linear[px * 3]), float(linear[px * 3 + 1]), float(linear[px * 3 + 2]), se * se);
}

RTK_DN float luminance(float4 c) { return (c.x + c.y + c.z) / 3.0f; }

// One a-trous iteration with taps 2^k apart.  A final iteration (out_cv null) writes the colour as `real` and / or bytes.
template <typename real>
__global__ __launch_bounds__(256) void rtk_denoise_step_kernel(DenoiseParams P, int step, const float4* __restrict__ cv, const float4* __restrict__ aov,
                                                                float4* __restrict__ out_cv, real* __restrict__ out_linear, uint8_t* __restrict__ out_rgb8) {
    int i, j;
    if (!lane_pixel(P.grid, i, j)) return;
    const int W = P.grid.width, H = P.grid.height;
    const size_t px = size_t(j) * W + i;
    const float4 cp = cv[px];
    const float4 ap = aov[px * 2], gp = aov[px * 2 + 1];  // {albedo, hit}, {normal, depth}
    // gv_p: 3x3 binomial (1 2 1)/4 x (1 2 1)/4 of the variance, edges clamped
    const float bw[3] = {0.25f, 0.5f, 0.25f};
    float gv = 0.0f;
    for (int b = -1; b <= 1; b++) {
        const size_t row = size_t(clampi(j + b, 0, H - 1)) * W;
        for (int a = -1; a <= 1; a++) gv += bw[b + 1] * bw[a + 1] * cv[row + clampi(i + a, 0, W - 1)].w;
    }
    // depth gradient: half the larger central difference, edges clamped
    const float zx = fabsf(aov[(size_t(j) * W + clampi(i + 1, 0, W - 1)) * 2 + 1].w - aov[(size_t(j) * W + clampi(i - 1, 0, W - 1)) * 2 + 1].w);
    const float zy = fabsf(aov[(size_t(clampi(j + 1, 0, H - 1)) * W + i) * 2 + 1].w - aov[(size_t(clampi(j - 1, 0, H - 1)) * W + i) * 2 + 1].w);
    const float grad = (zx > zy ? zx : zy) / 2.0f;
    const float yp = luminance(cp);
    const float l_den = P.sigma_l * sqrtf(gv > 0.0f ? gv : 0.0f) + 1e-6f;
    const bool np_zero = gp.x == 0.0f && gp.y == 0.0f && gp.z == 0.0f;
    const float np_len = sqrtf(gp.x * gp.x + gp.y * gp.y + gp.z * gp.z);
    const float h[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f;
    for (int dy = -2; dy <= 2; dy++) {
        const int qj = j + step * dy;
        if (qj < 0 || qj >= H) continue;
        for (int dx = -2; dx <= 2; dx++) {
            const int qi = i + step * dx;
            if (qi < 0 || qi >= W) continue;
            const size_t q = size_t(qj) * W + qi;
            const float4 cq = cv[q];
            const float4 aq = aov[q * 2], gq = aov[q * 2 + 1];
            const float wl = __expf(-fabsf(yp - luminance(cq)) / l_den);
            const bool nq_zero = gq.x == 0.0f && gq.y == 0.0f && gq.z == 0.0f;
            float wn;
            if (np_zero || nq_zero) {
                wn = np_zero && nq_zero ? 1.0f : 0.0f;
            } else {
                const float c = (gp.x * gq.x + gp.y * gq.y + gp.z * gq.z) / (np_len * sqrtf(gq.x * gq.x + gq.y * gq.y + gq.z * gq.z));
                wn = c > 0.0f ? __powf(c, P.sigma_n) : 0.0f;
            }
            float wz = 1.0f;
            if (ap.w != 0.0f && aq.w != 0.0f) {
                const float o = float(step) * sqrtf(float(dx * dx + dy * dy));
                wz = __expf(-fabsf(gp.w - gq.w) / (P.sigma_z * (grad * o + 1e-3f * gp.w) + 1e-6f));
            }
            const float ex = ap.x - aq.x, ey = ap.y - aq.y, ez = ap.z - aq.z;
            const float wa = __expf(-sqrtf(ex * ex + ey * ey + ez * ez) / P.sigma_a);
            const float w = h[dx + 2] * h[dy + 2] * wl * wn * wz * wa;
            sw += w;
            sr += w * cq.x;
            sg += w * cq.y;
            sb += w * cq.z;
            sv += w * w * cq.w;
        }
    }
    const float r = sr / sw, g = sg / sw, b = sb / sw;
    if (out_cv) {
        out_cv[px] = make_float4(r, g, b, sv / (sw * sw));
        return;
    }
    if (out_linear) {
        out_linear[px * 3] = real(r);
        out_linear[px * 3 + 1] = real(g);
        out_linear[px * 3 + 2] = real(b);
    }
    if (out_rgb8) {
        out_rgb8[px * 3] = to_byte(double(r));
        out_rgb8[px * 3 + 1] = to_byte(double(g));
        out_rgb8[px * 3 + 2] = to_byte(double(b));
    }
}

template <typename real>
hipError_t launch_denoise(const DenoiseParams& P, int iterations, const void* linear, const float* noise, const float4* aov, float4* ping, float4* pong,
                          void* out_linear, uint8_t* out_rgb8, hipStream_t stream) {
    const dim3 grid((P.grid.n_tiles + 3) / 4), block(256);
    rtk_denoise_pack_kernel<real><<<grid, block, 0, stream>>>(P, static_cast<const real*>(linear), noise, ping);
    hipError_t e = hipGetLastError();
    for (int k = 0; k < iterations && e == hipSuccess; k++) {
        const bool last = k == iterations - 1;
        rtk_denoise_step_kernel<real><<<grid, block, 0, stream>>>(P, 1 << k, ping, aov, last ? nullptr : pong, last ? static_cast<real*>(out_linear) : nullptr,
                                                                  last ? out_rgb8 : nullptr);
        e = hipGetLastError();
        float4* t = ping;
        ping = pong;
        pong = t;
    }
    return e;
}

// ---- the guided filter (rtk_denoise_guided): guides are the four float4s rtk_render_guides writes per pixel, {first albedo,
// hit}, {normal, depth}, {seen albedo, end hit}, {end normal, path length}.  A tap reads the colour, the last three and the
// first one's hit fraction (a 4-byte load): 4 x 16 B + 4 B.  The weights are the expressions of rtk_denoise_step_kernel, once
// per set, so guides whose second set equals the first give that kernel's bits.

// The weights (guide_depth_gradient, normal_weight, depth_weight, demodulation_albedo) are rtk_guide_weights.h's, shared with
// the upsampling pass.

// rtk_denoise_pack_kernel, and with DEMOD the division by the albedo: c' = c / A, var' = var / mean(A)^2.
template <typename real, bool DEMOD>
__global__ __launch_bounds__(256) void rtk_denoise_guided_pack_kernel(DenoiseParams P, const real* __restrict__ linear, const float* __restrict__ noise,
                                                                       const float4* __restrict__ guides, float4* __restrict__ cv) {
    int i, j;
    if (!lane_pixel(P.grid, i, j)) return;
    const size_t px = size_t(j) * P.grid.width + i;
    const float se = noise[px];
    float4 c = make_float4(float(linear[px * 3]), float(linear[px * 3 + 1]), float(linear[px * 3 + 2]), se * se);
    if constexpr (DEMOD) {
        const float4 A = demodulation_albedo(guides[px * 4 + 2]);
        const float m = (A.x + A.y + A.z) / 3.0f;
        c = make_float4(c.x / A.x, c.y / A.y, c.z / A.z, c.w / (m * m));
    }
    cv[px] = c;
}

// One guided a-trous iteration with taps 2^k apart (rtk_denoise_step_kernel's conventions).
template <typename real, bool DEMOD>
__global__ __launch_bounds__(256) void rtk_denoise_guided_step_kernel(DenoiseParams P, int step, const float4* __restrict__ cv, const float4* __restrict__ guides,
                                                                       float4* __restrict__ out_cv, real* __restrict__ out_linear, uint8_t* __restrict__ out_rgb8) {
    int i, j;
    if (!lane_pixel(P.grid, i, j)) return;
    const int W = P.grid.width, H = P.grid.height;
    const size_t px = size_t(j) * W + i;
    const float4 cp = cv[px];
    const float hit1_p = guides[px * 4].w;
    const float4 g1p = guides[px * 4 + 1], ap = guides[px * 4 + 2], g2p = guides[px * 4 + 3];  // {normal, depth}, {seen albedo, end hit}, {end normal, length}
    const float bw[3] = {0.25f, 0.5f, 0.25f};
    float gv = 0.0f;
    for (int b = -1; b <= 1; b++) {
        const size_t row = size_t(clampi(j + b, 0, H - 1)) * W;
        for (int a = -1; a <= 1; a++) gv += bw[b + 1] * bw[a + 1] * cv[row + clampi(i + a, 0, W - 1)].w;
    }
    const float grad1 = guide_depth_gradient(guides, 1, i, j, W, H), grad2 = guide_depth_gradient(guides, 3, i, j, W, H);
    const float yp = luminance(cp);
    const float l_den = P.sigma_l * sqrtf(gv > 0.0f ? gv : 0.0f) + 1e-6f;
    const bool n1p_zero = zero3(g1p), n2p_zero = zero3(g2p);
    const float n1p_len = sqrtf(g1p.x * g1p.x + g1p.y * g1p.y + g1p.z * g1p.z), n2p_len = sqrtf(g2p.x * g2p.x + g2p.y * g2p.y + g2p.z * g2p.z);
    const float h[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f;
    for (int dy = -2; dy <= 2; dy++) {
        const int qj = j + step * dy;
        if (qj < 0 || qj >= H) continue;
        for (int dx = -2; dx <= 2; dx++) {
            const int qi = i + step * dx;
            if (qi < 0 || qi >= W) continue;
            const size_t q = size_t(qj) * W + qi;
            const float4 cq = cv[q];
            const float hit1_q = guides[q * 4].w;
            const float4 g1q = guides[q * 4 + 1], aq = guides[q * 4 + 2], g2q = guides[q * 4 + 3];
            const float wl = __expf(-fabsf(yp - luminance(cq)) / l_den);
            const float wn1 = normal_weight(g1p, n1p_zero, n1p_len, g1q, P.sigma_n), wn2 = normal_weight(g2p, n2p_zero, n2p_len, g2q, P.sigma_n);
            const float wn = wn1 < wn2 ? wn1 : wn2;
            const float o = float(step) * sqrtf(float(dx * dx + dy * dy));
            const float wz1 = depth_weight(hit1_p, hit1_q, g1p.w, g1q.w, grad1, o, P.sigma_z), wz2 = depth_weight(ap.w, aq.w, g2p.w, g2q.w, grad2, o, P.sigma_z);
            const float wz = wz1 < wz2 ? wz1 : wz2;
            float wa = 1.0f;
            if constexpr (!DEMOD) {
                const float ex = ap.x - aq.x, ey = ap.y - aq.y, ez = ap.z - aq.z;
                wa = __expf(-sqrtf(ex * ex + ey * ey + ez * ez) / P.sigma_a);
            }
            const float w = h[dx + 2] * h[dy + 2] * wl * wn * wz * wa;
            sw += w;
            sr += w * cq.x;
            sg += w * cq.y;
            sb += w * cq.z;
            sv += w * w * cq.w;
        }
    }
    float r = sr / sw, g = sg / sw, b = sb / sw;
    if (out_cv) {
        out_cv[px] = make_float4(r, g, b, sv / (sw * sw));
        return;
    }
    if constexpr (DEMOD) {
        const float4 A = demodulation_albedo(ap);
        r *= A.x;
        g *= A.y;
        b *= A.z;
    }
    if (out_linear) {
        out_linear[px * 3] = real(r);
        out_linear[px * 3 + 1] = real(g);
        out_linear[px * 3 + 2] = real(b);
    }
    if (out_rgb8) {
        out_rgb8[px * 3] = to_byte(double(r));
        out_rgb8[px * 3 + 1] = to_byte(double(g));
        out_rgb8[px * 3 + 2] = to_byte(double(b));
    }
}

template <typename real, bool DEMOD>
hipError_t launch_denoise_guided(const DenoiseParams& P, int iterations, const void* linear, const float* noise, const float4* guides, float4* ping, float4* pong,
                                 void* out_linear, uint8_t* out_rgb8, hipStream_t stream) {
    const dim3 grid((P.grid.n_tiles + 3) / 4), block(256);
    rtk_denoise_guided_pack_kernel<real, DEMOD><<<grid, block, 0, stream>>>(P, static_cast<const real*>(linear), noise, guides, ping);
    hipError_t e = hipGetLastError();
    for (int k = 0; k < iterations && e == hipSuccess; k++) {
        const bool last = k == iterations - 1;
        rtk_denoise_guided_step_kernel<real, DEMOD><<<grid, block, 0, stream>>>(P, 1 << k, ping, guides, last ? nullptr : pong,
                                                                                last ? static_cast<real*>(out_linear) : nullptr, last ? out_rgb8 : nullptr);
        e = hipGetLastError();
        float4* t = ping;
        ping = pong;
        pong = t;
    }
    return e;
}

// The options with defaults for 0 fields; false (and the reason in g_error) when they are out of range.
bool resolve_opts(const rtk_denoise_opts* in, int& iterations, DenoiseParams& P, const char* who) {
    rtk_denoise_opts o{};
    if (in) o = *in;
    iterations = o.iterations == 0 ? 5 : o.iterations;
    if (iterations < 1 || iterations > 8) {
        fail(RTK_ERR_INVALID, "%s: iterations %d out of range (1..8, 0 = 5)", who, o.iterations);
        return false;
    }
    const float s[4] = {o.sigma_l, o.sigma_n, o.sigma_z, o.sigma_a};
    for (float v : s)
        if (!(v >= 0.0f) || v > 3.0e38f) {
            fail(RTK_ERR_INVALID, "%s: sigmas must be finite and >= 0 (0 = default)", who);
            return false;
        }
    if (o.reserved != 0) {
        fail(RTK_ERR_INVALID, "%s: reserved must be 0", who);
        return false;
    }
    P.sigma_l = o.sigma_l == 0.0f ? 4.0f : o.sigma_l;
    P.sigma_n = o.sigma_n == 0.0f ? 128.0f : o.sigma_n;
    P.sigma_z = o.sigma_z == 0.0f ? 1.0f : o.sigma_z;
    P.sigma_a = o.sigma_a == 0.0f ? 0.1f : o.sigma_a;
    return true;
}

}  // namespace

int check_denoise_opts(const rtk_denoise_opts* opts, const char* who) {
    DenoiseParams P{};
    int iterations = 0;
    return resolve_opts(opts, iterations, P, who) ? RTK_OK : RTK_ERR_INVALID;
}

int resolve_guide_opts(const rtk_guide_opts* gopts, int* follow, int* max_bounces, const char* who) {
    rtk_guide_opts o{};
    if (gopts) o = *gopts;
    if (o.follow & ~(RTK_GUIDE_FOLLOW_MIRROR | RTK_GUIDE_FOLLOW_DIELECTRIC)) return fail(RTK_ERR_INVALID, "%s: unknown follow bits 0x%x", who, unsigned(o.follow));
    if (o.max_bounces < 0 || o.max_bounces > 8) return fail(RTK_ERR_INVALID, "%s: max_bounces %d out of range (1..8, 0 = 4)", who, o.max_bounces);
    *follow = o.follow == 0 ? RTK_GUIDE_FOLLOW_MIRROR : o.follow;
    *max_bounces = o.max_bounces == 0 ? 4 : o.max_bounces;
    return RTK_OK;
}

int check_denoise_flags(int32_t flags, const char* who) {
    if (flags & ~RTK_DENOISE_DEMODULATE) return fail(RTK_ERR_INVALID, "%s: unknown flags 0x%x", who, unsigned(flags));
    return RTK_OK;
}

}  // namespace rtk

using namespace rtk;

extern "C" {

int rtk_render_aovs(rtk_ctx* ctx, const rtk_camera* cam, const rtk_render_opts* opts, int32_t n_samples, float* d_aov) {
    if (!ctx || !cam || !opts) return fail(RTK_ERR_INVALID, "rtk_render_aovs: null argument");
    uint64_t digest = 0;
    if (!ctx_scene(ctx, &digest)) return fail(RTK_ERR_NO_SCENE, "rtk_render_aovs: no scene uploaded");
    if (check_camera_size("rtk_render_aovs", *cam) != RTK_OK) return RTK_ERR_INVALID;
    if (opts->n_ranks != 1) return fail(RTK_ERR_INVALID, "rtk_render_aovs: whole images only (n_ranks must be 1, not %d)", opts->n_ranks);
    if (check_real_mode("rtk_render_aovs", opts->real_mode) != RTK_OK) return RTK_ERR_INVALID;
    if (n_samples <= 0) return fail(RTK_ERR_INVALID, "rtk_render_aovs: n_samples must be positive (%d)", n_samples);
    if (!d_aov) return fail(RTK_ERR_INVALID, "rtk_render_aovs: null output buffer");
    if (check_aligned16(d_aov, "rtk_render_aovs", "d_aov") != RTK_OK) return RTK_ERR_INVALID;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    const hipStream_t st = static_cast<hipStream_t>(opts->stream);
    const hipError_t e = opts->real_mode == RTK_REAL_F64 ? launch_aov<double>(ctx_view<double>(ctx), device_camera<double>(*cam), opts->seed, n_samples, d_aov, st)
                                                         : launch_aov<float>(ctx_view<float>(ctx), device_camera<float>(*cam), opts->seed, n_samples, d_aov, st);
    if (e != hipSuccess) return fail(RTK_ERR_HIP, "rtk_render_aovs: %s", hipGetErrorString(e));
    return RTK_OK;
}

int rtk_render_aovs_host(rtk_ctx* ctx, const rtk_camera* cam, const rtk_render_opts* opts, int32_t n_samples, float* h_aov) {
    if (!ctx || !cam || !opts) return fail(RTK_ERR_INVALID, "rtk_render_aovs_host: null argument");
    if (!h_aov) return fail(RTK_ERR_INVALID, "rtk_render_aovs_host: null output buffer");
    if (check_camera_size("rtk_render_aovs_host", *cam) != RTK_OK) return RTK_ERR_INVALID;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    HostStaging s(false);
    const int aov = s.piece(size_t(cam->image_width) * cam->image_height * 8 * sizeof(float));
    RTK_HIP(s.alloc());
    const int rc = rtk_render_aovs(ctx, cam, opts, n_samples, s.ptr<float>(aov));
    if (rc != RTK_OK) return rc;
    hipError_t e = hipStreamSynchronize(static_cast<hipStream_t>(opts->stream));
    if (e == hipSuccess) e = s.download(aov, h_aov);
    if (e != hipSuccess) return fail(RTK_ERR_HIP, "rtk_render_aovs_host: %s", hipGetErrorString(e));
    return RTK_OK;
}

int rtk_denoise(rtk_ctx* ctx, int32_t width, int32_t height, int32_t real_mode, const void* d_linear, const float* d_aov, const float* d_noise,
                const rtk_denoise_opts* opts, void* d_out_linear, uint8_t* d_out_rgb8, void* stream) {
    if (!ctx) return fail(RTK_ERR_INVALID, "rtk_denoise: null context");
    if (check_image_size("rtk_denoise", width, height) != RTK_OK || check_real_mode("rtk_denoise", real_mode) != RTK_OK) return RTK_ERR_INVALID;
    if (!d_linear || !d_aov || !d_noise) return fail(RTK_ERR_INVALID, "rtk_denoise: d_linear, d_aov and d_noise are required");
    if (check_aligned16(d_aov, "rtk_denoise", "d_aov") != RTK_OK) return RTK_ERR_INVALID;
    if (!d_out_linear && !d_out_rgb8) return fail(RTK_ERR_INVALID, "rtk_denoise: no output");
    DenoiseParams P{};
    int iterations = 0;
    if (!resolve_opts(opts, iterations, P, "rtk_denoise")) return RTK_ERR_INVALID;
    P.grid = tile_grid(width, height);
    hipError_t e = hipSetDevice(ctx_device(ctx));
    void* ws = nullptr;
    const size_t plane = size_t(width) * height * sizeof(float4);
    if (e == hipSuccess) e = denoise_workspace(ctx, 2 * plane, &ws);
    if (e == hipSuccess) {
        float4* ping = static_cast<float4*>(ws);
        float4* pong = reinterpret_cast<float4*>(static_cast<char*>(ws) + plane);
        const auto* aov = reinterpret_cast<const float4*>(d_aov);
        const hipStream_t st = static_cast<hipStream_t>(stream);
        e = real_mode == RTK_REAL_F64 ? launch_denoise<double>(P, iterations, d_linear, d_noise, aov, ping, pong, d_out_linear, d_out_rgb8, st)
                                      : launch_denoise<float>(P, iterations, d_linear, d_noise, aov, ping, pong, d_out_linear, d_out_rgb8, st);
    }
    if (e != hipSuccess) return fail(RTK_ERR_HIP, "rtk_denoise: %s", hipGetErrorString(e));
    return RTK_OK;
}

// Argument checks of rtk_render_guides / _host that need no device (options first: they need no context either).
static int check_guide_args(const char* who, rtk_ctx* ctx, const rtk_camera* cam, const rtk_render_opts* opts, int32_t n_samples, const rtk_guide_opts* gopts,
                            const float* out, int* follow, int* max_bounces) {
    int rc = resolve_guide_opts(gopts, follow, max_bounces, who);
    if (rc != RTK_OK) return rc;
    if (n_samples <= 0 || n_samples > (1 << 20)) return fail(RTK_ERR_INVALID, "%s: n_samples must be 1 .. 2^20 (%d)", who, n_samples);
    if (!ctx || !cam || !opts) return fail(RTK_ERR_INVALID, "%s: null argument", who);
    if (!out) return fail(RTK_ERR_INVALID, "%s: null output buffer", who);
    if (check_camera_size(who, *cam) != RTK_OK) return RTK_ERR_INVALID;
    if (opts->n_ranks != 1) return fail(RTK_ERR_INVALID, "%s: whole images only (n_ranks must be 1, not %d)", who, opts->n_ranks);
    return check_real_mode(who, opts->real_mode);
}

int rtk_render_guides(rtk_ctx* ctx, const rtk_camera* cam, const rtk_render_opts* opts, int32_t n_samples, const rtk_guide_opts* gopts, float* d_guides) {
    int follow = 0, max_bounces = 0;
    const int rc = check_guide_args("rtk_render_guides", ctx, cam, opts, n_samples, gopts, d_guides, &follow, &max_bounces);
    if (rc != RTK_OK) return rc;
    if (check_aligned16(d_guides, "rtk_render_guides", "d_guides") != RTK_OK) return RTK_ERR_INVALID;
    uint64_t digest = 0;
    if (!ctx_scene(ctx, &digest)) return fail(RTK_ERR_NO_SCENE, "rtk_render_guides: no scene uploaded");
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    const hipStream_t st = static_cast<hipStream_t>(opts->stream);
    const hipError_t e = opts->real_mode == RTK_REAL_F64
                             ? launch_guides<double>(ctx_view<double>(ctx), device_camera<double>(*cam), opts->seed, n_samples, follow, max_bounces, d_guides, st)
                             : launch_guides<float>(ctx_view<float>(ctx), device_camera<float>(*cam), opts->seed, n_samples, follow, max_bounces, d_guides, st);
    if (e != hipSuccess) return fail(RTK_ERR_HIP, "rtk_render_guides: %s", hipGetErrorString(e));
    return RTK_OK;
}

int rtk_render_guides_host(rtk_ctx* ctx, const rtk_camera* cam, const rtk_render_opts* opts, int32_t n_samples, const rtk_guide_opts* gopts, float* h_guides) {
    int follow = 0, max_bounces = 0;
    int rc = check_guide_args("rtk_render_guides_host", ctx, cam, opts, n_samples, gopts, h_guides, &follow, &max_bounces);
    if (rc != RTK_OK) return rc;
    uint64_t digest = 0;
    if (!ctx_scene(ctx, &digest)) return fail(RTK_ERR_NO_SCENE, "rtk_render_guides_host: no scene uploaded");
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    HostStaging s(false);
    const int guides = s.piece(size_t(cam->image_width) * cam->image_height * 16 * sizeof(float));
    RTK_HIP(s.alloc());
    rc = rtk_render_guides(ctx, cam, opts, n_samples, gopts, s.ptr<float>(guides));
    if (rc != RTK_OK) return rc;
    hipError_t e = hipStreamSynchronize(static_cast<hipStream_t>(opts->stream));
    if (e == hipSuccess) e = s.download(guides, h_guides);
    if (e != hipSuccess) return fail(RTK_ERR_HIP, "rtk_render_guides_host: %s", hipGetErrorString(e));
    return RTK_OK;
}

int rtk_denoise_guided(rtk_ctx* ctx, int32_t width, int32_t height, int32_t real_mode, const void* d_linear, const float* d_guides, const float* d_noise,
                       const rtk_denoise_opts* opts, int32_t flags, void* d_out_linear, uint8_t* d_out_rgb8, void* stream) {
    if (check_denoise_flags(flags, "rtk_denoise_guided") != RTK_OK) return RTK_ERR_INVALID;
    DenoiseParams P{};
    int iterations = 0;
    if (!resolve_opts(opts, iterations, P, "rtk_denoise_guided")) return RTK_ERR_INVALID;
    if (!ctx) return fail(RTK_ERR_INVALID, "rtk_denoise_guided: null context");
    if (check_image_size("rtk_denoise_guided", width, height) != RTK_OK || check_real_mode("rtk_denoise_guided", real_mode) != RTK_OK) return RTK_ERR_INVALID;
    if (!d_linear || !d_guides || !d_noise) return fail(RTK_ERR_INVALID, "rtk_denoise_guided: d_linear, d_guides and d_noise are required");
    if (check_aligned16(d_guides, "rtk_denoise_guided", "d_guides") != RTK_OK) return RTK_ERR_INVALID;
    if (!d_out_linear && !d_out_rgb8) return fail(RTK_ERR_INVALID, "rtk_denoise_guided: no output");
    P.grid = tile_grid(width, height);
    hipError_t e = hipSetDevice(ctx_device(ctx));
    void* ws = nullptr;
    const size_t plane = size_t(width) * height * sizeof(float4);
    if (e == hipSuccess) e = denoise_workspace(ctx, 2 * plane, &ws);
    if (e == hipSuccess) {
        float4* ping = static_cast<float4*>(ws);
        float4* pong = reinterpret_cast<float4*>(static_cast<char*>(ws) + plane);
        const auto* guides = reinterpret_cast<const float4*>(d_guides);
        const hipStream_t st = static_cast<hipStream_t>(stream);
        e = with_real_demod(real_mode == RTK_REAL_F64, (flags & RTK_DENOISE_DEMODULATE) != 0, [&](auto real, auto demod) {
            return launch_denoise_guided<decltype(real), decltype(demod)::value>(P, iterations, d_linear, d_noise, guides, ping, pong, d_out_linear, d_out_rgb8, st);
        });
    }
    if (e != hipSuccess) return fail(RTK_ERR_HIP, "rtk_denoise_guided: %s", hipGetErrorString(e));
    return RTK_OK;
}

// rtk_denoise_host (guide_floats 8) and rtk_denoise_guided_host (16): device copies of the inputs, the asynchronous entry point
// on the null stream, the outputs copied back.
static int denoise_host(const char* who, int guide_floats, int32_t flags, rtk_ctx* ctx, int32_t width, int32_t height, int32_t real_mode, const double* h_linear,
                        const float* h_aov, const float* h_noise, const rtk_denoise_opts* opts, double* h_out_linear, uint8_t* h_out_rgb8) {
    if (!ctx) return fail(RTK_ERR_INVALID, "%s: null context", who);
    if (check_image_size(who, width, height) != RTK_OK || check_real_mode(who, real_mode) != RTK_OK) return RTK_ERR_INVALID;
    if (!h_linear || !h_aov || !h_noise) return fail(RTK_ERR_INVALID, "%s: h_linear, %s and h_noise are required", who, guide_floats == 8 ? "h_aov" : "h_guides");
    if (!h_out_linear && !h_out_rgb8) return fail(RTK_ERR_INVALID, "%s: no output", who);
    {
        DenoiseParams P{};
        int it = 0;
        if (!resolve_opts(opts, it, P, who)) return RTK_ERR_INVALID;
    }
    hipError_t e = hipSetDevice(ctx_device(ctx));
    if (e != hipSuccess) return fail(RTK_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    const size_t px = size_t(width) * height;
    HostStaging s(real_mode == RTK_REAL_F64);
    const int lin = s.linear(px * 3), aov = s.piece(px * guide_floats * sizeof(float)), noise = s.piece(px * sizeof(float));
    const int out = s.linear(px * 3, h_out_linear != nullptr), rgb8 = s.piece(px * 3, h_out_rgb8 != nullptr);
    e = s.alloc();
    if (e == hipSuccess) e = s.upload_linear(lin, h_linear);
    if (e == hipSuccess) e = s.upload(aov, h_aov);
    if (e == hipSuccess) e = s.upload(noise, h_noise);
    if (e != hipSuccess) return fail(RTK_ERR_HIP, "%s: device buffers: %s", who, hipGetErrorString(e));
    const int rc = guide_floats == 8
                       ? rtk_denoise(ctx, width, height, real_mode, s.ptr(lin), s.ptr<float>(aov), s.ptr<float>(noise), opts, s.ptr(out), s.ptr<uint8_t>(rgb8), nullptr)
                       : rtk_denoise_guided(ctx, width, height, real_mode, s.ptr(lin), s.ptr<float>(aov), s.ptr<float>(noise), opts, flags, s.ptr(out),
                                            s.ptr<uint8_t>(rgb8), nullptr);
    if (rc != RTK_OK) return rc;
    e = hipStreamSynchronize(nullptr);
    if (e == hipSuccess) e = s.download_linear(out, h_out_linear);
    if (e == hipSuccess) e = s.download(rgb8, h_out_rgb8);
    if (e != hipSuccess) return fail(RTK_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    return RTK_OK;
}

int rtk_denoise_host(rtk_ctx* ctx, int32_t width, int32_t height, int32_t real_mode, const double* h_linear, const float* h_aov, const float* h_noise,
                     const rtk_denoise_opts* opts, double* h_out_linear, uint8_t* h_out_rgb8) {
    return denoise_host("rtk_denoise_host", 8, 0, ctx, width, height, real_mode, h_linear, h_aov, h_noise, opts, h_out_linear, h_out_rgb8);
}

int rtk_denoise_guided_host(rtk_ctx* ctx, int32_t width, int32_t height, int32_t real_mode, const double* h_linear, const float* h_guides,
                            const float* h_noise, const rtk_denoise_opts* opts, int32_t flags, double* h_out_linear, uint8_t* h_out_rgb8) {
    if (check_denoise_flags(flags, "rtk_denoise_guided_host") != RTK_OK || check_denoise_opts(opts, "rtk_denoise_guided_host") != RTK_OK) return RTK_ERR_INVALID;
    return denoise_host("rtk_denoise_guided_host", 16, flags, ctx, width, height, real_mode, h_linear, h_guides, h_noise, opts, h_out_linear, h_out_rgb8);
}

}  // extern "C"
