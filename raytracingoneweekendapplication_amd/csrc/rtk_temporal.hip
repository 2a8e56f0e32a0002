// rtk_temporal.hip -- temporal accumulation (include/rtk.h, "Temporal accumulation"): the reprojection half of SVGF (Schied et
// al. 2017) in front of the guided a-trous filter of rtk_denoise.hip.  One kernel per frame: reproject the pixel's first hit into
// the previous camera, gather the four history taps around it, reject those that belong to another surface, blend, and write the
// outputs and the next frame's history.  Hand-written HIP for gfx950, wave64.
//
// Layout.  The object owns two history sets (ping-pong); a set is four planes indexed by pixel: {r, g, b, var} float4,
// {normal, depth} float4 (guide float4 1 as it came), {seen albedo, first-hit fraction} float4 and n float.  A tap is three
// 16-byte loads and one 4-byte load.  One lane per pixel, one wave per 8x8 tile (the render's tile convention), four tiles per
// 256-thread block.  The taps of a wave cover a patch of about 9x9 history pixels, which the vector L1 / L2 serve; nothing is
// staged in LDS.  The kernel that reads set A writes set B, this frame's guides included: no second pass over the frame.
//
// Arithmetic.  The reprojection (about 40 flops) and the depth test run in double for both real modes; everything after the
// bilinear weights is float32, without atomics and in a fixed tap order (b outer, a inner): the same inputs give the same bits.
#include <hip/hip_runtime.h>

#include <cmath>

#include "rtk.h"
#include "rtk_image_pass.h"
#include "rtk_internal.h"

namespace rtk {
namespace {

struct TemporalParams {
    TileGrid grid;
    int have_prev;             // 0: every pixel starts a history
    int check_albedo;
    float max_history, depth_tol, normal_cos, albedo_tol;
    double center[3], p00[3], du[3], dv[3];  // this frame's camera
    double minv[9], pcenter[3];              // rtk_temporal_reproject_matrix of the previous frame's camera
};

struct History {
    float4* cv;   // {r, g, b, var}
    float4* nz;   // {normal, depth}
    float4* ah;   // {seen albedo, first-hit fraction}
    float* n;
};

template <typename real>
__global__ __launch_bounds__(256) void rtk_temporal_kernel(TemporalParams P, const real* linear, const float4* __restrict__ guides, const float* noise,
                                                            History prev, History next, real* out_linear, float* out_noise, uint8_t* __restrict__ out_rgb8,
                                                            float* __restrict__ out_history) {  // (out_linear / out_noise may be linear / noise: no __restrict__)
    int i, j;
    if (!lane_pixel(P.grid, i, j)) return;
    const int W = P.grid.width, H = P.grid.height;
    const size_t px = size_t(j) * W + i;
    const float4 g0 = guides[px * 4], g1 = guides[px * 4 + 1], g2 = guides[px * 4 + 2];  // {albedo, hit}, {normal, depth}, {seen albedo, end hit}
    const float cr = float(linear[px * 3]), cg = float(linear[px * 3 + 1]), cb = float(linear[px * 3 + 2]);
    const float se = noise[px];
    const float var_c = se * se;
    float r = cr, g = cg, b = cb, var = var_c, n = 1.0f;
    if (P.have_prev && g0.w != 0.0f) {
        const double fi = double(i), fj = double(j);
        const double dx = P.p00[0] + fi * P.du[0] + fj * P.dv[0] - P.center[0];
        const double dy = P.p00[1] + fi * P.du[1] + fj * P.dv[1] - P.center[1];
        const double dz = P.p00[2] + fi * P.du[2] + fj * P.dv[2] - P.center[2];
        const double s = double(g1.w) / __builtin_sqrt(dx * dx + dy * dy + dz * dz);
        const double qx = P.center[0] + s * dx - P.pcenter[0], qy = P.center[1] + s * dy - P.pcenter[1], qz = P.center[2] + s * dz - P.pcenter[2];
        const double u = P.minv[0] * qx + P.minv[1] * qy + P.minv[2] * qz;
        const double v = P.minv[3] * qx + P.minv[4] * qy + P.minv[5] * qz;
        const double w = P.minv[6] * qx + P.minv[7] * qy + P.minv[8] * qz;
        const double x = u / w, y = v / w;
        // the taps x0, x0 + 1 meet the image only for -1 <= x < W (a NaN fails the test)
        if (w > 0.0 && x >= -1.0 && x < double(W) && y >= -1.0 && y < double(H)) {
            const double z_exp = __builtin_sqrt(qx * qx + qy * qy + qz * qz), z_lim = double(P.depth_tol) * z_exp;
            const double xf = __builtin_floor(x), yf = __builtin_floor(y);
            const int x0 = int(xf), y0 = int(yf);
            const double fx = x - xf, fy = y - yf;
            const bool np_zero = zero3(g1);
            const float np_len = sqrtf(g1.x * g1.x + g1.y * g1.y + g1.z * g1.z);
            float so = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f, sn = 0.0f;
            for (int tb = 0; tb < 2; tb++) {
                const int tj = y0 + tb;
                if (tj < 0 || tj >= H) continue;
                for (int ta = 0; ta < 2; ta++) {
                    const int ti = x0 + ta;
                    if (ti < 0 || ti >= W) continue;
                    const size_t q = size_t(tj) * W + ti;
                    const float4 ahq = prev.ah[q], nzq = prev.nz[q];
                    if (!(ahq.w > 0.0f)) continue;
                    if (!(__builtin_fabs(double(nzq.w) - z_exp) <= z_lim)) continue;
                    const bool nq_zero = zero3(nzq);
                    if (np_zero || nq_zero) {
                        if (!(np_zero && nq_zero)) continue;
                    } else {
                        const float c = (g1.x * nzq.x + g1.y * nzq.y + g1.z * nzq.z) / (np_len * sqrtf(nzq.x * nzq.x + nzq.y * nzq.y + nzq.z * nzq.z));
                        if (!(c >= P.normal_cos)) continue;
                    }
                    if (P.check_albedo) {
                        const float ex = fabsf(g2.x - ahq.x), ey = fabsf(g2.y - ahq.y), ez = fabsf(g2.z - ahq.z);
                        const float m = ex > ey ? (ex > ez ? ex : ez) : (ey > ez ? ey : ez);
                        if (!(m <= P.albedo_tol)) continue;
                    }
                    const float om = float((ta ? fx : 1.0 - fx) * (tb ? fy : 1.0 - fy));
                    const float4 cq = prev.cv[q];
                    const float nq = prev.n[q];
                    so += om;
                    sr += om * cq.x;
                    sg += om * cq.y;
                    sb += om * cq.z;
                    sv += om * om * cq.w;
                    sn += om * nq;
                }
            }
            if (so >= 1e-3f) {
                const float nh = sn / so + 1.0f;
                n = nh < P.max_history ? nh : P.max_history;
                const float alpha = 1.0f / n, keep = 1.0f - alpha;
                r = keep * (sr / so) + alpha * cr;
                g = keep * (sg / so) + alpha * cg;
                b = keep * (sb / so) + alpha * cb;
                var = keep * keep * (sv / (so * so)) + alpha * alpha * var_c;
            }
        }
    }
    next.cv[px] = make_float4(r, g, b, var);
    next.nz[px] = g1;
    next.ah[px] = make_float4(g2.x, g2.y, g2.z, g0.w);
    next.n[px] = n;
    if (out_linear) {
        out_linear[px * 3] = real(r);
        out_linear[px * 3 + 1] = real(g);
        out_linear[px * 3 + 2] = real(b);
    }
    if (out_noise) out_noise[px] = sqrtf(var);
    if (out_history) out_history[px] = n;
    if (out_rgb8) {
        out_rgb8[px * 3] = to_byte(double(r));
        out_rgb8[px * 3 + 1] = to_byte(double(g));
        out_rgb8[px * 3 + 2] = to_byte(double(b));
    }
}

// The options with defaults for 0 fields, written into P; RTK_ERR_INVALID (reason in g_error) when they are out of range.
int resolve_temporal_opts(const rtk_temporal_opts* in, TemporalParams& P, const char* who) {
    rtk_temporal_opts o{};
    if (in) o = *in;
    if (o.flags & ~RTK_TEMPORAL_CHECK_ALBEDO) return fail(RTK_ERR_INVALID, "%s: unknown flags 0x%x", who, unsigned(o.flags));
    if (o.reserved != 0) return fail(RTK_ERR_INVALID, "%s: reserved must be 0", who);
    if (o.max_history < 0 || o.max_history > 1024) return fail(RTK_ERR_INVALID, "%s: max_history %d out of range (1..1024, 0 = 32)", who, o.max_history);
    const float tol[3] = {o.depth_tol, o.normal_cos, o.albedo_tol};
    for (float v : tol)
        if (!(v >= 0.0f) || v > 3.0e38f) return fail(RTK_ERR_INVALID, "%s: tolerances must be finite and >= 0 (0 = default)", who);
    if (o.normal_cos > 1.0f) return fail(RTK_ERR_INVALID, "%s: normal_cos %g is no cosine (<= 1)", who, double(o.normal_cos));
    P.max_history = float(o.max_history == 0 ? 32 : o.max_history);
    P.depth_tol = o.depth_tol == 0.0f ? 0.02f : o.depth_tol;
    P.normal_cos = o.normal_cos == 0.0f ? 0.9f : o.normal_cos;
    P.albedo_tol = o.albedo_tol == 0.0f ? 0.25f : o.albedo_tol;
    P.check_albedo = (o.flags & RTK_TEMPORAL_CHECK_ALBEDO) != 0;
    return RTK_OK;
}

}  // namespace
}  // namespace rtk

using namespace rtk;

struct rtk_temporal {
    rtk_ctx* ctx = nullptr;
    int device = 0;
    int width = 0, height = 0, real_mode = 0;
    hipStream_t stream = nullptr;
    void* memory = nullptr;     // both history sets, one allocation
    History set[2]{};
    int current = 0;            // the set the last frame wrote
    int frames = 0;             // since create / reset; 0: the next frame starts a history
    double prev[12]{};          // rtk_temporal_reproject_matrix of the last frame's camera
};

extern "C" {

int rtk_temporal_reproject_matrix(const rtk_camera* cam, double out[12]) {
    if (!cam || !out) return fail(RTK_ERR_INVALID, "rtk_temporal_reproject_matrix: null argument");
    const rtk_vec3 &a = cam->pixel_delta_u, &b = cam->pixel_delta_v, &o = cam->center;
    const double c[3] = {cam->pixel00_loc.x - o.x, cam->pixel00_loc.y - o.y, cam->pixel00_loc.z - o.z};
    // rows of the inverse = the cross products of the columns, over the determinant
    const double r0[3] = {b.y * c[2] - b.z * c[1], b.z * c[0] - b.x * c[2], b.x * c[1] - b.y * c[0]};
    const double r1[3] = {c[1] * a.z - c[2] * a.y, c[2] * a.x - c[0] * a.z, c[0] * a.y - c[1] * a.x};
    const double r2[3] = {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
    const double det = a.x * r0[0] + a.y * r0[1] + a.z * r0[2];
    const double scale = std::sqrt(a.x * a.x + a.y * a.y + a.z * a.z) * std::sqrt(b.x * b.x + b.y * b.y + b.z * b.z) * std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    if (!std::isfinite(det) || !std::isfinite(scale) || !(std::fabs(det) > 1e-12 * scale))
        return fail(RTK_ERR_INVALID, "rtk_temporal_reproject_matrix: singular camera (pixel_delta_u, pixel_delta_v and pixel00_loc - center do not span space)");
    for (int k = 0; k < 3; k++) {
        out[k] = r0[k] / det;
        out[3 + k] = r1[k] / det;
        out[6 + k] = r2[k] / det;
    }
    out[9] = o.x;
    out[10] = o.y;
    out[11] = o.z;
    return RTK_OK;
}

int rtk_temporal_create(rtk_ctx* ctx, int32_t width, int32_t height, int32_t real_mode, void* stream, rtk_temporal** out) {
    if (!ctx || !out) return fail(RTK_ERR_INVALID, "rtk_temporal_create: null argument");
    if (check_image_size("rtk_temporal_create", width, height) != RTK_OK || check_real_mode("rtk_temporal_create", real_mode) != RTK_OK) return RTK_ERR_INVALID;
    hipError_t e = hipSetDevice(ctx_device(ctx));
    if (e != hipSuccess) return fail(RTK_ERR_HIP, "rtk_temporal_create: %s", hipGetErrorString(e));
    const size_t px = size_t(width) * height, set_bytes = px * (3 * sizeof(float4) + sizeof(float));
    void* mem = nullptr;
    e = hipMalloc(&mem, 2 * set_bytes);
    if (e != hipSuccess) return fail(RTK_ERR_HIP, "rtk_temporal_create: history of %zu bytes: %s", 2 * set_bytes, hipGetErrorString(e));
    rtk_temporal* t = new rtk_temporal;
    t->ctx = ctx;
    t->device = ctx_device(ctx);
    t->width = width;
    t->height = height;
    t->real_mode = real_mode;
    t->stream = static_cast<hipStream_t>(stream);
    t->memory = mem;
    for (int k = 0; k < 2; k++) {  // the float4 planes first: the allocation is 256-byte aligned and px * 16 keeps 16
        char* base = static_cast<char*>(mem) + k * set_bytes;
        t->set[k].cv = reinterpret_cast<float4*>(base);
        t->set[k].nz = reinterpret_cast<float4*>(base + px * sizeof(float4));
        t->set[k].ah = reinterpret_cast<float4*>(base + 2 * px * sizeof(float4));
        t->set[k].n = reinterpret_cast<float*>(base + 3 * px * sizeof(float4));
    }
    *out = t;
    return RTK_OK;
}

int rtk_temporal_accumulate(rtk_temporal* t, const rtk_camera* cam, const void* d_linear, const float* d_guides, const float* d_noise,
                            const rtk_temporal_opts* opts, void* d_out_linear, float* d_out_noise, uint8_t* d_out_rgb8, float* d_out_history) {
    const char* who = "rtk_temporal_accumulate";
    TemporalParams P{};
    if (resolve_temporal_opts(opts, P, who) != RTK_OK) return RTK_ERR_INVALID;
    if (!t) return fail(RTK_ERR_INVALID, "%s: null object", who);
    if (!cam) return fail(RTK_ERR_INVALID, "%s: null camera", who);
    if (!d_linear || !d_guides || !d_noise) return fail(RTK_ERR_INVALID, "%s: d_linear, d_guides and d_noise are required", who);
    if (check_aligned16(d_guides, who, "d_guides") != RTK_OK) return RTK_ERR_INVALID;
    if (cam->image_width != t->width || cam->image_height != t->height)
        return fail(RTK_ERR_INVALID, "%s: the camera's image is %dx%d, the object's %dx%d", who, cam->image_width, cam->image_height, t->width, t->height);
    double now[12];
    if (rtk_temporal_reproject_matrix(cam, now) != RTK_OK) return RTK_ERR_INVALID;
    P.grid = tile_grid(t->width, t->height);
    P.have_prev = t->frames > 0;
    const rtk_vec3* v[4] = {&cam->center, &cam->pixel00_loc, &cam->pixel_delta_u, &cam->pixel_delta_v};
    double* dst[4] = {P.center, P.p00, P.du, P.dv};
    for (int k = 0; k < 4; k++) {
        dst[k][0] = v[k]->x;
        dst[k][1] = v[k]->y;
        dst[k][2] = v[k]->z;
    }
    for (int k = 0; k < 9; k++) P.minv[k] = t->prev[k];
    for (int k = 0; k < 3; k++) P.pcenter[k] = t->prev[9 + k];
    hipError_t e = hipSetDevice(t->device);
    if (e == hipSuccess) {
        const History prev = t->set[t->current], next = t->set[t->current ^ 1];
        const dim3 grid((P.grid.n_tiles + 3) / 4), block(256);
        const auto* guides = reinterpret_cast<const float4*>(d_guides);
        if (t->real_mode == RTK_REAL_F64)
            rtk_temporal_kernel<double><<<grid, block, 0, t->stream>>>(P, static_cast<const double*>(d_linear), guides, d_noise, prev, next,
                                                                       static_cast<double*>(d_out_linear), d_out_noise, d_out_rgb8, d_out_history);
        else
            rtk_temporal_kernel<float><<<grid, block, 0, t->stream>>>(P, static_cast<const float*>(d_linear), guides, d_noise, prev, next,
                                                                      static_cast<float*>(d_out_linear), d_out_noise, d_out_rgb8, d_out_history);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return fail(RTK_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    t->current ^= 1;
    t->frames++;
    for (int k = 0; k < 12; k++) t->prev[k] = now[k];
    return RTK_OK;
}

int rtk_temporal_accumulate_host(rtk_temporal* t, const rtk_camera* cam, const double* h_linear, const float* h_guides, const float* h_noise,
                                 const rtk_temporal_opts* opts, double* h_out_linear, float* h_out_noise, uint8_t* h_out_rgb8, float* h_out_history) {
    const char* who = "rtk_temporal_accumulate_host";
    {
        TemporalParams P{};
        if (resolve_temporal_opts(opts, P, who) != RTK_OK) return RTK_ERR_INVALID;
    }
    if (!t) return fail(RTK_ERR_INVALID, "%s: null object", who);
    if (!cam) return fail(RTK_ERR_INVALID, "%s: null camera", who);
    if (!h_linear || !h_guides || !h_noise) return fail(RTK_ERR_INVALID, "%s: h_linear, h_guides and h_noise are required", who);
    if (cam->image_width != t->width || cam->image_height != t->height)
        return fail(RTK_ERR_INVALID, "%s: the camera's image is %dx%d, the object's %dx%d", who, cam->image_width, cam->image_height, t->width, t->height);
    hipError_t e = hipSetDevice(t->device);
    if (e != hipSuccess) return fail(RTK_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    const size_t px = size_t(t->width) * t->height;
    HostStaging s(t->real_mode == RTK_REAL_F64);
    // linear and noise are in, then out in place
    const int lin = s.linear(px * 3), guides = s.piece(px * 16 * sizeof(float)), noise = s.piece(px * sizeof(float));
    const int hist = s.piece(px * sizeof(float), h_out_history != nullptr), rgb8 = s.piece(px * 3, h_out_rgb8 != nullptr);
    e = s.alloc();
    if (e == hipSuccess) e = s.upload_linear(lin, h_linear);
    if (e == hipSuccess) e = s.upload(guides, h_guides);
    if (e == hipSuccess) e = s.upload(noise, h_noise);
    if (e != hipSuccess) return fail(RTK_ERR_HIP, "%s: device buffers: %s", who, hipGetErrorString(e));
    const int rc = rtk_temporal_accumulate(t, cam, s.ptr(lin), s.ptr<float>(guides), s.ptr<float>(noise), opts, h_out_linear ? s.ptr(lin) : nullptr,
                                           h_out_noise ? s.ptr<float>(noise) : nullptr, s.ptr<uint8_t>(rgb8), s.ptr<float>(hist));
    if (rc != RTK_OK) return rc;
    e = hipStreamSynchronize(t->stream);
    if (e == hipSuccess) e = s.download_linear(lin, h_out_linear);
    if (e == hipSuccess) e = s.download(noise, h_out_noise);
    if (e == hipSuccess) e = s.download(hist, h_out_history);
    if (e == hipSuccess) e = s.download(rgb8, h_out_rgb8);
    if (e != hipSuccess) return fail(RTK_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    return RTK_OK;
}

int rtk_temporal_reset(rtk_temporal* t) {
    if (!t) return fail(RTK_ERR_INVALID, "rtk_temporal_reset: null object");
    t->frames = 0;  // the next frame's kernel is told to read no history: nothing to enqueue
    return RTK_OK;
}

int rtk_temporal_frames(const rtk_temporal* t) {
    if (!t) return fail(RTK_ERR_INVALID, "rtk_temporal_frames: null object");
    return t->frames;
}

int rtk_temporal_destroy(rtk_temporal* t) {
    if (!t) return RTK_OK;
    hipError_t e = hipSetDevice(t->device);
    if (e == hipSuccess) e = hipStreamSynchronize(t->stream);  // the last frame may still read and write the history
    (void)hipFree(t->memory);
    delete t;
    if (e != hipSuccess) return fail(RTK_ERR_HIP, "rtk_temporal_destroy: %s", hipGetErrorString(e));
    return RTK_OK;
}

}  // extern "C"
