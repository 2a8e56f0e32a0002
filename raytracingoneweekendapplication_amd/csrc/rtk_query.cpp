// rtk_query.cpp -- the C-ABI half of the ray queries (include/rtk.h "Ray queries"): argument checks that need no device, the
// launches on the caller's stream, and the blocking _host forms.  The kernels are rtk_trace.hip's, next to the device functions
// they share with the render, known-answer, AOV and guide kernels.
#include <hip/hip_runtime.h>

#include "rtk.h"
#include "rtk_internal.h"
#include "rtk_trace.h"

#define RTK_HIP(call)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess) return fail(RTK_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

namespace rtk {
namespace {

static_assert(sizeof(rtk_ray) == 88 && sizeof(rtk_ray_hit) == 96 && sizeof(rtk_query_opts) == 56, "ray query records");

int check_aligned(const void* p, size_t align, const char* who, const char* arg) {
    return (reinterpret_cast<uintptr_t>(p) & (align - 1)) == 0 ? RTK_OK : fail(RTK_ERR_INVALID, "%s: %s must be %zu-byte aligned", who, arg, align);
}

// include/rtk.h: outputs may not alias d_rays.  RTK_OK, or RTK_ERR_INVALID naming the output whose n elements of `bytes` each
// share an address with the n ray records (a null output overlaps nothing).
int check_apart(const void* rays, const void* out, int64_t n, size_t bytes, const char* who, const char* arg) {
    const uintptr_t r = reinterpret_cast<uintptr_t>(rays), o = reinterpret_cast<uintptr_t>(out);
    const bool apart = !out || n == 0 || o + uintptr_t(n) * bytes <= r || r + uintptr_t(n) * sizeof(rtk_ray) <= o;
    return apart ? RTK_OK : fail(RTK_ERR_INVALID, "%s: %s overlaps d_rays", who, arg);
}

// What every query checks before it touches a device: the arguments the three have in common.  The context comes last, so
// that every other refusal can be had -- and tested -- where there is no device to make a context on.
int check_query_args(const char* who, const rtk_query_opts* opts, int64_t n, const void* rays, const char* rays_name, const void* out, const char* out_name) {
    if (!opts) return fail(RTK_ERR_INVALID, "%s: null opts", who);
    if (n < 0 || n > int64_t(0x7FFFFFFF)) return fail(RTK_ERR_INVALID, "%s: n must be 0 .. 2^31 - 1 (%lld)", who, (long long)n);
    if (check_real_mode(who, opts->real_mode) != RTK_OK) return RTK_ERR_INVALID;
    if (opts->max_depth < 0) return fail(RTK_ERR_INVALID, "%s: max_depth must not be negative (%d)", who, opts->max_depth);
    if (opts->samples < 0) return fail(RTK_ERR_INVALID, "%s: samples must not be negative (%d)", who, opts->samples);
    if (opts->reserved[0] != 0 || opts->reserved[1] != 0) return fail(RTK_ERR_INVALID, "%s: reserved must be 0", who);
    if (!rays) return fail(RTK_ERR_INVALID, "%s: null %s", who, rays_name);
    if (!out) return fail(RTK_ERR_INVALID, "%s: null %s", who, out_name);
    return RTK_OK;
}

// ... then the context and its scene.
int check_ctx(const char* who, const rtk_ctx* ctx) {
    if (!ctx) return fail(RTK_ERR_INVALID, "%s: null context", who);
    uint64_t digest = 0;
    return ctx_scene(ctx, &digest) ? RTK_OK : fail(RTK_ERR_NO_SCENE, "%s: no scene uploaded", who);
}

int launched(const char* who, hipError_t e) { return e == hipSuccess ? RTK_OK : fail(RTK_ERR_HIP, "%s: %s", who, hipGetErrorString(e)); }

}  // namespace
}  // namespace rtk

using namespace rtk;

extern "C" {

int rtk_query_hits(rtk_ctx* ctx, const rtk_query_opts* opts, int64_t n, const rtk_ray* d_rays, rtk_ray_hit* d_hits) {
    const char* who = "rtk_query_hits";
    if (check_query_args(who, opts, n, d_rays, "d_rays", d_hits, "d_hits") != RTK_OK) return RTK_ERR_INVALID;
    if (check_aligned(d_rays, 8, who, "d_rays") != RTK_OK || check_aligned(d_hits, 8, who, "d_hits") != RTK_OK) return RTK_ERR_INVALID;
    if (check_apart(d_rays, d_hits, n, sizeof(rtk_ray_hit), who, "d_hits") != RTK_OK) return RTK_ERR_INVALID;
    const int rc = check_ctx(who, ctx);
    if (rc != RTK_OK || n == 0) return rc;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    const hipStream_t st = static_cast<hipStream_t>(opts->stream);
    return launched(who, opts->real_mode == RTK_REAL_F64 ? launch_query_hits<double>(ctx_view<double>(ctx), opts->seed, n, d_rays, d_hits, st)
                                                         : launch_query_hits<float>(ctx_view<float>(ctx), opts->seed, n, d_rays, d_hits, st));
}

int rtk_query_occluded(rtk_ctx* ctx, const rtk_query_opts* opts, int64_t n, const rtk_ray* d_rays, int32_t* d_occluded) {
    const char* who = "rtk_query_occluded";
    if (check_query_args(who, opts, n, d_rays, "d_rays", d_occluded, "d_occluded") != RTK_OK) return RTK_ERR_INVALID;
    if (check_aligned(d_rays, 8, who, "d_rays") != RTK_OK || check_aligned(d_occluded, 4, who, "d_occluded") != RTK_OK) return RTK_ERR_INVALID;
    if (check_apart(d_rays, d_occluded, n, sizeof(int32_t), who, "d_occluded") != RTK_OK) return RTK_ERR_INVALID;
    const int rc = check_ctx(who, ctx);
    if (rc != RTK_OK || n == 0) return rc;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    const hipStream_t st = static_cast<hipStream_t>(opts->stream);
    const bool any_hit = (ctx_features(ctx) & F_MEDIA) == 0;  // no constant_medium: the first accepted hit settles the flag
    return launched(who, opts->real_mode == RTK_REAL_F64 ? launch_query_occluded<double>(ctx_view<double>(ctx), opts->seed, any_hit, n, d_rays, d_occluded, st)
                                                         : launch_query_occluded<float>(ctx_view<float>(ctx), opts->seed, any_hit, n, d_rays, d_occluded, st));
}

int rtk_query_radiance(rtk_ctx* ctx, const rtk_query_opts* opts, int64_t n, const rtk_ray* d_rays, void* d_radiance, uint32_t* d_draws) {
    const char* who = "rtk_query_radiance";
    if (check_query_args(who, opts, n, d_rays, "d_rays", d_radiance, "d_radiance") != RTK_OK) return RTK_ERR_INVALID;
    const size_t real_bytes = opts->real_mode == RTK_REAL_F64 ? sizeof(double) : sizeof(float);
    if (check_aligned(d_rays, 8, who, "d_rays") != RTK_OK || check_aligned(d_radiance, real_bytes, who, "d_radiance") != RTK_OK ||
        check_aligned(d_draws, 4, who, "d_draws") != RTK_OK)
        return RTK_ERR_INVALID;
    if (check_apart(d_rays, d_radiance, n, 3 * real_bytes, who, "d_radiance") != RTK_OK || check_apart(d_rays, d_draws, n, sizeof(uint32_t), who, "d_draws") != RTK_OK)
        return RTK_ERR_INVALID;
    const int rc = check_ctx(who, ctx);
    if (rc != RTK_OK || n == 0) return rc;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    const hipStream_t st = static_cast<hipStream_t>(opts->stream);
    rtk_camera cam{};  // what the kernel reads of a camera: ray_color's background, max_depth and the samples per ray
    cam.background = opts->background;
    cam.max_depth = opts->max_depth;
    cam.samples_per_pixel = opts->samples > 0 ? opts->samples : 1;
    return launched(who, opts->real_mode == RTK_REAL_F64
                             ? launch_query_radiance<double>(ctx_view<double>(ctx), device_camera<double>(cam), opts->seed, n, d_rays, d_radiance, d_draws, st)
                             : launch_query_radiance<float>(ctx_view<float>(ctx), device_camera<float>(cam), opts->seed, n, d_rays, d_radiance, d_draws, st));
}

int rtk_query_hits_host(rtk_ctx* ctx, const rtk_query_opts* opts, int64_t n, const rtk_ray* h_rays, rtk_ray_hit* h_hits) {
    const char* who = "rtk_query_hits_host";
    if (check_query_args(who, opts, n, h_rays, "h_rays", h_hits, "h_hits") != RTK_OK) return RTK_ERR_INVALID;
    const int rc = check_ctx(who, ctx);
    if (rc != RTK_OK || n == 0) return rc;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    HostStaging s(true);
    const int rays = s.piece(size_t(n) * sizeof(rtk_ray)), hits = s.piece(size_t(n) * sizeof(rtk_ray_hit));
    RTK_HIP(s.alloc());
    RTK_HIP(s.upload(rays, h_rays));
    const int q = rtk_query_hits(ctx, opts, n, s.ptr<rtk_ray>(rays), s.ptr<rtk_ray_hit>(hits));
    if (q != RTK_OK) return q;
    hipError_t e = hipStreamSynchronize(static_cast<hipStream_t>(opts->stream));
    if (e == hipSuccess) e = s.download(hits, h_hits);
    return launched(who, e);
}

int rtk_query_occluded_host(rtk_ctx* ctx, const rtk_query_opts* opts, int64_t n, const rtk_ray* h_rays, int32_t* h_occluded) {
    const char* who = "rtk_query_occluded_host";
    if (check_query_args(who, opts, n, h_rays, "h_rays", h_occluded, "h_occluded") != RTK_OK) return RTK_ERR_INVALID;
    const int rc = check_ctx(who, ctx);
    if (rc != RTK_OK || n == 0) return rc;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    HostStaging s(true);
    const int rays = s.piece(size_t(n) * sizeof(rtk_ray)), occ = s.piece(size_t(n) * sizeof(int32_t));
    RTK_HIP(s.alloc());
    RTK_HIP(s.upload(rays, h_rays));
    const int q = rtk_query_occluded(ctx, opts, n, s.ptr<rtk_ray>(rays), s.ptr<int32_t>(occ));
    if (q != RTK_OK) return q;
    hipError_t e = hipStreamSynchronize(static_cast<hipStream_t>(opts->stream));
    if (e == hipSuccess) e = s.download(occ, h_occluded);
    return launched(who, e);
}

int rtk_query_radiance_host(rtk_ctx* ctx, const rtk_query_opts* opts, int64_t n, const rtk_ray* h_rays, double* h_radiance, uint32_t* h_draws) {
    const char* who = "rtk_query_radiance_host";
    if (check_query_args(who, opts, n, h_rays, "h_rays", h_radiance, "h_radiance") != RTK_OK) return RTK_ERR_INVALID;
    const int rc = check_ctx(who, ctx);
    if (rc != RTK_OK || n == 0) return rc;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    HostStaging s(opts->real_mode == RTK_REAL_F64);
    const int rays = s.piece(size_t(n) * sizeof(rtk_ray)), rad = s.linear(size_t(n) * 3), draws = s.piece(size_t(n) * sizeof(uint32_t), h_draws != nullptr);
    RTK_HIP(s.alloc());
    RTK_HIP(s.upload(rays, h_rays));
    const int q = rtk_query_radiance(ctx, opts, n, s.ptr<rtk_ray>(rays), s.ptr<void>(rad), s.ptr<uint32_t>(draws));
    if (q != RTK_OK) return q;
    hipError_t e = hipStreamSynchronize(static_cast<hipStream_t>(opts->stream));
    if (e == hipSuccess) e = s.download_linear(rad, h_radiance);
    if (e == hipSuccess) e = s.download(draws, h_draws);
    return launched(who, e);
}

}  // extern "C"
