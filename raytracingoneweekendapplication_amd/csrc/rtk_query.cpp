// rtk_query.cpp -- the C-ABI half of every lane-per-ray entry point.  The ray queries (include/rtk.h "Ray queries"): argument
// checks that need no device, the launches on the caller's stream, and the blocking _host forms.  The known-answer entry
// points (rtk_debug_*): host arrays in and out, on the null stream.  The kernels are rtk_trace.hip's, next to the device
// functions they share with the render, AOV and guide kernels.
#include <hip/hip_runtime.h>

#include <initializer_list>
#include <utility>

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
int check_scene(const char* who, const rtk_ctx* ctx) {
    uint64_t digest = 0;
    return ctx_scene(ctx, &digest) ? RTK_OK : fail(RTK_ERR_NO_SCENE, "%s: no scene uploaded", who);
}
int check_ctx(const char* who, const rtk_ctx* ctx) { return ctx ? check_scene(who, ctx) : fail(RTK_ERR_INVALID, "%s: null context", who); }

int launched(const char* who, hipError_t e) { return e == hipSuccess ? RTK_OK : fail(RTK_ERR_HIP, "%s: %s", who, hipGetErrorString(e)); }

// What the known-answer entry points refuse first, in this order: a null or negative argument (args_ok false), a context
// without a scene (where the entry point reads one), an arithmetic type that is neither F64 nor F32.
int check_debug_args(const char* who, bool args_ok, const rtk_ctx* scene_of, int real_mode) {
    if (!args_ok) return fail(RTK_ERR_INVALID, "%s: bad argument", who);
    if (scene_of && check_scene(who, scene_of) != RTK_OK) return RTK_ERR_NO_SCENE;
    return check_real_mode(who, real_mode);
}

// A known-answer call on the device: the staged inputs go up, `launch` (real{}) enqueues the kernel on the null stream, the
// device drains, the outputs come down; inputs and outputs are {piece, host array}.  The first HIP error ends it and is the result.
template <typename Launch>
int run_debug(const char* who, int real_mode, HostStaging& s, std::initializer_list<std::pair<int, const void*>> inputs, Launch&& launch,
              std::initializer_list<std::pair<int, void*>> outputs) {
    hipError_t e = s.alloc();
    for (const auto& in : inputs)
        if (e == hipSuccess) e = s.upload(in.first, in.second);
    if (e == hipSuccess) e = real_mode == RTK_REAL_F64 ? launch(double{}) : launch(float{});
    if (e == hipSuccess) e = hipDeviceSynchronize();
    for (const auto& out : outputs)
        if (e == hipSuccess) e = s.download(out.first, out.second);
    return launched(who, e);
}

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

// Known-answer entry points (include/rtk.h): n cases in host arrays, staged, run one lane each, read back.

int rtk_debug_closest_hit(rtk_ctx* ctx, int real_mode, int n, const double* h_rays, const uint32_t* h_keys, double* h_out, uint64_t* h_draws) {
    const char* who = "rtk_debug_closest_hit";
    const int rc = check_debug_args(who, ctx && n >= 0 && h_rays && h_keys && h_out && h_draws, ctx, real_mode);
    if (rc != RTK_OK || n == 0) return rc;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    HostStaging s(true);
    const int rays = s.piece(size_t(n) * 9 * sizeof(double)), keys = s.piece(size_t(n) * 3 * sizeof(uint32_t));
    const int out = s.piece(size_t(n) * 12 * sizeof(double)), draws = s.piece(size_t(n) * sizeof(uint64_t));
    return run_debug(who, real_mode, s, {{rays, h_rays}, {keys, h_keys}}, [&](auto real) {
        return launch_debug_hit(ctx_view<decltype(real)>(ctx), n, s.ptr<double>(rays), s.ptr<uint32_t>(keys), s.ptr<double>(out), s.ptr<unsigned long long>(draws), nullptr);
    }, {{out, h_out}, {draws, h_draws}});
}

int rtk_debug_scatter(rtk_ctx* ctx, int real_mode, int n, const int32_t* h_materials, const double* h_rays, const double* h_records, const uint32_t* h_keys,
                      double* h_out, uint64_t* h_draws) {
    const char* who = "rtk_debug_scatter";
    const int rc = check_debug_args(who, ctx && n >= 0 && h_materials && h_rays && h_records && h_keys && h_out && h_draws, ctx, real_mode);
    if (rc != RTK_OK) return rc;
    for (int k = 0; k < n; k++)
        if (h_materials[k] < 0 || h_materials[k] >= ctx_n_materials(ctx)) return fail(RTK_ERR_INVALID, "%s: material %d of case %d out of range", who, h_materials[k], k);
    if (n == 0) return RTK_OK;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    HostStaging s(true);
    const int mat = s.piece(size_t(n) * sizeof(int32_t)), ray = s.piece(size_t(n) * 7 * sizeof(double)), rec = s.piece(size_t(n) * 11 * sizeof(double));
    const int keys = s.piece(size_t(n) * 3 * sizeof(uint32_t)), out = s.piece(size_t(n) * 14 * sizeof(double)), draws = s.piece(size_t(n) * sizeof(uint64_t));
    return run_debug(who, real_mode, s, {{mat, h_materials}, {ray, h_rays}, {rec, h_records}, {keys, h_keys}}, [&](auto real) {
        return launch_debug_scatter(ctx_view<decltype(real)>(ctx), n, s.ptr<int32_t>(mat), s.ptr<double>(ray), s.ptr<double>(rec), s.ptr<uint32_t>(keys), s.ptr<double>(out),
                                    s.ptr<unsigned long long>(draws), nullptr);
    }, {{out, h_out}, {draws, h_draws}});
}

int rtk_debug_texture(rtk_ctx* ctx, int real_mode, int n, const int32_t* h_textures, const double* h_uvp, double* h_out, uint64_t* h_work) {
    const char* who = "rtk_debug_texture";
    const int rc = check_debug_args(who, ctx && n >= 0 && h_textures && h_uvp && h_out && h_work, ctx, real_mode);
    if (rc != RTK_OK) return rc;
    for (int k = 0; k < n; k++)
        if (h_textures[k] < 0 || h_textures[k] >= ctx_n_textures(ctx)) return fail(RTK_ERR_INVALID, "%s: texture %d of case %d out of range", who, h_textures[k], k);
    if (n == 0) return RTK_OK;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    HostStaging s(true);
    const int tex = s.piece(size_t(n) * sizeof(int32_t)), uvp = s.piece(size_t(n) * 5 * sizeof(double));
    const int out = s.piece(size_t(n) * 3 * sizeof(double)), work = s.piece(size_t(n) * 2 * sizeof(uint64_t));
    return run_debug(who, real_mode, s, {{tex, h_textures}, {uvp, h_uvp}}, [&](auto real) {
        return launch_debug_texture(ctx_view<decltype(real)>(ctx), n, s.ptr<int32_t>(tex), s.ptr<double>(uvp), s.ptr<double>(out), s.ptr<unsigned long long>(work), nullptr);
    }, {{out, h_out}, {work, h_work}});
}

int rtk_debug_get_ray(rtk_ctx* ctx, int real_mode, const rtk_camera* cam, uint32_t seed, int n, const int32_t* h_pixel_sample, double* h_out, uint64_t* h_draws) {
    const char* who = "rtk_debug_get_ray";
    const int rc = check_debug_args(who, ctx && cam && n >= 0 && h_pixel_sample && h_out && h_draws, nullptr, real_mode);  // (reads no scene)
    if (rc != RTK_OK) return rc;
    if (cam->image_width <= 0 || cam->image_height <= 0) return fail(RTK_ERR_INVALID, "%s: bad camera dimensions", who);
    if (n == 0) return RTK_OK;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    HostStaging s(true);
    const int ijs = s.piece(size_t(n) * 3 * sizeof(int32_t)), out = s.piece(size_t(n) * 7 * sizeof(double)), draws = s.piece(size_t(n) * sizeof(uint64_t));
    return run_debug(who, real_mode, s, {{ijs, h_pixel_sample}}, [&](auto real) {
        return launch_debug_get_ray(device_camera<decltype(real)>(*cam), seed, n, s.ptr<int32_t>(ijs), s.ptr<double>(out), s.ptr<unsigned long long>(draws), nullptr);
    }, {{out, h_out}, {draws, h_draws}});
}

}  // extern "C"
