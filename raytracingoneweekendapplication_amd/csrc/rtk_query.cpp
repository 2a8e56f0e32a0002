// rtk_query.cpp -- the C-ABI half of the ray queries (include/rtk.h "Ray queries") and of the known-answer entry points
// (rtk_debug_*).  Here: the queries' own argument checks, one launch each on the caller's stream, the pieces a _host form
// stages.  What every lane-per-ray family shares -- the alignment, overlap and context checks, with_real, run_host_form -- is
// rtk_internal.h's.  The known-answer entry points take host arrays in and out, on the null stream.  The kernels are
// rtk_trace.hip's, next to the device functions they share with the render, AOV and guide kernels.
#include <hip/hip_runtime.h>

#include "rtk.h"
#include "rtk_internal.h"
#include "rtk_trace.h"

namespace rtk {
namespace {

static_assert(sizeof(rtk_ray) == 88 && sizeof(rtk_ray_hit) == 96 && sizeof(rtk_query_opts) == 56, "ray query records");

// What every query checks before it touches a device: the arguments the three have in common.  Alignment, overlap (outputs
// may not alias d_rays) and the context come afterwards, the context last, so that every other refusal can be had -- and
// tested -- where there is no device to make a context on.
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

Span ray_span(const rtk_ray* d_rays, int64_t n) { return Span{d_rays, size_t(n) * sizeof(rtk_ray), "d_rays"}; }

// What the known-answer entry points refuse first, in this order: a null or negative argument (args_ok false), a context
// without a scene (where the entry point reads one), an arithmetic type that is neither F64 nor F32.
int check_debug_args(const char* who, bool args_ok, const rtk_ctx* scene_of, int real_mode) {
    if (!args_ok) return fail(RTK_ERR_INVALID, "%s: bad argument", who);
    if (scene_of && check_ctx(who, scene_of, true) != RTK_OK) return RTK_ERR_NO_SCENE;
    return check_real_mode(who, real_mode);
}

// A known-answer call on the device: run_host_form around `launch` (real{}), which enqueues the kernel on the null stream.
template <typename Launch>
int run_debug(const char* who, int real_mode, HostStaging& s, std::initializer_list<HostIn> inputs, Launch&& launch, std::initializer_list<HostOut> outputs) {
    return run_host_form(who, nullptr, s, inputs, [&] { return launched(who, with_real(real_mode, launch)); }, outputs);
}

}  // namespace
}  // namespace rtk

using namespace rtk;

extern "C" {

int rtk_query_hits(rtk_ctx* ctx, const rtk_query_opts* opts, int64_t n, const rtk_ray* d_rays, rtk_ray_hit* d_hits) {
    const char* who = "rtk_query_hits";
    if (check_query_args(who, opts, n, d_rays, "d_rays", d_hits, "d_hits") != RTK_OK) return RTK_ERR_INVALID;
    if (check_aligned(d_rays, 8, who, "d_rays") != RTK_OK || check_aligned(d_hits, 8, who, "d_hits") != RTK_OK) return RTK_ERR_INVALID;
    if (check_apart(who, {d_hits, size_t(n) * sizeof(rtk_ray_hit), "d_hits"}, {ray_span(d_rays, n)}) != RTK_OK) return RTK_ERR_INVALID;
    const int rc = check_ctx(who, ctx, true);
    if (rc != RTK_OK || n == 0) return rc;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    const hipStream_t st = static_cast<hipStream_t>(opts->stream);
    return launched(who, with_real(opts->real_mode, [&](auto real) { return launch_query_hits(ctx_view<decltype(real)>(ctx), opts->seed, n, d_rays, d_hits, st); }));
}

int rtk_query_occluded(rtk_ctx* ctx, const rtk_query_opts* opts, int64_t n, const rtk_ray* d_rays, int32_t* d_occluded) {
    const char* who = "rtk_query_occluded";
    if (check_query_args(who, opts, n, d_rays, "d_rays", d_occluded, "d_occluded") != RTK_OK) return RTK_ERR_INVALID;
    if (check_aligned(d_rays, 8, who, "d_rays") != RTK_OK || check_aligned(d_occluded, 4, who, "d_occluded") != RTK_OK) return RTK_ERR_INVALID;
    if (check_apart(who, {d_occluded, size_t(n) * sizeof(int32_t), "d_occluded"}, {ray_span(d_rays, n)}) != RTK_OK) return RTK_ERR_INVALID;
    const int rc = check_ctx(who, ctx, true);
    if (rc != RTK_OK || n == 0) return rc;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    const hipStream_t st = static_cast<hipStream_t>(opts->stream);
    const bool any_hit = (ctx_features(ctx) & F_MEDIA) == 0;  // no constant_medium: the first accepted hit settles the flag
    return launched(who, with_real(opts->real_mode, [&](auto real) {
        return launch_query_occluded(ctx_view<decltype(real)>(ctx), opts->seed, any_hit, n, d_rays, d_occluded, st);
    }));
}

int rtk_query_radiance(rtk_ctx* ctx, const rtk_query_opts* opts, int64_t n, const rtk_ray* d_rays, void* d_radiance, uint32_t* d_draws) {
    const char* who = "rtk_query_radiance";
    if (check_query_args(who, opts, n, d_rays, "d_rays", d_radiance, "d_radiance") != RTK_OK) return RTK_ERR_INVALID;
    const size_t real_bytes = opts->real_mode == RTK_REAL_F64 ? sizeof(double) : sizeof(float);
    if (check_aligned(d_rays, 8, who, "d_rays") != RTK_OK || check_aligned(d_radiance, real_bytes, who, "d_radiance") != RTK_OK ||
        check_aligned(d_draws, 4, who, "d_draws") != RTK_OK)
        return RTK_ERR_INVALID;
    if (check_apart(who, {d_radiance, size_t(n) * 3 * real_bytes, "d_radiance"}, {ray_span(d_rays, n)}) != RTK_OK ||
        check_apart(who, {d_draws, size_t(n) * sizeof(uint32_t), "d_draws"}, {ray_span(d_rays, n)}) != RTK_OK)
        return RTK_ERR_INVALID;
    const int rc = check_ctx(who, ctx, true);
    if (rc != RTK_OK || n == 0) return rc;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    const hipStream_t st = static_cast<hipStream_t>(opts->stream);
    const rtk_camera cam = path_camera(opts->background, opts->max_depth, opts->samples);
    return launched(who, with_real(opts->real_mode, [&](auto real) {
        using R = decltype(real);
        return launch_query_radiance(ctx_view<R>(ctx), device_camera<R>(cam), opts->seed, n, d_rays, d_radiance, d_draws, st);
    }));
}

int rtk_query_hits_host(rtk_ctx* ctx, const rtk_query_opts* opts, int64_t n, const rtk_ray* h_rays, rtk_ray_hit* h_hits) {
    const char* who = "rtk_query_hits_host";
    if (check_query_args(who, opts, n, h_rays, "h_rays", h_hits, "h_hits") != RTK_OK) return RTK_ERR_INVALID;
    const int rc = check_ctx(who, ctx, true);
    if (rc != RTK_OK || n == 0) return rc;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    HostStaging s(true);
    const int rays = s.piece(size_t(n) * sizeof(rtk_ray)), hits = s.piece(size_t(n) * sizeof(rtk_ray_hit));
    return run_host_form(who, static_cast<hipStream_t>(opts->stream), s, {{rays, h_rays}},
                         [&] { return rtk_query_hits(ctx, opts, n, s.ptr<rtk_ray>(rays), s.ptr<rtk_ray_hit>(hits)); }, {{hits, h_hits}});
}

int rtk_query_occluded_host(rtk_ctx* ctx, const rtk_query_opts* opts, int64_t n, const rtk_ray* h_rays, int32_t* h_occluded) {
    const char* who = "rtk_query_occluded_host";
    if (check_query_args(who, opts, n, h_rays, "h_rays", h_occluded, "h_occluded") != RTK_OK) return RTK_ERR_INVALID;
    const int rc = check_ctx(who, ctx, true);
    if (rc != RTK_OK || n == 0) return rc;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    HostStaging s(true);
    const int rays = s.piece(size_t(n) * sizeof(rtk_ray)), occ = s.piece(size_t(n) * sizeof(int32_t));
    return run_host_form(who, static_cast<hipStream_t>(opts->stream), s, {{rays, h_rays}},
                         [&] { return rtk_query_occluded(ctx, opts, n, s.ptr<rtk_ray>(rays), s.ptr<int32_t>(occ)); }, {{occ, h_occluded}});
}

int rtk_query_radiance_host(rtk_ctx* ctx, const rtk_query_opts* opts, int64_t n, const rtk_ray* h_rays, double* h_radiance, uint32_t* h_draws) {
    const char* who = "rtk_query_radiance_host";
    if (check_query_args(who, opts, n, h_rays, "h_rays", h_radiance, "h_radiance") != RTK_OK) return RTK_ERR_INVALID;
    const int rc = check_ctx(who, ctx, true);
    if (rc != RTK_OK || n == 0) return rc;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    HostStaging s(opts->real_mode == RTK_REAL_F64);
    const int rays = s.piece(size_t(n) * sizeof(rtk_ray)), rad = s.linear(size_t(n) * 3), draws = s.piece(size_t(n) * sizeof(uint32_t), h_draws != nullptr);
    return run_host_form(who, static_cast<hipStream_t>(opts->stream), s, {{rays, h_rays}},
                         [&] { return rtk_query_radiance(ctx, opts, n, s.ptr<rtk_ray>(rays), s.ptr<void>(rad), s.ptr<uint32_t>(draws)); },
                         {{rad, h_radiance, true}, {draws, h_draws}});
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
