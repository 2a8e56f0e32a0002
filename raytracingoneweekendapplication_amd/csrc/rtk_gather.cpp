// rtk_gather.cpp -- the C-ABI half of the surface gathers (include/rtk.h "Surface gathers"): rtk_gather_rays, rtk_gather_irradiance
// and rtk_gather_occlusion with their _host forms.  Here: the gathers' own argument checks, the batches of points the workspace
// budget allows, the two launches per batch on the caller's stream, the pieces a _host form stages; the checks and the staging
// every lane-per-ray family shares are rtk_internal.h's.  Stage 1 is rtk_trace.hip's (rtk_gather_irradiance_kernel,
// rtk_gather_occlusion_kernel), the ray records and stage 2 are rtk_gather.hip's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <limits>

#include "rtk.h"
#include "rtk_internal.h"
#include "rtk_trace.h"

namespace rtk {
namespace {

static_assert(sizeof(rtk_gather_opts) == 96, "surface gather options");

constexpr size_t kUnitBytes = 4 * sizeof(double);  // a (point, pass) unit's partial sums in the workspace

int gather_rays_of(const rtk_gather_opts* opts) { return opts->rays != 0 ? opts->rays : 256; }
double gather_tmax(const rtk_gather_opts* opts) { return opts->max_distance > 0.0 ? opts->max_distance : std::numeric_limits<double>::infinity(); }

// Points per launch: batch_points when given, else what RTK_GATHER_WORKSPACE_BYTES holds (at least 8192: a point has at most 256 units).
int64_t gather_batch(const rtk_gather_opts* opts, int64_t n) {
    const int64_t budget = int64_t(RTK_GATHER_WORKSPACE_BYTES / (size_t(gather_rays_of(opts) / 64) * kUnitBytes));
    return std::min(n, opts->batch_points > 0 ? int64_t(opts->batch_points) : budget);
}

// What the entry points and their _host forms check before they touch a device; alignment, overlap (an output may not share an
// address with the n points or the n normals) and the context come afterwards.
int check_gather_args(const char* who, const rtk_gather_opts* opts, int64_t n, const void* points, const char* points_name, const void* normals,
                      const char* normals_name, const void* out, const char* out_name) {
    if (!opts) return fail(RTK_ERR_INVALID, "%s: null opts", who);
    if (n < 0) return fail(RTK_ERR_INVALID, "%s: n must not be negative (%lld)", who, (long long)n);
    if (check_real_mode(who, opts->real_mode) != RTK_OK) return RTK_ERR_INVALID;
    if (opts->max_depth < 0) return fail(RTK_ERR_INVALID, "%s: max_depth must not be negative (%d)", who, opts->max_depth);
    if (opts->samples < 0) return fail(RTK_ERR_INVALID, "%s: samples must not be negative (%d)", who, opts->samples);
    for (int r : opts->reserved)
        if (r != 0) return fail(RTK_ERR_INVALID, "%s: reserved must be 0", who);
    const int rays = gather_rays_of(opts);
    if (rays < 64 || rays > 16384 || rays % 64 != 0) return fail(RTK_ERR_INVALID, "%s: rays must be a multiple of 64 in 64 .. 16384 (%d)", who, opts->rays);
    if (n > int64_t(0x7FFFFFFF) / rays) return fail(RTK_ERR_INVALID, "%s: n * rays must not exceed 2^31 - 1 (%lld points of %d)", who, (long long)n, rays);
    if (opts->rotate != 0 && opts->rotate != 1) return fail(RTK_ERR_INVALID, "%s: rotate must be 0 or 1 (%d)", who, opts->rotate);
    if (opts->batch_points < 0) return fail(RTK_ERR_INVALID, "%s: batch_points must not be negative (%d)", who, opts->batch_points);
    if (!(opts->max_distance >= 0.0)) return fail(RTK_ERR_INVALID, "%s: max_distance must not be negative (%g)", who, opts->max_distance);
    if (!points) return fail(RTK_ERR_INVALID, "%s: null %s", who, points_name);
    if (!normals) return fail(RTK_ERR_INVALID, "%s: null %s", who, normals_name);
    if (!out) return fail(RTK_ERR_INVALID, "%s: null %s", who, out_name);
    return RTK_OK;
}

int check_apart_from_inputs(const char* who, int64_t n, const double* d_points, const double* d_normals, const Span& out) {
    const size_t in_bytes = size_t(n) * 3 * sizeof(double);
    return check_apart(who, out, {{d_points, in_bytes, "d_points"}, {d_normals, in_bytes, "d_normals"}});
}

// The context's workspace for batches of `batch` points.
hipError_t batch_workspace(rtk_ctx* ctx, const rtk_gather_opts* opts, int64_t batch, double** out) {
    void* ws = nullptr;
    const hipError_t e = gather_workspace(ctx, size_t(batch) * size_t(gather_rays_of(opts) / 64) * kUnitBytes, &ws);
    *out = static_cast<double*>(ws);
    return e;
}

}  // namespace
}  // namespace rtk

using namespace rtk;

extern "C" {

int rtk_gather_rays(rtk_ctx* ctx, const rtk_gather_opts* opts, int64_t n, const double* d_points, const double* d_normals, rtk_ray* d_rays) {
    const char* who = "rtk_gather_rays";
    if (check_gather_args(who, opts, n, d_points, "d_points", d_normals, "d_normals", d_rays, "d_rays") != RTK_OK) return RTK_ERR_INVALID;
    if (check_aligned(d_points, 8, who, "d_points") != RTK_OK || check_aligned(d_normals, 8, who, "d_normals") != RTK_OK ||
        check_aligned(d_rays, 8, who, "d_rays") != RTK_OK)
        return RTK_ERR_INVALID;
    const int rays = gather_rays_of(opts);
    if (check_apart_from_inputs(who, n, d_points, d_normals, {d_rays, size_t(n) * size_t(rays) * sizeof(rtk_ray), "d_rays"}) != RTK_OK) return RTK_ERR_INVALID;
    const int rc = check_ctx(who, ctx, false);
    if (rc != RTK_OK || n == 0) return rc;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    return launched(who, launch_gather_rays(n, rays, opts->samples > 0 ? opts->samples : 1, opts->first_key, uint32_t(opts->rotate), opts->time, gather_tmax(opts),
                                            d_points, d_normals, d_rays, static_cast<hipStream_t>(opts->stream)));
}

int rtk_gather_irradiance(rtk_ctx* ctx, const rtk_gather_opts* opts, int64_t n, const double* d_points, const double* d_normals, void* d_irradiance) {
    const char* who = "rtk_gather_irradiance";
    if (check_gather_args(who, opts, n, d_points, "d_points", d_normals, "d_normals", d_irradiance, "d_irradiance") != RTK_OK) return RTK_ERR_INVALID;
    const size_t real_bytes = opts->real_mode == RTK_REAL_F64 ? sizeof(double) : sizeof(float);
    if (check_aligned(d_points, 8, who, "d_points") != RTK_OK || check_aligned(d_normals, 8, who, "d_normals") != RTK_OK ||
        check_aligned(d_irradiance, real_bytes, who, "d_irradiance") != RTK_OK)
        return RTK_ERR_INVALID;
    if (check_apart_from_inputs(who, n, d_points, d_normals, {d_irradiance, size_t(n) * 3 * real_bytes, "d_irradiance"}) != RTK_OK) return RTK_ERR_INVALID;
    const int rc = check_ctx(who, ctx, true);
    if (rc != RTK_OK || n == 0) return rc;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    const hipStream_t st = static_cast<hipStream_t>(opts->stream);
    const rtk_camera cam = path_camera(opts->background, opts->max_depth, opts->samples);
    const int rays = gather_rays_of(opts);
    const int64_t batch = gather_batch(opts, n);
    double* ws = nullptr;
    RTK_HIP(batch_workspace(ctx, opts, batch, &ws));
    return launched(who, with_real(opts->real_mode, [&](auto real) {
        using R = decltype(real);
        for (int64_t k0 = 0; k0 < n; k0 += batch) {
            const int64_t m = std::min(batch, n - k0);
            const double *p = d_points + k0 * 3, *nrm = d_normals + k0 * 3;
            const uint32_t key = opts->first_key + uint32_t(k0), rot = uint32_t(opts->rotate);
            void* out = static_cast<char*>(d_irradiance) + size_t(k0) * 3 * real_bytes;
            hipError_t e = launch_gather_irradiance(ctx_view<R>(ctx), device_camera<R>(cam), opts->seed, key, rays, rot, opts->time, m, p, nrm, ws, st);
            if (e == hipSuccess) e = launch_gather_irradiance_reduce<R>(m, rays, ws, out, st);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }));
}

int rtk_gather_occlusion(rtk_ctx* ctx, const rtk_gather_opts* opts, int64_t n, const double* d_points, const double* d_normals, void* d_open, void* d_bent) {
    const char* who = "rtk_gather_occlusion";
    if (check_gather_args(who, opts, n, d_points, "d_points", d_normals, "d_normals", d_open ? d_open : d_bent, "d_open and d_bent") != RTK_OK)
        return RTK_ERR_INVALID;
    const size_t real_bytes = opts->real_mode == RTK_REAL_F64 ? sizeof(double) : sizeof(float);
    if (check_aligned(d_points, 8, who, "d_points") != RTK_OK || check_aligned(d_normals, 8, who, "d_normals") != RTK_OK ||
        check_aligned(d_open, real_bytes, who, "d_open") != RTK_OK || check_aligned(d_bent, real_bytes, who, "d_bent") != RTK_OK)
        return RTK_ERR_INVALID;
    if (check_apart_from_inputs(who, n, d_points, d_normals, {d_open, size_t(n) * real_bytes, "d_open"}) != RTK_OK ||
        check_apart_from_inputs(who, n, d_points, d_normals, {d_bent, size_t(n) * 3 * real_bytes, "d_bent"}) != RTK_OK)
        return RTK_ERR_INVALID;
    const int rc = check_ctx(who, ctx, true);
    if (rc != RTK_OK || n == 0) return rc;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    const hipStream_t st = static_cast<hipStream_t>(opts->stream);
    const bool any_hit = (ctx_features(ctx) & F_MEDIA) == 0;  // no constant_medium: the first accepted hit settles a ray
    const int rays = gather_rays_of(opts), samples = opts->samples > 0 ? opts->samples : 1;
    const double tmax = gather_tmax(opts);
    const int64_t batch = gather_batch(opts, n);
    double* ws = nullptr;
    RTK_HIP(batch_workspace(ctx, opts, batch, &ws));
    return launched(who, with_real(opts->real_mode, [&](auto real) {
        using R = decltype(real);
        for (int64_t k0 = 0; k0 < n; k0 += batch) {
            const int64_t m = std::min(batch, n - k0);
            const double *p = d_points + k0 * 3, *nrm = d_normals + k0 * 3;
            const uint32_t key = opts->first_key + uint32_t(k0), rot = uint32_t(opts->rotate);
            void* open = d_open ? static_cast<char*>(d_open) + size_t(k0) * real_bytes : nullptr;
            void* bent = d_bent ? static_cast<char*>(d_bent) + size_t(k0) * 3 * real_bytes : nullptr;
            hipError_t e = launch_gather_occlusion(ctx_view<R>(ctx), opts->seed, any_hit, key, rays, samples, rot, opts->time, tmax, m, p, nrm, ws, st);
            if (e == hipSuccess) e = launch_gather_occlusion_reduce<R>(m, rays, ws, open, bent, st);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }));
}

int rtk_gather_rays_host(rtk_ctx* ctx, const rtk_gather_opts* opts, int64_t n, const double* h_points, const double* h_normals, rtk_ray* h_rays) {
    const char* who = "rtk_gather_rays_host";
    if (check_gather_args(who, opts, n, h_points, "h_points", h_normals, "h_normals", h_rays, "h_rays") != RTK_OK) return RTK_ERR_INVALID;
    const int rc = check_ctx(who, ctx, false);
    if (rc != RTK_OK || n == 0) return rc;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    HostStaging s(true);
    const int pts = s.piece(size_t(n) * 3 * sizeof(double)), nrm = s.piece(size_t(n) * 3 * sizeof(double));
    const int rays = s.piece(size_t(n) * size_t(gather_rays_of(opts)) * sizeof(rtk_ray));
    return run_host_form(who, static_cast<hipStream_t>(opts->stream), s, {{pts, h_points}, {nrm, h_normals}},
                         [&] { return rtk_gather_rays(ctx, opts, n, s.ptr<double>(pts), s.ptr<double>(nrm), s.ptr<rtk_ray>(rays)); }, {{rays, h_rays}});
}

int rtk_gather_irradiance_host(rtk_ctx* ctx, const rtk_gather_opts* opts, int64_t n, const double* h_points, const double* h_normals, double* h_irradiance) {
    const char* who = "rtk_gather_irradiance_host";
    if (check_gather_args(who, opts, n, h_points, "h_points", h_normals, "h_normals", h_irradiance, "h_irradiance") != RTK_OK) return RTK_ERR_INVALID;
    const int rc = check_ctx(who, ctx, true);
    if (rc != RTK_OK || n == 0) return rc;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    HostStaging s(opts->real_mode == RTK_REAL_F64);
    const int pts = s.piece(size_t(n) * 3 * sizeof(double)), nrm = s.piece(size_t(n) * 3 * sizeof(double)), out = s.linear(size_t(n) * 3);
    return run_host_form(who, static_cast<hipStream_t>(opts->stream), s, {{pts, h_points}, {nrm, h_normals}},
                         [&] { return rtk_gather_irradiance(ctx, opts, n, s.ptr<double>(pts), s.ptr<double>(nrm), s.ptr<void>(out)); }, {{out, h_irradiance, true}});
}

int rtk_gather_occlusion_host(rtk_ctx* ctx, const rtk_gather_opts* opts, int64_t n, const double* h_points, const double* h_normals, double* h_open,
                              double* h_bent) {
    const char* who = "rtk_gather_occlusion_host";
    if (check_gather_args(who, opts, n, h_points, "h_points", h_normals, "h_normals", h_open ? h_open : h_bent, "h_open and h_bent") != RTK_OK)
        return RTK_ERR_INVALID;
    const int rc = check_ctx(who, ctx, true);
    if (rc != RTK_OK || n == 0) return rc;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    HostStaging s(opts->real_mode == RTK_REAL_F64);
    const int pts = s.piece(size_t(n) * 3 * sizeof(double)), nrm = s.piece(size_t(n) * 3 * sizeof(double));
    const int open = s.linear(size_t(n), h_open != nullptr), bent = s.linear(size_t(n) * 3, h_bent != nullptr);
    return run_host_form(who, static_cast<hipStream_t>(opts->stream), s, {{pts, h_points}, {nrm, h_normals}},
                         [&] { return rtk_gather_occlusion(ctx, opts, n, s.ptr<double>(pts), s.ptr<double>(nrm), s.ptr<void>(open), s.ptr<void>(bent)); },
                         {{open, h_open, true}, {bent, h_bent, true}});
}

}  // extern "C"
