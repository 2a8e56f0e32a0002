// rtk_gather.cpp -- the C-ABI half of the surface gathers (include/rtk.h "Surface gathers"): rtk_gather_rays, rtk_gather_irradiance
// and rtk_gather_occlusion with their _host forms.  Argument checks that need no device, the batches of points the workspace
// budget allows, the two launches per batch on the caller's stream, the staging of the blocking forms.  Stage 1 is rtk_trace.hip's
// (rtk_gather_irradiance_kernel, rtk_gather_occlusion_kernel), the ray records and stage 2 are rtk_gather.hip's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <initializer_list>
#include <limits>

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

static_assert(sizeof(rtk_gather_opts) == 96, "surface gather options");

constexpr size_t kUnitBytes = 4 * sizeof(double);  // a (point, pass) unit's partial sums in the workspace

int gather_rays_of(const rtk_gather_opts* opts) { return opts->rays != 0 ? opts->rays : 256; }
double gather_tmax(const rtk_gather_opts* opts) { return opts->max_distance > 0.0 ? opts->max_distance : std::numeric_limits<double>::infinity(); }

// Points per launch: batch_points when given, else what RTK_GATHER_WORKSPACE_BYTES holds (at least 8192: a point has at most 256 units).
int64_t gather_batch(const rtk_gather_opts* opts, int64_t n) {
    const int64_t budget = int64_t(RTK_GATHER_WORKSPACE_BYTES / (size_t(gather_rays_of(opts) / 64) * kUnitBytes));
    return std::min(n, opts->batch_points > 0 ? int64_t(opts->batch_points) : budget);
}

// What the entry points and their _host forms check before they touch a device, in the light probes' order (check_probe_args);
// alignment, overlap and the context come afterwards.
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

// An output of `bytes` bytes may not share an address with the n points or the n normals (a null output overlaps nothing).
int check_apart(const char* who, int64_t n, const void* points, const void* normals, const void* out, size_t bytes, const char* arg) {
    if (!out || n == 0) return RTK_OK;
    const uintptr_t o = reinterpret_cast<uintptr_t>(out), in_bytes = uintptr_t(n) * 3 * sizeof(double);
    for (const void* in : {points, normals}) {
        const uintptr_t i = reinterpret_cast<uintptr_t>(in);
        if (!(o + bytes <= i || i + in_bytes <= o)) return fail(RTK_ERR_INVALID, "%s: %s overlaps %s", who, arg, in == points ? "d_points" : "d_normals");
    }
    return RTK_OK;
}

int check_gather_ctx(const char* who, const rtk_ctx* ctx, bool needs_scene) {
    if (!ctx) return fail(RTK_ERR_INVALID, "%s: null context", who);
    uint64_t digest = 0;
    return !needs_scene || ctx_scene(ctx, &digest) ? RTK_OK : fail(RTK_ERR_NO_SCENE, "%s: no scene uploaded", who);
}

int launched(const char* who, hipError_t e) { return e == hipSuccess ? RTK_OK : fail(RTK_ERR_HIP, "%s: %s", who, hipGetErrorString(e)); }

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
    if (check_apart(who, n, d_points, d_normals, d_rays, size_t(n) * size_t(rays) * sizeof(rtk_ray), "d_rays") != RTK_OK) return RTK_ERR_INVALID;
    const int rc = check_gather_ctx(who, ctx, false);
    if (rc != RTK_OK || n == 0) return rc;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    return launched(who, launch_gather_rays(n, rays, opts->samples > 0 ? opts->samples : 1, opts->first_key, uint32_t(opts->rotate), opts->time, gather_tmax(opts),
                                            d_points, d_normals, d_rays, static_cast<hipStream_t>(opts->stream)));
}

int rtk_gather_irradiance(rtk_ctx* ctx, const rtk_gather_opts* opts, int64_t n, const double* d_points, const double* d_normals, void* d_irradiance) {
    const char* who = "rtk_gather_irradiance";
    if (check_gather_args(who, opts, n, d_points, "d_points", d_normals, "d_normals", d_irradiance, "d_irradiance") != RTK_OK) return RTK_ERR_INVALID;
    const bool f64 = opts->real_mode == RTK_REAL_F64;
    const size_t real_bytes = f64 ? sizeof(double) : sizeof(float);
    if (check_aligned(d_points, 8, who, "d_points") != RTK_OK || check_aligned(d_normals, 8, who, "d_normals") != RTK_OK ||
        check_aligned(d_irradiance, real_bytes, who, "d_irradiance") != RTK_OK)
        return RTK_ERR_INVALID;
    if (check_apart(who, n, d_points, d_normals, d_irradiance, size_t(n) * 3 * real_bytes, "d_irradiance") != RTK_OK) return RTK_ERR_INVALID;
    const int rc = check_gather_ctx(who, ctx, true);
    if (rc != RTK_OK || n == 0) return rc;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    const hipStream_t st = static_cast<hipStream_t>(opts->stream);
    rtk_camera cam{};  // what the kernel reads of a camera, as rtk_query_radiance: background, max_depth and the samples per ray
    cam.background = opts->background;
    cam.max_depth = opts->max_depth;
    cam.samples_per_pixel = opts->samples > 0 ? opts->samples : 1;
    const int rays = gather_rays_of(opts);
    const int64_t batch = gather_batch(opts, n);
    double* ws = nullptr;
    RTK_HIP(batch_workspace(ctx, opts, batch, &ws));
    for (int64_t k0 = 0; k0 < n; k0 += batch) {
        const int64_t m = std::min(batch, n - k0);
        const double *p = d_points + k0 * 3, *nrm = d_normals + k0 * 3;
        const uint32_t key = opts->first_key + uint32_t(k0), rot = uint32_t(opts->rotate);
        void* out = static_cast<char*>(d_irradiance) + size_t(k0) * 3 * real_bytes;
        hipError_t e = f64 ? launch_gather_irradiance<double>(ctx_view<double>(ctx), device_camera<double>(cam), opts->seed, key, rays, rot, opts->time, m, p, nrm, ws, st)
                           : launch_gather_irradiance<float>(ctx_view<float>(ctx), device_camera<float>(cam), opts->seed, key, rays, rot, opts->time, m, p, nrm, ws, st);
        if (e == hipSuccess) e = f64 ? launch_gather_irradiance_reduce<double>(m, rays, ws, out, st) : launch_gather_irradiance_reduce<float>(m, rays, ws, out, st);
        if (e != hipSuccess) return launched(who, e);
    }
    return RTK_OK;
}

int rtk_gather_occlusion(rtk_ctx* ctx, const rtk_gather_opts* opts, int64_t n, const double* d_points, const double* d_normals, void* d_open, void* d_bent) {
    const char* who = "rtk_gather_occlusion";
    if (check_gather_args(who, opts, n, d_points, "d_points", d_normals, "d_normals", d_open ? d_open : d_bent, "d_open and d_bent") != RTK_OK)
        return RTK_ERR_INVALID;
    const bool f64 = opts->real_mode == RTK_REAL_F64;
    const size_t real_bytes = f64 ? sizeof(double) : sizeof(float);
    if (check_aligned(d_points, 8, who, "d_points") != RTK_OK || check_aligned(d_normals, 8, who, "d_normals") != RTK_OK ||
        check_aligned(d_open, real_bytes, who, "d_open") != RTK_OK || check_aligned(d_bent, real_bytes, who, "d_bent") != RTK_OK)
        return RTK_ERR_INVALID;
    if (check_apart(who, n, d_points, d_normals, d_open, size_t(n) * real_bytes, "d_open") != RTK_OK ||
        check_apart(who, n, d_points, d_normals, d_bent, size_t(n) * 3 * real_bytes, "d_bent") != RTK_OK)
        return RTK_ERR_INVALID;
    const int rc = check_gather_ctx(who, ctx, true);
    if (rc != RTK_OK || n == 0) return rc;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    const hipStream_t st = static_cast<hipStream_t>(opts->stream);
    const bool any_hit = (ctx_features(ctx) & F_MEDIA) == 0;  // no constant_medium: the first accepted hit settles a ray
    const int rays = gather_rays_of(opts), samples = opts->samples > 0 ? opts->samples : 1;
    const double tmax = gather_tmax(opts);
    const int64_t batch = gather_batch(opts, n);
    double* ws = nullptr;
    RTK_HIP(batch_workspace(ctx, opts, batch, &ws));
    for (int64_t k0 = 0; k0 < n; k0 += batch) {
        const int64_t m = std::min(batch, n - k0);
        const double *p = d_points + k0 * 3, *nrm = d_normals + k0 * 3;
        const uint32_t key = opts->first_key + uint32_t(k0), rot = uint32_t(opts->rotate);
        void* open = d_open ? static_cast<char*>(d_open) + size_t(k0) * real_bytes : nullptr;
        void* bent = d_bent ? static_cast<char*>(d_bent) + size_t(k0) * 3 * real_bytes : nullptr;
        hipError_t e = f64 ? launch_gather_occlusion<double>(ctx_view<double>(ctx), opts->seed, any_hit, key, rays, samples, rot, opts->time, tmax, m, p, nrm, ws, st)
                           : launch_gather_occlusion<float>(ctx_view<float>(ctx), opts->seed, any_hit, key, rays, samples, rot, opts->time, tmax, m, p, nrm, ws, st);
        if (e == hipSuccess) e = f64 ? launch_gather_occlusion_reduce<double>(m, rays, ws, open, bent, st) : launch_gather_occlusion_reduce<float>(m, rays, ws, open, bent, st);
        if (e != hipSuccess) return launched(who, e);
    }
    return RTK_OK;
}

int rtk_gather_rays_host(rtk_ctx* ctx, const rtk_gather_opts* opts, int64_t n, const double* h_points, const double* h_normals, rtk_ray* h_rays) {
    const char* who = "rtk_gather_rays_host";
    if (check_gather_args(who, opts, n, h_points, "h_points", h_normals, "h_normals", h_rays, "h_rays") != RTK_OK) return RTK_ERR_INVALID;
    const int rc = check_gather_ctx(who, ctx, false);
    if (rc != RTK_OK || n == 0) return rc;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    HostStaging s(true);
    const int pts = s.piece(size_t(n) * 3 * sizeof(double)), nrm = s.piece(size_t(n) * 3 * sizeof(double));
    const int rays = s.piece(size_t(n) * size_t(gather_rays_of(opts)) * sizeof(rtk_ray));
    RTK_HIP(s.alloc());
    RTK_HIP(s.upload(pts, h_points));
    RTK_HIP(s.upload(nrm, h_normals));
    const int q = rtk_gather_rays(ctx, opts, n, s.ptr<double>(pts), s.ptr<double>(nrm), s.ptr<rtk_ray>(rays));
    if (q != RTK_OK) return q;
    hipError_t e = hipStreamSynchronize(static_cast<hipStream_t>(opts->stream));
    if (e == hipSuccess) e = s.download(rays, h_rays);
    return launched(who, e);
}

int rtk_gather_irradiance_host(rtk_ctx* ctx, const rtk_gather_opts* opts, int64_t n, const double* h_points, const double* h_normals, double* h_irradiance) {
    const char* who = "rtk_gather_irradiance_host";
    if (check_gather_args(who, opts, n, h_points, "h_points", h_normals, "h_normals", h_irradiance, "h_irradiance") != RTK_OK) return RTK_ERR_INVALID;
    const int rc = check_gather_ctx(who, ctx, true);
    if (rc != RTK_OK || n == 0) return rc;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    HostStaging s(opts->real_mode == RTK_REAL_F64);
    const int pts = s.piece(size_t(n) * 3 * sizeof(double)), nrm = s.piece(size_t(n) * 3 * sizeof(double)), out = s.linear(size_t(n) * 3);
    RTK_HIP(s.alloc());
    RTK_HIP(s.upload(pts, h_points));
    RTK_HIP(s.upload(nrm, h_normals));
    const int q = rtk_gather_irradiance(ctx, opts, n, s.ptr<double>(pts), s.ptr<double>(nrm), s.ptr<void>(out));
    if (q != RTK_OK) return q;
    hipError_t e = hipStreamSynchronize(static_cast<hipStream_t>(opts->stream));
    if (e == hipSuccess) e = s.download_linear(out, h_irradiance);
    return launched(who, e);
}

int rtk_gather_occlusion_host(rtk_ctx* ctx, const rtk_gather_opts* opts, int64_t n, const double* h_points, const double* h_normals, double* h_open,
                              double* h_bent) {
    const char* who = "rtk_gather_occlusion_host";
    if (check_gather_args(who, opts, n, h_points, "h_points", h_normals, "h_normals", h_open ? h_open : h_bent, "h_open and h_bent") != RTK_OK)
        return RTK_ERR_INVALID;
    const int rc = check_gather_ctx(who, ctx, true);
    if (rc != RTK_OK || n == 0) return rc;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    HostStaging s(opts->real_mode == RTK_REAL_F64);
    const int pts = s.piece(size_t(n) * 3 * sizeof(double)), nrm = s.piece(size_t(n) * 3 * sizeof(double));
    const int open = s.linear(size_t(n), h_open != nullptr), bent = s.linear(size_t(n) * 3, h_bent != nullptr);
    RTK_HIP(s.alloc());
    RTK_HIP(s.upload(pts, h_points));
    RTK_HIP(s.upload(nrm, h_normals));
    const int q = rtk_gather_occlusion(ctx, opts, n, s.ptr<double>(pts), s.ptr<double>(nrm), s.ptr<void>(open), s.ptr<void>(bent));
    if (q != RTK_OK) return q;
    hipError_t e = hipStreamSynchronize(static_cast<hipStream_t>(opts->stream));
    if (e == hipSuccess) e = s.download_linear(open, h_open);
    if (e == hipSuccess) e = s.download_linear(bent, h_bent);
    return launched(who, e);
}

}  // extern "C"
