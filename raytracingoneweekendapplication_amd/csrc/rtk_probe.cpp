// rtk_probe.cpp -- the C-ABI half of the light probes' ray side (include/rtk.h "Light probes"): rtk_probe_rays and
// rtk_probe_bake with their _host forms.  Argument checks that need no device, the launches on the caller's stream, the staging
// of the blocking forms.  The kernels are rtk_trace.hip's (rtk_probe_rays_kernel, rtk_probe_bake_kernel), next to the radiance
// query whose path loop they run; the lookup (rtk_probe_irradiance) is rtk_probe.hip.
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

static_assert(sizeof(rtk_probe_opts) == 72 && sizeof(rtk_probe_grid) == 64, "light probe records");

int probe_rays_of(const rtk_probe_opts* opts) { return opts->rays != 0 ? opts->rays : 1024; }

// What both entry points and their _host forms check before they touch a device, in the ray queries' order (check_query_args);
// the context comes afterwards.
int check_probe_args(const char* who, const rtk_probe_opts* opts, int64_t n, const void* positions, const char* positions_name, const void* out,
                     const char* out_name) {
    if (!opts) return fail(RTK_ERR_INVALID, "%s: null opts", who);
    if (n < 0) return fail(RTK_ERR_INVALID, "%s: n must not be negative (%lld)", who, (long long)n);
    if (check_real_mode(who, opts->real_mode) != RTK_OK) return RTK_ERR_INVALID;
    if (opts->max_depth < 0) return fail(RTK_ERR_INVALID, "%s: max_depth must not be negative (%d)", who, opts->max_depth);
    if (opts->samples < 0) return fail(RTK_ERR_INVALID, "%s: samples must not be negative (%d)", who, opts->samples);
    if (opts->reserved[0] != 0 || opts->reserved[1] != 0) return fail(RTK_ERR_INVALID, "%s: reserved must be 0", who);
    const int rays = probe_rays_of(opts);
    if (rays < 256 || rays > 65536 || rays % 256 != 0) return fail(RTK_ERR_INVALID, "%s: rays must be a multiple of 256 in 256 .. 65536 (%d)", who, opts->rays);
    if (n > int64_t(0x7FFFFFFF) / rays) return fail(RTK_ERR_INVALID, "%s: n * rays must not exceed 2^31 - 1 (%lld probes of %d)", who, (long long)n, rays);
    if (!positions) return fail(RTK_ERR_INVALID, "%s: null %s", who, positions_name);
    if (!out) return fail(RTK_ERR_INVALID, "%s: null %s", who, out_name);
    return RTK_OK;
}

int check_probe_ctx(const char* who, const rtk_ctx* ctx, bool needs_scene) {
    if (!ctx) return fail(RTK_ERR_INVALID, "%s: null context", who);
    uint64_t digest = 0;
    return !needs_scene || ctx_scene(ctx, &digest) ? RTK_OK : fail(RTK_ERR_NO_SCENE, "%s: no scene uploaded", who);
}

int launched(const char* who, hipError_t e) { return e == hipSuccess ? RTK_OK : fail(RTK_ERR_HIP, "%s: %s", who, hipGetErrorString(e)); }

}  // namespace
}  // namespace rtk

using namespace rtk;

extern "C" {

int rtk_probe_rays(rtk_ctx* ctx, const rtk_probe_opts* opts, int64_t n, const double* d_positions, rtk_ray* d_rays) {
    const char* who = "rtk_probe_rays";
    if (check_probe_args(who, opts, n, d_positions, "d_positions", d_rays, "d_rays") != RTK_OK) return RTK_ERR_INVALID;
    if (check_aligned(d_positions, 8, who, "d_positions") != RTK_OK || check_aligned(d_rays, 8, who, "d_rays") != RTK_OK) return RTK_ERR_INVALID;
    const int rc = check_probe_ctx(who, ctx, false);
    if (rc != RTK_OK || n == 0) return rc;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    return launched(who, launch_probe_rays(n, probe_rays_of(opts), opts->samples > 0 ? opts->samples : 1, opts->first_key, opts->time, d_positions, d_rays,
                                           static_cast<hipStream_t>(opts->stream)));
}

int rtk_probe_bake(rtk_ctx* ctx, const rtk_probe_opts* opts, int64_t n, const double* d_positions, void* d_sh) {
    const char* who = "rtk_probe_bake";
    if (check_probe_args(who, opts, n, d_positions, "d_positions", d_sh, "d_sh") != RTK_OK) return RTK_ERR_INVALID;
    const size_t real_bytes = opts->real_mode == RTK_REAL_F64 ? sizeof(double) : sizeof(float);
    if (check_aligned(d_positions, 8, who, "d_positions") != RTK_OK || check_aligned(d_sh, real_bytes, who, "d_sh") != RTK_OK) return RTK_ERR_INVALID;
    const int rc = check_probe_ctx(who, ctx, true);
    if (rc != RTK_OK || n == 0) return rc;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    const hipStream_t st = static_cast<hipStream_t>(opts->stream);
    rtk_camera cam{};  // what the kernel reads of a camera, as rtk_query_radiance: background, max_depth and the samples per ray
    cam.background = opts->background;
    cam.max_depth = opts->max_depth;
    cam.samples_per_pixel = opts->samples > 0 ? opts->samples : 1;
    const int rays = probe_rays_of(opts);
    return launched(who, opts->real_mode == RTK_REAL_F64
                             ? launch_probe_bake<double>(ctx_view<double>(ctx), device_camera<double>(cam), opts->seed, opts->first_key, rays, opts->time, n, d_positions, d_sh, st)
                             : launch_probe_bake<float>(ctx_view<float>(ctx), device_camera<float>(cam), opts->seed, opts->first_key, rays, opts->time, n, d_positions, d_sh, st));
}

int rtk_probe_rays_host(rtk_ctx* ctx, const rtk_probe_opts* opts, int64_t n, const double* h_positions, rtk_ray* h_rays) {
    const char* who = "rtk_probe_rays_host";
    if (check_probe_args(who, opts, n, h_positions, "h_positions", h_rays, "h_rays") != RTK_OK) return RTK_ERR_INVALID;
    const int rc = check_probe_ctx(who, ctx, false);
    if (rc != RTK_OK || n == 0) return rc;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    HostStaging s(true);
    const int pos = s.piece(size_t(n) * 3 * sizeof(double)), rays = s.piece(size_t(n) * size_t(probe_rays_of(opts)) * sizeof(rtk_ray));
    RTK_HIP(s.alloc());
    RTK_HIP(s.upload(pos, h_positions));
    const int q = rtk_probe_rays(ctx, opts, n, s.ptr<double>(pos), s.ptr<rtk_ray>(rays));
    if (q != RTK_OK) return q;
    hipError_t e = hipStreamSynchronize(static_cast<hipStream_t>(opts->stream));
    if (e == hipSuccess) e = s.download(rays, h_rays);
    return launched(who, e);
}

int rtk_probe_bake_host(rtk_ctx* ctx, const rtk_probe_opts* opts, int64_t n, const double* h_positions, double* h_sh) {
    const char* who = "rtk_probe_bake_host";
    if (check_probe_args(who, opts, n, h_positions, "h_positions", h_sh, "h_sh") != RTK_OK) return RTK_ERR_INVALID;
    const int rc = check_probe_ctx(who, ctx, true);
    if (rc != RTK_OK || n == 0) return rc;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    HostStaging s(opts->real_mode == RTK_REAL_F64);
    const int pos = s.piece(size_t(n) * 3 * sizeof(double)), sh = s.linear(size_t(n) * 3 * RTK_PROBE_COEFFS);
    RTK_HIP(s.alloc());
    RTK_HIP(s.upload(pos, h_positions));
    const int q = rtk_probe_bake(ctx, opts, n, s.ptr<double>(pos), s.ptr<void>(sh));
    if (q != RTK_OK) return q;
    hipError_t e = hipStreamSynchronize(static_cast<hipStream_t>(opts->stream));
    if (e == hipSuccess) e = s.download_linear(sh, h_sh);
    return launched(who, e);
}

}  // extern "C"
