// rtk_probe.cpp -- the C-ABI half of the light probes' ray side (include/rtk.h "Light probes"): rtk_probe_rays and
// rtk_probe_bake with their _host forms.  Here: the probes' own argument checks, one launch each on the caller's stream, the
// pieces a _host form stages; the checks and the staging every lane-per-ray family shares are rtk_internal.h's.  The kernels
// are rtk_trace.hip's (rtk_probe_rays_kernel, rtk_probe_bake_kernel), next to the radiance query whose path loop they run; the
// lookup (rtk_probe_irradiance) is rtk_probe.hip.
#include <hip/hip_runtime.h>

#include "rtk.h"
#include "rtk_internal.h"
#include "rtk_trace.h"

namespace rtk {
namespace {

static_assert(sizeof(rtk_probe_opts) == 72 && sizeof(rtk_probe_grid) == 64, "light probe records");

int probe_rays_of(const rtk_probe_opts* opts) { return opts->rays != 0 ? opts->rays : 1024; }

// What both entry points and their _host forms check before they touch a device; alignment and the context come afterwards.
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

}  // namespace
}  // namespace rtk

using namespace rtk;

extern "C" {

int rtk_probe_rays(rtk_ctx* ctx, const rtk_probe_opts* opts, int64_t n, const double* d_positions, rtk_ray* d_rays) {
    const char* who = "rtk_probe_rays";
    if (check_probe_args(who, opts, n, d_positions, "d_positions", d_rays, "d_rays") != RTK_OK) return RTK_ERR_INVALID;
    if (check_aligned(d_positions, 8, who, "d_positions") != RTK_OK || check_aligned(d_rays, 8, who, "d_rays") != RTK_OK) return RTK_ERR_INVALID;
    const int rc = check_ctx(who, ctx, false);
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
    const int rc = check_ctx(who, ctx, true);
    if (rc != RTK_OK || n == 0) return rc;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    const hipStream_t st = static_cast<hipStream_t>(opts->stream);
    const rtk_camera cam = path_camera(opts->background, opts->max_depth, opts->samples);
    const int rays = probe_rays_of(opts);
    return launched(who, with_real(opts->real_mode, [&](auto real) {
        using R = decltype(real);
        return launch_probe_bake(ctx_view<R>(ctx), device_camera<R>(cam), opts->seed, opts->first_key, rays, opts->time, n, d_positions, d_sh, st);
    }));
}

int rtk_probe_rays_host(rtk_ctx* ctx, const rtk_probe_opts* opts, int64_t n, const double* h_positions, rtk_ray* h_rays) {
    const char* who = "rtk_probe_rays_host";
    if (check_probe_args(who, opts, n, h_positions, "h_positions", h_rays, "h_rays") != RTK_OK) return RTK_ERR_INVALID;
    const int rc = check_ctx(who, ctx, false);
    if (rc != RTK_OK || n == 0) return rc;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    HostStaging s(true);
    const int pos = s.piece(size_t(n) * 3 * sizeof(double)), rays = s.piece(size_t(n) * size_t(probe_rays_of(opts)) * sizeof(rtk_ray));
    return run_host_form(who, static_cast<hipStream_t>(opts->stream), s, {{pos, h_positions}},
                         [&] { return rtk_probe_rays(ctx, opts, n, s.ptr<double>(pos), s.ptr<rtk_ray>(rays)); }, {{rays, h_rays}});
}

int rtk_probe_bake_host(rtk_ctx* ctx, const rtk_probe_opts* opts, int64_t n, const double* h_positions, double* h_sh) {
    const char* who = "rtk_probe_bake_host";
    if (check_probe_args(who, opts, n, h_positions, "h_positions", h_sh, "h_sh") != RTK_OK) return RTK_ERR_INVALID;
    const int rc = check_ctx(who, ctx, true);
    if (rc != RTK_OK || n == 0) return rc;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    HostStaging s(opts->real_mode == RTK_REAL_F64);
    const int pos = s.piece(size_t(n) * 3 * sizeof(double)), sh = s.linear(size_t(n) * 3 * RTK_PROBE_COEFFS);
    return run_host_form(who, static_cast<hipStream_t>(opts->stream), s, {{pos, h_positions}},
                         [&] { return rtk_probe_bake(ctx, opts, n, s.ptr<double>(pos), s.ptr<void>(sh)); }, {{sh, h_sh, true}});
}

}  // extern "C"
