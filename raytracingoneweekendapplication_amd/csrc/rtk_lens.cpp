// rtk_lens.cpp -- the C-ABI half of the lens models (include/rtk.h "Lens models"): rtk_lens_look_at, rtk_lens_rays / _render /
// _aovs / _guides and their _host forms.  Here: the lens's own argument checks, one launch each on the caller's stream, the
// pieces a _host form stages; the checks and the staging every lane-per-ray family shares are rtk_internal.h's.  The kernels
// are rtk_trace.hip's (rtk_lens_rays_kernel, rtk_lens_render_kernel and rtk_guide_kernel with the lens generator), next to the
// radiance query whose path loop they run.
#include <hip/hip_runtime.h>

#include <cmath>

#include "rtk.h"
#include "rtk_internal.h"
#include "rtk_trace.h"

namespace rtk {
namespace {

static_assert(sizeof(rtk_lens) == 312 && sizeof(rtk_camera) == 200, "lens record");

constexpr double kPi = 3.14159265358979323846, kTwoPi = 2.0 * kPi;

bool finite3(const rtk_vec3& v) { return std::isfinite(v.x) && std::isfinite(v.y) && std::isfinite(v.z); }

// What every entry point checks of the lens and opts before it touches a device: null arguments, then the lens, then opts, then
// the sample range.  n_samples = the samples per pixel the call makes (min_samples = the fewest it accepts).  Alignment and the
// context come afterwards.
int check_lens_args(const char* who, const rtk_lens* lens, const rtk_render_opts* opts, int32_t first_sample, int64_t n_samples, int min_samples,
                    const char* samples_name, const void* out, const char* out_name) {
    if (!lens) return fail(RTK_ERR_INVALID, "%s: null lens", who);
    if (!opts) return fail(RTK_ERR_INVALID, "%s: null opts", who);
    if (!out) return fail(RTK_ERR_INVALID, "%s: null %s", who, out_name);
    if (lens->model < RTK_LENS_PERSPECTIVE || lens->model > RTK_LENS_ORTHOGRAPHIC) return fail(RTK_ERR_INVALID, "%s: unknown model %d", who, lens->model);
    if (lens->reserved != 0) return fail(RTK_ERR_INVALID, "%s: reserved must be 0", who);
    const rtk_camera& c = lens->cam;
    if (check_camera_size(who, c) != RTK_OK) return RTK_ERR_INVALID;
    if (c.max_depth < 0) return fail(RTK_ERR_INVALID, "%s: cam.max_depth must not be negative (%d)", who, c.max_depth);
    if (c.samples_per_pixel < 0) return fail(RTK_ERR_INVALID, "%s: cam.samples_per_pixel must not be negative (%d)", who, c.samples_per_pixel);
    const struct { const rtk_vec3& v; const char* name; } vecs[] = {
        {c.background, "cam.background"}, {c.center, "cam.center"}, {c.pixel00_loc, "cam.pixel00_loc"}, {c.pixel_delta_u, "cam.pixel_delta_u"},
        {c.pixel_delta_v, "cam.pixel_delta_v"}, {c.defocus_disk_u, "cam.defocus_disk_u"}, {c.defocus_disk_v, "cam.defocus_disk_v"},
        {lens->u, "u"}, {lens->v, "v"}, {lens->w, "w"}};
    for (const auto& f : vecs)
        if (!finite3(f.v)) return fail(RTK_ERR_INVALID, "%s: %s must be finite", who, f.name);
    const struct { double v; const char* name; } reals[] = {{c.defocus_angle, "cam.defocus_angle"}, {c.pixel_samples_scale, "cam.pixel_samples_scale"},
                                                            {lens->fov_h, "fov_h"}, {lens->fov_v, "fov_v"}, {lens->ortho_width, "ortho_width"},
                                                            {lens->ortho_height, "ortho_height"}};
    for (const auto& f : reals)
        if (!std::isfinite(f.v)) return fail(RTK_ERR_INVALID, "%s: %s must be finite", who, f.name);
    if (lens->fov_h < 0.0 || lens->fov_h > kTwoPi) return fail(RTK_ERR_INVALID, "%s: fov_h must lie in (0, 2 pi], or be 0 for the default (%g)", who, lens->fov_h);
    if (lens->model == RTK_LENS_EQUIRECT && (lens->fov_v < 0.0 || lens->fov_v > kPi))
        return fail(RTK_ERR_INVALID, "%s: fov_v must lie in (0, pi], or be 0 for the default (%g)", who, lens->fov_v);
    if (lens->model == RTK_LENS_ORTHOGRAPHIC) {
        if (!(lens->ortho_width > 0.0)) return fail(RTK_ERR_INVALID, "%s: ortho_width must be positive (%g)", who, lens->ortho_width);
        if (!(lens->ortho_height > 0.0)) return fail(RTK_ERR_INVALID, "%s: ortho_height must be positive (%g)", who, lens->ortho_height);
    }
    if (check_real_mode(who, opts->real_mode) != RTK_OK) return RTK_ERR_INVALID;
    if (opts->n_ranks != 1) return fail(RTK_ERR_INVALID, "%s: whole images only (n_ranks must be 1, not %d)", who, opts->n_ranks);
    if (n_samples < min_samples) return fail(RTK_ERR_INVALID, "%s: %s must be at least %d (%lld)", who, samples_name, min_samples, (long long)n_samples);
    if (first_sample < 0) return fail(RTK_ERR_INVALID, "%s: first_sample must not be negative (%d)", who, first_sample);
    if (int64_t(c.image_width) * c.image_height * n_samples > int64_t(0x7FFFFFFF))
        return fail(RTK_ERR_INVALID, "%s: H * W * %s must not exceed 2^31 - 1 (%d x %d x %lld)", who, samples_name, c.image_height, c.image_width, (long long)n_samples);
    return RTK_OK;
}

// What the kernels read of the lens besides its camera: the halves of the extents, defaults resolved (rtk_trace.h).
LensRec lens_record(const rtk_lens& l) {
    LensRec r{};
    const rtk_vec3* src[4] = {&l.cam.center, &l.u, &l.v, &l.w};
    double* dst[4] = {r.center, r.u, r.v, r.w};
    for (int k = 0; k < 4; k++) {
        dst[k][0] = src[k]->x;
        dst[k][1] = src[k]->y;
        dst[k][2] = src[k]->z;
    }
    r.model = l.model;
    if (l.model == RTK_LENS_ORTHOGRAPHIC) {
        r.half_h = l.ortho_width / 2;
        r.half_v = l.ortho_height / 2;
    } else {
        r.half_h = (l.fov_h != 0.0 ? l.fov_h : (l.model == RTK_LENS_FISHEYE ? kPi : kTwoPi)) / 2;
        r.half_v = (l.fov_v != 0.0 ? l.fov_v : kPi) / 2;
    }
    return r;
}

// vec3.h's operations in their order (host/rtk_math.h): length_squared (x x + y y) + z z, unit_vector = (1 / length) * v.
rtk_vec3 sub(rtk_vec3 a, rtk_vec3 b) { return rtk_vec3{a.x - b.x, a.y - b.y, a.z - b.z}; }
rtk_vec3 cross(rtk_vec3 a, rtk_vec3 b) { return rtk_vec3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
rtk_vec3 unit_vector(rtk_vec3 a) {
    const double t = 1 / std::sqrt(a.x * a.x + a.y * a.y + a.z * a.z);
    return rtk_vec3{t * a.x, t * a.y, t * a.z};
}

}  // namespace
}  // namespace rtk

using namespace rtk;

extern "C" {

int rtk_lens_look_at(rtk_lens* lens, rtk_vec3 lookfrom, rtk_vec3 lookat, rtk_vec3 vup) {
    if (!lens) return fail(RTK_ERR_INVALID, "rtk_lens_look_at: null lens");
    lens->cam.center = lookfrom;
    lens->w = unit_vector(sub(lookfrom, lookat));
    lens->u = unit_vector(cross(vup, lens->w));
    lens->v = cross(lens->w, lens->u);
    return RTK_OK;
}

int rtk_lens_rays(rtk_ctx* ctx, const rtk_lens* lens, const rtk_render_opts* opts, int32_t first_sample, int32_t n_samples, rtk_ray* d_rays) {
    const char* who = "rtk_lens_rays";
    if (check_lens_args(who, lens, opts, first_sample, n_samples, 0, "n_samples", d_rays, "d_rays") != RTK_OK) return RTK_ERR_INVALID;
    if (check_aligned(d_rays, 8, who, "d_rays") != RTK_OK) return RTK_ERR_INVALID;
    const int rc = check_ctx(who, ctx, false);
    if (rc != RTK_OK || n_samples == 0) return rc;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    const hipStream_t st = static_cast<hipStream_t>(opts->stream);
    const LensRec rec = lens_record(*lens);
    return launched(who, with_real(opts->real_mode, [&](auto real) {
        return launch_lens_rays(rec, device_camera<decltype(real)>(lens->cam), opts->seed, uint32_t(first_sample), n_samples, d_rays, st);
    }));
}

int rtk_lens_render(rtk_ctx* ctx, const rtk_lens* lens, const rtk_render_opts* opts, int32_t first_sample, void* d_linear, float* d_noise) {
    const char* who = "rtk_lens_render";
    if (check_lens_args(who, lens, opts, first_sample, lens ? lens->cam.samples_per_pixel : 0, 1, "cam.samples_per_pixel", d_linear, "d_linear") != RTK_OK)
        return RTK_ERR_INVALID;
    const size_t real_bytes = opts->real_mode == RTK_REAL_F64 ? sizeof(double) : sizeof(float);
    if (check_aligned(d_linear, real_bytes, who, "d_linear") != RTK_OK || check_aligned(d_noise, 4, who, "d_noise") != RTK_OK) return RTK_ERR_INVALID;
    const int rc = check_ctx(who, ctx, true);
    if (rc != RTK_OK) return rc;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    const hipStream_t st = static_cast<hipStream_t>(opts->stream);
    const LensRec rec = lens_record(*lens);
    return launched(who, with_real(opts->real_mode, [&](auto real) {
        using R = decltype(real);
        return launch_lens_render(ctx_view<R>(ctx), rec, device_camera<R>(lens->cam), opts->seed, uint32_t(first_sample), d_linear, d_noise, st);
    }));
}

int rtk_lens_aovs(rtk_ctx* ctx, const rtk_lens* lens, const rtk_render_opts* opts, int32_t n_samples, float* d_aov) {
    const char* who = "rtk_lens_aovs";
    if (check_lens_args(who, lens, opts, 0, n_samples, 1, "n_samples", d_aov, "d_aov") != RTK_OK) return RTK_ERR_INVALID;
    if (check_aligned16(d_aov, who, "d_aov") != RTK_OK) return RTK_ERR_INVALID;
    const int rc = check_ctx(who, ctx, true);
    if (rc != RTK_OK) return rc;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    const hipStream_t st = static_cast<hipStream_t>(opts->stream);
    const LensRec rec = lens_record(*lens);
    return launched(who, with_real(opts->real_mode, [&](auto real) {
        using R = decltype(real);
        return launch_lens_aov(ctx_view<R>(ctx), rec, device_camera<R>(lens->cam), opts->seed, n_samples, d_aov, st);
    }));
}

int rtk_lens_guides(rtk_ctx* ctx, const rtk_lens* lens, const rtk_render_opts* opts, int32_t n_samples, const rtk_guide_opts* gopts, float* d_guides) {
    const char* who = "rtk_lens_guides";
    int follow = 0, max_bounces = 0;
    if (resolve_guide_opts(gopts, &follow, &max_bounces, who) != RTK_OK) return RTK_ERR_INVALID;
    if (check_lens_args(who, lens, opts, 0, n_samples, 1, "n_samples", d_guides, "d_guides") != RTK_OK) return RTK_ERR_INVALID;
    if (n_samples > (1 << 20)) return fail(RTK_ERR_INVALID, "%s: n_samples must be 1 .. 2^20 (%d)", who, n_samples);
    if (check_aligned16(d_guides, who, "d_guides") != RTK_OK) return RTK_ERR_INVALID;
    const int rc = check_ctx(who, ctx, true);
    if (rc != RTK_OK) return rc;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    const hipStream_t st = static_cast<hipStream_t>(opts->stream);
    const LensRec rec = lens_record(*lens);
    return launched(who, with_real(opts->real_mode, [&](auto real) {
        using R = decltype(real);
        return launch_lens_guides(ctx_view<R>(ctx), rec, device_camera<R>(lens->cam), opts->seed, n_samples, follow, max_bounces, d_guides, st);
    }));
}

int rtk_lens_rays_host(rtk_ctx* ctx, const rtk_lens* lens, const rtk_render_opts* opts, int32_t first_sample, int32_t n_samples, rtk_ray* h_rays) {
    const char* who = "rtk_lens_rays_host";
    if (check_lens_args(who, lens, opts, first_sample, n_samples, 0, "n_samples", h_rays, "h_rays") != RTK_OK) return RTK_ERR_INVALID;
    const int rc = check_ctx(who, ctx, false);
    if (rc != RTK_OK || n_samples == 0) return rc;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    HostStaging s(true);
    const int rays = s.piece(size_t(lens->cam.image_width) * lens->cam.image_height * n_samples * sizeof(rtk_ray));
    return run_host_form(who, static_cast<hipStream_t>(opts->stream), s, {},
                         [&] { return rtk_lens_rays(ctx, lens, opts, first_sample, n_samples, s.ptr<rtk_ray>(rays)); }, {{rays, h_rays}});
}

int rtk_lens_render_host(rtk_ctx* ctx, const rtk_lens* lens, const rtk_render_opts* opts, int32_t first_sample, double* h_linear, float* h_noise) {
    const char* who = "rtk_lens_render_host";
    if (check_lens_args(who, lens, opts, first_sample, lens ? lens->cam.samples_per_pixel : 0, 1, "cam.samples_per_pixel", h_linear, "h_linear") != RTK_OK)
        return RTK_ERR_INVALID;
    const int rc = check_ctx(who, ctx, true);
    if (rc != RTK_OK) return rc;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    HostStaging s(opts->real_mode == RTK_REAL_F64);
    const size_t px = size_t(lens->cam.image_width) * lens->cam.image_height;
    const int linear = s.linear(px * 3), noise = s.piece(px * sizeof(float), h_noise != nullptr);
    return run_host_form(who, static_cast<hipStream_t>(opts->stream), s, {},
                         [&] { return rtk_lens_render(ctx, lens, opts, first_sample, s.ptr<void>(linear), s.ptr<float>(noise)); },
                         {{linear, h_linear, true}, {noise, h_noise}});
}

int rtk_lens_aovs_host(rtk_ctx* ctx, const rtk_lens* lens, const rtk_render_opts* opts, int32_t n_samples, float* h_aov) {
    const char* who = "rtk_lens_aovs_host";
    if (check_lens_args(who, lens, opts, 0, n_samples, 1, "n_samples", h_aov, "h_aov") != RTK_OK) return RTK_ERR_INVALID;
    const int rc = check_ctx(who, ctx, true);
    if (rc != RTK_OK) return rc;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    HostStaging s(true);
    const int aov = s.piece(size_t(lens->cam.image_width) * lens->cam.image_height * 8 * sizeof(float));
    return run_host_form(who, static_cast<hipStream_t>(opts->stream), s, {}, [&] { return rtk_lens_aovs(ctx, lens, opts, n_samples, s.ptr<float>(aov)); },
                         {{aov, h_aov}});
}

int rtk_lens_guides_host(rtk_ctx* ctx, const rtk_lens* lens, const rtk_render_opts* opts, int32_t n_samples, const rtk_guide_opts* gopts, float* h_guides) {
    const char* who = "rtk_lens_guides_host";
    int follow = 0, max_bounces = 0;
    if (resolve_guide_opts(gopts, &follow, &max_bounces, who) != RTK_OK) return RTK_ERR_INVALID;
    if (check_lens_args(who, lens, opts, 0, n_samples, 1, "n_samples", h_guides, "h_guides") != RTK_OK) return RTK_ERR_INVALID;
    if (n_samples > (1 << 20)) return fail(RTK_ERR_INVALID, "%s: n_samples must be 1 .. 2^20 (%d)", who, n_samples);
    const int rc = check_ctx(who, ctx, true);
    if (rc != RTK_OK) return rc;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    HostStaging s(true);
    const int guides = s.piece(size_t(lens->cam.image_width) * lens->cam.image_height * 16 * sizeof(float));
    return run_host_form(who, static_cast<hipStream_t>(opts->stream), s, {},
                         [&] { return rtk_lens_guides(ctx, lens, opts, n_samples, gopts, s.ptr<float>(guides)); }, {{guides, h_guides}});
}

}  // extern "C"
