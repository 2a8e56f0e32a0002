// rtk_views.hip -- view batches (include/rtk.h "View batches"): the entry points rtk_render_views / _host and
// rtk_view_kernel_name, and the resolve of rtk_view_batch_kernel's partial sums partial[chunk][view * tiles + tile][3][64] into the
// planes [view][H][W][3] of the batch's outputs.  The kernel that traces the batch is rtk_trace.hip's (the render kernel's body
// with a camera per lane); what is added here per pixel is rtk_frame_steps.h's, so a view is the single frame bit for bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <vector>

#include "rtk.h"
#include "rtk_device_layout.h"
#include "rtk_device_math.h"
#include "rtk_frame_steps.h"
#include "rtk_internal.h"
#include "rtk_trace.h"

namespace rtk {

// rtk_resolve_kernel over the tiles [view][tile] of a batch: one thread per (tile of the batch, pixel), the fold over this
// pass's chunks, the running sum carried in `acc` [view * tiles + tile][3][64] between passes, and on the last pass the pixel
// scaled by 1 / spp and written at (i, j) of its view's plane.
template <typename real>
__global__ __launch_bounds__(256) void rtk_resolve_views_kernel(const real* __restrict__ partial, TileMap tmap, int tiles_per_view, int width, int height,
                                                                 real samples_scale, real* __restrict__ out_linear, uint8_t* __restrict__ out_rgb8,
                                                                 real* __restrict__ acc, int first_pass, int last_pass) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    PixelSlot p;
    p.pix = int(gid & 63);
    p.local_tile = gid >> 6;
    if (p.local_tile >= tmap.n_tiles_local) return;
    const long long view = p.local_tile / tiles_per_view;
    const int tile = int(p.local_tile % tiles_per_view);
    p.i = (tile % tmap.tiles_x) * 8 + (p.pix & 7);
    p.j = (tile / tmap.tiles_x) * 8 + (p.pix >> 3);
    p.in_grid = true;
    p.inside = p.i < width && p.j < height;
    if (!p.inside) return;
    V3<real> sum = fold_planes<false>(partial, tmap, p, first_pass != 0, acc);
    if (!last_pass) {
        store3(acc + p.plane(), sum);
        return;
    }
    sum = scale(samples_scale, sum);
    const size_t at = size_t(view) * size_t(height) * size_t(width) * 3;
    write_pixel<real>(p, false, width, sum, 0.0, out_linear ? out_linear + at : nullptr, out_rgb8 ? out_rgb8 + at : nullptr, nullptr);
}

template <typename real>
hipError_t launch_resolve_views(const void* partial, const TileMap& tmap, int width, int height, double samples_scale, void* out_linear, uint8_t* out_rgb8,
                                void* acc, bool first_pass, bool last_pass, hipStream_t stream) {
    if (tmap.n_tiles_local <= 0) return hipSuccess;
    rtk_resolve_views_kernel<real><<<dim3(pixel_slot_blocks(tmap)), dim3(256), 0, stream>>>(static_cast<const real*>(partial), tmap, tmap.tiles_x * tmap.tiles_y, width,
                                                                                           height, real(samples_scale), static_cast<real*>(out_linear), out_rgb8,
                                                                                           static_cast<real*>(acc), first_pass ? 1 : 0, last_pass ? 1 : 0);
    return hipGetLastError();
}
template hipError_t launch_resolve_views<double>(const void*, const TileMap&, int, int, double, void*, uint8_t*, void*, bool, bool, hipStream_t);
template hipError_t launch_resolve_views<float>(const void*, const TileMap&, int, int, double, void*, uint8_t*, void*, bool, bool, hipStream_t);

}  // namespace rtk

using namespace rtk;

// What a batch dispatches for these options: the view kernel, or (false) the plain kernel once per view.
static bool batch_uses_view_kernel(const rtk_ctx* ctx, int real_mode, int variant, bool count, const char** name) {
    const Variant v = decode_variant(variant);
    bool view = false;
    const char* n = with_real(real_mode, [&](auto real) {
        return view_kernel_name<decltype(real)>(ctx_view<decltype(real)>(ctx), ctx_features(ctx), v.allow_lds, v.diag, &view);
    });
    if (name) *name = n;
    return view && !count;
}

extern "C" {

int rtk_render_views(rtk_ctx* ctx, int32_t n_views, const rtk_camera* h_cams, const uint32_t* h_seeds, const rtk_render_opts* opts, void* d_linear,
                     uint8_t* d_rgb8, rtk_work_counters* d_counters) {
    const char* who = "rtk_render_views";
    if (!ctx || !h_cams || !opts) return fail(RTK_ERR_INVALID, "%s: null argument", who);
    uint64_t digest = 0;
    if (!ctx_scene(ctx, &digest)) return fail(RTK_ERR_NO_SCENE, "%s: no scene uploaded", who);
    if (n_views < 1 || n_views > 65536) return fail(RTK_ERR_INVALID, "%s: n_views %d out of range (1..65536)", who, n_views);
    const rtk_camera& c0 = h_cams[0];
    if (c0.image_width <= 0 || c0.image_height <= 0 || c0.samples_per_pixel <= 0 || c0.samples_per_pixel > 32767)  // (max_depth: per view, below)
        return fail(RTK_ERR_INVALID, "%s: bad camera dimensions (samples_per_pixel must be 1..32767)", who);
    for (int32_t v = 0; v < n_views; v++) {
        const rtk_camera& c = h_cams[v];
        if (c.image_width != c0.image_width || c.image_height != c0.image_height || c.samples_per_pixel != c0.samples_per_pixel ||
            c.pixel_samples_scale != c0.pixel_samples_scale)
            return fail(RTK_ERR_INVALID, "%s: view %d differs from view 0 in image_width, image_height, samples_per_pixel or pixel_samples_scale", who, v);
        if (c.max_depth < 0) return fail(RTK_ERR_INVALID, "%s: view %d has a negative max_depth", who, v);
    }
    if (opts->n_ranks != 1 || opts->rank != 0)
        return fail(RTK_ERR_INVALID, "rtk_render_views renders whole views (n_ranks must be 1, got rank %d of %d)", opts->rank, opts->n_ranks);
    if (decode_variant(opts->variant).compact) return fail(RTK_ERR_INVALID, "%s: variant bit 22 (compact tile buffers) does not apply to a batch", who);
    if (opts->count_work && !d_counters) return fail(RTK_ERR_INVALID, "%s: count_work needs d_counters", who);
    if (check_real_mode(who, opts->real_mode) != RTK_OK) return RTK_ERR_INVALID;
    const FramePlan one = plan_frame(c0, *opts), f = plan_views(one, n_views);
    if (f.n_items() > int64_t(INT_MAX))
        return fail(RTK_ERR_INVALID, "%s: %d views x %lld tiles x %d sample chunks are more work items than fit in 31 bits", who, n_views, (long long)one.n_tiles,
                    one.tm.n_chunks);
    const size_t view_values = size_t(c0.image_width) * size_t(c0.image_height) * 3;
    if (!batch_uses_view_kernel(ctx, opts->real_mode, opts->variant, opts->count_work != 0, nullptr)) {
        // The per-view form: one plain frame per view into the view's plane -- the same bits by construction; counters add up.
        for (int32_t v = 0; v < n_views; v++) {
            rtk_render_opts o = *opts;
            if (h_seeds) o.seed = h_seeds[v];
            void* lin = d_linear ? static_cast<char*>(d_linear) + size_t(v) * view_values * f.elem : nullptr;
            uint8_t* rgb = d_rgb8 ? d_rgb8 + size_t(v) * view_values : nullptr;
            if (const int rc = render_frame_apart(ctx, &h_cams[v], &o, lin, rgb, d_counters); rc != RTK_OK) return rc;
        }
        return RTK_OK;
    }
    ViewBatch b;
    if (const int rc = stage_view_batch(ctx, f, n_views, h_cams, h_seeds, opts, b); rc != RTK_OK) return rc;
    hipError_t e = hipSuccess;
    for (int k = 0; k < f.n_passes && e == hipSuccess; k++) {
        const FramePass p = frame_pass(f, k, b.d_partial);
        e = with_real(opts->real_mode, [&](auto real) {
            using R = decltype(real);
            const hipError_t le = launch_view_batch<R>(ctx_view<R>(ctx), static_cast<const ViewRec<R>*>(b.d_views), p.tm, ctx_features(ctx), f.variant.allow_lds,
                                                       f.variant.diag, b.d_partial, b.pass_counter[k], f.stream);
            return le != hipSuccess ? le
                                    : launch_resolve_views<R>(b.d_partial, p.tm, c0.image_width, c0.image_height, c0.pixel_samples_scale, d_linear, d_rgb8, p.acc,
                                                              p.first, p.last, f.stream);
        });
    }
    if (e != hipSuccess) return fail(RTK_ERR_HIP, "view batch launch failed: %s", hipGetErrorString(e));
    return RTK_OK;
}

int rtk_render_views_host(rtk_ctx* ctx, int32_t n_views, const rtk_camera* h_cams, const uint32_t* h_seeds, const rtk_render_opts* opts, double* h_linear,
                          uint8_t* h_rgb8, rtk_work_counters* counters) {
    const char* who = "rtk_render_views_host";
    if (!ctx || !h_cams || !opts) return fail(RTK_ERR_INVALID, "%s: null argument", who);
    if (n_views < 1 || n_views > 65536) return fail(RTK_ERR_INVALID, "%s: n_views %d out of range (1..65536)", who, n_views);
    if (h_cams[0].image_width <= 0 || h_cams[0].image_height <= 0) return fail(RTK_ERR_INVALID, "%s: bad camera dimensions", who);
    if (const hipError_t sd = hipSetDevice(ctx_device(ctx)); sd != hipSuccess) return fail(RTK_ERR_HIP, "%s: hipSetDevice failed: %s", who, hipGetErrorString(sd));
    const size_t n = size_t(n_views) * size_t(h_cams[0].image_width) * size_t(h_cams[0].image_height) * 3;
    HostStaging s(opts->real_mode == RTK_REAL_F64);
    const int lin = s.linear(n), rgb8 = s.piece(n), cnt = s.piece(sizeof(rtk_work_counters), counters != nullptr);
    rtk_render_opts o = *opts;
    o.count_work = counters ? 1 : 0;
    hipStream_t stream = static_cast<hipStream_t>(o.stream);
    return run_host_form_waiting(
        who, s, {},
        [&] {
            const hipError_t e = counters ? hipMemsetAsync(s.ptr(cnt), 0, sizeof(rtk_work_counters), stream) : hipSuccess;
            return e != hipSuccess ? launched(who, e)
                                   : rtk_render_views(ctx, n_views, h_cams, h_seeds, &o, s.ptr(lin), s.ptr<uint8_t>(rgb8), s.ptr<rtk_work_counters>(cnt));
        },
        [&] { return wait_with_progress(&ctx, &stream, 1); }, {{lin, h_linear, true}, {rgb8, h_rgb8}, {cnt, counters}});
}

const char* rtk_view_kernel_name(rtk_ctx* ctx, int real_mode, int variant) {
    uint64_t digest = 0;
    if (!ctx || !ctx_scene(ctx, &digest)) return "";
    const char* name = "";
    (void)batch_uses_view_kernel(ctx, real_mode, variant, false, &name);
    return name;
}

}  // extern "C"

