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
    const bool allow_lds = (variant & 1) == 0;
    const uint32_t diag = uint32_t(variant) & 0xBFFF00u;  // (rtk_kernel_name's reading of the variant word)
    bool view = false;
    const char* n = real_mode == RTK_REAL_F64 ? view_kernel_name<double>(ctx_view<double>(ctx), ctx_features(ctx), allow_lds, diag, &view)
                                              : view_kernel_name<float>(ctx_view<float>(ctx), ctx_features(ctx), allow_lds, diag, &view);
    if (name) *name = n;
    return view && !count;
}

extern "C" {

int rtk_render_views(rtk_ctx* ctx, int32_t n_views, const rtk_camera* h_cams, const uint32_t* h_seeds, const rtk_render_opts* opts, void* d_linear,
                     uint8_t* d_rgb8, rtk_work_counters* d_counters) {
    if (!ctx || !h_cams || !opts) return fail(RTK_ERR_INVALID, "rtk_render_views: null argument");
    uint64_t digest = 0;
    if (!ctx_scene(ctx, &digest)) return fail(RTK_ERR_NO_SCENE, "rtk_render_views: no scene uploaded");
    if (n_views < 1 || n_views > 65536) return fail(RTK_ERR_INVALID, "rtk_render_views: n_views %d out of range (1..65536)", n_views);
    const rtk_camera& c0 = h_cams[0];
    if (c0.image_width <= 0 || c0.image_height <= 0 || c0.samples_per_pixel <= 0 || c0.samples_per_pixel > 32767)
        return fail(RTK_ERR_INVALID, "rtk_render_views: bad camera dimensions (samples_per_pixel must be 1..32767)");
    for (int32_t v = 0; v < n_views; v++) {
        const rtk_camera& c = h_cams[v];
        if (c.image_width != c0.image_width || c.image_height != c0.image_height || c.samples_per_pixel != c0.samples_per_pixel ||
            c.pixel_samples_scale != c0.pixel_samples_scale)
            return fail(RTK_ERR_INVALID, "rtk_render_views: view %d differs from view 0 in image_width, image_height, samples_per_pixel or pixel_samples_scale", v);
        if (c.max_depth < 0) return fail(RTK_ERR_INVALID, "rtk_render_views: view %d has a negative max_depth", v);
    }
    if (opts->n_ranks != 1 || opts->rank != 0)
        return fail(RTK_ERR_INVALID, "rtk_render_views renders whole views (n_ranks must be 1, got rank %d of %d)", opts->rank, opts->n_ranks);
    if (opts->variant & (1 << 22)) return fail(RTK_ERR_INVALID, "rtk_render_views: variant bit 22 (compact tile buffers) does not apply to a batch");
    if (opts->count_work && !d_counters) return fail(RTK_ERR_INVALID, "rtk_render_views: count_work needs d_counters");
    if (opts->real_mode != RTK_REAL_F64 && opts->real_mode != RTK_REAL_F32) return fail(RTK_ERR_INVALID, "rtk_render_views: unknown real_mode %d", opts->real_mode);
    const int64_t tiles = rtk_tiles_per_rank(c0.image_width, c0.image_height, 1);
    const int chunks = frame_chunk_count(c0.samples_per_pixel, opts->variant);
    if (int64_t(n_views) * tiles * chunks > int64_t(INT_MAX))
        return fail(RTK_ERR_INVALID, "rtk_render_views: %d views x %lld tiles x %d sample chunks are more work items than fit in 31 bits", n_views, (long long)tiles,
                    chunks);
    const size_t elem = opts->real_mode == RTK_REAL_F64 ? sizeof(double) : sizeof(float);
    const size_t view_values = size_t(c0.image_width) * size_t(c0.image_height) * 3;
    if (!batch_uses_view_kernel(ctx, opts->real_mode, opts->variant, opts->count_work != 0, nullptr)) {
        // The per-view form: one plain frame per view into the view's plane -- the same bits by construction; counters add up.
        for (int32_t v = 0; v < n_views; v++) {
            rtk_render_opts o = *opts;
            if (h_seeds) o.seed = h_seeds[v];
            void* lin = d_linear ? static_cast<char*>(d_linear) + size_t(v) * view_values * elem : nullptr;
            uint8_t* rgb = d_rgb8 ? d_rgb8 + size_t(v) * view_values : nullptr;
            if (const int rc = render_frame_apart(ctx, &h_cams[v], &o, lin, rgb, d_counters); rc != RTK_OK) return rc;
        }
        return RTK_OK;
    }
    ViewBatch b;
    if (const int rc = stage_view_batch(ctx, n_views, h_cams, h_seeds, opts, b); rc != RTK_OK) return rc;
    hipError_t e = hipSuccess;
    void* const acc = b.n_passes > 1 ? static_cast<char*>(b.d_partial) + b.plane * size_t(b.planes_per_pass) : nullptr;
    for (int pass = 0; pass < b.n_passes && e == hipSuccess; pass++) {
        const int k0 = pass * b.planes_per_pass, k1 = std::min(b.tm.n_chunks, k0 + b.planes_per_pass);
        TileMap tp = b.tm;  // this pass's chunks, numbered from 0 (as rtk_render_device's passes)
        tp.n_chunks = k1 - k0;
        for (int k = 0; k <= kMaxChunks; k++) tp.chunk_start[k] = b.tm.chunk_start[std::min(k0 + k, int(b.tm.n_chunks))];
        const bool first = pass == 0, last = pass + 1 == b.n_passes;
        if (opts->real_mode == RTK_REAL_F64) {
            e = launch_view_batch<double>(ctx_view<double>(ctx), static_cast<const ViewRec<double>*>(b.d_views), tp, ctx_features(ctx), b.allow_lds, b.diag,
                                          b.d_partial, b.pass_counter[pass], b.stream);
            if (e == hipSuccess)
                e = launch_resolve_views<double>(b.d_partial, tp, c0.image_width, c0.image_height, c0.pixel_samples_scale, d_linear, d_rgb8, acc, first, last, b.stream);
        } else {
            e = launch_view_batch<float>(ctx_view<float>(ctx), static_cast<const ViewRec<float>*>(b.d_views), tp, ctx_features(ctx), b.allow_lds, b.diag, b.d_partial,
                                         b.pass_counter[pass], b.stream);
            if (e == hipSuccess)
                e = launch_resolve_views<float>(b.d_partial, tp, c0.image_width, c0.image_height, c0.pixel_samples_scale, d_linear, d_rgb8, acc, first, last, b.stream);
        }
    }
    if (e != hipSuccess) return fail(RTK_ERR_HIP, "view batch launch failed: %s", hipGetErrorString(e));
    return RTK_OK;
}

int rtk_render_views_host(rtk_ctx* ctx, int32_t n_views, const rtk_camera* h_cams, const uint32_t* h_seeds, const rtk_render_opts* opts, double* h_linear,
                          uint8_t* h_rgb8, rtk_work_counters* counters) {
    if (!ctx || !h_cams || !opts) return fail(RTK_ERR_INVALID, "rtk_render_views_host: null argument");
    if (n_views < 1 || n_views > 65536) return fail(RTK_ERR_INVALID, "rtk_render_views_host: n_views %d out of range (1..65536)", n_views);
    if (h_cams[0].image_width <= 0 || h_cams[0].image_height <= 0) return fail(RTK_ERR_INVALID, "rtk_render_views_host: bad camera dimensions");
    if (const hipError_t sd = hipSetDevice(ctx_device(ctx)); sd != hipSuccess) return fail(RTK_ERR_HIP, "rtk_render_views_host: hipSetDevice failed: %s", hipGetErrorString(sd));
    const size_t n =size_t(n_views) * size_t(h_cams[0].image_width) * size_t(h_cams[0].image_height) * 3;
    const bool f64 = opts->real_mode == RTK_REAL_F64;
    void* d_linear = nullptr;
    uint8_t* d_rgb8 = nullptr;
    rtk_work_counters* d_cnt = nullptr;
    rtk_render_opts o = *opts;
    o.count_work = counters ? 1 : 0;
    hipStream_t stream = static_cast<hipStream_t>(o.stream);
    hipError_t e = hipMalloc(&d_linear, n * (f64 ? sizeof(double) : sizeof(float)));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_rgb8), n);
    if (e == hipSuccess && counters) e = hipMalloc(reinterpret_cast<void**>(&d_cnt), sizeof(rtk_work_counters));
    if (e == hipSuccess && counters) e = hipMemsetAsync(d_cnt, 0, sizeof(rtk_work_counters), stream);
    int rc = e == hipSuccess ? RTK_OK : fail(RTK_ERR_HIP, "rtk_render_views_host: device allocation failed: %s", hipGetErrorString(e));
    if (rc == RTK_OK) rc = rtk_render_views(ctx, n_views, h_cams, h_seeds, &o, d_linear, d_rgb8, d_cnt);
    if (rc == RTK_OK) rc = wait_with_progress(&ctx, &stream, 1);
    if (rc == RTK_OK) {
        if (h_linear && f64) e = hipMemcpy(h_linear, d_linear, n * sizeof(double), hipMemcpyDeviceToHost);
        if (h_linear && !f64) {
            std::vector<float> tmp(n);
            e = hipMemcpy(tmp.data(), d_linear, n * sizeof(float), hipMemcpyDeviceToHost);
            for (size_t k = 0; k < n; k++) h_linear[k] = double(tmp[k]);
        }
        if (e == hipSuccess && h_rgb8) e = hipMemcpy(h_rgb8, d_rgb8, n, hipMemcpyDeviceToHost);
        if (e == hipSuccess && counters) e = hipMemcpy(counters, d_cnt, sizeof(rtk_work_counters), hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(RTK_ERR_HIP, "rtk_render_views_host: copy to the host failed: %s", hipGetErrorString(e));
    }
    if (d_linear) (void)hipFree(d_linear);
    if (d_rgb8) (void)hipFree(d_rgb8);
    if (d_cnt) (void)hipFree(d_cnt);
    return rc;
}

const char* rtk_view_kernel_name(rtk_ctx* ctx, int real_mode, int variant) {
    uint64_t digest = 0;
    if (!ctx || !ctx_scene(ctx, &digest)) return "";
    const char* name = "";
    (void)batch_uses_view_kernel(ctx, real_mode, variant, false, &name);
    return name;
}

}  // extern "C"
