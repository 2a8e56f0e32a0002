// rtk_tiles.hip -- tile lists (include/rtk.h, "Tile lists"): rtk_tiles_select, the kernel that turns per-pixel maps into per-tile
// flags; rtk_render_tiles, which renders the flagged tiles with the render kernel over a compacted list (the frame set-up is
// rtk_frame_host.cpp's stage_tile_frame, the list's kernels are rtk_frame.hip's); and their _host forms.  Hand-written HIP for gfx950, wave64.
//
// Layout.  One wave per 8x8 tile on the image passes' grid (rtk_image_pass.h), four tiles per 256-thread block.  A tile is
// flagged when a raw-flagged pixel lies in its window: its in-image pixels grown by r = dilate on every side and clipped to the
// image, at most 24 x 24 pixels.  The wave's lanes walk the window 64 positions at a time in row-major order (at most nine
// rounds), each lane tests its pixels with the two comparisons of the rule, one __ballot decides, and lane 0 stores the flag.
// Neighbouring tiles' windows overlap, so a map value is read by up to nine waves: the second to ninth reads are L2 hits, and
// the whole pass moves 4 (or 8) bytes per pixel from memory -- nothing worth staging.
//
// Arithmetic.  Two float comparisons per pixel, integers otherwise; no atomics: the same inputs give the same flags.
#include <hip/hip_runtime.h>

#include <cmath>

#include "rtk.h"
#include "rtk_image_pass.h"
#include "rtk_internal.h"
#include "rtk_trace.h"

namespace rtk {
namespace {

struct SelectParams {
    TileGrid grid;
    float below, above;
    int dilate;
};

__global__ __launch_bounds__(256) void rtk_tiles_select_kernel(SelectParams P, const float* __restrict__ below_map, const float* __restrict__ above_map,
                                                                int32_t* __restrict__ tile_flags) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const int tile = int(gid >> 6), lane = int(gid & 63);
    if (tile >= P.grid.n_tiles) return;  // (wave-uniform: one wave is one tile)
    const int W = P.grid.width, H = P.grid.height, r = P.dilate;
    const int tx = (tile % P.grid.tiles_x) * 8, ty = (tile / P.grid.tiles_x) * 8;
    const int x0 = clampi(tx - r, 0, W - 1), x1 = clampi(tx + 7 + r, 0, W - 1);
    const int y0 = clampi(ty - r, 0, H - 1), y1 = clampi(ty + 7 + r, 0, H - 1);
    const int ww = x1 - x0 + 1, n = ww * (y1 - y0 + 1);  // <= 24 * 24
    bool raw = false;
    for (int k = lane; k < n; k += 64) {
        const size_t q = size_t(y0 + k / ww) * W + (x0 + k % ww);
        if (below_map) raw = raw || !(below_map[q] >= P.below);
        if (above_map) raw = raw || !(above_map[q] <= P.above);
    }
    const unsigned long long any = __ballot(raw);
    if (lane == 0) tile_flags[tile] = any != 0ull ? 1 : 0;
}

// The checks rtk_tiles_select and rtk_tiles_select_host share: none needs a context or a device.
int check_select_args(const char* who, int32_t width, int32_t height, const float* below_map, const float* above_map, const rtk_tile_select_opts* opts,
                      const int32_t* flags, SelectParams& P) {
    if (check_image_size(who, width, height) != RTK_OK) return RTK_ERR_INVALID;
    if (!below_map && !above_map) return fail(RTK_ERR_INVALID, "%s: d_below_map and d_above_map are both null", who);
    if (!flags) return fail(RTK_ERR_INVALID, "%s: d_tile_flags is null", who);
    if (!opts) return fail(RTK_ERR_INVALID, "%s: opts is null", who);
    if (opts->dilate < 0 || opts->dilate > 8) return fail(RTK_ERR_INVALID, "%s: dilate %d out of range (0..8)", who, opts->dilate);
    if (below_map && !std::isfinite(opts->below)) return fail(RTK_ERR_INVALID, "%s: below must be finite", who);
    if (above_map && !std::isfinite(opts->above)) return fail(RTK_ERR_INVALID, "%s: above must be finite", who);
    if (opts->reserved != 0) return fail(RTK_ERR_INVALID, "%s: reserved must be 0", who);
    if (check_aligned(below_map, 4, who, "d_below_map") != RTK_OK || check_aligned(above_map, 4, who, "d_above_map") != RTK_OK ||
        check_aligned(flags, 4, who, "d_tile_flags") != RTK_OK)
        return RTK_ERR_INVALID;
    P.grid = tile_grid(width, height);
    P.below = opts->below;
    P.above = opts->above;
    P.dilate = opts->dilate;
    return RTK_OK;
}

}  // namespace
}  // namespace rtk

using namespace rtk;

extern "C" {

int rtk_tiles_select(rtk_ctx* ctx, int32_t width, int32_t height, const float* d_below_map, const float* d_above_map, const rtk_tile_select_opts* opts,
                     int32_t* d_tile_flags, void* stream) {
    const char* who = "rtk_tiles_select";
    SelectParams P{};
    if (check_select_args(who, width, height, d_below_map, d_above_map, opts, d_tile_flags, P) != RTK_OK) return RTK_ERR_INVALID;
    if (!ctx) return fail(RTK_ERR_INVALID, "%s: null context", who);
    hipError_t e = hipSetDevice(ctx_device(ctx));
    if (e == hipSuccess) {
        rtk_tiles_select_kernel<<<dim3((P.grid.n_tiles + 3) / 4), dim3(256), 0, static_cast<hipStream_t>(stream)>>>(P, d_below_map, d_above_map, d_tile_flags);
        e = hipGetLastError();
    }
    return launched(who, e);
}

int rtk_tiles_select_host(rtk_ctx* ctx, int32_t width, int32_t height, const float* h_below_map, const float* h_above_map, const rtk_tile_select_opts* opts,
                          int32_t* h_tile_flags) {
    const char* who = "rtk_tiles_select_host";
    SelectParams P{};
    if (check_select_args(who, width, height, h_below_map, h_above_map, opts, h_tile_flags, P) != RTK_OK) return RTK_ERR_INVALID;
    if (!ctx) return fail(RTK_ERR_INVALID, "%s: null context", who);
    if (const hipError_t e = hipSetDevice(ctx_device(ctx)); e != hipSuccess) return launched(who, e);
    const size_t px = size_t(width) * height;
    HostStaging s(false);
    const int below = s.piece(px * sizeof(float), h_below_map != nullptr), above = s.piece(px * sizeof(float), h_above_map != nullptr);
    const int flags = s.piece(size_t(P.grid.n_tiles) * sizeof(int32_t));
    return run_host_form(
        who, nullptr, s, {{below, h_below_map}, {above, h_above_map}},
        [&] { return rtk_tiles_select(ctx, width, height, s.ptr<float>(below), s.ptr<float>(above), opts, s.ptr<int32_t>(flags), nullptr); },
        {{flags, h_tile_flags}});
}

int rtk_render_tiles(rtk_ctx* ctx, const rtk_camera* cam, const rtk_render_opts* opts, const int32_t* d_tile_flags, int32_t max_tiles, void* d_linear,
                     uint8_t* d_rgb8, float* d_noise, float* d_support, int32_t* d_info) {
    const char* who = "rtk_render_tiles";
    if (!cam || !opts) return fail(RTK_ERR_INVALID, "%s: null camera or options", who);
    if (check_frame_camera(who, *cam) != RTK_OK) return RTK_ERR_INVALID;
    if (opts->n_ranks != 1 || opts->rank != 0) return fail(RTK_ERR_INVALID, "%s: tile lists are one rank's (n_ranks must be 1, rank 0; got %d of %d)", who, opts->rank, opts->n_ranks);
    if (decode_variant(opts->variant).compact) return fail(RTK_ERR_INVALID, "%s: the tile-buffer layout (variant bit 22) is not supported", who);
    if (check_real_mode(who, opts->real_mode) != RTK_OK) return RTK_ERR_INVALID;
    if (!d_tile_flags) return fail(RTK_ERR_INVALID, "%s: d_tile_flags is null", who);
    if (max_tiles < 0) return fail(RTK_ERR_INVALID, "%s: max_tiles %d is negative (0 = no limit)", who, max_tiles);
    if (!d_linear && !d_rgb8 && !d_noise && !d_support) return fail(RTK_ERR_INVALID, "%s: no output", who);
    if (check_aligned(d_tile_flags, 4, who, "d_tile_flags") != RTK_OK || check_aligned(d_linear, opts->real_mode == RTK_REAL_F64 ? 8 : 4, who, "d_linear") != RTK_OK ||
        check_aligned(d_noise, 4, who, "d_noise") != RTK_OK || check_aligned(d_support, 4, who, "d_support") != RTK_OK ||
        check_aligned(d_info, 4, who, "d_info") != RTK_OK)
        return RTK_ERR_INVALID;
    TileFrame t;
    if (const int rc = stage_tile_frame(ctx, cam, opts, who, t); rc != RTK_OK) return rc;  // more than one launch, null context, no scene
    const FramePlan& f = t.plan;
    // flags -> list (ascending tile index) -> its length, gated by max_tiles -> the render kernel over the list -> the list's resolve
    hipError_t e = launch_adaptive_compact(d_tile_flags, nullptr, f.tm.n_tiles_local, t.d_list, t.d_count, f.stream);
    if (e == hipSuccess) e = launch_tile_gate(t.d_count, max_tiles, d_info, f.stream);
    TileMap tp = f.tm;
    tp.active_count = t.d_count;
    void* partial = nullptr;
    // no counters, no cost buffer: the context's learned tile order is neither read nor replaced
    if (e == hipSuccess) e = render_chunks(ctx, opts->real_mode, t.d_cam, tp, opts->seed, nullptr, t.d_list, nullptr, f.workspace_bytes(), f.stream, &partial, f.variant);
    if (e == hipSuccess)
        e = with_real(opts->real_mode, [&](auto real) {
            return launch_resolve_tiles<decltype(real)>(partial, tp, cam->image_width, cam->image_height, f.chunk_size, cam->pixel_samples_scale, t.d_list, t.d_count,
                                                        d_linear, d_rgb8, d_noise, d_support, f.stream);
        });
    if (e != hipSuccess) return fail(RTK_ERR_HIP, "%s: launch failed: %s", who, hipGetErrorString(e));
    return RTK_OK;
}

int rtk_render_tiles_host(rtk_ctx* ctx, const rtk_camera* cam, const rtk_render_opts* opts, const int32_t* h_tile_flags, int32_t max_tiles, double* h_linear,
                          uint8_t* h_rgb8, float* h_noise, float* h_support, int32_t* h_info) {
    const char* who = "rtk_render_tiles_host";
    // the device form's checks, made on the host pointers first: nothing is allocated or copied for a call it would refuse
    if (!h_tile_flags) return fail(RTK_ERR_INVALID, "%s: h_tile_flags is null", who);
    if (!cam || !opts) return fail(RTK_ERR_INVALID, "%s: null camera or options", who);
    if (check_camera_size(who, *cam) != RTK_OK || check_real_mode(who, opts->real_mode) != RTK_OK) return RTK_ERR_INVALID;
    if (!h_linear && !h_rgb8 && !h_noise && !h_support) return fail(RTK_ERR_INVALID, "%s: no output", who);
    // without a context the device form refuses before it touches a buffer: its remaining checks, in its words and its order
    if (!ctx) return rtk_render_tiles(nullptr, cam, opts, h_tile_flags, max_tiles, h_linear, h_rgb8, h_noise, h_support, nullptr);
    if (const hipError_t e = hipSetDevice(ctx_device(ctx)); e != hipSuccess) return launched(who, e);
    const size_t px = size_t(cam->image_width) * cam->image_height;
    const size_t n_tiles = size_t(rtk_tiles_per_rank(cam->image_width, cam->image_height, 1));
    HostStaging s(opts->real_mode == RTK_REAL_F64);
    const int flags = s.piece(n_tiles * sizeof(int32_t)), info = s.piece(2 * sizeof(int32_t));
    const int linear = s.linear(px * 3, h_linear != nullptr), rgb8 = s.piece(px * 3, h_rgb8 != nullptr);
    const int noise = s.piece(px * sizeof(float), h_noise != nullptr), support = s.piece(px * sizeof(float), h_support != nullptr);
    // the outputs go up as well: pixels of tiles that are not listed keep the caller's values
    return run_host_form(
        who, static_cast<hipStream_t>(opts->stream), s, {{flags, h_tile_flags}, {linear, h_linear, true}, {rgb8, h_rgb8}, {noise, h_noise}, {support, h_support}},
        [&] {
            const hipError_t e = hipMemset(s.ptr(info), 0, 2 * sizeof(int32_t));
            return e != hipSuccess ? launched(who, e)
                                   : rtk_render_tiles(ctx, cam, opts, s.ptr<int32_t>(flags), max_tiles, s.ptr(linear), s.ptr<uint8_t>(rgb8), s.ptr<float>(noise),
                                                      s.ptr<float>(support), s.ptr<int32_t>(info));
        },
        {{linear, h_linear, true}, {rgb8, h_rgb8}, {noise, h_noise}, {support, h_support}, {info, h_info}});
}

}  // extern "C"
