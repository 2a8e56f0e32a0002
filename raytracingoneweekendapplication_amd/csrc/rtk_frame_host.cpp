// rtk_frame_host.cpp -- the host side of the frame entry points of include/rtk.h: rtk_render_device / _host, rtk_tiles_unpermute,
// rtk_frame_launches and rtk_kernel_name, and what rtk_render_views (rtk_views.hip), rtk_render_tiles (rtk_tiles.hip) and the
// progressive sessions (rtk_progressive.cpp) share with them.  One plan (FramePlan: the arithmetic of a frame and the reading of
// the variant word), one pass loop (frame_pass, take_pass_counters), one rule for the context's workspaces (grow_device) and
// the wait that feeds the progress callback.  The kernels are rtk_trace.hip's and rtk_frame.hip's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <thread>
#include <vector>

#include "rtk.h"
#include "rtk_ctx.h"
#include "rtk_device_layout.h"
#include "rtk_internal.h"
#include "rtk_trace.h"

namespace rtk {

// ------------------------------------------------------------------------------------------------------------ the plan --
// Sample chunks per launch: the partial-sum workspace holds up to this many planes [local tile][3][64] at 1920x1080 f64 (+ one
// for the running sum of a frame that needs several launches): 21 + 1 planes = 1.09 GB, where the 63 chunks of a 1000-spp
// frame used to take 3.14 GB per context.  Every launch has a fixed cost -- staging the program, the drain of its last long
// paths -- measured on the full-size frames (same box, same image): one launch / passes of 16 chunks: C5 999.6 / 1014.6 ms,
// C3 247.7 / 254.5 ms; 21 chunks per pass makes a 1000-spp frame three launches instead of four.  Frames of up to 168 spp
// (C2: 13 chunks) are one launch as before.
// The plane count is a BUDGET, not a constant: 22 planes of a 1920x1080 f64 frame = 1.095 GB per context.  A smaller
// frame -- 800x800, or one rank's share of the tiles on several GPUs -- gets as many planes as that budget holds (up to all
// 64 chunks: the Cornell box at 1000 spp is one launch again, 247.7 instead of 251.8 ms), a larger one at least 8.
constexpr size_t kWorkspaceBudgetBytes = size_t(22) * 32400 * 192 * 8;
constexpr int kMinPlanesPerPass = 8;
constexpr int kMaxPasses = (kMaxChunks + kMinPlanesPerPass - 1) / kMinPlanesPerPass;
static_assert(kMaxPasses <= 8, "rtk_ctx keeps eight pass counters");

static int planes_per_pass_for(size_t plane_bytes, const Variant& v) {
    if (v.one_pass || plane_bytes == 0) return kMaxChunks;
    const size_t fit = kWorkspaceBudgetBytes / plane_bytes;  // planes the budget holds, one of them the running sum
    return fit > size_t(kMaxChunks) ? kMaxChunks : (fit < size_t(kMinPlanesPerPass + 1) ? kMinPlanesPerPass : int(fit) - 1);
}
// Samples per chunk: 8, or the smallest size that keeps a pixel's chunks within kMaxChunks -- a function of spp only.
static int chunk_size_for(int spp, const Variant& v) {
    int size = v.chunk_ab == 0 ? 8 : (v.chunk_ab == 1 ? 4 : (v.chunk_ab == 2 ? 2 : 16));
    if (v.whole_pixel) size = spp;
    while ((spp + size - 1) / size > kMaxChunks) size++;
    return size;
}
int frame_chunk_size(int spp) { return chunk_size_for(spp, decode_variant(0)); }

// Up to planes_per_pass chunks per launch; a frame with more is rendered in consecutive passes, the resolve kernel carrying
// the running sum in one extra plane -- the same additions in the same order as one pass over all chunks.
static void set_tiles(FramePlan& f, int64_t n_tiles) {
    f.n_tiles = n_tiles;
    f.tm.n_tiles_local = int32_t(n_tiles);
    f.plane = size_t(n_tiles) * 192 * f.elem;
    f.planes_per_pass = planes_per_pass_for(f.plane, f.variant);
    f.n_passes = (f.tm.n_chunks + f.planes_per_pass - 1) / f.planes_per_pass;
}

FramePlan plan_frame(const rtk_camera& cam, const rtk_render_opts& opts) {
    FramePlan f{};
    f.variant = decode_variant(opts.variant);
    f.stream = static_cast<hipStream_t>(opts.stream);
    f.elem = opts.real_mode == RTK_REAL_F64 ? sizeof(double) : sizeof(float);
    TileMap& tm = f.tm;
    tm.tiles_x = (cam.image_width + RTK_TILE_W - 1) / RTK_TILE_W;
    tm.tiles_y = (cam.image_height + RTK_TILE_H - 1) / RTK_TILE_H;
    tm.rank = opts.rank;
    tm.n_ranks = opts.n_ranks;
    tm.compact = opts.n_ranks > 1 || f.variant.compact ? 1 : 0;
    // Split every pixel's samples into chunks of 8 (at most 64 chunks) so that no lane is stuck with a whole
    // heavy pixel: a glass pixel's samples cost ~0.2 ms each, and the largest (pixel, chunk) bounds the end of
    // the frame whatever the GPU count.  Measured on C2 (v16 kernel time, N = 1 / one of 8 shards): 4-sample chunks
    // 22.8 / 3.21 ms, 8-sample 21.8 / 3.21 ms, 16-sample 21.7 / 3.60 ms (with the v9 kernel, whose refills were
    // dearer, 4 was the optimum).  A function of spp only.
    const int spp = cam.samples_per_pixel;
    f.chunk_size = chunk_size_for(spp, f.variant);
    int n = 0;
    for (int s0 = f.chunk_size; s0 < spp; s0 += f.chunk_size) tm.chunk_start[++n] = int16_t(s0);
    tm.n_chunks = n + 1;
    for (int k = n + 1; k <= kMaxChunks; k++) tm.chunk_start[k] = int16_t(spp);
    set_tiles(f, rtk_tiles_per_rank(cam.image_width, cam.image_height, opts.n_ranks));
    return f;
}

FramePlan plan_views(const FramePlan& one, int32_t n_views) {
    FramePlan b = one;
    b.tm.rank = 0;
    b.tm.n_ranks = 1;
    set_tiles(b, int64_t(n_views) * one.n_tiles);
    return b;
}

FramePass frame_pass(const FramePlan& f, int k, void* d_partial) {
    const int n = f.tm.n_chunks, c0 = k * f.planes_per_pass, c1 = std::min(n, c0 + f.planes_per_pass);
    FramePass p{f.tm, k == 0, k + 1 == f.n_passes, f.n_passes > 1 ? static_cast<char*>(d_partial) + f.plane * size_t(f.planes_per_pass) : nullptr};
    p.tm.n_chunks = c1 - c0;
    for (int j = 0; j <= kMaxChunks; j++) p.tm.chunk_start[j] = f.tm.chunk_start[std::min(c0 + j, n)];
    return p;
}

hipError_t take_pass_counters(rtk_ctx* ctx, const FramePlan& f, unsigned int** counters) {
    ctx->last_n_passes = f.n_passes;
    ctx->last_n_items = f.n_items();
    for (int k = 0; k < f.n_passes; k++) {
        counters[k] = ctx->tile_counters + (ctx->next_counter++ % kCounterRing);
        if (f.n_passes > 1)
            if (const hipError_t e = hipMemsetAsync(counters[k], 0, sizeof(unsigned int), f.stream); e != hipSuccess) return e;
        ctx->last_tile_counter[k] = counters[k];
        ctx->last_pass_items[k] = f.n_tiles * std::min(f.planes_per_pass, f.tm.n_chunks - k * f.planes_per_pass);
    }
    return hipSuccess;
}

// ------------------------------------------------------------------------------------------------------ the workspaces --
hipError_t denoise_workspace(rtk_ctx* ctx, size_t bytes, void** out) {
    const hipError_t e = grow_device(&ctx->d_denoise, &ctx->denoise_bytes, bytes);
    *out = ctx->d_denoise;
    return e;
}

hipError_t gather_workspace(rtk_ctx* ctx, size_t bytes, void** out) {
    const hipError_t e = grow_device(&ctx->d_gather, &ctx->gather_bytes, bytes);
    *out = ctx->d_gather;
    return e;
}

// The partial-sum workspace of every frame, batch and session step.
static hipError_t partial_workspace(rtk_ctx* ctx, size_t bytes) { return grow_device(&ctx->d_partial, &ctx->partial_bytes, bytes); }

// Block until every stream[i] (a stream of ctxs[i]'s device) has drained.  When ctxs[0] has a progress callback, the
// work-item counters of the launches in flight are sampled meanwhile -- a 4-byte device-to-host copy per context on a
// stream of its own (the copy engine, not a CU; the persistent kernel is not touched) -- and the callback gets the sums.
// A sample that has not landed by the next tick is simply skipped, so a copy stuck behind the kernel can only mean
// fewer reports, never a stall.
int wait_with_progress(rtk_ctx* const* ctxs, const hipStream_t* streams, int n) {
    rtk_ctx* reporter = n > 0 ? ctxs[0] : nullptr;
    if (!reporter || !reporter->progress_fn) {
        for (int i = 0; i < n; i++) {
            hipError_t e = hipSetDevice(ctxs[i]->device);
            if (e == hipSuccess) e = hipStreamSynchronize(streams[i]);
            if (e != hipSuccess) return fail(RTK_ERR_HIP, "hipStreamSynchronize failed: %s", hipGetErrorString(e));
        }
        return RTK_OK;
    }
    int64_t total = 0;
    std::vector<int64_t> seen(size_t(n), 0);
    for (int i = 0; i < n; i++) {
        rtk_ctx* c = ctxs[i];
        total += c->last_n_items;
        if (!c->progress_stream) {
            (void)hipSetDevice(c->device);
            if (hipStreamCreateWithFlags(&c->progress_stream, hipStreamNonBlocking) != hipSuccess) c->progress_stream = nullptr;
            if (hipHostMalloc(reinterpret_cast<void**>(&c->progress_word), 8 * sizeof(unsigned int), hipHostMallocDefault) != hipSuccess) c->progress_word = nullptr;
        }
        c->progress_pending = false;
    }
    const auto tick = std::chrono::milliseconds(reporter->progress_interval_ms);
    auto next_report = std::chrono::steady_clock::now();
    for (;;) {
        bool all_done = true;
        for (int i = 0; i < n; i++) {
            (void)hipSetDevice(ctxs[i]->device);
            const hipError_t q = hipStreamQuery(streams[i]);
            if (q == hipErrorNotReady) all_done = false;
            else if (q != hipSuccess) return fail(RTK_ERR_HIP, "hipStreamQuery failed: %s", hipGetErrorString(q));
        }
        if (all_done) break;
        if (std::chrono::steady_clock::now() >= next_report) {
            int64_t done = 0;
            for (int i = 0; i < n; i++) {
                rtk_ctx* c = ctxs[i];
                if (c->progress_stream && c->progress_word && c->last_n_passes > 0) {
                    (void)hipSetDevice(c->device);
                    if (c->progress_pending && hipStreamQuery(c->progress_stream) == hipSuccess) {
                        int64_t sum = 0;  // a pass that has not started yet still shows the zero its counter was reset to at enqueue time ... or an older launch's count: clamp, and count a pass only once every earlier one is complete
                        bool earlier_done = true;
                        for (int p = 0; p < c->last_n_passes; p++) {
                            const int64_t v = earlier_done ? std::min<int64_t>(int64_t(c->progress_word[p]), c->last_pass_items[p]) : 0;
                            sum += v;
                            earlier_done = earlier_done && v == c->last_pass_items[p];
                        }
                        seen[size_t(i)] = std::max(seen[size_t(i)], sum);
                        c->progress_pending = false;
                    }
                    if (!c->progress_pending) {
                        bool ok = true;
                        for (int p = 0; p < c->last_n_passes && ok; p++)
                            ok = hipMemcpyAsync(c->progress_word + p, c->last_tile_counter[p], sizeof(unsigned int), hipMemcpyDeviceToHost, c->progress_stream) == hipSuccess;
                        c->progress_pending = ok;
                    }
                }
                done += seen[size_t(i)];
            }
            reporter->progress_fn(done, total, reporter->progress_user);
            next_report = std::chrono::steady_clock::now() + tick;
        }
        std::this_thread::sleep_for(std::chrono::microseconds(200));
    }
    for (int i = 0; i < n; i++)
        if (ctxs[i]->progress_stream) {
            (void)hipSetDevice(ctxs[i]->device);
            (void)hipStreamSynchronize(ctxs[i]->progress_stream);
            ctxs[i]->progress_pending = false;
        }
    reporter->progress_fn(total, total, reporter->progress_user);
    return RTK_OK;
}

// ------------------------------------------------------------------------------------------------------- frame set-up --
// What rtk_render_device and rtk_render_tiles share besides the plan: the partial-sum workspace grown to the frame's need, the
// camera record in its device slot *d_cam (copied on the frame's stream unless it is the cached one).
static int stage_frame(rtk_ctx* ctx, const rtk_camera* cam, int real_mode, const FramePlan& f, unsigned char** d_cam) {
    RTK_HIP(partial_workspace(ctx, f.workspace_bytes()));
    const int cam_mode = real_mode == RTK_REAL_F64 ? 0 : 1;
    const bool cam_cached = ctx->cam_valid[cam_mode] && std::memcmp(&ctx->cam_last[cam_mode], cam, sizeof(rtk_camera)) == 0;
    const unsigned int cslot = cam_cached ? ctx->cam_slot[cam_mode] : (ctx->next_camera++ % kCounterRing);
    *d_cam = ctx->d_cameras + cslot * kCameraStride;
    if (cam_cached) return RTK_OK;
    // a slot about to be overwritten may still be the other mode's cached camera
    for (int m = 0; m < 2; m++)
        if (ctx->cam_valid[m] && ctx->cam_slot[m] == cslot) ctx->cam_valid[m] = false;
    ctx->cam_last[cam_mode] = *cam;
    ctx->cam_slot[cam_mode] = cslot;
    ctx->cam_valid[cam_mode] = true;
    unsigned char* const h_cam = ctx->h_cameras.data() + cslot * kCameraStride;
    const hipError_t e = with_real(real_mode, [&](auto real) {
        const CameraRec<decltype(real)> rec = device_camera<decltype(real)>(*cam);
        std::memcpy(h_cam, &rec, sizeof rec);
        return hipMemcpyAsync(*d_cam, h_cam, sizeof rec, hipMemcpyHostToDevice, f.stream);
    });
    if (e != hipSuccess) return fail(RTK_ERR_HIP, "hipMemcpyAsync of the camera record failed: %s", hipGetErrorString(e));
    return RTK_OK;
}

// rtk_render_device; use_order = false (a view batch's per-view fallback): the frame neither reads nor touches the context's
// learned tile order -- row-major hand-out, no cost measured, the stored order and the shape it belongs to left as they are.
static int render_frame(rtk_ctx* ctx, const rtk_camera* cam, const rtk_render_opts* opts, void* d_linear, uint8_t* d_rgb8, rtk_work_counters* d_counters,
                        bool use_order) {
    const char* who = "rtk_render_device";
    if (!ctx || !cam || !opts) return fail(RTK_ERR_INVALID, "%s: null argument", who);
    if (!ctx->has_scene) return fail(RTK_ERR_NO_SCENE, "%s: no scene uploaded", who);
    if (check_frame_camera(who, *cam) != RTK_OK || check_rank(who, *opts) != RTK_OK) return RTK_ERR_INVALID;
    const Variant v = decode_variant(opts->variant);
    if ((opts->n_ranks > 1 || v.compact) && d_rgb8) return fail(RTK_ERR_INVALID, "%s: d_rgb8 must be null when n_ranks > 1 (use rtk_tiles_unpermute)", who);
    if (opts->count_work && !d_counters) return fail(RTK_ERR_INVALID, "%s: count_work needs d_counters", who);
    if (check_real_mode(who, opts->real_mode) != RTK_OK) return RTK_ERR_INVALID;
    RTK_HIP(hipSetDevice(ctx->device));
    const FramePlan f = plan_frame(*cam, *opts);
    unsigned char* d_cam = nullptr;
    if (const int rc = stage_frame(ctx, cam, opts->real_mode, f, &d_cam); rc != RTK_OK) return rc;
    // tile order / cost buffers for this shape
    const int n_tiles = f.tm.n_tiles_local;
    const size_t order_need = size_t(n_tiles) * sizeof(int32_t);
    const int shape[5] = {cam->image_width, cam->image_height, opts->rank, opts->n_ranks, n_tiles};
    if (use_order && order_need > ctx->order_bytes) {
        size_t cost_bytes = ctx->order_bytes;  // one capacity for the pair
        RTK_HIP(grow_device(&ctx->d_tile_cost, &cost_bytes, order_need));
        RTK_HIP(grow_device(&ctx->d_tile_order, &ctx->order_bytes, order_need));
        ctx->order_valid = false;
    }
    if (use_order && std::memcmp(shape, ctx->order_shape, sizeof shape) != 0) ctx->order_valid = false;
    const bool learn = use_order && !v.fixed_order;
    if (!ctx->order_valid && learn) RTK_HIP(hipMemsetAsync(ctx->d_tile_cost, 0, order_need, f.stream));
    const int32_t* tile_order = (ctx->order_valid && learn) ? ctx->d_tile_order : nullptr;
    unsigned int* tile_cost = learn ? ctx->d_tile_cost : nullptr;
    unsigned int* pass_counter[kMaxPasses];
    RTK_HIP(take_pass_counters(ctx, f, pass_counter));
    hipError_t e = hipSuccess;
    for (int k = 0; k < f.n_passes && e == hipSuccess; k++) {
        const FramePass p = frame_pass(f, k, ctx->d_partial);
        e = with_real(opts->real_mode, [&](auto real) {
            using R = decltype(real);
            const hipError_t le = launch_render<R>(ctx_view<R>(ctx), reinterpret_cast<const CameraRec<R>*>(d_cam), p.tm, opts->seed, ctx->features,
                                                   opts->count_work != 0, v.allow_lds, v.diag, ctx->d_partial, reinterpret_cast<unsigned long long*>(d_counters),
                                                   pass_counter[k], tile_order, p.first ? tile_cost : nullptr,  // a tile's cost is measured on every pixel's first chunk
                                                   f.stream);
            return le != hipSuccess ? le
                                    : launch_resolve<R>(ctx->d_partial, p.tm, cam->image_width, cam->image_height, cam->pixel_samples_scale, d_linear, d_rgb8, p.acc,
                                                        p.first, p.last, f.stream);
        });
    }
    if (e == hipSuccess && learn) {  // this frame's costs become the next frame's hand-out order
        e = launch_tile_order(ctx->d_tile_cost, n_tiles, ctx->d_tile_order, f.stream);
        ctx->order_valid = e == hipSuccess;
        std::memcpy(ctx->order_shape, shape, sizeof shape);
    }
    if (e != hipSuccess) return fail(RTK_ERR_HIP, "render kernel launch failed: %s", hipGetErrorString(e));
    return RTK_OK;
}

int render_frame_apart(rtk_ctx* ctx, const rtk_camera* cam, const rtk_render_opts* opts, void* d_linear, uint8_t* d_rgb8, rtk_work_counters* d_counters) {
    return render_frame(ctx, cam, opts, d_linear, d_rgb8, d_counters, false);
}

hipError_t render_chunks(rtk_ctx* ctx, int real_mode, const void* d_cam, const TileMap& tp, uint32_t seed, unsigned long long* counters,
                         const int32_t* tile_order, unsigned int* tile_cost, size_t workspace_bytes, hipStream_t stream, void** partial, const Variant& v) {
    if (const hipError_t e = partial_workspace(ctx, workspace_bytes); e != hipSuccess) return e;
    *partial = ctx->d_partial;
    unsigned int* tile_counter = ctx->tile_counters + (ctx->next_counter++ % kCounterRing);
    return with_real(real_mode, [&](auto real) {
        using R = decltype(real);
        return launch_render<R>(ctx_view<R>(ctx), static_cast<const CameraRec<R>*>(d_cam), tp, seed, ctx->features, counters != nullptr, v.allow_lds, v.diag,
                                ctx->d_partial, counters, tile_counter, tile_order, tile_cost, stream);
    });
}

// View batches (rtk_render_views): a view's record as the view kernel reads it.
static uint32_t seed_hash_of(uint32_t v) {  // pcg_hash (rtk_trace.hip): what the render kernel makes of opts->seed before it keys a sample's stream
    const uint32_t st = v * 747796405u + 2891336453u;
    const uint32_t w = ((st >> ((st >> 28u) + 4u)) ^ st) * 277803737u;
    return (w >> 22u) ^ w;
}

int stage_view_batch(rtk_ctx* ctx, const FramePlan& batch, int32_t n_views, const rtk_camera* cams, const uint32_t* seeds, const rtk_render_opts* opts, ViewBatch& out) {
    RTK_HIP(hipSetDevice(ctx->device));
    RTK_HIP(partial_workspace(ctx, batch.workspace_bytes()));
    out.d_partial = ctx->d_partial;
    const size_t rec_bytes = size_t(n_views) * (opts->real_mode == RTK_REAL_F64 ? sizeof(ViewRec<double>) : sizeof(ViewRec<float>));
    RTK_HIP(grow_device(&ctx->d_views, &ctx->views_bytes, rec_bytes));  // (earlier batches may still read the old table)
    out.d_views = ctx->d_views;
    rtk_ctx::ViewStage& stage = ctx->view_stage[ctx->next_view_stage++ % 4u];
    if (!stage.done) RTK_HIP(hipEventCreateWithFlags(&stage.done, hipEventDisableTiming));
    RTK_HIP(hipEventSynchronize(stage.done));  // the upload that last read this buffer (four batches ago) has run
    if (rec_bytes > stage.bytes) {
        if (stage.host) RTK_HIP(hipHostFree(stage.host));
        stage.host = nullptr;
        stage.bytes = 0;
        RTK_HIP(hipHostMalloc(&stage.host, rec_bytes, hipHostMallocDefault));
        stage.bytes = rec_bytes;
    }
    with_real(opts->real_mode, [&](auto real) {
        auto* rec = static_cast<ViewRec<decltype(real)>*>(stage.host);
        for (int32_t v = 0; v < n_views; v++) {
            rec[v].cam = device_camera<decltype(real)>(cams[v]);
            rec[v].seed_hash = seed_hash_of(seeds ? seeds[v] : opts->seed);
            rec[v].reserved = 0;
        }
        return 0;
    });
    RTK_HIP(hipMemcpyAsync(ctx->d_views, stage.host, rec_bytes, hipMemcpyHostToDevice, batch.stream));
    RTK_HIP(hipEventRecord(stage.done, batch.stream));
    RTK_HIP(take_pass_counters(ctx, batch, out.pass_counter));
    return RTK_OK;
}

int stage_tile_frame(rtk_ctx* ctx, const rtk_camera* cam, const rtk_render_opts* opts, const char* who, TileFrame& out) {
    out.plan = plan_frame(*cam, *opts);
    if (out.plan.n_passes > 1)
        return fail(RTK_ERR_INVALID, "%s: a frame of %d launches (rtk_frame_launches: more sample chunks than the workspace holds planes for) is not supported", who,
                    out.plan.n_passes);
    if (!ctx) return fail(RTK_ERR_INVALID, "%s: null context", who);
    if (!ctx->has_scene) return fail(RTK_ERR_NO_SCENE, "%s: no scene uploaded", who);
    RTK_HIP(hipSetDevice(ctx->device));
    unsigned char* d_cam = nullptr;
    if (const int rc = stage_frame(ctx, cam, opts->real_mode, out.plan, &d_cam); rc != RTK_OK) return rc;
    const size_t list_need = (size_t(out.plan.n_tiles) + 1) * sizeof(int32_t);
    if (list_need > ctx->list_bytes) {
        RTK_HIP(grow_device(&ctx->d_tile_list, &ctx->list_bytes, list_need));
        // positions beyond the list's length are read (the render kernel stages the whole array) and never used: defined bytes
        RTK_HIP(hipMemset(ctx->d_tile_list, 0, list_need));
    }
    out.d_cam = d_cam;
    out.d_list = ctx->d_tile_list;
    out.d_count = ctx->d_tile_list + ctx->list_bytes / sizeof(int32_t) - 1;
    return RTK_OK;
}

}  // namespace rtk

using namespace rtk;

extern "C" {

int64_t rtk_tiles_per_rank(int image_width, int image_height, int n_ranks) {
    if (image_width <= 0 || image_height <= 0 || n_ranks <= 0) return 0;
    const int64_t tiles = int64_t((image_width + RTK_TILE_W - 1) / RTK_TILE_W) * ((image_height + RTK_TILE_H - 1) / RTK_TILE_H);
    return (tiles + n_ranks - 1) / n_ranks;
}

int rtk_render_device(rtk_ctx* ctx, const rtk_camera* cam, const rtk_render_opts* opts, void* d_linear, uint8_t* d_rgb8, rtk_work_counters* d_counters) {
    return render_frame(ctx, cam, opts, d_linear, d_rgb8, d_counters, true);
}

int rtk_tiles_unpermute(rtk_ctx* ctx, int image_width, int image_height, int n_ranks, int real_mode, const void* d_gathered, void* d_linear, uint8_t* d_rgb8,
                        void* stream) {
    if (!ctx || !d_gathered || image_width <= 0 || image_height <= 0 || n_ranks < 1) return fail(RTK_ERR_INVALID, "rtk_tiles_unpermute: bad argument");
    RTK_HIP(hipSetDevice(ctx->device));
    const hipError_t e = with_real(real_mode, [&](auto real) {
        return launch_unpermute<decltype(real)>(d_gathered, image_width, image_height, n_ranks, rtk_tiles_per_rank(image_width, image_height, n_ranks), d_linear, d_rgb8,
                                                static_cast<hipStream_t>(stream));
    });
    if (e != hipSuccess) return fail(RTK_ERR_HIP, "unpermute kernel launch failed: %s", hipGetErrorString(e));
    return RTK_OK;
}

int rtk_render_host(rtk_ctx* ctx, const rtk_camera* cam, const rtk_render_opts* opts, double* h_linear, uint8_t* h_rgb8, rtk_work_counters* counters) {
    const char* who = "rtk_render_host";
    if (!ctx || !cam || !opts) return fail(RTK_ERR_INVALID, "%s: null argument", who);
    if (opts->n_ranks != 1) return fail(RTK_ERR_INVALID, "rtk_render_host renders whole images (n_ranks must be 1)");
    RTK_HIP(hipSetDevice(ctx->device));
    const size_t n = size_t(cam->image_width) * cam->image_height * 3;
    HostStaging s(opts->real_mode == RTK_REAL_F64);
    const int lin = s.linear(n), rgb8 = s.piece(n), cnt = s.piece(sizeof(rtk_work_counters), counters != nullptr);
    rtk_render_opts o = *opts;
    o.count_work = counters ? 1 : 0;
    hipStream_t stream = static_cast<hipStream_t>(o.stream);
    return run_host_form_waiting(
        who, s, {},
        [&] {
            const hipError_t e = counters ? hipMemsetAsync(s.ptr(cnt), 0, sizeof(rtk_work_counters), stream) : hipSuccess;
            return e != hipSuccess ? launched(who, e) : rtk_render_device(ctx, cam, &o, s.ptr(lin), s.ptr<uint8_t>(rgb8), s.ptr<rtk_work_counters>(cnt));
        },
        [&] { return wait_with_progress(&ctx, &stream, 1); }, {{lin, h_linear, true}, {rgb8, h_rgb8}, {cnt, counters}});
}

int rtk_frame_launches(const rtk_camera* cam, const rtk_render_opts* opts) {
    if (!cam || !opts || cam->samples_per_pixel <= 0 || cam->samples_per_pixel > 32767 || cam->image_width <= 0 || cam->image_height <= 0 || opts->n_ranks < 1)
        return fail(RTK_ERR_INVALID, "rtk_frame_launches: bad camera or options");
    return plan_frame(*cam, *opts).n_passes;
}

const char* rtk_kernel_name(rtk_ctx* ctx, int real_mode, int variant) {
    if (!ctx || !ctx->has_scene) return "";
    const Variant v = decode_variant(variant);
    return with_real(real_mode, [&](auto real) { return render_kernel_name<decltype(real)>(ctx_view<decltype(real)>(ctx), ctx->features, false, v.allow_lds, v.diag); });
}

}  // extern "C"
