// rtk_progressive.cpp -- progressive, resumable rendering (include/rtk.h, "Progressive, resumable rendering").
//
// A session renders one frame in steps into running sums of its own (include/rtk.h, "Progressive, resumable rendering").  A
// step is the one-shot frame's chunk loop restricted to an absolute chunk range: the render kernel is launched unchanged on a
// TileMap whose chunk_start holds the step's absolute sample indices (in launches of at most the plan's planes_per_pass chunks, into
// the context's partial-sum workspace), and rtk_accumulate_kernel folds every launch's planes into the session's sum in the
// resolve's order -- so the image does not depend on how the frame was cut into steps.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "rtk.h"
#include "rtk_device_layout.h"
#include "rtk_internal.h"
#include "rtk_trace.h"

using namespace rtk;

struct rtk_progressive {
    rtk_ctx* ctx = nullptr;
    rtk_camera cam{};
    uint32_t seed = 0;
    int real_mode = RTK_REAL_F64;
    int rank = 0, n_ranks = 1;
    hipStream_t stream = nullptr;
    int target = 0, chunk = 0, done = 0;
    uint64_t digest = 0;
    bool poisoned = false;
    TileMap tm{};        // tile geometry; chunk fields are filled per launch
    size_t elem = 8;     // bytes per real
    size_t plane = 0;    // bytes of one chunk plane [local tile][3][64] ...
    int per_launch = 0;  // ... and how many a launch may fill (the one-shot frame's plan)
    void* d_sum = nullptr;              // [local tile][3][64] reals
    double* d_s1 = nullptr;             // [local tile][64]
    double* d_s2 = nullptr;
    void* d_cam = nullptr;              // CameraRec<real>
    unsigned int* d_cost = nullptr;     // tile costs measured by the first step's first launch ...
    int32_t* d_order = nullptr;         // ... become the hand-out order of the later launches
    bool order_valid = false;
    double* d_stats = nullptr;          // noise partials [blocks][3] + the 3 reduced values
    // tile-adaptive sampling (rtk_progressive_set_adaptive): per local tile active (1 / 0) and sample count, the hand-out list
    // of the active tiles and its length (built on the device after every step, read by the next step's render launches)
    bool adaptive = false;
    double rel_target = 0.0;
    int min_samples = 0;
    int32_t* d_active = nullptr;
    int32_t* d_tile_spp = nullptr;
    int32_t* d_list = nullptr;          // [n_tiles_local] + the count behind it
    bool list_valid = false;
    // rtk_progressive_denoise: the AOVs of the session's camera and seed per sample count (never in checkpoints) and the
    // preview / se it rebuilds from the sums
    std::vector<std::pair<int, float*>> aovs;
    // rtk_progressive_denoise_guided: the guides of rtk_render_guides per resolved option set
    struct GuideSet { int samples, follow, max_bounces; float* d; };
    std::vector<GuideSet> guides;
    void* d_preview = nullptr;          // H*W*3 reals
    float* d_preview_se = nullptr;      // H*W
    int full_chunks() const { return done / chunk; }  // every chunk before the target's end is full
    size_t n_slots() const { return size_t(tm.n_tiles_local) * 64; }
};

namespace {

constexpr char kCheckpointMagic[8] = {'R', 'T', 'K', 'P', 'R', 'O', 'G', '\0'};
constexpr size_t kCheckpointHeader = 256;
static_assert(sizeof(rtk_camera) == 200, "checkpoint layout: rtk_camera is 200 bytes");
static_assert(56 + sizeof(rtk_camera) == kCheckpointHeader, "checkpoint header");

constexpr int32_t kCheckpointAdaptive = 2;  // the version of an adaptive session's checkpoint

// Version 1; version 2 inserts the adaptive block (rel_target, min_samples, pad, tile_spp[tiles]) before the checksum.
int64_t checkpoint_bytes_for(int width, int height, int n_ranks, int real_mode, bool adaptive = false) {
    const int64_t tiles = rtk_tiles_per_rank(width, height, n_ranks);
    return int64_t(kCheckpointHeader) + tiles * 192 * (real_mode == RTK_REAL_F64 ? 8 : 4) + 2 * tiles * 64 * 8 + (adaptive ? 16 + tiles * 4 : 0) + 8;
}

// In-image pixels of local tile lt of `rank` (0 for a rank's padding tiles past the last tile).
int tile_pixels(int width, int height, int rank, int n_ranks, int64_t lt) {
    const int tiles_x = (width + RTK_TILE_W - 1) / RTK_TILE_W, tiles_y = (height + RTK_TILE_H - 1) / RTK_TILE_H;
    const int64_t t = lt * n_ranks + rank;
    if (t >= int64_t(tiles_x) * tiles_y) return 0;
    return std::min(8, width - int(t % tiles_x) * 8) * std::min(8, height - int(t / tiles_x) * 8);
}

// The adaptive options' rules (rtk_progressive_set_adaptive and version-2 checkpoints).
bool adaptive_opts_ok(double rel_target, int min_samples, int chunk, int target) {
    return rel_target > 0.0 && rel_target <= 1e300 && min_samples % chunk == 0 && min_samples >= 2 * chunk && min_samples <= target;
}

void release(rtk_progressive* p) {
    if (!p) return;
    if (p->ctx) (void)hipSetDevice(ctx_device(p->ctx));
    for (void* d : {p->d_sum, static_cast<void*>(p->d_s1), static_cast<void*>(p->d_s2), p->d_cam, static_cast<void*>(p->d_cost),
                    static_cast<void*>(p->d_order), static_cast<void*>(p->d_stats), static_cast<void*>(p->d_active), static_cast<void*>(p->d_tile_spp),
                    static_cast<void*>(p->d_list)})
        if (d) (void)hipFree(d);
    for (auto& a : p->aovs) (void)hipFree(a.second);
    for (auto& g : p->guides) (void)hipFree(g.d);
    if (p->d_preview) (void)hipFree(p->d_preview);
    if (p->d_preview_se) (void)hipFree(p->d_preview_se);
    delete p;
}

// The kernel's camera record, stored on `stream` from a kernel argument (no host wait, no host memory that outlives the call).
static_assert(sizeof(CameraRec<double>) % 4 == 0 && sizeof(CameraRec<float>) % 4 == 0, "launch_store_record stores 4-byte words");
hipError_t upload_camera(const rtk_camera& cam, int real_mode, void* d_dst, hipStream_t stream) {
    return with_real(real_mode, [&](auto real) {
        const CameraRec<decltype(real)> rec = device_camera<decltype(real)>(cam);
        return launch_store_record(&rec, sizeof rec, d_dst, stream);
    });
}

// Argument checks and device state of a new session.  The state is set up ON THE SESSION'S STREAM, by asynchronous memsets and
// a kernel that stores the camera record: nothing here blocks, so a session can be created while its stream is busy without
// waiting for it (a blocking call on the NULL stream may be queued behind any stream's backlog).  zero_sums = false: the
// caller fills the sums itself (resume; a memset on the stream would run after its blocking copies).
int make_session(rtk_ctx* ctx, const rtk_camera* cam, const rtk_render_opts* opts, const char* who, rtk_progressive** out, bool zero_sums = true) {
    if (!ctx || !cam || !opts || !out) return fail(RTK_ERR_INVALID, "%s: null argument", who);
    *out = nullptr;
    uint64_t digest = 0;
    if (!ctx_scene(ctx, &digest)) return fail(RTK_ERR_NO_SCENE, "%s: no scene uploaded", who);
    if (check_frame_camera(who, *cam) != RTK_OK || check_rank(who, *opts) != RTK_OK || check_real_mode(who, opts->real_mode) != RTK_OK) return RTK_ERR_INVALID;
    RTK_HIP(hipSetDevice(ctx_device(ctx)));
    rtk_render_opts plain = *opts;
    plain.variant = 0;  // sessions render with variant 0: the default chunk size, compact tile buffers for several ranks only
    const FramePlan f = plan_frame(*cam, plain);
    auto* p = new rtk_progressive;
    p->ctx = ctx;
    p->cam = *cam;
    p->seed = opts->seed;
    p->real_mode = opts->real_mode;
    p->rank = opts->rank;
    p->n_ranks = opts->n_ranks;
    p->stream = static_cast<hipStream_t>(opts->stream);
    p->target = cam->samples_per_pixel;
    p->chunk = f.chunk_size;
    p->digest = digest;
    p->elem = f.elem;
    p->plane = f.plane;
    p->per_launch = f.planes_per_pass;
    TileMap& tm = p->tm;
    tm = f.tm;
    tm.n_chunks = 0;
    std::memset(tm.chunk_start, 0, sizeof tm.chunk_start);
    const size_t slots = p->n_slots();
    hipError_t e = hipMalloc(&p->d_sum, slots * 3 * p->elem);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&p->d_s1), slots * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&p->d_s2), slots * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&p->d_cam, camera_record_bytes());
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&p->d_cost), size_t(tm.n_tiles_local) * sizeof(unsigned int));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&p->d_order), size_t(tm.n_tiles_local) * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&p->d_stats), (size_t(noise_partial_blocks(tm)) + 1) * 3 * sizeof(double));
    // zeroed sums: a checkpoint holds defined bytes for the pixels outside the image too
    if (e == hipSuccess && zero_sums) e = hipMemsetAsync(p->d_sum, 0, slots * 3 * p->elem, p->stream);
    if (e == hipSuccess && zero_sums) e = hipMemsetAsync(p->d_s1, 0, slots * sizeof(double), p->stream);
    if (e == hipSuccess && zero_sums) e = hipMemsetAsync(p->d_s2, 0, slots * sizeof(double), p->stream);
    if (e == hipSuccess) e = hipMemsetAsync(p->d_cost, 0, size_t(tm.n_tiles_local) * sizeof(unsigned int), p->stream);
    if (e == hipSuccess) e = upload_camera(*cam, p->real_mode, p->d_cam, p->stream);
    if (e != hipSuccess) {
        release(p);
        return fail(RTK_ERR_HIP, "%s: device allocation failed: %s", who, hipGetErrorString(e));
    }
    *out = p;
    return RTK_OK;
}

// Device state of an adaptive session: every in-image tile active with 0 samples, set up on the session's stream without a
// blocking call (rtk_progressive_set_adaptive) -- or tile_spp = h_spp when given (resume, which copies the caller's
// checkpoint with blocking calls anyway).
hipError_t make_adaptive(rtk_progressive* p, const int32_t* h_spp) {
    const size_t n = size_t(p->tm.n_tiles_local);
    hipError_t e = hipSuccess;
    if (!p->d_active) e = hipMalloc(reinterpret_cast<void**>(&p->d_active), n * sizeof(int32_t));
    if (e == hipSuccess && !p->d_tile_spp) e = hipMalloc(reinterpret_cast<void**>(&p->d_tile_spp), n * sizeof(int32_t));
    if (e == hipSuccess && !p->d_list) e = hipMalloc(reinterpret_cast<void**>(&p->d_list), (n + 1) * sizeof(int32_t));
    p->list_valid = false;
    if (!h_spp) {
        if (e == hipSuccess) e = hipMemsetAsync(p->d_list, 0, (n + 1) * sizeof(int32_t), p->stream);
        if (e == hipSuccess) e = launch_adaptive_init(p->tm, p->d_active, p->d_tile_spp, p->stream);
        return e;
    }
    if (e == hipSuccess) e = hipMemset(p->d_list, 0, (n + 1) * sizeof(int32_t));
    std::vector<int32_t> active(n), spp(n, 0);
    for (size_t lt = 0; lt < n; lt++) active[lt] = tile_pixels(p->cam.image_width, p->cam.image_height, p->rank, p->n_ranks, int64_t(lt)) > 0 ? 1 : 0;
    if (e == hipSuccess) e = hipMemcpy(p->d_tile_spp, h_spp ? h_spp : spp.data(), n * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(p->d_active, active.data(), n * sizeof(int32_t), hipMemcpyHostToDevice);
    p->list_valid = false;
    return e;
}

// The next step's hand-out list: the active tiles in the learned cost order (identity until there is one).
hipError_t compact(rtk_progressive* p) {
    const hipError_t e = launch_adaptive_compact(p->d_active, p->order_valid ? p->d_order : nullptr, p->tm.n_tiles_local, p->d_list,
                                                 p->d_list + p->tm.n_tiles_local, p->stream);
    p->list_valid = e == hipSuccess;
    return e;
}

// Every check of a call on an existing session: poisoned, scene changed.
int usable(const rtk_progressive* p, const char* who) {
    if (!p) return fail(RTK_ERR_INVALID, "%s: null session", who);
    if (p->poisoned) return fail(RTK_ERR_INVALID, "%s: the session is poisoned by an earlier failed step", who);
    uint64_t now = 0;
    if (!ctx_scene(p->ctx, &now) || now != p->digest)
        return fail(RTK_ERR_INVALID, "%s: the context's scene changed since the session was created (digest %016llx, now %016llx)", who,
                    (unsigned long long)p->digest, (unsigned long long)now);
    return RTK_OK;
}

// The step's launches: render + accumulate per range of at most per_launch chunks (a loop of its own, in absolute chunks of the session: DESIGN.md, "What a frame entry point is made of").
hipError_t enqueue_step(rtk_progressive* p, int n_samples, void* d_linear, uint8_t* d_rgb8, float* d_noise, rtk_work_counters* d_counters, bool& launched) {
    const int c = p->chunk, s_end = p->done + n_samples;
    const int k0 = p->done / c, k1 = (s_end + c - 1) / c;  // absolute chunk range [k0, k1)
    const int per_launch = p->per_launch;
    const size_t workspace = p->plane * size_t(std::min(per_launch, k1 - k0));
    // Adaptive sessions: a fresh session's first step renders every tile (all are active) and learns the cost order like any
    // other; every later step hands out the compacted list of the active tiles, up to its device-side length.
    const bool all_tiles = !p->adaptive || p->done == 0;
    hipError_t e = hipSuccess;
    if (!all_tiles && !p->list_valid && (e = compact(p)) != hipSuccess) return e;  // (a resumed session)
    const int32_t* order = !all_tiles ? p->d_list : (p->order_valid ? p->d_order : nullptr);
    auto* counters = reinterpret_cast<unsigned long long*>(d_counters);
    const bool measure = !p->order_valid && all_tiles;
    for (int a = k0; a < k1 && e == hipSuccess; a += per_launch) {
        const int b = std::min(k1, a + per_launch);
        TileMap tp = p->tm;
        tp.n_chunks = b - a;
        for (int k = 0; k <= kMaxChunks; k++) tp.chunk_start[k] = int16_t(std::min(std::min(a + k, b) * c, p->target));
        if (!all_tiles) tp.active_count = p->d_list + p->tm.n_tiles_local;
        unsigned int* cost = (measure && a == k0) ? p->d_cost : nullptr;  // a tile's cost is measured on its first launch
        void* partial = nullptr;
        e = render_chunks(p->ctx, p->real_mode, p->d_cam, tp, p->seed, counters, order, cost, workspace, p->stream, &partial);
        launched = launched || e == hipSuccess;
        if (e != hipSuccess) break;
        const bool last = b == k1;
        const int k_full = s_end / c;  // full chunks after the step (every chunk but a final partial one; read on the last launch only)
        const bool retire_ok = last && p->min_samples <= s_end && s_end < p->target;
        e = with_real(p->real_mode, [&](auto real) {
            using R = decltype(real);
            return p->adaptive ? launch_accumulate_adaptive<R>(partial, tp, p->cam.image_width, p->cam.image_height, c, a == 0, p->d_sum, p->d_s1, p->d_s2,
                                                               p->d_active, p->d_tile_spp, last, s_end, retire_ok, p->rel_target, d_linear, d_rgb8, d_noise, p->stream)
                               : launch_accumulate<R>(partial, tp, p->cam.image_width, p->cam.image_height, c, a == 0, p->d_sum, p->d_s1, p->d_s2, last,
                                                      1.0 / double(s_end), k_full, d_linear, d_rgb8, d_noise, p->stream);
        });
    }
    if (e == hipSuccess && measure) {  // the first step's costs become the hand-out order of every later launch
        e = launch_tile_order(p->d_cost, p->tm.n_tiles_local, p->d_order, p->stream);
        p->order_valid = e == hipSuccess;
    }
    if (e == hipSuccess && p->adaptive) e = compact(p);
    return e;
}

// Parse and check a checkpoint of version 1 or 2 (rtk_checkpoint_read_info); a version-2 one also yields its adaptive options
// and where its tile_spp table starts (*tile_spp_out stays null for version 1, *adaptive_out all 0).
int parse_checkpoint(const void* h_buf, int64_t n, rtk_checkpoint_info* out, rtk_adaptive_opts* adaptive_out, const unsigned char** tile_spp_out) {
    const unsigned char* b = static_cast<const unsigned char*>(h_buf);
    if (n < int64_t(kCheckpointHeader) + 8) return fail(RTK_ERR_INVALID, "rtk_checkpoint_read_info: %lld bytes is too short for a checkpoint", (long long)n);
    if (std::memcmp(b, kCheckpointMagic, 8) != 0) return fail(RTK_ERR_INVALID, "rtk_checkpoint_read_info: not a checkpoint (bad magic)");
    int32_t f[9];
    std::memcpy(f, b + 8, sizeof f);
    rtk_checkpoint_info info{};
    info.version = f[0];
    info.width = f[1];
    info.height = f[2];
    info.rank = f[3];
    info.n_ranks = f[4];
    info.real_mode = f[5];
    info.target_spp = f[6];
    info.chunk_size = f[7];
    info.samples_done = f[8];
    std::memcpy(&info.seed, b + 44, 4);
    std::memcpy(&info.scene_digest, b + 48, 8);
    if (info.version != RTK_CHECKPOINT_VERSION && info.version != kCheckpointAdaptive)
        return fail(RTK_ERR_INVALID, "rtk_checkpoint_read_info: checkpoint version %d, this library reads versions %d and %d", info.version,
                    RTK_CHECKPOINT_VERSION, kCheckpointAdaptive);
    const bool adaptive = info.version == kCheckpointAdaptive;
    if (!image_size_ok(info.width, info.height) || info.n_ranks < 1 || info.n_ranks > 65536 || info.rank < 0 ||
        info.rank >= info.n_ranks || (info.real_mode != RTK_REAL_F64 && info.real_mode != RTK_REAL_F32) || info.target_spp < 1 || info.target_spp > 32767 ||
        info.chunk_size != frame_chunk_size(info.target_spp) || info.samples_done < 0 || info.samples_done > info.target_spp)
        return fail(RTK_ERR_INVALID, "rtk_checkpoint_read_info: inconsistent header fields");
    rtk_camera cam;
    std::memcpy(&cam, b + 56, sizeof cam);
    if (cam.image_width != info.width || cam.image_height != info.height || cam.samples_per_pixel != info.target_spp)
        return fail(RTK_ERR_INVALID, "rtk_checkpoint_read_info: the stored camera disagrees with the header");
    const int64_t size = checkpoint_bytes_for(info.width, info.height, info.n_ranks, info.real_mode, adaptive);
    if (n != size)
        return fail(RTK_ERR_INVALID, "rtk_checkpoint_read_info: %lld bytes, a %dx%d checkpoint of rank %d of %d (%s) has %lld", (long long)n, info.width, info.height,
                    info.rank, info.n_ranks, info.real_mode == RTK_REAL_F64 ? "f64" : "f32", (long long)size);
    Fnv64 h;
    h.add(b, size_t(size - 8));
    uint64_t stored = 0;
    std::memcpy(&stored, b + size - 8, 8);
    if (stored != h.h) return fail(RTK_ERR_INVALID, "rtk_checkpoint_read_info: checksum mismatch (corrupted checkpoint)");
    rtk_adaptive_opts ad{};
    const unsigned char* spp_at = nullptr;
    if (adaptive) {  // the options' rules, and every tile either active (samples_done) or retired at a chunk boundary in [min_samples, samples_done)
        const int64_t tiles = rtk_tiles_per_rank(info.width, info.height, info.n_ranks);
        const unsigned char* at = b + size - 8 - tiles * 4 - 16;
        std::memcpy(&ad.rel_target, at, 8);
        std::memcpy(&ad.min_samples, at + 8, 4);
        std::memcpy(&ad.reserved, at + 12, 4);
        if (!adaptive_opts_ok(ad.rel_target, ad.min_samples, info.chunk_size, info.target_spp) || ad.reserved != 0)
            return fail(RTK_ERR_INVALID, "rtk_checkpoint_read_info: bad adaptive options (rel_target %g, min_samples %d)", ad.rel_target, ad.min_samples);
        spp_at = at + 16;
        for (int64_t lt = 0; lt < tiles; lt++) {
            int32_t v;
            std::memcpy(&v, spp_at + lt * 4, 4);
            const bool ok = tile_pixels(info.width, info.height, info.rank, info.n_ranks, lt) == 0
                                ? v == 0
                                : (v == info.samples_done || (v % info.chunk_size == 0 && v >= ad.min_samples && v < info.samples_done));
            if (!ok) return fail(RTK_ERR_INVALID, "rtk_checkpoint_read_info: tile %lld holds %d samples (samples_done %d)", (long long)lt, v, info.samples_done);
        }
    }
    *out = info;
    if (adaptive_out) *adaptive_out = ad;
    if (tile_spp_out) *tile_spp_out = spp_at;
    return RTK_OK;
}

}  // namespace

extern "C" {

int rtk_progressive_create(rtk_ctx* ctx, const rtk_camera* cam, const rtk_render_opts* opts, rtk_progressive** out) {
    return make_session(ctx, cam, opts, "rtk_progressive_create", out);
}

int rtk_progressive_step(rtk_progressive* p, int32_t n_samples, void* d_linear, uint8_t* d_rgb8, float* d_noise, rtk_work_counters* d_counters) {
    int rc = usable(p, "rtk_progressive_step");
    if (rc != RTK_OK) return rc;
    if (p->done >= p->target) return fail(RTK_ERR_INVALID, "rtk_progressive_step: the session is finished (%d samples)", p->target);
    if (n_samples <= 0) return fail(RTK_ERR_INVALID, "rtk_progressive_step: n_samples must be positive (%d)", n_samples);
    if (n_samples > p->target - p->done)
        return fail(RTK_ERR_INVALID, "rtk_progressive_step: %d samples after %d pass the target of %d", n_samples, p->done, p->target);
    if (n_samples % p->chunk != 0 && p->done + n_samples != p->target)
        return fail(RTK_ERR_INVALID, "rtk_progressive_step: %d samples is not a multiple of the chunk size %d (only the step that ends at the target may be)",
                    n_samples, p->chunk);
    if (p->n_ranks > 1 && d_rgb8) return fail(RTK_ERR_INVALID, "rtk_progressive_step: d_rgb8 must be null when n_ranks > 1 (use rtk_tiles_unpermute)");
    RTK_HIP(hipSetDevice(ctx_device(p->ctx)));
    bool launched = false;
    const hipError_t e = enqueue_step(p, n_samples, d_linear, d_rgb8, d_noise, d_counters, launched);
    if (e != hipSuccess) {
        if (launched) p->poisoned = true;  // part of the step is in the sums: the session cannot continue
        return fail(RTK_ERR_HIP, "rtk_progressive_step: launch failed: %s%s", hipGetErrorString(e), launched ? " (the session is poisoned)" : "");
    }
    p->done += n_samples;
    return RTK_OK;
}

int rtk_progressive_step_host(rtk_progressive* p, int32_t n_samples, double* h_linear, uint8_t* h_rgb8, float* h_noise, rtk_work_counters* counters) {
    int rc = usable(p, "rtk_progressive_step_host");
    if (rc != RTK_OK) return rc;
    RTK_HIP(hipSetDevice(ctx_device(p->ctx)));
    const bool compact = p->n_ranks > 1;
    const size_t pixels = compact ? p->n_slots() : size_t(p->cam.image_width) * p->cam.image_height;
    HostStaging s(p->real_mode == RTK_REAL_F64);
    const int lin = s.linear(pixels * 3, h_linear != nullptr), rgb8 = s.piece(pixels * 3, h_rgb8 != nullptr);
    const int noise = s.piece(pixels * sizeof(float), h_noise != nullptr), cnt = s.piece(sizeof(rtk_work_counters), counters != nullptr);
    hipError_t e = s.alloc();
    if (e == hipSuccess && counters) e = hipMemsetAsync(s.ptr(cnt), 0, sizeof(rtk_work_counters), p->stream);
    if (e != hipSuccess) return fail(RTK_ERR_HIP, "rtk_progressive_step_host: device buffers: %s", hipGetErrorString(e));
    rc = rtk_progressive_step(p, n_samples, s.ptr(lin), s.ptr<uint8_t>(rgb8), s.ptr<float>(noise), s.ptr<rtk_work_counters>(cnt));
    if (rc != RTK_OK) return rc;
    e = hipStreamSynchronize(p->stream);
    if (e == hipSuccess) e = s.download_linear(lin, h_linear);
    if (e == hipSuccess) e = s.download(rgb8, h_rgb8);
    if (e == hipSuccess) e = s.download(noise, h_noise);
    if (e == hipSuccess) e = s.download(cnt, counters);
    if (e != hipSuccess) {
        p->poisoned = true;
        return fail(RTK_ERR_HIP, "rtk_progressive_step_host: %s (the session is poisoned)", hipGetErrorString(e));
    }
    return RTK_OK;
}

int rtk_progressive_samples_done(const rtk_progressive* p) { return p ? p->done : fail(RTK_ERR_INVALID, "rtk_progressive_samples_done: null session"); }

int rtk_progressive_chunk_size(const rtk_progressive* p) { return p ? p->chunk : fail(RTK_ERR_INVALID, "rtk_progressive_chunk_size: null session"); }

int rtk_progressive_noise(rtk_progressive* p, rtk_noise_stats* out) {
    if (!out) return fail(RTK_ERR_INVALID, "rtk_progressive_noise: null argument");
    if (!p || p->poisoned) return fail(RTK_ERR_INVALID, "rtk_progressive_noise: null or poisoned session");
    RTK_HIP(hipSetDevice(ctx_device(p->ctx)));
    const int k = p->full_chunks();
    *out = rtk_noise_stats{};
    out->samples_done = p->done;
    out->full_chunks = k;
    out->valid = k >= 2 ? 1 : 0;
    if (k < 2) return RTK_OK;
    const int blocks = noise_partial_blocks(p->tm);
    double* result = p->d_stats + size_t(blocks) * 3;
    if (p->adaptive)  // per-tile K: a retired tile's estimate is the one it retired with
        RTK_HIP(launch_noise_stats_adaptive(p->d_s1, p->d_s2, p->tm, p->cam.image_width, p->cam.image_height, p->chunk, p->d_tile_spp, p->d_stats, result,
                                            p->stream));
    else
        RTK_HIP(launch_noise_stats(p->d_s1, p->d_s2, p->tm, p->cam.image_width, p->cam.image_height, k, p->d_stats, result, p->stream));
    double h[3];
    RTK_HIP(hipMemcpyAsync(h, result, sizeof h, hipMemcpyDeviceToHost, p->stream));
    RTK_HIP(hipStreamSynchronize(p->stream));
    // in-image pixels of this rank
    int64_t n_px = 0;
    for (int64_t lt = 0; lt < p->tm.n_tiles_local; lt++) n_px += tile_pixels(p->cam.image_width, p->cam.image_height, p->rank, p->n_ranks, lt);
    out->mean_se = n_px > 0 ? h[0] / double(n_px) : 0.0;
    out->max_se = h[1];
    out->mean_rel_se = n_px > 0 ? h[2] / double(n_px) : 0.0;
    return RTK_OK;
}

int64_t rtk_progressive_checkpoint_bytes(const rtk_progressive* p) {
    if (!p) return fail(RTK_ERR_INVALID, "rtk_progressive_checkpoint_bytes: null session");
    return checkpoint_bytes_for(p->cam.image_width, p->cam.image_height, p->n_ranks, p->real_mode, p->adaptive);
}

int rtk_progressive_save(rtk_progressive* p, void* h_buf, int64_t n) {
    if (!p || !h_buf) return fail(RTK_ERR_INVALID, "rtk_progressive_save: null argument");
    if (p->poisoned) return fail(RTK_ERR_INVALID, "rtk_progressive_save: the session is poisoned by an earlier failed step");
    const int64_t size = rtk_progressive_checkpoint_bytes(p);
    if (n < size) return fail(RTK_ERR_INVALID, "rtk_progressive_save: buffer of %lld bytes, the checkpoint needs %lld", (long long)n, (long long)size);
    RTK_HIP(hipSetDevice(ctx_device(p->ctx)));
    RTK_HIP(hipStreamSynchronize(p->stream));
    unsigned char* b = static_cast<unsigned char*>(h_buf);
    std::memset(b, 0, kCheckpointHeader);
    std::memcpy(b, kCheckpointMagic, 8);
    const int32_t fields[9] = {p->adaptive ? kCheckpointAdaptive : RTK_CHECKPOINT_VERSION, p->cam.image_width, p->cam.image_height, p->rank, p->n_ranks, p->real_mode, p->target, p->chunk, p->done};
    std::memcpy(b + 8, fields, sizeof fields);
    std::memcpy(b + 44, &p->seed, 4);
    std::memcpy(b + 48, &p->digest, 8);
    std::memcpy(b + 56, &p->cam, sizeof(rtk_camera));
    const size_t slots = p->n_slots();
    unsigned char* at = b + kCheckpointHeader;
    RTK_HIP(hipMemcpy(at, p->d_sum, slots * 3 * p->elem, hipMemcpyDeviceToHost));
    at += slots * 3 * p->elem;
    RTK_HIP(hipMemcpy(at, p->d_s1, slots * sizeof(double), hipMemcpyDeviceToHost));
    at += slots * sizeof(double);
    RTK_HIP(hipMemcpy(at, p->d_s2, slots * sizeof(double), hipMemcpyDeviceToHost));
    at += slots * sizeof(double);
    if (p->adaptive) {
        const int32_t ms[2] = {p->min_samples, 0};
        std::memcpy(at, &p->rel_target, 8);
        std::memcpy(at + 8, ms, 8);
        at += 16;
        RTK_HIP(hipMemcpy(at, p->d_tile_spp, size_t(p->tm.n_tiles_local) * sizeof(int32_t), hipMemcpyDeviceToHost));
        at += size_t(p->tm.n_tiles_local) * sizeof(int32_t);
    }
    Fnv64 f;
    f.add(b, size_t(at - b));
    std::memcpy(at, &f.h, 8);
    return RTK_OK;
}

int rtk_checkpoint_read_info(const void* h_buf, int64_t n, rtk_checkpoint_info* out) {
    if (!h_buf || !out) return fail(RTK_ERR_INVALID, "rtk_checkpoint_read_info: null argument");
    return parse_checkpoint(h_buf, n, out, nullptr, nullptr);
}

int rtk_checkpoint_read_adaptive(const void* h_buf, int64_t n, rtk_adaptive_opts* out, int32_t* h_tile_spp) {
    if (!h_buf || !out) return fail(RTK_ERR_INVALID, "rtk_checkpoint_read_adaptive: null argument");
    rtk_checkpoint_info info;
    const unsigned char* spp = nullptr;
    const int rc = parse_checkpoint(h_buf, n, &info, out, &spp);
    if (rc == RTK_OK && spp && h_tile_spp) std::memcpy(h_tile_spp, spp, size_t(rtk_tiles_per_rank(info.width, info.height, info.n_ranks)) * sizeof(int32_t));
    return rc;
}

int rtk_progressive_resume(rtk_ctx* ctx, const rtk_camera* cam, const rtk_render_opts* opts, const void* h_buf, int64_t n, rtk_progressive** out) {
    if (!ctx || !cam || !opts || !h_buf || !out) return fail(RTK_ERR_INVALID, "rtk_progressive_resume: null argument");
    *out = nullptr;
    rtk_checkpoint_info info;
    rtk_adaptive_opts ad{};
    const unsigned char* spp_at = nullptr;
    int rc = parse_checkpoint(h_buf, n, &info, &ad, &spp_at);
    if (rc != RTK_OK) return fail(rc, "rtk_progressive_resume: %s", std::string(g_error).c_str());
    const unsigned char* b = static_cast<const unsigned char*>(h_buf);
    if (info.target_spp != cam->samples_per_pixel)
        return fail(RTK_ERR_INVALID, "rtk_progressive_resume: the checkpoint's target is %d samples, the camera's %d", info.target_spp, cam->samples_per_pixel);
    if (std::memcmp(b + 56, cam, sizeof(rtk_camera)) != 0) return fail(RTK_ERR_INVALID, "rtk_progressive_resume: the checkpoint was made with another camera");
    if (info.seed != opts->seed) return fail(RTK_ERR_INVALID, "rtk_progressive_resume: the checkpoint's seed is %u, the call's %u", info.seed, opts->seed);
    if (info.real_mode != opts->real_mode)
        return fail(RTK_ERR_INVALID, "rtk_progressive_resume: the checkpoint's real mode is %d, the call's %d", info.real_mode, opts->real_mode);
    if (info.rank != opts->rank || info.n_ranks != opts->n_ranks)
        return fail(RTK_ERR_INVALID, "rtk_progressive_resume: the checkpoint is rank %d of %d, the call rank %d of %d", info.rank, info.n_ranks, opts->rank,
                    opts->n_ranks);
    uint64_t digest = 0;
    if (!ctx_scene(ctx, &digest)) return fail(RTK_ERR_NO_SCENE, "rtk_progressive_resume: no scene uploaded");
    if (info.scene_digest != digest)
        return fail(RTK_ERR_INVALID, "rtk_progressive_resume: the checkpoint was made on another scene or visiting order (digest %016llx, uploaded %016llx)",
                    (unsigned long long)info.scene_digest, (unsigned long long)digest);
    rtk_progressive* p = nullptr;
    if ((rc = make_session(ctx, cam, opts, "rtk_progressive_resume", &p, /*zero_sums=*/false)) != RTK_OK) return rc;  // the copies below fill every sum
    const size_t slots = p->n_slots();
    const unsigned char* at = b + kCheckpointHeader;
    hipError_t e = hipMemcpy(p->d_sum, at, slots * 3 * p->elem, hipMemcpyHostToDevice);
    at += slots * 3 * p->elem;
    if (e == hipSuccess) e = hipMemcpy(p->d_s1, at, slots * sizeof(double), hipMemcpyHostToDevice);
    at += slots * sizeof(double);
    if (e == hipSuccess) e = hipMemcpy(p->d_s2, at, slots * sizeof(double), hipMemcpyHostToDevice);
    p->done = info.samples_done;
    if (e == hipSuccess && spp_at) {  // version 2: the adaptive state -- retired tiles from the retire test of the step that ended at `done`
        std::vector<int32_t> spp(size_t(p->tm.n_tiles_local));
        std::memcpy(spp.data(), spp_at, spp.size() * sizeof(int32_t));
        p->adaptive = true;
        p->rel_target = ad.rel_target;
        p->min_samples = ad.min_samples;
        e = make_adaptive(p, spp.data());
        if (e == hipSuccess)
            e = launch_adaptive_restore(p->d_s1, p->d_s2, p->tm, p->cam.image_width, p->cam.image_height, p->chunk, p->d_tile_spp, p->done,
                                        p->min_samples <= p->done && p->done < p->target, p->rel_target, p->d_active, p->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
    }
    if (e != hipSuccess) {
        release(p);
        return fail(RTK_ERR_HIP, "rtk_progressive_resume: upload of the sums failed: %s", hipGetErrorString(e));
    }
    *out = p;
    return RTK_OK;
}

int rtk_progressive_set_adaptive(rtk_progressive* p, const rtk_adaptive_opts* opts) {
    int rc = usable(p, "rtk_progressive_set_adaptive");
    if (rc != RTK_OK) return rc;
    if (!opts) return fail(RTK_ERR_INVALID, "rtk_progressive_set_adaptive: null options");
    if (p->done != 0) return fail(RTK_ERR_INVALID, "rtk_progressive_set_adaptive: only before the first step (%d samples done)", p->done);
    if (!adaptive_opts_ok(opts->rel_target, opts->min_samples, p->chunk, p->target) || opts->reserved != 0)
        return fail(RTK_ERR_INVALID,
                    "rtk_progressive_set_adaptive: rel_target must be > 0 (%g); min_samples (%d) a multiple of the chunk size %d, at least 2 chunks and at "
                    "most the target %d; reserved 0",
                    opts->rel_target, opts->min_samples, p->chunk, p->target);
    RTK_HIP(hipSetDevice(ctx_device(p->ctx)));
    RTK_HIP(make_adaptive(p, nullptr));
    p->adaptive = true;
    p->rel_target = opts->rel_target;
    p->min_samples = opts->min_samples;
    return RTK_OK;
}

int rtk_adaptive_tile_samples(rtk_progressive* p, int32_t* h_out) {
    if (!p || !h_out) return fail(RTK_ERR_INVALID, "rtk_adaptive_tile_samples: null argument");
    if (p->poisoned) return fail(RTK_ERR_INVALID, "rtk_adaptive_tile_samples: the session is poisoned by an earlier failed step");
    const int64_t n = p->tm.n_tiles_local;
    if (!p->adaptive) {  // every in-image tile holds samples_done samples
        for (int64_t lt = 0; lt < n; lt++) h_out[lt] = tile_pixels(p->cam.image_width, p->cam.image_height, p->rank, p->n_ranks, lt) > 0 ? p->done : 0;
        return RTK_OK;
    }
    RTK_HIP(hipSetDevice(ctx_device(p->ctx)));
    RTK_HIP(hipStreamSynchronize(p->stream));
    RTK_HIP(hipMemcpy(h_out, p->d_tile_spp, size_t(n) * sizeof(int32_t), hipMemcpyDeviceToHost));
    return RTK_OK;
}

int rtk_adaptive_status(rtk_progressive* p, rtk_adaptive_state* out) {
    if (!p || !out) return fail(RTK_ERR_INVALID, "rtk_adaptive_status: null argument");
    const int64_t n = p->tm.n_tiles_local;
    std::vector<int32_t> spp(static_cast<size_t>(n)), active(static_cast<size_t>(n), 1);
    int rc = rtk_adaptive_tile_samples(p, spp.data());
    if (rc != RTK_OK) return fail(rc, "rtk_adaptive_status: %s", std::string(g_error).c_str());
    if (p->adaptive) RTK_HIP(hipMemcpy(active.data(), p->d_active, size_t(n) * sizeof(int32_t), hipMemcpyDeviceToHost));
    *out = rtk_adaptive_state{};
    int64_t pixels = 0;
    for (int64_t lt = 0; lt < n; lt++) {
        const int px = tile_pixels(p->cam.image_width, p->cam.image_height, p->rank, p->n_ranks, lt);
        if (px == 0) continue;  // a padding tile
        (active[size_t(lt)] ? out->active_tiles : out->retired_tiles)++;
        out->pixel_samples += int64_t(px) * spp[size_t(lt)];
        pixels += px;
    }
    out->mean_spp = pixels > 0 ? double(out->pixel_samples) / double(pixels) : 0.0;
    return RTK_OK;
}

int rtk_progressive_destroy(rtk_progressive* p) {
    if (!p) return RTK_OK;
    (void)hipSetDevice(ctx_device(p->ctx));
    (void)hipStreamSynchronize(p->stream);  // launches in flight still read the session's buffers
    release(p);
    return RTK_OK;
}

// rtk_progressive_denoise (guided false: first-hit AOVs, rtk_denoise) and rtk_progressive_denoise_guided (the guides of
// rtk_render_guides, rtk_denoise_guided): argument checks, the guides from the session's cache, the preview rebuilt, the filter.
static int progressive_denoise(const char* who, bool guided, rtk_progressive* p, int32_t aov_samples, const rtk_guide_opts* gopts, const rtk_denoise_opts* opts,
                               int32_t flags, void* d_out_linear, uint8_t* d_out_rgb8) {
    int follow = 0, max_bounces = 0;
    int rc = RTK_OK;
    if (guided && ((rc = resolve_guide_opts(gopts, &follow, &max_bounces, who)) != RTK_OK || (rc = check_denoise_flags(flags, who)) != RTK_OK)) return rc;
    if (guided && (rc = check_denoise_opts(opts, who)) != RTK_OK) return rc;
    if ((rc = usable(p, who)) != RTK_OK) return rc;
    if (p->n_ranks != 1) return fail(RTK_ERR_INVALID, "%s: whole images only (n_ranks must be 1, not %d)", who, p->n_ranks);
    if (aov_samples <= 0 || (guided && aov_samples > (1 << 20))) return fail(RTK_ERR_INVALID, "%s: aov_samples must be positive (%d)", who, aov_samples);
    if (p->full_chunks() < 2)
        return fail(RTK_ERR_INVALID, "%s: the noise estimate needs 2 full chunks in every tile (%d samples done, chunk %d)", who, p->done, p->chunk);
    if (!d_out_linear && !d_out_rgb8) return fail(RTK_ERR_INVALID, "%s: no output", who);
    if (!guided && (rc = check_denoise_opts(opts, who)) != RTK_OK) return rc;
    RTK_HIP(hipSetDevice(ctx_device(p->ctx)));
    const int W = p->cam.image_width, H = p->cam.image_height;
    const size_t px = size_t(W) * H;
    float* aov = nullptr;
    const rtk_render_opts ro{p->seed, p->real_mode, 0, 1, 0, 0, p->stream};
    if (guided) {
        for (auto& g : p->guides)
            if (g.samples == aov_samples && g.follow == follow && g.max_bounces == max_bounces) aov = g.d;
        if (!aov) {
            RTK_HIP(hipMalloc(reinterpret_cast<void**>(&aov), px * 16 * sizeof(float)));
            const rtk_guide_opts go{follow, max_bounces};
            if ((rc = rtk_render_guides(p->ctx, &p->cam, &ro, aov_samples, &go, aov)) != RTK_OK) {
                (void)hipFree(aov);
                return rc;
            }
            p->guides.push_back({aov_samples, follow, max_bounces, aov});
        }
    } else {
        for (auto& a : p->aovs)
            if (a.first == aov_samples) aov = a.second;
        if (!aov) {
            RTK_HIP(hipMalloc(reinterpret_cast<void**>(&aov), px * 8 * sizeof(float)));
            if ((rc = rtk_render_aovs(p->ctx, &p->cam, &ro, aov_samples, aov)) != RTK_OK) {
                (void)hipFree(aov);
                return rc;
            }
            p->aovs.emplace_back(aov_samples, aov);
        }
    }
    if (!p->d_preview) RTK_HIP(hipMalloc(&p->d_preview, px * 3 * p->elem));
    if (!p->d_preview_se) RTK_HIP(hipMalloc(reinterpret_cast<void**>(&p->d_preview_se), px * sizeof(float)));
    const int32_t* spp = p->adaptive ? p->d_tile_spp : nullptr;
    const hipError_t pe = with_real(p->real_mode, [&](auto real) {
        return launch_preview<decltype(real)>(p->d_sum, p->d_s1, p->d_s2, p->tm, W, H, p->chunk, p->done, spp, p->d_preview, p->d_preview_se, p->stream);
    });
    if (pe != hipSuccess) return launched(who, pe);
    return guided ? rtk_denoise_guided(p->ctx, W, H, p->real_mode, p->d_preview, aov, p->d_preview_se, opts, flags, d_out_linear, d_out_rgb8, p->stream)
                  : rtk_denoise(p->ctx, W, H, p->real_mode, p->d_preview, aov, p->d_preview_se, opts, d_out_linear, d_out_rgb8, p->stream);
}

static int progressive_denoise_host(const char* who, bool guided, rtk_progressive* p, int32_t aov_samples, const rtk_guide_opts* gopts,
                                    const rtk_denoise_opts* opts, int32_t flags, double* h_linear, uint8_t* h_rgb8) {
    int follow = 0, max_bounces = 0;
    int rc = RTK_OK;
    if (guided && ((rc = resolve_guide_opts(gopts, &follow, &max_bounces, who)) != RTK_OK || (rc = check_denoise_flags(flags, who)) != RTK_OK)) return rc;
    if (guided && (rc = check_denoise_opts(opts, who)) != RTK_OK) return rc;
    if ((rc = usable(p, who)) != RTK_OK) return rc;
    if (p->n_ranks != 1) return fail(RTK_ERR_INVALID, "%s: whole images only (n_ranks must be 1, not %d)", who, p->n_ranks);
    if (!h_linear && !h_rgb8) return fail(RTK_ERR_INVALID, "%s: no output", who);
    RTK_HIP(hipSetDevice(ctx_device(p->ctx)));
    const size_t n = size_t(p->cam.image_width) * p->cam.image_height * 3;
    HostStaging s(p->real_mode == RTK_REAL_F64);
    const int lin = s.linear(n, h_linear != nullptr), rgb8 = s.piece(n, h_rgb8 != nullptr);
    hipError_t e = s.alloc();
    if (e == hipSuccess) {
        rc = guided ? rtk_progressive_denoise_guided(p, aov_samples, gopts, opts, flags, s.ptr(lin), s.ptr<uint8_t>(rgb8))
                    : rtk_progressive_denoise(p, aov_samples, opts, s.ptr(lin), s.ptr<uint8_t>(rgb8));
        if (rc != RTK_OK) return rc;
        e = hipStreamSynchronize(p->stream);
    }
    if (e == hipSuccess) e = s.download_linear(lin, h_linear);
    if (e == hipSuccess) e = s.download(rgb8, h_rgb8);
    return launched(who, e);
}

int rtk_progressive_denoise(rtk_progressive* p, int32_t aov_samples, const rtk_denoise_opts* opts, void* d_out_linear, uint8_t* d_out_rgb8) {
    return progressive_denoise("rtk_progressive_denoise", false, p, aov_samples, nullptr, opts, 0, d_out_linear, d_out_rgb8);
}

int rtk_progressive_denoise_host(rtk_progressive* p, int32_t aov_samples, const rtk_denoise_opts* opts, double* h_linear, uint8_t* h_rgb8) {
    return progressive_denoise_host("rtk_progressive_denoise_host", false, p, aov_samples, nullptr, opts, 0, h_linear, h_rgb8);
}

int rtk_progressive_denoise_guided(rtk_progressive* p, int32_t aov_samples, const rtk_guide_opts* gopts, const rtk_denoise_opts* opts, int32_t flags,
                                   void* d_out_linear, uint8_t* d_out_rgb8) {
    return progressive_denoise("rtk_progressive_denoise_guided", true, p, aov_samples, gopts, opts, flags, d_out_linear, d_out_rgb8);
}

int rtk_progressive_denoise_guided_host(rtk_progressive* p, int32_t aov_samples, const rtk_guide_opts* gopts, const rtk_denoise_opts* opts, int32_t flags,
                                        double* h_out_linear, uint8_t* h_out_rgb8) {
    return progressive_denoise_host("rtk_progressive_denoise_guided_host", true, p, aov_samples, gopts, opts, flags, h_out_linear, h_out_rgb8);
}

}  // extern "C"
