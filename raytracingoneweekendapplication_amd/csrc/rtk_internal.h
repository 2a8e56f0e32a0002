// rtk_internal.h -- what the translation units of librtk_hip.so share besides the public ABI (include/rtk.h).
#ifndef RTK_INTERNAL_H
#define RTK_INTERNAL_H

#include <hip/hip_runtime.h>

#include <initializer_list>
#include <string>
#include <type_traits>
#include <vector>

#include "rtk_device_layout.h"

#include "rtk.h"

namespace rtk {

extern thread_local std::string g_error;            // text behind rtk_last_error()
int fail(int code, const char* fmt, ...);           // records the text, returns `code`

// A HIP runtime call inside an entry point: on failure the entry point returns RTK_ERR_HIP, the text naming the call.
#define RTK_HIP(call)                                                                                     \
    do {                                                                                                  \
        hipError_t e_ = (call);                                                                           \
        if (e_ != hipSuccess) return ::rtk::fail(RTK_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

// What an entry point returns for the HIP result of its launches, its stream wait and its copies: the text names the entry point.
inline int launched(const char* who, hipError_t e) { return e == hipSuccess ? RTK_OK : fail(RTK_ERR_HIP, "%s: %s", who, hipGetErrorString(e)); }

// FNV-1a 64 over byte ranges: the scene digest of progressive sessions and the checksum of their checkpoints.
struct Fnv64 {
    uint64_t h = 1469598103934665603ull;
    void add(const void* p, size_t n) {
        const unsigned char* b = static_cast<const unsigned char*>(p);
        for (size_t k = 0; k < n; k++) h = (h ^ b[k]) * 1099511628211ull;
    }
    template <typename T>
    void add_pod(const T& v) { add(&v, sizeof v); }
    template <typename T>
    void add_table(const T* t, int64_t n) {  // explicit _pad fields are zeroed: a caller may leave them unset
        for (int64_t k = 0; k < n; k++) {
            T v = t[k];
            if constexpr (std::is_same_v<T, rtk_sphere> || std::is_same_v<T, rtk_quad> || std::is_same_v<T, rtk_triangle> || std::is_same_v<T, rtk_medium>)
                v._pad = 0;
            add_pod(v);
        }
    }
};

// include/rtk.h: guide and AOV buffers are accessed 16 bytes at a time.  RTK_OK, or RTK_ERR_INVALID with `arg` named in g_error.
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline int check_aligned16(const void* p, const char* who, const char* arg) {
    return aligned16(p) ? RTK_OK : fail(RTK_ERR_INVALID, "%s: %s must be 16-byte aligned", who, arg);
}

// Every other device buffer needs the alignment of its element type (`align`, a power of two); null is aligned.
inline int check_aligned(const void* p, size_t align, const char* who, const char* arg) {
    return (reinterpret_cast<uintptr_t>(p) & (align - 1)) == 0 ? RTK_OK : fail(RTK_ERR_INVALID, "%s: %s must be %zu-byte aligned", who, arg, align);
}

// The checks every image entry point makes of its size and arithmetic type: RTK_OK, or RTK_ERR_INVALID with the text in g_error.
// The passes that take a camera say "bad camera dimensions", the ones that take a width and a height name the size.
inline bool image_size_ok(int w, int h) { return w > 0 && h > 0 && w <= 65536 && h <= 65536; }
inline int check_image_size(const char* who, int w, int h) {
    return image_size_ok(w, h) ? RTK_OK : fail(RTK_ERR_INVALID, "%s: bad image size %dx%d", who, w, h);
}
inline int check_camera_size(const char* who, const rtk_camera& cam) {
    return image_size_ok(cam.image_width, cam.image_height) ? RTK_OK : fail(RTK_ERR_INVALID, "%s: bad camera dimensions", who);
}
inline int check_real_mode(const char* who, int mode) {
    return mode == RTK_REAL_F64 || mode == RTK_REAL_F32 ? RTK_OK : fail(RTK_ERR_INVALID, "%s: unknown real_mode %d", who, mode);
}
// The frame entry points' camera (a frame's samples are cut into chunks whose boundaries are 16-bit) and rank.
inline int check_frame_camera(const char* who, const rtk_camera& cam) {
    return cam.image_width > 0 && cam.image_height > 0 && cam.samples_per_pixel > 0 && cam.samples_per_pixel <= 32767 && cam.max_depth >= 0
               ? RTK_OK
               : fail(RTK_ERR_INVALID, "%s: bad camera dimensions (samples_per_pixel must be 1..32767)", who);
}
inline int check_rank(const char* who, const rtk_render_opts& opts) {
    return opts.n_ranks >= 1 && opts.rank >= 0 && opts.rank < opts.n_ranks ? RTK_OK : fail(RTK_ERR_INVALID, "%s: bad rank %d of %d", who, opts.rank, opts.n_ranks);
}

// f(real{}) for the arithmetic type asked for at run time: a lane-per-ray entry point writes its launch once, as a generic lambda
// over the tag (rtk_image_pass.h's with_real_demod is the image passes' form, with the demodulation as a second tag).
template <typename F>
auto with_real(int real_mode, F&& f) {
    return real_mode == RTK_REAL_F64 ? f(double{}) : f(float{});
}

// Device memory that its owner keeps and grows on demand: *p holds *have bytes; a larger need waits for the device (earlier
// launches may still read the old buffer), frees it and allocates `need` bytes (their contents undefined).  Otherwise nothing.
template <typename T>
hipError_t grow_device(T** p, size_t* have, size_t need) {
    if (need <= *have) return hipSuccess;
    hipError_t e = hipSuccess;
    if (*p) {
        if ((e = hipDeviceSynchronize()) != hipSuccess || (e = hipFree(*p)) != hipSuccess) return e;
        *p = nullptr;
        *have = 0;
    }
    if ((e = hipMalloc(reinterpret_cast<void**>(p), need)) == hipSuccess) *have = need;
    return e;
}

// What a path kernel that is given its rays reads of a camera: ray_color's background, max_depth and the samples per ray.
inline rtk_camera path_camera(const rtk_vec3& background, int max_depth, int samples) {
    rtk_camera cam{};
    cam.background = background;
    cam.max_depth = max_depth;
    cam.samples_per_pixel = samples > 0 ? samples : 1;
    return cam;
}

// include/rtk.h: an output may not alias an input.  RTK_OK, or RTK_ERR_INVALID naming the output and the first of `inputs` it
// shares an address with.  A null output overlaps nothing, and neither do arrays of no bytes (n == 0).
struct Span {
    const void* p;
    size_t bytes;
    const char* name;
};
inline int check_apart(const char* who, const Span& out, std::initializer_list<Span> inputs) {
    if (!out.p) return RTK_OK;
    const uintptr_t o = reinterpret_cast<uintptr_t>(out.p);
    for (const Span& in : inputs) {
        const uintptr_t i = reinterpret_cast<uintptr_t>(in.p);
        if (!(o + out.bytes <= i || i + in.bytes <= o)) return fail(RTK_ERR_INVALID, "%s: %s overlaps %s", who, out.name, in.name);
    }
    return RTK_OK;
}

// n reals in device memory (doubles, or floats unless f64) as n doubles on the host; tmp holds the floats in between.
inline hipError_t download_reals(bool f64, const void* d, size_t n, double* h, std::vector<float>& tmp) {
    if (f64) return hipMemcpy(h, d, n * sizeof(double), hipMemcpyDeviceToHost);
    tmp.resize(n);
    const hipError_t e = hipMemcpy(tmp.data(), d, n * sizeof(float), hipMemcpyDeviceToHost);
    for (size_t k = 0; k < n; k++) h[k] = double(tmp[k]);
    return e;
}

// The device side of a *_host entry point: one allocation cut into pieces, each on a 16-byte boundary (guides, AOVs and every
// 16-byte access need it), freed when the object goes out of scope.  The entry point plans the pieces; then alloc(), the uploads,
// the asynchronous entry point called with ptr() of each piece, its stream synchronised, the downloads -- the sequence
// run_host_form (below) performs for the lane-per-ray and frame families and the image passes still write out.  A piece planned with
// wanted = false (an optional output the caller passed as null) takes no memory and has a null ptr(); a download into a null
// host pointer does nothing.
// "Linear" pieces hold `real`s (double or float, by f64) that the host sees as doubles.
class HostStaging {
public:
    explicit HostStaging(bool f64) : f64_(f64) {}
    HostStaging(const HostStaging&) = delete;
    HostStaging& operator=(const HostStaging&) = delete;
    ~HostStaging() { (void)hipFree(base_); }

    int piece(size_t bytes, bool wanted = true) {  // the piece's index
        pieces_.push_back(Piece{wanted ? total_ : kAbsent, bytes});
        if (wanted) total_ = (total_ + bytes + 15) / 16 * 16;
        return int(pieces_.size()) - 1;
    }
    int linear(size_t n_reals, bool wanted = true) { return piece(n_reals * (f64_ ? sizeof(double) : sizeof(float)), wanted); }
    hipError_t alloc() { return total_ ? hipMalloc(reinterpret_cast<void**>(&base_), total_) : hipSuccess; }

    template <typename T = void>
    T* ptr(int k) const { return pieces_[k].offset == kAbsent ? nullptr : reinterpret_cast<T*>(base_ + pieces_[k].offset); }

    hipError_t upload(int k, const void* h) { return h ? hipMemcpy(ptr(k), h, pieces_[k].bytes, hipMemcpyHostToDevice) : hipSuccess; }
    hipError_t download(int k, void* h) { return h ? hipMemcpy(h, ptr(k), pieces_[k].bytes, hipMemcpyDeviceToHost) : hipSuccess; }
    hipError_t upload_linear(int k, const double* h) {  // in F32 mode each double is rounded to float here, on the host
        if (f64_ || !h) return upload(k, h);
        tmp_.resize(pieces_[k].bytes / sizeof(float));
        for (size_t n = 0; n < tmp_.size(); n++) tmp_[n] = float(h[n]);
        return upload(k, tmp_.data());
    }
    hipError_t download_linear(int k, double* h) {
        return h ? download_reals(f64_, ptr(k), pieces_[k].bytes / (f64_ ? sizeof(double) : sizeof(float)), h, tmp_) : hipSuccess;
    }

private:
    static constexpr size_t kAbsent = ~size_t(0);
    struct Piece {
        size_t offset, bytes;
    };
    bool f64_;
    char* base_ = nullptr;
    size_t total_ = 0;
    std::vector<Piece> pieces_;
    std::vector<float> tmp_;   // the float image between the host's doubles and an F32 piece
};

// A *_host entry point after its checks, hipSetDevice and the plan of `s`: alloc, the inputs up, `call` (the device form on the
// staged pieces, after whatever it zeroes of them; RTK_OK or its own refusal, which is returned as it is), `stream` synchronised,
// the outputs down.  The first HIP error ends it and is the result (RTK_ERR_HIP, the text naming `who`).  A linear array is
// doubles on the host.  run_host_form_waiting is the same with the wait as the caller's function (RTK_OK or its refusal): the
// render forms wait with wait_with_progress.
struct HostIn {
    int piece;
    const void* host;
    bool linear = false;
};
struct HostOut {
    int piece;
    void* host;
    bool linear = false;
};
template <typename Call, typename Wait>
int run_host_form_waiting(const char* who, HostStaging& s, std::initializer_list<HostIn> inputs, Call&& call, Wait&& wait, std::initializer_list<HostOut> outputs) {
    hipError_t e = s.alloc();
    for (const HostIn& in : inputs)
        if (e == hipSuccess) e = in.linear ? s.upload_linear(in.piece, static_cast<const double*>(in.host)) : s.upload(in.piece, in.host);
    if (e != hipSuccess) return launched(who, e);
    int rc = call();
    if (rc == RTK_OK) rc = wait();
    if (rc != RTK_OK) return rc;
    for (const HostOut& out : outputs)
        if (e == hipSuccess) e = out.linear ? s.download_linear(out.piece, static_cast<double*>(out.host)) : s.download(out.piece, out.host);
    return launched(who, e);
}
template <typename Call>
int run_host_form(const char* who, hipStream_t stream, HostStaging& s, std::initializer_list<HostIn> inputs, Call&& call, std::initializer_list<HostOut> outputs) {
    return run_host_form_waiting(who, s, inputs, call, [&] { return launched(who, hipStreamSynchronize(stream)); }, outputs);
}

int ctx_device(const rtk_ctx* ctx);
// Progressive sessions (rtk_progressive.cpp) -- what they use of a context and of the one-shot frame's rules:
int ctx_scene(const rtk_ctx* ctx, uint64_t* digest);  // 1 when a scene is uploaded; *digest = its digest
// The last refusal of a lane-per-ray entry point, after every check that needs no device: the context, then its scene where
// the entry point reads one.
inline int check_ctx(const char* who, const rtk_ctx* ctx, bool needs_scene) {
    if (!ctx) return fail(RTK_ERR_INVALID, "%s: null context", who);
    uint64_t digest = 0;
    return !needs_scene || ctx_scene(ctx, &digest) ? RTK_OK : fail(RTK_ERR_NO_SCENE, "%s: no scene uploaded", who);
}
uint32_t ctx_features(const rtk_ctx* ctx);            // Feature bits of the uploaded scene (F_MEDIA: rtk_query_occluded's early exit)
int32_t ctx_n_materials(const rtk_ctx* ctx);          // table sizes of the uploaded description (index checks of rtk_debug_scatter
int32_t ctx_n_textures(const rtk_ctx* ctx);           // and rtk_debug_texture)
int frame_chunk_size(int spp);                        // the one-shot frame's chunk size (variant 0): what a checkpoint's header must hold
size_t camera_record_bytes();

// ---- the frame entry points (rtk_frame_host.cpp) ----
// rtk_render_opts.variant as every frame entry point reads it (the other bits are not used).
struct Variant {
    bool allow_lds;    // bit 0 clear; set = keep the program in global memory (A/B)
    bool whole_pixel;  // bit 1: one lane per pixel for all samples (tests)
    bool fixed_order;  // bit 2: row-major tile hand-out, no order learned (A/B, tests)
    int chunk_ab;      // bits 3..4, tools/: chunk size A/B (0 = default 8, 1 = 4, 2 = 2, 3 = 16)
    uint32_t diag;     // bits 5..7: grid cap, host only (rtk_grid_plan.h; tests, tools); bits 8..21, 23: scheduler policy / program layout A/B used by tools/ and tests only
    bool compact;      // bit 22: the tile-buffer layout for a single rank too
    bool one_pass;     // bit 24: one pass whatever the chunk count (tests: same image)
};
inline Variant decode_variant(int v) {
    return Variant{(v & 1) == 0, (v & 2) != 0, (v & 4) != 0, (v >> 3) & 3, uint32_t(v) & 0xBFFFE0u, (v & (1 << 22)) != 0, (v & (1 << 24)) != 0};
}

// The arithmetic of a frame, host only: the tile map of a camera and a rank with every chunk boundary, the bytes of a chunk
// plane, the chunk planes a launch may fill under the workspace budget and so the launches ("passes") of the frame.  A frame
// of several passes carries its running sum in one more plane behind the passes' planes.
struct FramePlan {
    TileMap tm;        // every chunk of the frame; n_tiles_local = int32_t(n_tiles)
    int64_t n_tiles;   // local tiles -- of every view of a batch
    int chunk_size, planes_per_pass, n_passes;
    size_t elem, plane;  // bytes of a real; of one chunk plane [local tile][3][64]
    Variant variant;
    hipStream_t stream;
    int64_t n_items() const { return n_tiles * tm.n_chunks; }
    size_t workspace_bytes() const { return plane * size_t(n_passes > 1 ? planes_per_pass + 1 : tm.n_chunks); }
};
// cam: check_frame_camera's conditions but max_depth; opts: n_ranks >= 1.
FramePlan plan_frame(const rtk_camera& cam, const rtk_render_opts& opts);
// The batch of n_views frames of `one`: local tiles [view][tile of a view's grid], one rank, the single frame's chunk boundaries.
// n_items() may pass 31 bits: the caller refuses such a batch before it uses tm.
FramePlan plan_views(const FramePlan& one, int32_t n_views);
// Pass k of a plan over the workspace at d_partial: its chunks numbered from 0 -- planes, work items and chunk boundaries are
// the pass's own -- and the running-sum plane (null for a frame of one pass).
struct FramePass {
    TileMap tm;
    bool first, last;
    void* acc;
};
FramePass frame_pass(const FramePlan& f, int k, void* d_partial);
// A frame's work-item counters, one per pass, from the context's ring; with several passes each is zeroed on the stream here,
// before the first launch (progress reports add them up).  The context's progress bookkeeping describes this frame afterwards.
hipError_t take_pass_counters(rtk_ctx* ctx, const FramePlan& f, unsigned int** counters);

// One render launch over tp's chunks into the context's partial-sum workspace (grown to workspace_bytes; *partial = it).
// v: opts->variant decoded (sessions render with variant 0).
hipError_t render_chunks(rtk_ctx* ctx, int real_mode, const void* d_cam, const TileMap& tp, uint32_t seed, unsigned long long* counters,
                         const int32_t* tile_order, unsigned int* tile_cost, size_t workspace_bytes, hipStream_t stream, void** partial,
                         const Variant& v = decode_variant(0));

// rtk_render_tiles (rtk_tiles.hip): rtk_render_device's own frame set-up for `cam` and `opts` -- the plan, the partial-sum
// workspace grown, the camera record in its device slot on the frame's stream -- plus the context's tile list (d_list[n_tiles],
// its length at d_count).  The learned tile order is not touched.  Refuses, in this order: a frame of more than one launch
// (RTK_ERR_INVALID; host arithmetic only), a null context, RTK_ERR_NO_SCENE; `who` names the caller in the text.
struct TileFrame {
    FramePlan plan;
    const void* d_cam = nullptr;
    int32_t* d_list = nullptr;
    int32_t* d_count = nullptr;
};
int stage_tile_frame(rtk_ctx* ctx, const rtk_camera* cam, const rtk_render_opts* opts, const char* who, TileFrame& out);

// rtk_render_views (rtk_views.hip).  stage_view_batch: the set-up on the plan's stream of a batch (plan_views) of n_views
// validated cameras -- the partial-sum workspace grown, the view records (camera + hashed seed; seeds null = opts->seed)
// uploaded into the context's table through its ring of pinned buffers, a work-item counter per pass, the progress callback's
// items.  The learned tile order is not touched.
struct ViewBatch {
    void* d_partial = nullptr;
    const void* d_views = nullptr;
    unsigned int* pass_counter[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
};
int stage_view_batch(rtk_ctx* ctx, const FramePlan& batch, int32_t n_views, const rtk_camera* cams, const uint32_t* seeds, const rtk_render_opts* opts, ViewBatch& out);
// rtk_render_device apart from the context's learned tile order: row-major hand-out, no cost measured, the stored order and the
// shape it belongs to left as they are (a batch's per-view form).
int render_frame_apart(rtk_ctx* ctx, const rtk_camera* cam, const rtk_render_opts* opts, void* d_linear, uint8_t* d_rgb8, rtk_work_counters* d_counters);

// The uploaded scene's device view per arithmetic type, and a camera's device record (for the AOV pass, rtk_denoise.hip).
template <typename real>
const SceneView<real>& ctx_view(const rtk_ctx* ctx);
template <typename real>
CameraRec<real> device_camera(const rtk_camera& cam);

// The denoiser's ping-pong buffers: context-owned device memory of at least `bytes`, grown on demand (apart from the render's
// partial-sum workspace).  Growing waits for the device: earlier launches may still read the old buffers.
hipError_t denoise_workspace(rtk_ctx* ctx, size_t bytes, void** out);
// The surface gathers' partial sums (rtk_gather.cpp): context-owned device memory of at least `bytes`, grown like the render's
// workspace (growing waits for the device) and apart from it.
hipError_t gather_workspace(rtk_ctx* ctx, size_t bytes, void** out);
// RTK_OK, or RTK_ERR_INVALID with the reason in g_error, for rtk_denoise_opts out of range (null = every default).
int check_denoise_opts(const rtk_denoise_opts* opts, const char* who);
// The same for rtk_guide_opts (null = every default) and the guided filter's flags; *follow / *max_bounces = the resolved options.
int resolve_guide_opts(const rtk_guide_opts* gopts, int* follow, int* max_bounces, const char* who);
int check_denoise_flags(int32_t flags, const char* who);

// Block until streams[i] (on ctxs[i]'s device) has drained, i = 0..n-1, feeding ctxs[0]'s progress callback
// (rtk_set_progress_callback) from the work-item counters of the launches in flight.
int wait_with_progress(rtk_ctx* const* ctxs, const hipStream_t* streams, int n);

}  // namespace rtk

#endif  // RTK_INTERNAL_H
