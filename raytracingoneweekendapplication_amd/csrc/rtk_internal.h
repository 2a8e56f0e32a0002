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

// f(real{}) for the arithmetic type asked for at run time: a lane-per-ray entry point writes its launch once, as a generic lambda
// over the tag (rtk_image_pass.h's with_real_demod is the image passes' form, with the demodulation as a second tag).
template <typename F>
auto with_real(int real_mode, F&& f) {
    return real_mode == RTK_REAL_F64 ? f(double{}) : f(float{});
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

// The device side of a *_host entry point: one allocation cut into pieces, each on a 16-byte boundary (guides, AOVs and every
// 16-byte access need it), freed when the object goes out of scope.  The entry point plans the pieces; then alloc(), the uploads,
// the asynchronous entry point called with ptr() of each piece, its stream synchronised, the downloads -- the sequence
// run_host_form (below) performs for the lane-per-ray families and the image passes still write out.  A piece planned with
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

    hipError_t upload(int k, const void* h) { return hipMemcpy(ptr(k), h, pieces_[k].bytes, hipMemcpyHostToDevice); }
    hipError_t download(int k, void* h) { return h ? hipMemcpy(h, ptr(k), pieces_[k].bytes, hipMemcpyDeviceToHost) : hipSuccess; }
    hipError_t upload_linear(int k, const double* h) {  // in F32 mode each double is rounded to float here, on the host
        if (f64_) return upload(k, h);
        tmp_.resize(pieces_[k].bytes / sizeof(float));
        for (size_t n = 0; n < tmp_.size(); n++) tmp_[n] = float(h[n]);
        return upload(k, tmp_.data());
    }
    hipError_t download_linear(int k, double* h) {
        if (f64_ || !h) return download(k, h);
        tmp_.resize(pieces_[k].bytes / sizeof(float));
        const hipError_t e = download(k, tmp_.data());
        for (size_t n = 0; n < tmp_.size(); n++) h[n] = double(tmp_[n]);
        return e;
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
// staged pieces; RTK_OK or its own refusal, which is returned as it is), `stream` synchronised, the outputs down.  The first
// HIP error ends it and is the result (RTK_ERR_HIP, the text naming `who`).  A linear array is doubles on the host.
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
template <typename Call>
int run_host_form(const char* who, hipStream_t stream, HostStaging& s, std::initializer_list<HostIn> inputs, Call&& call, std::initializer_list<HostOut> outputs) {
    hipError_t e = s.alloc();
    for (const HostIn& in : inputs)
        if (e == hipSuccess) e = in.linear ? s.upload_linear(in.piece, static_cast<const double*>(in.host)) : s.upload(in.piece, in.host);
    if (e != hipSuccess) return launched(who, e);
    const int rc = call();
    if (rc != RTK_OK) return rc;
    e = hipStreamSynchronize(stream);
    for (const HostOut& out : outputs)
        if (e == hipSuccess) e = out.linear ? s.download_linear(out.piece, static_cast<double*>(out.host)) : s.download(out.piece, out.host);
    return launched(who, e);
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
int frame_chunk_size(int spp);                        // the one-shot frame's chunk size (variant 0)
int chunks_per_launch(size_t plane_bytes);            // ... and chunk planes per launch
size_t camera_record_bytes();
// One render launch over tp's chunks into the context's partial-sum workspace (grown to workspace_bytes; *partial = it).
// allow_lds / diag: what rtk_render_device derives from opts->variant (sessions render with variant 0).
hipError_t render_chunks(rtk_ctx* ctx, int real_mode, const void* d_cam, const TileMap& tp, uint32_t seed, unsigned long long* counters,
                         const int32_t* tile_order, unsigned int* tile_cost, size_t workspace_bytes, hipStream_t stream, void** partial, bool allow_lds = true,
                         uint32_t diag = 0u);

// rtk_render_tiles (rtk_tiles.hip): rtk_render_device's own frame set-up for `cam` and `opts` -- tile map and chunk boundaries, the
// partial-sum workspace grown, the camera record in its device slot on the frame's stream -- plus the context's tile list
// (d_list[n_tiles_local], its length at d_count).  The learned tile order is not touched.  Refuses, in this order: a frame of more
// than one launch (RTK_ERR_INVALID; host arithmetic only), a null context, RTK_ERR_NO_SCENE; `who` names the caller in the text.
struct TileFrame {
    TileMap tm;
    int chunk_size = 0;
    size_t workspace_bytes = 0;
    const void* d_cam = nullptr;
    bool allow_lds = true;
    uint32_t diag = 0;
    hipStream_t stream = nullptr;
    int32_t* d_list = nullptr;
    int32_t* d_count = nullptr;
};
int stage_tile_frame(rtk_ctx* ctx, const rtk_camera* cam, const rtk_render_opts* opts, const char* who, TileFrame& out);

// rtk_render_views (rtk_views.hip).  stage_view_batch: the batch's set-up on opts->stream for n_views validated cameras of one
// size -- the tile map over local tiles [view][tile of a view's grid] with the single frame's chunk boundaries, the passes
// under the workspace budget, the partial-sum workspace grown, the view records (camera + hashed seed; seeds null = opts->seed)
// uploaded into the context's table through its ring of pinned buffers, a work-item counter per pass, the progress
// callback's items.  The learned tile order is not touched.
struct ViewBatch {
    TileMap tm;  // every chunk of the batch
    int planes_per_pass = 0, n_passes = 0;
    size_t plane = 0;  // bytes of one chunk plane [view * tiles + tile][3][64]
    void* d_partial = nullptr;
    const void* d_views = nullptr;
    unsigned int* pass_counter[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    bool allow_lds = true;
    uint32_t diag = 0;
    hipStream_t stream = nullptr;
};
int stage_view_batch(rtk_ctx* ctx, int32_t n_views, const rtk_camera* cams, const uint32_t* seeds, const rtk_render_opts* opts, ViewBatch& out);
// rtk_render_device apart from the context's learned tile order: row-major hand-out, no cost measured, the stored order and the
// shape it belongs to left as they are (a batch's per-view form).
int render_frame_apart(rtk_ctx* ctx, const rtk_camera* cam, const rtk_render_opts* opts, void* d_linear, uint8_t* d_rgb8, rtk_work_counters* d_counters);
int frame_chunk_count(int spp, int variant);  // sample chunks of a pixel (rtk_render_opts.variant's chunk-size bits included)

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
