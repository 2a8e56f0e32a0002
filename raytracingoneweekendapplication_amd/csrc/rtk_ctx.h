// rtk_ctx.h -- struct rtk_ctx, for the two files that own it: rtk_api.cpp (its life: rtk_init, rtk_destroy, the scene uploads) and
// rtk_frame_host.cpp (the frame entry points, which use its workspaces and rings).  Every other file sees a context through the
// ctx_* accessors of rtk_internal.h.
#ifndef RTK_CTX_H
#define RTK_CTX_H

#include <vector>

#include "rtk_internal.h"

namespace rtk {

// Device image of a scene for one arithmetic type
template <typename real>
struct DeviceScene {
    std::vector<void*> allocations;
    SceneView<real> view{};
    int64_t bytes = 0;

    void release() {
        for (void* p : allocations) (void)hipFree(p);
        allocations.clear();
        view = SceneView<real>{};
        bytes = 0;
    }
    template <typename T>
    int upload(const std::vector<T>& host, const T** out) {
        *out = nullptr;
        if (host.empty()) return RTK_OK;
        void* d = nullptr;
        RTK_HIP(hipMalloc(&d, host.size() * sizeof(T)));
        allocations.push_back(d);
        RTK_HIP(hipMemcpy(d, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
        bytes += int64_t(host.size() * sizeof(T));
        *out = static_cast<const T*>(d);
        return RTK_OK;
    }
};

// Slots of the per-launch rings (work-item counters, camera records); rtk_api.cpp, which allocates them, holds the value.
extern const unsigned int kCounterRing;
constexpr size_t kCameraStride = 256;
static_assert(sizeof(CameraRec<double>) <= kCameraStride, "camera stride");

}  // namespace rtk

struct rtk_ctx {
    int device = 0;
    bool has_scene = false;
    uint32_t features = 0;
    int32_t n_ops = 0;
    int32_t n_materials = 0, n_textures = 0;  // of the uploaded description (index checks of the known-answer entry points)
    uint64_t scene_digest = 0;                // of the uploaded program and tables (progressive sessions refuse another scene)
    rtk::DeviceScene<double> scene64;
    rtk::DeviceScene<float> scene32;
    // Words the persistent waves pull tile indices from; one per launch in a
    // small ring so that back-to-back launches on a stream never share one.
    unsigned int* tile_counters = nullptr;
    unsigned int next_counter = 0;
    // Camera records in device memory (the kernel reads them with scalar loads),
    // same ring discipline; the host copies [slot][kCameraStride] stay alive until the async copy ran.
    unsigned char* d_cameras = nullptr;
    std::vector<unsigned char> h_cameras;
    // Partial-sum workspace [work item][3][64] reals, grown on demand and reused by
    // successive launches (they are ordered on the caller's stream).
    void* d_partial = nullptr;
    size_t partial_bytes = 0;
    // Longest-processing-time-first tile order, learned from the previous frame of the same shape: the render
    // kernel accumulates a per-tile cost, rtk_tile_order_kernel turns it into the hand-out order of the next launch.
    unsigned int* d_tile_cost = nullptr;
    int32_t* d_tile_order = nullptr;
    size_t order_bytes = 0;  // of each of the two
    bool order_valid = false;
    int order_shape[5] = {0, 0, 0, 0, 0};  // width, height, rank, n_ranks, tiles: what the stored order was measured on
    // The camera of the previous launch per arithmetic type: a frame loop renders the same camera again and again, and
    // re-sending 256 bytes through a pageable-memory copy costs a host/stream round trip per frame for nothing.
    unsigned int next_camera = 0;
    bool cam_valid[2] = {false, false};
    rtk_camera cam_last[2];
    unsigned int cam_slot[2] = {0, 0};
    // Progress reporting (rtk_set_progress_callback): the work-item counter of the last launch and how many items it
    // hands out; a blocking render polls the counter with a 4-byte device-to-host copy on a stream of its own.
    rtk_progress_fn progress_fn = nullptr;
    void* progress_user = nullptr;
    int progress_interval_ms = 100;
    // a frame is up to kMaxPasses launches (one per range of sample chunks): the work-item counter of each and what it hands out
    const unsigned int* last_tile_counter[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int64_t last_pass_items[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int last_n_passes = 0;
    int64_t last_n_items = 0;               // of the whole frame
    hipStream_t progress_stream = nullptr;
    unsigned int* progress_word = nullptr;  // pinned host memory, one word per pass
    bool progress_pending = false;
    // The denoiser's ping-pong colour / variance buffers (rtk_denoise), grown on demand.
    void* d_denoise = nullptr;
    size_t denoise_bytes = 0;
    // rtk_render_tiles: the compacted list of the flagged tiles and, in the last word of the allocation, its length.
    int32_t* d_tile_list = nullptr;
    size_t list_bytes = 0;
    // The surface gathers' per-unit partial sums (rtk_gather_*), grown on demand up to their byte budget.
    void* d_gather = nullptr;
    size_t gather_bytes = 0;
    // rtk_render_views: the batch's view records in device memory, grown on demand like the partial-sum workspace and reused
    // in stream order, and a ring of pinned host buffers they are uploaded from -- a buffer is rewritten only after the
    // event behind its last upload has passed, so batches enqueued back to back never share one.
    void* d_views = nullptr;
    size_t views_bytes = 0;
    struct ViewStage {
        void* host = nullptr;
        size_t bytes = 0;
        hipEvent_t done = nullptr;
    };
    ViewStage view_stage[4];
    unsigned int next_view_stage = 0;
};

#endif  // RTK_CTX_H
