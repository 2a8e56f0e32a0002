// rtk_view_batch.h -- many cameras' frames in one launch, from the drop-in C++ API.
//
// camera::render makes one image per call.  A reflection capture, a turntable, a strip of thumbnails or a light field is a set of
// small frames of ONE size, and rendered one by one each of them leaves most of the device idle.  This object flattens and
// uploads the scene once, as camera::render_to does, collects cameras, and renders them all through rtk_render_views
// (include/rtk.h "View batches"): view v is, bit for bit, the frame camera v would have rendered alone.
//
//     rtk::view_batch batch(world, lights);
//     for (const camera& cam : path) batch.add(cam);          // same image_width, aspect_ratio and samples_per_pixel
//     std::vector<double> linear;  std::vector<uint8_t> rgb8;  // [n][H][W][3]
//     if (batch.render(&linear, &rgb8)) ...
//
//     for (const rtk_camera& face : rtk::view_batch::cube_faces(point3(0, 1, 0), 256, 16, 10, color(0.7, 0.8, 1.0))) batch.add(face);
//
// cube_faces: six square cameras with a 90-degree field of view at `center`, derived like any camera (camera::derive), in the
// order +x, -x, +y, -y, +z, -z with the up vectors (0,-1,0), (0,-1,0), (0,0,1), (0,0,-1), (0,-1,0), (0,-1,0) -- the cube-map
// layout of graphics APIs.  Neighbouring faces meet exactly along their edges: the corner rays of every face are center +
// (+-1, +-1, +-1).
//
// Every call blocks.  The scene is uploaded in the fast visiting order when `fast_order` is set (eye = the first camera's
// position is not known at construction, so the optimisation runs without one), else in the reference's.  ok() / status() tell
// whether the upload or a render failed (rtk_last_error() has the text); status() keeps the first failure.
#ifndef RTK_VIEW_BATCH_H
#define RTK_VIEW_BATCH_H

#include <cstdint>
#include <vector>

#include "rtk.h"
#include "rtk_camera.h"  // camera::derive; hittable, point_light, scene_builder, flatten through rtk_scene_api.h

namespace rtk {

class view_batch {
public:
    uint32_t seed = 1;              // the render seed of every view without one of its own (rtk_render_opts.seed)
    int real_mode = RTK_REAL_F64;

    explicit view_batch(const hittable& world, const std::vector<point_light>& lights = {}, int device = 0, bool fast_order = false) {
        scene_builder sb;
        const rtk_scene_desc desc = flatten(world, lights, sb);
        status_ = rtk_init(device, &ctx_);
        if (status_ == RTK_OK) status_ = fast_order ? rtk_scene_upload_fast(ctx_, &desc, nullptr, nullptr) : rtk_scene_upload(ctx_, &desc);
    }
    view_batch(const view_batch&) = delete;
    view_batch& operator=(const view_batch&) = delete;
    ~view_batch() {
        if (ctx_) rtk_destroy(ctx_);
    }

    bool ok() const { return status_ == RTK_OK; }
    int status() const { return status_; }

    // One more view: a drop-in camera (its derive()), or the derived values themselves; with or without a seed of its own.
    void add(const camera& cam) { add(cam.derive()); }
    void add(const camera& cam, uint32_t view_seed) { add(cam.derive(), view_seed); }
    void add(const rtk_camera& cam) {
        cams_.push_back(cam);
        seeds_.push_back(seed);
        own_seed_.push_back(0);
    }
    void add(const rtk_camera& cam, uint32_t view_seed) {
        cams_.push_back(cam);
        seeds_.push_back(view_seed);
        own_seed_.push_back(1);
    }
    void clear() {
        cams_.clear();
        seeds_.clear();
        own_seed_.clear();
    }
    size_t size() const { return cams_.size(); }
    int width() const { return cams_.empty() ? 0 : cams_[0].image_width; }
    int height() const { return cams_.empty() ? 0 : cams_[0].image_height; }

    // Render every view: linear [n][H][W][3] doubles (the colour after the 1 / spp scale, before gamma), rgb8 [n][H][W][3]
    // bytes; either may be null.  false when there is no view or the call failed (status()).
    bool render(std::vector<double>* linear, std::vector<uint8_t>* rgb8, rtk_work_counters* counters = nullptr) {
        if (cams_.empty() || !ok()) return false;
        const size_t n = cams_.size() * size_t(width()) * size_t(height()) * 3;
        if (linear) linear->assign(n, 0.0);
        if (rgb8) rgb8->assign(n, 0);
        std::vector<uint32_t> seeds(seeds_);
        for (size_t v = 0; v < seeds.size(); v++)
            if (!own_seed_[v]) seeds[v] = seed;  // `seed` as it is now, not as it was at add()
        rtk_render_opts opts{};
        opts.seed = seed;
        opts.real_mode = real_mode;
        opts.n_ranks = 1;
        return call(rtk_render_views_host(ctx_, int32_t(cams_.size()), cams_.data(), seeds.data(), &opts, linear ? linear->data() : nullptr,
                                          rgb8 ? rgb8->data() : nullptr, counters));
    }

    // The kernel symbol render() dispatches (rtk_view_kernel_name).
    const char* kernel_name() const { return rtk_view_kernel_name(ctx_, real_mode, 0); }

    // Six 90-degree square cameras at `center`: +x, -x, +y, -y, +z, -z (see the top of this file for the up vectors).
    static std::vector<rtk_camera> cube_faces(const point3& center, int face_size, int samples_per_pixel, int max_depth, const color& background) {
        static const double axis[6][3] = {{1, 0, 0}, {-1, 0, 0}, {0, 1, 0}, {0, -1, 0}, {0, 0, 1}, {0, 0, -1}};
        static const double up[6][3] = {{0, -1, 0}, {0, -1, 0}, {0, 0, 1}, {0, 0, -1}, {0, -1, 0}, {0, -1, 0}};
        std::vector<rtk_camera> faces;
        for (int f = 0; f < 6; f++) {
            camera cam;
            cam.image_width = face_size;
            cam.aspect_ratio = 1.0;
            cam.samples_per_pixel = samples_per_pixel;
            cam.max_depth = max_depth;
            cam.background = background;
            cam.vfov = 90;
            cam.lookfrom = center;
            cam.lookat = center + vec3(axis[f][0], axis[f][1], axis[f][2]);
            cam.vup = vec3(up[f][0], up[f][1], up[f][2]);
            cam.defocus_angle = 0;
            cam.focus_dist = 1;
            faces.push_back(cam.derive());
        }
        return faces;
    }

private:
    rtk_ctx* ctx_ = nullptr;
    int status_ = RTK_OK;
    std::vector<rtk_camera> cams_;
    std::vector<uint32_t> seeds_;
    std::vector<uint8_t> own_seed_;

    bool call(int rc) {
        if (rc != RTK_OK && status_ == RTK_OK) status_ = rc;
        return rc == RTK_OK;
    }
};

}  // namespace rtk

#endif  // RTK_VIEW_BATCH_H
