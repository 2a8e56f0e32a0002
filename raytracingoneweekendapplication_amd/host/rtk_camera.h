// rtk_camera.h -- camera with the reference's public surface (Camera.txt:36-119)
// whose render() drives the MI355X kernel library instead of host threads.
//
//   reference                               here
//   ---------                               ----
//   initialize()      Camera.txt:136-175    camera::derive()   (host, double, same op order)
//   render_rows λ     Camera.txt:65-93      rtk_render_host()  (device: csrc/rtk_trace.hip)
//   stbi_write_png    Camera.txt:118        rtk::write_png()   (host, after the path)
//
// image_width / aspect_ratio are `const` in the reference (Camera.txt:39-40,
// SURVEY Q15), which pins it to 1024x576; here they are assignable (a strict
// superset -- reference scene code never writes them).
#ifndef RTK_CAMERA_H
#define RTK_CAMERA_H

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "rtk.h"
#include "rtk_scene_api.h"

namespace rtk {

// Minimal PNG encoder (8-bit RGB, stored deflate blocks).  Output stage only.
inline bool write_png(const char* path, int w, int h, const uint8_t* rgb) {
    auto crc_table = [] {
        std::vector<uint32_t> t(256);
        for (uint32_t n = 0; n < 256; n++) {
            uint32_t c = n;
            for (int k = 0; k < 8; k++) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            t[n] = c;
        }
        return t;
    }();
    auto crc = [&](const std::vector<uint8_t>& buf, size_t from) {
        uint32_t c = 0xFFFFFFFFu;
        for (size_t i = from; i < buf.size(); i++) c = crc_table[(c ^ buf[i]) & 0xFF] ^ (c >> 8);
        return c ^ 0xFFFFFFFFu;
    };
    auto be32 = [](std::vector<uint8_t>& b, uint32_t v) {
        b.push_back(uint8_t(v >> 24)); b.push_back(uint8_t(v >> 16)); b.push_back(uint8_t(v >> 8)); b.push_back(uint8_t(v));
    };
    std::vector<uint8_t> out = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    auto chunk = [&](const char* tag, const std::vector<uint8_t>& body) {
        be32(out, uint32_t(body.size()));
        size_t from = out.size();
        out.insert(out.end(), tag, tag + 4);
        out.insert(out.end(), body.begin(), body.end());
        be32(out, crc(out, from));
    };
    std::vector<uint8_t> ihdr;
    be32(ihdr, uint32_t(w)); be32(ihdr, uint32_t(h));
    ihdr.insert(ihdr.end(), {8, 2, 0, 0, 0});
    chunk("IHDR", ihdr);
    std::vector<uint8_t> raw;
    raw.reserve(size_t(h) * (size_t(w) * 3 + 1));
    for (int j = 0; j < h; j++) {
        raw.push_back(0);
        raw.insert(raw.end(), rgb + size_t(j) * w * 3, rgb + size_t(j + 1) * w * 3);
    }
    std::vector<uint8_t> z = {0x78, 0x01};
    uint32_t a = 1, b = 0;
    for (uint8_t byte : raw) { a = (a + byte) % 65521u; b = (b + a) % 65521u; }
    for (size_t pos = 0; pos < raw.size() || pos == 0;) {
        size_t n = std::min<size_t>(65535, raw.size() - pos);
        bool last = pos + n >= raw.size();
        z.push_back(last ? 1 : 0);
        z.push_back(uint8_t(n)); z.push_back(uint8_t(n >> 8));
        z.push_back(uint8_t(~n)); z.push_back(uint8_t((~n) >> 8));
        z.insert(z.end(), raw.begin() + pos, raw.begin() + pos + n);
        pos += n;
        if (last) break;
    }
    be32(z, (b << 16) | a);
    chunk("IDAT", z);
    chunk("IEND", {});
    FILE* f = std::fopen(path, "wb");
    if (!f) return false;
    bool ok = std::fwrite(out.data(), 1, out.size(), f) == out.size();
    std::fclose(f);
    return ok;
}

}  // namespace rtk

class camera {
public:
    int image_width = 1024;
    double aspect_ratio = 16.0 / 9.0;
    const char* image_name = "Default Image";
    int samples_per_pixel = 10;
    int max_depth = 10;
    color background = vec3(0, 0, 0);

    double vfov = 90;
    point3 lookfrom = point3(0, 0, 0);
    point3 lookat = point3(0, 0, -1);
    vec3 vup = vec3(0, 1, 0);

    double defocus_angle = 0;
    double focus_dist = 10;

    // --- additions (defaults reproduce the reference behaviour) -------------
    uint32_t seed = 1;                 // render seed: per-sample RNG streams are f(seed, pixel, sample)
    int real_mode = RTK_REAL_F64;      // the reference computes in double
    int device = 0;                    // HIP device ordinal
    // More than one entry: render() splits the image over these HIP devices (interleaved 8x8 tiles, replicated scene,
    // one gather to devices[0] -- rtk_render_multi); render() owns the whole parallel split, as the reference's does
    // (Camera.txt:59-61,96-100).  The image does not depend on the list.  Empty or one entry: `device` / that entry.
    std::vector<int> devices;
    bool write_image = true;           // write image_name as PNG after rendering
    // Progress: the reference prints "Percent Rendered: N%" every 100 ms while its row workers run (Camera.txt:102-106).
    // show_progress does the same from the render kernel's work-item counter; `progress` (if set) is called instead.
    bool show_progress = true;
    rtk_progress_fn progress = nullptr;
    void* progress_user = nullptr;
    // Visiting order of the hierarchy.  auto_order (default): the fast order of rtk_scene_upload_fast (same primitives, SAH
    // grouping, ~half the aabb::hit calls) whenever it is PROVEN bit-identical to the reference's bvh_node order
    // (rtk_optimize_info.exact == 2: every scene without triangles, unless free_media_order is set) and the reference order
    // otherwise, so the image never depends on this choice.  Triangle scenes are identical in every measurement but not
    // provably so (exact == 1: triangle.h:72,77 scales t by a float reciprocal): auto_order takes the fast order for them
    // only when accept_empirical_order is set; order = fast_order always takes it.
    enum visiting_order { reference_order = 0, fast_order = 1, auto_order = 2 };
    int order = auto_order;
    bool accept_empirical_order = false;
    // A constant_medium draws a random number inside hit() (constant_medium.h:40); by default media keep their place in the
    // reference's order (rtk_optimize_opts.free_media_order = 0).  true: media are re-grouped as well -- a little faster,
    // same estimator, but another image than the reference order's (auto_order then stays on the reference order).
    bool free_media_order = false;
    bool used_fast_order = false;      // set by render(): which order the last render used ...
    bool fast_order_exact = false;     // ... whether the fast order is bit-identical for this scene (proven or measured) ...
    int fast_order_exactness = 0;      // ... and which: rtk_optimize_info.exact (2 proven, 1 empirical, 0 statistical)
    double last_render_ms = 0;         // device render time of the last render()
    // Progressive rendering (rtk_progressive_*; one device: devices[0] or `device` -- not split over rtk_multi's devices).
    // progressive_step > 0: render() adds that many samples per step (rounded up to the session's chunk size, 8 up to 512 spp)
    // and writes image_name after every step when write_previews is set; the finished image is bit-identical to the one-shot
    // render's.  0 (default): the one-shot path.  With progressive_step > 0 only:
    //   checkpoint_file  the session is saved there after every step, and render() resumes from it when it matches this
    //                    scene, camera, seed and real mode (otherwise it warns and starts over);
    //   noise_target     > 0: stop at the first step boundary where the frame's mean relative standard error
    //                    (rtk_noise_stats.mean_rel_se) is <= noise_target; samples_per_pixel is then the maximum.
    //   adaptive_target  > 0: tile-adaptive sampling (rtk_progressive_set_adaptive, rel_target): an 8x8 tile stops rendering once,
    //                    after adaptive_min_samples (0 = two chunks), the largest relative standard error of its pixels is <=
    //                    adaptive_target; render() stops at samples_per_pixel or when no tile is active.  A resumed
    //                    checkpoint keeps the options it was made with.
    int progressive_step = 0;
    bool write_previews = false;
    const char* checkpoint_file = nullptr;
    double noise_target = 0;
    double adaptive_target = 0;
    int adaptive_min_samples = 0;
    int last_samples_rendered = 0;     // set by a progressive render(): samples per pixel this call added ...
    int last_samples_done = 0;         // ... the samples per pixel in the image it wrote ...
    rtk_noise_stats last_noise{};      // ... and the noise estimate after its last step (valid = 0 before two full chunks)
    rtk_adaptive_state last_adaptive{};  // ... and the tiles' state after it (without adaptive_target every tile is active)
    // Denoising (rtk_progressive_denoise): denoise_image_name set -> render() also writes the denoised image there as PNG,
    // guided by aov_samples first-hit samples per pixel.  Without progressive_step the frame is rendered as ONE progressive step
    // of the whole target, which is bit-identical to the one-shot frame (image_name is unchanged); the noise estimate needs
    // two full chunks, so a target below that fails with a message.
    // denoise_follow: RTK_GUIDE_FOLLOW_* bits -> the guides follow mirrors (and glass) to the surface they show
    // (rtk_progressive_denoise_guided); 0 = the first-hit path above.  denoise_demodulate filters colour / albedo (it takes the
    // guided path; with denoise_follow 0 it follows mirrors).
    const char* denoise_image_name = nullptr;
    int aov_samples = 4;
    int denoise_follow = 0;
    bool denoise_demodulate = false;
    // Temporal accumulation (rtk_temporal_*; one device, as progressive rendering).  temporal_history > 0: successive render()
    // calls on this camera object (and its copies) keep one rtk_temporal -- created on the first call; recreated, with a warning,
    // when the image size, real mode or device changes -- and each call
    //   1. renders its frame as one progressive step with seed `seed + frames accumulated so far` (samples_per_pixel must give
    //      two full chunks for the noise estimate, else render() warns and renders without history),
    //   2. renders the guides of this camera (aov_samples, denoise_follow; the same seed),
    //   3. accumulates with max_history = temporal_history and writes the ACCUMULATED frame to image_name,
    //   4. with denoise_image_name set, writes the guided filter of the accumulated colour and se there (denoise_demodulate).
    // Move lookfrom / lookat between calls; geometry is taken as static.  0 (default): nothing changes, bit for bit.
    int temporal_history = 0;
    int last_temporal_frames = 0;      // set by render(): frames in the history the image was written from (0: no history used)
    void temporal_reset() { if (temporal_) temporal_->reset(); }  // the next render() starts a new history
    // Guided upsampling (rtk_upsample; one device, as progressive rendering).  render_scale = 2..4: render()
    //   1. derives the low camera (rtk_upsample_camera: 1 / render_scale of the width and height, rounded up) and renders it as one
    //      progressive step of the whole target -- samples_per_pixel samples per LOW pixel, render_scale^2 times fewer rays;
    //      samples_per_pixel must give two full chunks for the noise estimate, else render() warns and renders at full resolution,
    //   2. renders the guides of both cameras (aov_samples, denoise_follow; the same seed),
    //   3. rebuilds the full-resolution frame with rtk_upsample (upsample_demodulate: on colour / seen albedo, which brings textures
    //      back at full resolution) and writes it to image_name.
    // With temporal_history > 0 the upsampled colour and se are what is accumulated; with denoise_image_name set the guided filter
    // runs on the result at full resolution.  1 (default): nothing changes, bit for bit.
    int render_scale = 1;
    bool upsample_demodulate = false;
    bool last_render_upsampled = false;  // set by render(): the image was rebuilt from a low-resolution frame
    // Refinement of the upsampled frame (rtk_tiles_select + rtk_render_tiles).  refine_support > 0: after step 3 the 8x8 tiles with
    // a pixel whose support is not >= refine_support -- the interpolation had nothing to go on there: silhouettes, the borders of
    // lights -- grown by refine_dilate pixels (0..8), are rendered at full resolution with samples_per_pixel samples and replace
    // the upsampled colour, se and bytes.  With more than refine_max_share of the tiles chosen (0 = no limit) nothing is
    // re-rendered and render() says so in one line: the full-resolution frame is the cheaper way there.  0 (default): nothing
    // changes, bit for bit.
    double refine_support = 0;
    int refine_dilate = 1;
    double refine_max_share = 0.5;
    int last_refined_tiles = 0;          // set by render(): tiles re-rendered at full resolution
    // Display transform (rtk_display_*; one device, as progressive rendering).  display = true: every PNG render() writes -- the
    // plain, progressive, denoised, temporal and upsampled paths alike -- is made from the linear frame by one rtk_display object
    // instead of the reference's sqrt / clamp / quantise.  The object is kept across render() calls on this camera object (and its
    // copies), like the temporal history, so the exposure adapts along a camera path.  One render() is one adaptation step: the
    // first image it makes is metered (or takes display_exposure), the further images of the same call -- later previews, the
    // final image, denoise_image_name -- take that image's exposure (as a float).  false (default): nothing changes, bit for bit.
    bool display = false;
    int display_curve = RTK_DISPLAY_CLAMP;   // RTK_DISPLAY_CLAMP / REINHARD / ACES
    float display_exposure = 0;              // 0 = metered; > 0 sets the exposure
    float display_adapt = 0;                 // 0 = 1: no lag; else (0, 1], the share of the way to the target (in log) per render()
    float display_bloom = 0;                 // 0 = off; strength
    bool display_srgb = false;               // sRGB bytes instead of the reference's gamma 2
    double last_exposure = 0;                // set by render(): the exposure its images were made with (0: display off)
    void display_reset() { if (display_) rtk_display_reset(display_->display); }  // the next render() adapts from nothing
    // Lens models (rtk_lens_*; one device, as progressive rendering).  projection = equirect / fisheye / orthographic: render()
    // makes the frame with rtk_lens_render -- lookfrom / lookat / vup give the frame (rtk_lens_look_at), image_width and
    // aspect_ratio the size, samples_per_pixel, max_depth and background their usual meaning; vfov, defocus_angle and focus_dist
    // are not read -- and writes it to image_name through the reference's sqrt / clamp / quantise, or through `display`.  With
    // denoise_image_name set it also writes the guided filter (rtk_lens_guides with aov_samples and denoise_follow, then
    // rtk_denoise_guided on the frame and its se; samples_per_pixel >= 2 for the se).  temporal_history > 0 or render_scale > 1
    // with such a projection make render() fail with a message: reprojection and the low-resolution camera assume a pinhole.
    // perspective (default): nothing changes, bit for bit.
    enum projection_kind { perspective = RTK_LENS_PERSPECTIVE, equirect = RTK_LENS_EQUIRECT, fisheye = RTK_LENS_FISHEYE, orthographic = RTK_LENS_ORTHOGRAPHIC };
    int projection = perspective;
    double fov_h = 0, fov_v = 0;             // radians; equirect: the extents (0 = 2 pi, pi); fisheye: fov_h across the width (0 = pi)
    double ortho_width = 0, ortho_height = 0;  // orthographic: the window in world units

    // The rtk_lens of a non-perspective projection.
    rtk_lens derive_lens() const {
        rtk_lens l{};
        int image_height = int(image_width / aspect_ratio);
        l.cam.image_width = image_width;
        l.cam.image_height = (image_height < 1) ? 1 : image_height;
        l.cam.samples_per_pixel = samples_per_pixel;
        l.cam.max_depth = max_depth;
        l.cam.background = rtk::to_abi(background);
        l.cam.pixel_samples_scale = 1.0 / samples_per_pixel;
        l.model = projection;
        l.fov_h = fov_h;
        l.fov_v = fov_v;
        l.ortho_width = ortho_width;
        l.ortho_height = ortho_height;
        rtk_lens_look_at(&l, rtk::to_abi(lookfrom), rtk::to_abi(lookat), rtk::to_abi(vup));
        return l;
    }

    // Camera.txt:136-175.
    rtk_camera derive() const {
        rtk_camera c;
        int image_height = int(image_width / aspect_ratio);
        image_height = (image_height < 1) ? 1 : image_height;
        c.image_width = image_width;
        c.image_height = image_height;
        c.samples_per_pixel = samples_per_pixel;
        c.max_depth = max_depth;
        c.background = rtk::to_abi(background);
        c.pixel_samples_scale = 1.0 / samples_per_pixel;
        point3 center = lookfrom;

        double theta = degrees_to_radians(vfov);
        double h = std::tan(theta / 2);
        double viewport_height = 2 * h * focus_dist;
        double viewport_width = viewport_height * (double(image_width) / image_height);

        vec3 w = unit_vector(lookfrom - lookat);
        vec3 u = unit_vector(cross(vup, w));
        vec3 v = cross(w, u);

        vec3 viewport_u = viewport_width * u;
        vec3 viewport_v = viewport_height * -v;
        vec3 pixel_delta_u = viewport_u / image_width;
        vec3 pixel_delta_v = viewport_v / image_height;

        vec3 viewport_upper_left = center - (focus_dist * w) - viewport_u / 2 - viewport_v / 2;
        vec3 pixel00_loc = viewport_upper_left + 0.5 * (pixel_delta_u + pixel_delta_v);

        double defocus_radius = focus_dist * std::tan(degrees_to_radians(defocus_angle / 2));
        c.center = rtk::to_abi(center);
        c.pixel00_loc = rtk::to_abi(pixel00_loc);
        c.pixel_delta_u = rtk::to_abi(pixel_delta_u);
        c.pixel_delta_v = rtk::to_abi(pixel_delta_v);
        c.defocus_disk_u = rtk::to_abi(u * defocus_radius);
        c.defocus_disk_v = rtk::to_abi(v * defocus_radius);
        c.defocus_angle = defocus_angle;
        return c;
    }

    // Render into caller-provided buffers (either may be null).  Returns an
    // rtk_status; never falls back to the host.
    int render_to(const hittable& world, const std::vector<point_light>& lights, std::vector<double>* linear,
                  std::vector<uint8_t>* rgb8, rtk_work_counters* counters = nullptr) {
        rtk::scene_builder sb;
        rtk_scene_desc desc = rtk::flatten(world, lights, sb);
        rtk_camera cam = derive();
        std::vector<int> devs = devices.empty() ? std::vector<int>{device} : devices;
        if (counters && devs.size() > 1) devs.resize(1);  // work counters are per device: a counting render uses the first one
        rtk_multi* multi = nullptr;
        int rc = rtk_init_multi(int(devs.size()), devs.data(), RTK_GATHER_AUTO, &multi);
        if (rc != RTK_OK) return rc;
        rc = upload(multi, desc, cam);
        if (rc == RTK_OK) {
            size_t n = size_t(cam.image_width) * cam.image_height * 3;
            if (linear) linear->assign(n, 0.0);
            if (rgb8) rgb8->assign(n, 0);
            rtk_render_opts opts{};
            opts.seed = seed;
            opts.real_mode = real_mode;
            opts.rank = 0;
            opts.n_ranks = 1;
            opts.count_work = counters ? 1 : 0;
            if (progress) rtk_set_progress_callback(rtk_multi_ctx(multi, 0), progress, progress_user, 100);
            else if (show_progress) rtk_set_progress_callback(rtk_multi_ctx(multi, 0), &camera::print_progress, nullptr, 100);
            auto t0 = std::chrono::steady_clock::now();
            if (counters) rc = rtk_render_host(rtk_multi_ctx(multi, 0), &cam, &opts, linear ? linear->data() : nullptr, rgb8 ? rgb8->data() : nullptr, counters);
            else rc = rtk_render_multi(multi, &cam, &opts, linear ? linear->data() : nullptr, rgb8 ? rgb8->data() : nullptr);
            last_render_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
        rtk_multi_destroy(multi);
        return rc;
    }

    // The scene upload of render_to and render_progressive: the visiting order `order` asks for.
    int upload(rtk_multi* multi, const rtk_scene_desc& desc, const rtk_camera& cam) {
        int rc = RTK_OK;
        used_fast_order = false;
        fast_order_exact = false;
        fast_order_exactness = 0;
        if (order != reference_order) {  // same primitives, SAH grouping, children ordered by distance to this camera
            rtk_optimize_opts oo{};
            oo.has_eye = 1;
            oo.eye = cam.center;
            oo.free_media_order = free_media_order ? 1 : 0;
            rtk_optimize_info info{};
            rc = rtk_multi_scene_upload_fast(multi, &desc, &oo, &info);
            fast_order_exact = rc == RTK_OK && info.exact != 0;
            fast_order_exactness = rc == RTK_OK ? info.exact : 0;
            used_fast_order = rc == RTK_OK && (order == fast_order || info.exact == 2 || (info.exact == 1 && accept_empirical_order));
            // auto_order never makes render() fail on a scene the reference order accepts: fall back to it
            if (rc != RTK_OK && order == auto_order) rc = RTK_OK;
        }
        if (rc == RTK_OK && !used_fast_order) rc = rtk_multi_scene_upload(multi, &desc);  // the reference's own hierarchy and order
        return rc;
    }

    // render() with progressive_step > 0: one rtk_progressive session on one device, stepped to the target (or to noise_target),
    // checkpointed to checkpoint_file after every step.  rgb8 receives the last step's preview.
    int render_progressive(const hittable& world, const std::vector<point_light>& lights, std::vector<uint8_t>* rgb8) {
        rtk::scene_builder sb;
        rtk_scene_desc desc = rtk::flatten(world, lights, sb);
        rtk_camera cam = derive();
        int dev = devices.empty() ? device : devices[0];
        rtk_multi* multi = nullptr;
        int rc = rtk_init_multi(1, &dev, RTK_GATHER_PEER, &multi);
        if (rc != RTK_OK) return rc;
        rtk_progressive* p = nullptr;
        last_samples_rendered = 0;
        last_samples_done = 0;
        last_noise = rtk_noise_stats{};
        last_adaptive = rtk_adaptive_state{};
        rc = upload(multi, desc, cam);
        rtk_render_opts opts{};
        opts.seed = seed;
        opts.real_mode = real_mode;
        opts.rank = 0;
        opts.n_ranks = 1;
        rtk_ctx* ctx = rtk_multi_ctx(multi, 0);
        const bool stepped = progressive_step > 0;  // (otherwise one step of the whole target, for denoise_image_name)
        if (rc == RTK_OK && stepped && checkpoint_file) {
            std::vector<unsigned char> blob;
            if (FILE* f = std::fopen(checkpoint_file, "rb")) {
                unsigned char buf[65536];
                size_t got;
                while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) blob.insert(blob.end(), buf, buf + got);
                std::fclose(f);
                if (rtk_progressive_resume(ctx, &cam, &opts, blob.data(), int64_t(blob.size()), &p) != RTK_OK) {
                    std::cerr << "camera::render: " << checkpoint_file << " does not match this render (" << rtk_last_error() << "); starting over" << std::endl;
                    p = nullptr;
                } else if (rtk_progressive_samples_done(p) >= cam.samples_per_pixel) {  // finished: no step is left to write the image
                    rtk_progressive_destroy(p);
                    p = nullptr;
                }
            }
        }
        if (rc == RTK_OK && !p) {
            rc = rtk_progressive_create(ctx, &cam, &opts, &p);
            if (rc == RTK_OK && stepped && adaptive_target > 0) {
                rtk_adaptive_opts ad{};
                ad.rel_target = adaptive_target;
                ad.min_samples = adaptive_min_samples > 0 ? adaptive_min_samples : 2 * rtk_progressive_chunk_size(p);
                rc = rtk_progressive_set_adaptive(p, &ad);
            }
        }
        if (rc == RTK_OK) {
            const int chunk = rtk_progressive_chunk_size(p);
            const int step = stepped ? (progressive_step + chunk - 1) / chunk * chunk : cam.samples_per_pixel;
            const int start = rtk_progressive_samples_done(p);
            rgb8->assign(size_t(cam.image_width) * cam.image_height * 3, 0);
            std::vector<double> shown(display ? rgb8->size() : 0);  // the linear frame behind the bytes, for the display transform
            bool pending = false;                                   // ... which the last step's bytes have yet to go through
            const char* checkpoint = stepped ? checkpoint_file : nullptr;
            std::vector<unsigned char> blob(checkpoint ? size_t(rtk_progressive_checkpoint_bytes(p)) : 0);
            auto t0 = std::chrono::steady_clock::now();
            for (int done = start; rc == RTK_OK && done < cam.samples_per_pixel;) {
                rc = rtk_progressive_step_host(p, std::min(step, cam.samples_per_pixel - done), display ? shown.data() : nullptr, rgb8->data(), nullptr, nullptr);
                pending = display;
                if (rc == RTK_OK && stepped && write_previews && write_image) {  // a preview is about to be written
                    rc = display_bytes(cam, shown.data(), rgb8->data());
                    pending = false;
                }
                if (rc != RTK_OK) break;
                done = rtk_progressive_samples_done(p);
                last_samples_done = done;
                last_samples_rendered = done - start;
                if (checkpoint && (rc = rtk_progressive_save(p, blob.data(), int64_t(blob.size()))) == RTK_OK) {
                    const std::string tmp = std::string(checkpoint_file) + ".tmp";  // replace the old checkpoint only once the new one is whole
                    FILE* f = std::fopen(tmp.c_str(), "wb");
                    const bool ok = f && std::fwrite(blob.data(), 1, blob.size(), f) == blob.size();
                    if (f) std::fclose(f);
                    if (!ok || std::rename(tmp.c_str(), checkpoint_file) != 0) std::cerr << "camera::render: cannot write " << checkpoint_file << std::endl;
                }
                if (rc == RTK_OK && stepped && write_previews && write_image) rtk::write_png(image_name, cam.image_width, cam.image_height, rgb8->data());
                if (rc == RTK_OK && (noise_target > 0 || done >= cam.samples_per_pixel)) rc = rtk_progressive_noise(p, &last_noise);
                if (rc == RTK_OK) rc = rtk_adaptive_status(p, &last_adaptive);
                if (rc == RTK_OK && stepped && noise_target > 0 && last_noise.valid && last_noise.mean_rel_se <= noise_target) break;
                if (rc == RTK_OK && stepped && adaptive_target > 0 && last_adaptive.active_tiles == 0) break;  // every tile retired
                if (show_progress) print_progress(done, cam.samples_per_pixel, nullptr);
            }
            last_render_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (rc == RTK_OK && pending) rc = display_bytes(cam, shown.data(), rgb8->data());
            if (rc == RTK_OK && denoise_image_name) {
                std::vector<uint8_t> den(rgb8->size());
                double* den_linear = display ? shown.data() : nullptr;
                if (denoise_follow != 0 || denoise_demodulate) {
                    const rtk_guide_opts go{denoise_follow, 0};
                    rc = rtk_progressive_denoise_guided_host(p, aov_samples, &go, nullptr, denoise_demodulate ? RTK_DENOISE_DEMODULATE : 0, den_linear, den.data());
                } else {
                    rc = rtk_progressive_denoise_host(p, aov_samples, nullptr, den_linear, den.data());
                }
                if (rc == RTK_OK) rc = display_bytes(cam, shown.data(), den.data());
                if (rc == RTK_OK && write_image) rtk::write_png(denoise_image_name, cam.image_width, cam.image_height, den.data());
            }
        }
        if (p) rtk_progressive_destroy(p);
        rtk_multi_destroy(multi);
        return rc;
    }

    // The rtk_temporal that temporal_history keeps between render() calls, for this image size, real mode and device: created on
    // first use, recreated (with a warning) when one of them changed.
    int temporal_context(const rtk_camera& cam, int dev) {
        if (temporal_ && (temporal_->width != cam.image_width || temporal_->height != cam.image_height || temporal_->real_mode != real_mode || temporal_->device != dev)) {
            std::cerr << "camera::render: image size, real mode or device changed; the temporal history starts over" << std::endl;
            temporal_.reset();
        }
        if (!temporal_) {
            auto st = std::make_shared<temporal_state>();
            int rc = rtk_init_multi(1, &dev, RTK_GATHER_PEER, &st->multi);
            if (rc == RTK_OK) rc = rtk_temporal_create(rtk_multi_ctx(st->multi, 0), cam.image_width, cam.image_height, real_mode, nullptr, &st->temporal);
            if (rc != RTK_OK) return rc;
            st->width = cam.image_width;
            st->height = cam.image_height;
            st->real_mode = real_mode;
            st->device = dev;
            temporal_ = st;
        }
        return RTK_OK;
    }

    // render() with temporal_history > 0 (see the member).  RTK_OK with *used = false: too few samples for a noise estimate, the
    // caller renders without history.
    int render_temporal(const hittable& world, const std::vector<point_light>& lights, std::vector<uint8_t>* rgb8, bool* used) {
        *used = false;
        last_temporal_frames = 0;
        rtk::scene_builder sb;
        rtk_scene_desc desc = rtk::flatten(world, lights, sb);
        rtk_camera cam = derive();
        const int dev = devices.empty() ? device : devices[0];
        int rc = temporal_context(cam, dev);
        if (rc != RTK_OK) return rc;
        rtk_ctx* ctx = rtk_multi_ctx(temporal_->multi, 0);
        rc = upload(temporal_->multi, desc, cam);
        if (rc != RTK_OK) return rc;
        rtk_render_opts opts{};
        opts.seed = seed + uint32_t(rtk_temporal_frames(temporal_->temporal));
        opts.real_mode = real_mode;
        opts.rank = 0;
        opts.n_ranks = 1;
        rtk_progressive* p = nullptr;
        rc = rtk_progressive_create(ctx, &cam, &opts, &p);
        if (rc != RTK_OK) return rc;
        if (cam.samples_per_pixel < 2 * rtk_progressive_chunk_size(p)) {
            std::cerr << "camera::render: temporal_history needs samples_per_pixel >= " << 2 * rtk_progressive_chunk_size(p)
                      << " (two full chunks for the noise estimate); rendering without history" << std::endl;
            rtk_progressive_destroy(p);
            return RTK_OK;
        }
        const size_t px = size_t(cam.image_width) * cam.image_height;
        std::vector<double> linear(px * 3);
        std::vector<float> noise(px), guides(px * 16);
        rgb8->assign(px * 3, 0);
        auto t0 = std::chrono::steady_clock::now();
        rc = rtk_progressive_step_host(p, cam.samples_per_pixel, linear.data(), nullptr, noise.data(), nullptr);
        rtk_progressive_destroy(p);
        const rtk_guide_opts go{denoise_follow, 0};
        if (rc == RTK_OK) rc = rtk_render_guides_host(ctx, &cam, &opts, aov_samples, &go, guides.data());
        rtk_temporal_opts to{};
        to.max_history = temporal_history;
        if (rc == RTK_OK) rc = rtk_temporal_accumulate_host(temporal_->temporal, &cam, linear.data(), guides.data(), noise.data(), &to, linear.data(), noise.data(),
                                                            rgb8->data(), nullptr);
        last_render_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (rc == RTK_OK) rc = display_bytes(cam, linear.data(), rgb8->data());
        if (rc != RTK_OK) return rc;
        *used = true;
        last_temporal_frames = rtk_temporal_frames(temporal_->temporal);
        if (denoise_image_name) {
            std::vector<uint8_t> den(px * 3);
            std::vector<double> den_linear(display ? px * 3 : 0);
            rc = rtk_denoise_guided_host(ctx, cam.image_width, cam.image_height, real_mode, linear.data(), guides.data(), noise.data(), nullptr,
                                         denoise_demodulate ? RTK_DENOISE_DEMODULATE : 0, display ? den_linear.data() : nullptr, den.data());
            if (rc == RTK_OK) rc = display_bytes(cam, den_linear.data(), den.data());
            if (rc == RTK_OK && write_image) rtk::write_png(denoise_image_name, cam.image_width, cam.image_height, den.data());
        }
        return rc;
    }

    // render() with render_scale > 1 (see the member).  RTK_OK with *used = false: render_scale out of range or too few samples
    // for a noise estimate, the caller renders plainly.
    int render_scaled(const hittable& world, const std::vector<point_light>& lights, std::vector<uint8_t>* rgb8, bool* used) {
        *used = false;
        last_temporal_frames = 0;
        rtk_camera cam = derive(), low;
        if (rtk_upsample_camera(&cam, render_scale, &low) != RTK_OK) {
            std::cerr << "camera::render: render_scale must be 1..4 (" << render_scale << "); rendering at full resolution" << std::endl;
            return RTK_OK;
        }
        rtk::scene_builder sb;
        rtk_scene_desc desc = rtk::flatten(world, lights, sb);
        const int dev = devices.empty() ? device : devices[0];
        const bool temporal = temporal_history > 0;
        rtk_multi* own = nullptr;  // without a history the context lives for this call
        int rc = temporal ? temporal_context(cam, dev) : rtk_init_multi(1, &dev, RTK_GATHER_PEER, &own);
        if (rc != RTK_OK) return rc;
        rtk_multi* multi = temporal ? temporal_->multi : own;
        rtk_ctx* ctx = rtk_multi_ctx(multi, 0);
        rtk_render_opts opts{};
        opts.seed = seed + (temporal ? uint32_t(rtk_temporal_frames(temporal_->temporal)) : 0u);
        opts.real_mode = real_mode;
        opts.rank = 0;
        opts.n_ranks = 1;
        rtk_progressive* p = nullptr;
        rc = upload(multi, desc, cam);
        if (rc == RTK_OK) rc = rtk_progressive_create(ctx, &low, &opts, &p);
        if (rc == RTK_OK && low.samples_per_pixel < 2 * rtk_progressive_chunk_size(p)) {
            std::cerr << "camera::render: render_scale needs samples_per_pixel >= " << 2 * rtk_progressive_chunk_size(p)
                      << " (two full chunks for the noise estimate); rendering at full resolution" << std::endl;
            rtk_progressive_destroy(p);
            if (own) rtk_multi_destroy(own);
            return RTK_OK;
        }
        const size_t px = size_t(cam.image_width) * cam.image_height, lpx = size_t(low.image_width) * low.image_height;
        std::vector<double> linear(px * 3), low_linear(lpx * 3);
        std::vector<float> noise(px), guides(px * 16), low_noise(lpx), low_guides(lpx * 16);
        const bool refine = refine_support > 0;
        std::vector<float> support(refine ? px : 0);
        last_refined_tiles = 0;
        rgb8->assign(px * 3, 0);
        auto t0 = std::chrono::steady_clock::now();
        if (rc == RTK_OK) rc = rtk_progressive_step_host(p, low.samples_per_pixel, low_linear.data(), nullptr, low_noise.data(), nullptr);
        if (p) rtk_progressive_destroy(p);
        const rtk_guide_opts go{denoise_follow, 0};
        if (rc == RTK_OK) rc = rtk_render_guides_host(ctx, &low, &opts, aov_samples, &go, low_guides.data());
        if (rc == RTK_OK) rc = rtk_render_guides_host(ctx, &cam, &opts, aov_samples, &go, guides.data());
        rtk_upsample_opts uo{};
        uo.factor = render_scale;
        uo.flags = upsample_demodulate ? RTK_UPSAMPLE_DEMODULATE : 0;
        if (rc == RTK_OK) rc = rtk_upsample_host(ctx, &cam, real_mode, low_linear.data(), low_noise.data(), low_guides.data(), guides.data(), &uo, linear.data(),
                                                 noise.data(), rgb8->data(), refine ? support.data() : nullptr);
        if (rc == RTK_OK && refine) rc = refine_tiles(ctx, cam, opts, support, linear, noise, rgb8);
        if (rc == RTK_OK && temporal) {  // the upsampled colour and se are what is accumulated
            rtk_temporal_opts to{};
            to.max_history = temporal_history;
            rc = rtk_temporal_accumulate_host(temporal_->temporal, &cam, linear.data(), guides.data(), noise.data(), &to, linear.data(), noise.data(), rgb8->data(),
                                              nullptr);
            if (rc == RTK_OK) last_temporal_frames = rtk_temporal_frames(temporal_->temporal);
        }
        last_render_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (rc == RTK_OK) rc = display_bytes(cam, linear.data(), rgb8->data());
        if (rc == RTK_OK && denoise_image_name) {
            std::vector<uint8_t> den(px * 3);
            std::vector<double> den_linear(display ? px * 3 : 0);
            rc = rtk_denoise_guided_host(ctx, cam.image_width, cam.image_height, real_mode, linear.data(), guides.data(), noise.data(), nullptr,
                                         denoise_demodulate ? RTK_DENOISE_DEMODULATE : 0, display ? den_linear.data() : nullptr, den.data());
            if (rc == RTK_OK) rc = display_bytes(cam, den_linear.data(), den.data());
            if (rc == RTK_OK && write_image) rtk::write_png(denoise_image_name, cam.image_width, cam.image_height, den.data());
        }
        if (own) rtk_multi_destroy(own);
        *used = rc == RTK_OK;
        return rc;
    }

    // render_scaled's refinement (see refine_support): the low-support tiles of the upsampled frame rendered at full resolution.
    int refine_tiles(rtk_ctx* ctx, const rtk_camera& cam, const rtk_render_opts& opts, const std::vector<float>& support, std::vector<double>& linear,
                     std::vector<float>& noise, std::vector<uint8_t>* rgb8) {
        const int64_t n_tiles = rtk_tiles_per_rank(cam.image_width, cam.image_height, 1);
        std::vector<int32_t> flags(size_t(n_tiles), 0);
        rtk_tile_select_opts so{};
        so.below = float(refine_support);
        so.dilate = refine_dilate;
        int rc = rtk_tiles_select_host(ctx, cam.image_width, cam.image_height, support.data(), nullptr, &so, flags.data());
        if (rc != RTK_OK) return rc;
        const int32_t max_tiles = refine_max_share > 0 ? std::max<int32_t>(1, int32_t(refine_max_share * double(n_tiles))) : 0;
        int32_t info[2] = {0, 0};
        rc = rtk_render_tiles_host(ctx, &cam, &opts, flags.data(), max_tiles, linear.data(), rgb8->data(), noise.data(), nullptr, info);
        if (rc != RTK_OK) return rc;
        last_refined_tiles = info[1];
        if (info[1] < info[0])
            std::cerr << "camera::render: refine_support chose " << info[0] << " of " << n_tiles << " tiles, more than refine_max_share allows; none re-rendered"
                      << std::endl;
        return RTK_OK;
    }

    // render()'s one-shot path: render_to, and with `display` the bytes from the linear frame through the display object.
    int render_plain(const hittable& world, const std::vector<point_light>& lights, std::vector<uint8_t>* rgb8) {
        if (!display) return render_to(world, lights, nullptr, rgb8);
        std::vector<double> linear;
        int rc = render_to(world, lights, &linear, rgb8);
        if (rc == RTK_OK) rc = display_bytes(derive(), linear.data(), rgb8->data());
        return rc;
    }

    // render() with another projection than perspective (see the member): one device, the frame and its se from rtk_lens_render,
    // the bytes by the reference's conversion (Camera.txt:29-34,77-83) or the display object.
    int render_lens(const hittable& world, const std::vector<point_light>& lights, std::vector<uint8_t>* rgb8) {
        rtk::scene_builder sb;
        rtk_scene_desc desc = rtk::flatten(world, lights, sb);
        const rtk_lens lens = derive_lens();
        const rtk_camera& cam = lens.cam;
        int dev = devices.empty() ? device : devices[0];
        rtk_multi* multi = nullptr;
        int rc = rtk_init_multi(1, &dev, RTK_GATHER_PEER, &multi);
        if (rc != RTK_OK) return rc;
        rc = upload(multi, desc, cam);
        rtk_render_opts opts{};
        opts.seed = seed;
        opts.real_mode = real_mode;
        opts.rank = 0;
        opts.n_ranks = 1;
        rtk_ctx* ctx = rtk_multi_ctx(multi, 0);
        const size_t px = size_t(cam.image_width) * cam.image_height;
        std::vector<double> linear(px * 3);
        std::vector<float> noise(denoise_image_name ? px : 0);
        if (rc == RTK_OK) {
            auto t0 = std::chrono::steady_clock::now();
            rc = rtk_lens_render_host(ctx, &lens, &opts, 0, linear.data(), denoise_image_name ? noise.data() : nullptr);
            last_render_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
        if (rc == RTK_OK) {
            rgb8->resize(px * 3);
            for (size_t k = 0; k < px * 3; k++) {
                double g = linear[k] > 0 ? std::sqrt(linear[k]) : 0.0;
                g = g < 0.000 ? 0.000 : (g > 0.999 ? 0.999 : g);
                (*rgb8)[k] = uint8_t(int(255.999 * g));
            }
            rc = display_bytes(cam, linear.data(), rgb8->data());
        }
        if (rc == RTK_OK && denoise_image_name) {
            std::vector<float> guides(px * 16);
            std::vector<uint8_t> den(px * 3);
            std::vector<double> den_linear(display ? px * 3 : 0);
            const rtk_guide_opts go{denoise_follow, 0};
            rc = rtk_lens_guides_host(ctx, &lens, &opts, aov_samples, &go, guides.data());
            if (rc == RTK_OK)
                rc = rtk_denoise_guided_host(ctx, cam.image_width, cam.image_height, real_mode, linear.data(), guides.data(), noise.data(), nullptr,
                                             denoise_demodulate ? RTK_DENOISE_DEMODULATE : 0, display ? den_linear.data() : nullptr, den.data());
            if (rc == RTK_OK) rc = display_bytes(cam, den_linear.data(), den.data());
            if (rc == RTK_OK && write_image) rtk::write_png(denoise_image_name, cam.image_width, cam.image_height, den.data());
        }
        rtk_multi_destroy(multi);
        return rc;
    }

    // With `display`: rgb8 = the display transform of `linear` (see the member); without: nothing.
    int display_bytes(const rtk_camera& cam, const double* linear, uint8_t* rgb8) {
        if (!display) return RTK_OK;
        const int dev = devices.empty() ? device : devices[0];
        if (display_ && (display_->width != cam.image_width || display_->height != cam.image_height || display_->real_mode != real_mode || display_->device != dev)) {
            std::cerr << "camera::render: image size, real mode or device changed; the display's exposure starts over" << std::endl;
            display_.reset();
        }
        if (!display_) {
            auto st = std::make_shared<display_state>();
            int rc = rtk_init_multi(1, &dev, RTK_GATHER_PEER, &st->multi);
            if (rc == RTK_OK) rc = rtk_display_create(rtk_multi_ctx(st->multi, 0), cam.image_width, cam.image_height, real_mode, nullptr, &st->display);
            if (rc != RTK_OK) return rc;
            st->width = cam.image_width;
            st->height = cam.image_height;
            st->real_mode = real_mode;
            st->device = dev;
            display_ = st;
        }
        rtk_display_opts o{};
        o.exposure = display_metered_ ? float(last_exposure) : display_exposure;
        o.adapt = display_adapt;
        o.curve = display_curve;
        o.encode = display_srgb ? RTK_DISPLAY_SRGB : RTK_DISPLAY_GAMMA2;
        o.bloom = display_bloom;
        int rc = rtk_display_apply_host(display_->display, linear, &o, nullptr, rgb8);
        if (rc == RTK_OK && !display_metered_) {
            double e[2];
            rc = rtk_display_exposure(display_->display, e);
            if (rc == RTK_OK) last_exposure = e[0];
            display_metered_ = rc == RTK_OK;
        }
        return rc;
    }

    // Camera.txt:102-106: "\rPercent Rendered: N% " on stderr.
    static void print_progress(int64_t done, int64_t total, void*) {
        const float percent = total > 0 ? 100.0f * float(done) / float(total) : 100.0f;
        std::cerr << "\rPercent Rendered: " << static_cast<int>(percent) << "% " << std::flush;
    }

    // Camera.txt:54.  Blocking; borrows world and lights for the call.
    void render(const hittable& world, std::vector<point_light>& lights) {
        std::vector<uint8_t> rgb8;
        bool temporal = false, scaled = false;
        last_render_upsampled = false;
        last_exposure = 0;
        display_metered_ = false;
        const bool lens = projection != perspective;
        if (lens && (temporal_history > 0 || render_scale > 1)) {
            std::cerr << "camera::render failed: temporal_history and render_scale need the perspective projection (reprojection and the low-resolution "
                         "camera assume a pinhole)" << std::endl;
            return;
        }
        int rc = lens ? render_lens(world, lights, &rgb8) : (render_scale != 1 ? render_scaled(world, lights, &rgb8, &scaled) : RTK_OK);
        last_render_upsampled = scaled;
        if (rc == RTK_OK && !lens && !scaled && temporal_history > 0) rc = render_temporal(world, lights, &rgb8, &temporal);
        if (rc == RTK_OK && !lens && !temporal && !scaled)
            rc = progressive_step > 0 || denoise_image_name ? render_progressive(world, lights, &rgb8) : render_plain(world, lights, &rgb8);
        if (rc != RTK_OK) {
            std::cerr << "camera::render failed: " << rtk_last_error() << std::endl;
            return;
        }
        rtk_camera cam = derive();
        double msamples = double(cam.image_width) * cam.image_height * (progressive_step > 0 ? last_samples_rendered : samples_per_pixel) / 1e6;
        std::cout << "\nDone rendering " << image_name << " in " << last_render_ms / 1000.0 << " seconds ("
                  << msamples / (last_render_ms / 1000.0) << " Msamples/s)" << std::endl;
        if (write_image) rtk::write_png(image_name, cam.image_width, cam.image_height, rgb8.data());
    }

private:
    // What temporal_history keeps between render() calls: the context the history lives on and the history.  Copies of the
    // camera share it.
    struct temporal_state {
        rtk_multi* multi = nullptr;
        rtk_temporal* temporal = nullptr;
        int width = 0, height = 0, real_mode = 0, device = 0;
        void reset() { if (temporal) rtk_temporal_reset(temporal); }
        temporal_state() = default;
        temporal_state(const temporal_state&) = delete;
        temporal_state& operator=(const temporal_state&) = delete;
        ~temporal_state() {
            if (temporal) rtk_temporal_destroy(temporal);
            if (multi) rtk_multi_destroy(multi);
        }
    };
    std::shared_ptr<temporal_state> temporal_;
    // What `display` keeps between render() calls: the context the object lives on and the object.  Copies of the camera share it.
    struct display_state {
        rtk_multi* multi = nullptr;
        rtk_display* display = nullptr;
        int width = 0, height = 0, real_mode = 0, device = 0;
        display_state() = default;
        display_state(const display_state&) = delete;
        display_state& operator=(const display_state&) = delete;
        ~display_state() {
            if (display) rtk_display_destroy(display);
            if (multi) rtk_multi_destroy(multi);
        }
    };
    std::shared_ptr<display_state> display_;
    bool display_metered_ = false;  // within one render(): an image was already metered, the others take last_exposure
};

#endif  // RTK_CAMERA_H
