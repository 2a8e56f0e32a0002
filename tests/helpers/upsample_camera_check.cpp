// GPU test helper: camera::render() of the drop-in C++ API with render_scale, on a library scene built exactly as
// librtk_host.so builds it.  Writes into <out_dir>:
//   up.png               render_scale = 2
//   updemod.png, den.png render_scale = 2 with upsample_demodulate, and its denoise_image_name
//   plain.png            render_scale = 1
//   low.png              render_scale = 2 with too few samples for a noise estimate: rendered at full resolution
//   ut0.png, ut1.png     two calls with render_scale = 2 and temporal_history = 8, lookfrom moved by <dx> along x
// and prints a one-line JSON verdict with last_render_upsampled / last_temporal_frames after each call.
//   upsample_camera_check <out_dir> <scene> <earth_texture> <width> <height> <spp> <depth> <dx>
#include "camera.h"
#include "mesh.h"
#include "scenes/scene_library.h"

#include <cstdio>
#include <cstdlib>
#include <string>

static void configure(camera& cam, const rtk_scene_def& def, char** argv) {
    cam.image_width = std::atoi(argv[4]);
    cam.aspect_ratio = double(cam.image_width) / double(std::atoi(argv[5]));
    cam.samples_per_pixel = std::atoi(argv[6]);
    cam.max_depth = std::atoi(argv[7]);
    cam.background = def.view.background;
    cam.vfov = def.view.vfov;
    cam.lookfrom = def.view.lookfrom;
    cam.lookat = def.view.lookat;
    cam.vup = def.view.vup;
    cam.defocus_angle = def.view.defocus_angle;
    cam.focus_dist = def.view.focus_dist;
    cam.show_progress = false;
    cam.aov_samples = 4;
}

int main(int argc, char** argv) {
    if (argc != 9) return 2;
    const std::string out = argv[1];
    const double dx = std::atof(argv[8]);
    rtk::seed_scene_rng(0x5EED2025u);  // SCENE_SEED of the Python package
    rtk_scene_def def;
    if (!rtk_build_named_scene(argv[2], argv[3], def)) return 3;
    std::vector<point_light> lights;
    for (const auto& l : def.lights) lights.emplace_back(l.position, l.intensity, l.size);
    int upsampled[7], frames[7], n = 0;
    auto render = [&](camera& cam, const std::string& name) {
        const std::string img = out + "/" + name;
        cam.image_name = img.c_str();
        cam.render(def.world, lights);
        upsampled[n] = cam.last_render_upsampled ? 1 : 0;
        frames[n++] = cam.last_temporal_frames;
    };

    camera cam;
    configure(cam, def, argv);
    cam.render_scale = 2;
    render(cam, "up.png");
    const std::string den = out + "/den.png";
    cam.upsample_demodulate = true;
    cam.denoise_image_name = den.c_str();
    render(cam, "updemod.png");

    camera plain;
    configure(plain, def, argv);
    render(plain, "plain.png");
    plain.render_scale = 2;
    plain.samples_per_pixel = 8;  // one chunk: no noise estimate, rendered at full resolution
    render(plain, "low.png");

    camera moving;
    configure(moving, def, argv);
    moving.render_scale = 2;
    moving.temporal_history = 8;
    for (int k = 0; k < 2; k++) {
        moving.lookfrom = def.view.lookfrom + vec3(dx * k, 0, 0);
        render(moving, "ut" + std::to_string(k) + ".png");
    }
    std::printf("{\"upsampled\": [%d, %d, %d, %d, %d, %d], \"frames\": [%d, %d, %d, %d, %d, %d]}\n", upsampled[0], upsampled[1], upsampled[2], upsampled[3],
                upsampled[4], upsampled[5], frames[0], frames[1], frames[2], frames[3], frames[4], frames[5]);
    return 0;
}
