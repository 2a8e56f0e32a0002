// GPU test helper: camera::render() of the drop-in C++ API with temporal_history, on a library scene built exactly as
// librtk_host.so builds it.  Three render() calls with temporal_history = 8 and lookfrom moved by <dx> along x per call write
// t0.png, t1.png, t2.png (the accumulated frames) and d2.png (the third call's denoise_image_name); then, on a fresh camera, one call
// with temporal_history = 0 writes plain.png and one with too few samples for a noise estimate writes low.png.  Prints a
// one-line JSON verdict with last_temporal_frames after each call.
//   temporal_camera_check <out_dir> <scene> <earth_texture> <width> <height> <spp> <depth> <dx>
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

    camera cam;
    configure(cam, def, argv);
    cam.temporal_history = 8;
    int frames[3];
    const std::string den = out + "/d2.png";
    for (int k = 0; k < 3; k++) {
        const std::string img = out + "/t" + std::to_string(k) + ".png";
        cam.image_name = img.c_str();
        cam.lookfrom = def.view.lookfrom + vec3(dx * k, 0, 0);
        cam.denoise_image_name = k == 2 ? den.c_str() : nullptr;
        cam.render(def.world, lights);
        frames[k] = cam.last_temporal_frames;
    }

    camera plain;
    configure(plain, def, argv);
    const std::string one = out + "/plain.png", low = out + "/low.png";
    plain.image_name = one.c_str();
    plain.render(def.world, lights);
    const int plain_frames = plain.last_temporal_frames;
    plain.temporal_history = 8;
    plain.samples_per_pixel = 8;  // one chunk: no noise estimate, rendered without history
    plain.image_name = low.c_str();
    plain.render(def.world, lights);
    std::printf("{\"frames\": [%d, %d, %d], \"plain_frames\": %d, \"low_frames\": %d}\n", frames[0], frames[1], frames[2], plain_frames, plain.last_temporal_frames);
    return 0;
}
