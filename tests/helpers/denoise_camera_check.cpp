// GPU test helper: camera::render() of the drop-in C++ API with denoise_image_name, on a library scene built exactly as
// librtk_host.so builds it.  Renders one-shot (one.png), then with denoise_image_name set (two.png and den.png), then once more
// with a target below two chunks, which must fail and write nothing.  Prints a one-line JSON verdict.
//   denoise_camera_check <out_dir> <scene> <earth_texture> <width> <height> <spp> <depth>
#include "camera.h"
#include "mesh.h"
#include "scenes/scene_library.h"

#include <cstdio>
#include <cstdlib>
#include <string>

int main(int argc, char** argv) {
    if (argc != 8) return 2;
    const std::string out = argv[1];
    rtk::seed_scene_rng(0x5EED2025u);  // SCENE_SEED of the Python package
    rtk_scene_def def;
    if (!rtk_build_named_scene(argv[2], argv[3], def)) return 3;
    std::vector<point_light> lights;
    for (const auto& l : def.lights) lights.emplace_back(l.position, l.intensity, l.size);
    camera cam;
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

    const std::string one = out + "/one.png", two = out + "/two.png", den = out + "/den.png", low = out + "/low.png", low_den = out + "/low_den.png";
    cam.image_name = one.c_str();
    cam.render(def.world, lights);  // one-shot
    cam.image_name = two.c_str();
    cam.denoise_image_name = den.c_str();
    cam.aov_samples = 4;
    cam.render(def.world, lights);  // one progressive step of the whole target, then the denoised image
    cam.samples_per_pixel = 8;      // one chunk: no noise estimate
    cam.image_name = low.c_str();
    cam.denoise_image_name = low_den.c_str();
    cam.render(def.world, lights);
    const bool failed = std::fopen(low.c_str(), "rb") == nullptr && std::fopen(low_den.c_str(), "rb") == nullptr;
    std::printf("{\"low_spp_failed\": %d}\n", failed ? 1 : 0);
    return 0;
}
