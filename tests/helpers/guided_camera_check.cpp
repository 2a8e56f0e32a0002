// GPU test helper: camera::render() of the drop-in C++ API with denoise_image_name and the guided denoiser's switches, on a
// library scene built exactly as librtk_host.so builds it.  Writes first.png (denoise_follow left 0), mirror.png (denoise_follow =
// RTK_GUIDE_FOLLOW_MIRROR) and demod.png (denoise_demodulate as well).  Prints a one-line JSON verdict.
//   guided_camera_check <out_dir> <scene> <earth_texture> <width> <height> <spp> <depth>
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

    const std::string img = out + "/img.png", first = out + "/first.png", mirror = out + "/mirror.png", demod = out + "/demod.png";
    cam.image_name = img.c_str();
    cam.aov_samples = 4;
    cam.denoise_image_name = first.c_str();
    cam.render(def.world, lights);
    cam.denoise_follow = RTK_GUIDE_FOLLOW_MIRROR;
    cam.denoise_image_name = mirror.c_str();
    cam.render(def.world, lights);
    cam.denoise_demodulate = true;
    cam.denoise_image_name = demod.c_str();
    cam.render(def.world, lights);
    std::printf("{\"rendered\": 3}\n");
    return 0;
}
