// GPU test helper: camera::render() of the drop-in C++ API with render_scale = 2 and refine_support, on a library scene built
// exactly as librtk_host.so builds it.  Writes into <out_dir>:
//   refined.png    refine_support = <support>, refine_dilate = <dilate>, refine_max_share 0 (no limit)
//   unrefined.png  refine_support = 0: render_scale alone
//   over.png       refine_support = <support> with refine_max_share = 0.001: more tiles chosen than allowed, none re-rendered
// and prints a one-line JSON verdict with last_refined_tiles after each call.
//   refine_camera_check <out_dir> <scene> <earth_texture> <width> <height> <spp> <depth> <support> <dilate>
#include "camera.h"
#include "mesh.h"
#include "scenes/scene_library.h"

#include <cstdio>
#include <cstdlib>
#include <string>

int main(int argc, char** argv) {
    if (argc != 10) return 2;
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
    cam.aov_samples = 4;
    cam.render_scale = 2;
    int refined[3], upsampled[3], n = 0;
    auto render = [&](const std::string& name) {
        const std::string img = out + "/" + name;
        cam.image_name = img.c_str();
        cam.render(def.world, lights);
        upsampled[n] = cam.last_render_upsampled ? 1 : 0;
        refined[n++] = cam.last_refined_tiles;
    };
    cam.refine_support = std::atof(argv[8]);
    cam.refine_dilate = std::atoi(argv[9]);
    cam.refine_max_share = 0;
    render("refined.png");
    cam.refine_support = 0;
    render("unrefined.png");
    cam.refine_support = std::atof(argv[8]);
    cam.refine_max_share = 0.001;
    render("over.png");
    std::printf("{\"upsampled\": [%d, %d, %d], \"refined\": [%d, %d, %d]}\n", upsampled[0], upsampled[1], upsampled[2], refined[0], refined[1], refined[2]);
    return 0;
}
