// GPU test helper: camera::render() of the drop-in C++ API with progressive_step and adaptive_target, on a library scene built
// exactly as librtk_host.so builds it.  Renders one-shot, then adaptively with a rel_target no tile reaches, a middling one and
// one every tile meets at once.  Writes PNGs into argv[1] and prints a one-line JSON verdict.
//   adaptive_camera_check <out_dir> <scene> <earth_texture> <width> <height> <spp> <depth> <unreachable_rel_target> <rel_target>
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

    const std::string one = out + "/one.png", never = out + "/never.png", mid = out + "/mid.png", all = out + "/all.png";
    cam.image_name = one.c_str();
    cam.render(def.world, lights);                       // one-shot

    struct Run {
        int done, rendered;
        rtk_adaptive_state st;
    } runs[3];
    const double targets[3] = {std::atof(argv[8]), std::atof(argv[9]), 1e9};
    const std::string* names[3] = {&never, &mid, &all};
    cam.progressive_step = 8;
    cam.adaptive_min_samples = 16;
    for (int k = 0; k < 3; k++) {
        cam.adaptive_target = targets[k];
        cam.image_name = names[k]->c_str();
        cam.render(def.world, lights);
        runs[k] = {cam.last_samples_done, cam.last_samples_rendered, cam.last_adaptive};
    }
    const char* keys[3] = {"never", "mid", "all"};
    std::printf("{");
    for (int k = 0; k < 3; k++)
        std::printf("%s\"%s_done\": %d, \"%s_rendered\": %d, \"%s_active\": %d, \"%s_retired\": %d, \"%s_pixel_samples\": %lld, \"%s_mean_spp\": %.17g",
                    k ? ", " : "", keys[k], runs[k].done, keys[k], runs[k].rendered, keys[k], runs[k].st.active_tiles, keys[k], runs[k].st.retired_tiles,
                    keys[k], (long long)runs[k].st.pixel_samples, keys[k], runs[k].st.mean_spp);
    std::printf("}\n");
    return 0;
}
