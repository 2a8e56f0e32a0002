// GPU test helper: camera::render() of the drop-in C++ API with progressive_step / checkpoint_file / noise_target, on the
// library scene book1_final built exactly as librtk_host.so builds it (so that a checkpoint written through the Python API
// matches).  Writes PNGs into argv[1] and prints a one-line JSON verdict.
//   progressive_camera_check <out_dir> <checkpoint_file> <width> <height> <spp> <depth> <noise_target>
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
    if (!rtk_build_named_scene("book1_final", "", def)) return 3;
    std::vector<point_light> lights;
    for (const auto& l : def.lights) lights.emplace_back(l.position, l.intensity, l.size);
    camera cam;
    cam.image_width = std::atoi(argv[3]);
    cam.aspect_ratio = double(cam.image_width) / double(std::atoi(argv[4]));
    cam.samples_per_pixel = std::atoi(argv[5]);
    cam.max_depth = std::atoi(argv[6]);
    cam.background = def.view.background;
    cam.vfov = def.view.vfov;
    cam.lookfrom = def.view.lookfrom;
    cam.lookat = def.view.lookat;
    cam.vup = def.view.vup;
    cam.defocus_angle = def.view.defocus_angle;
    cam.focus_dist = def.view.focus_dist;
    cam.show_progress = false;

    const std::string one = out + "/one.png", prog = out + "/prog.png", resumed = out + "/resumed.png", noisy = out + "/noise.png";
    cam.image_name = one.c_str();
    cam.render(def.world, lights);                       // one-shot

    cam.progressive_step = 8;
    cam.image_name = prog.c_str();
    cam.render(def.world, lights);                       // steps of 8
    const int prog_rendered = cam.last_samples_rendered, prog_done = cam.last_samples_done;
    const int prog_valid = cam.last_noise.valid;

    cam.checkpoint_file = argv[2];                       // resumes the Python API's checkpoint, saves after every step
    cam.image_name = resumed.c_str();
    cam.render(def.world, lights);
    const int resumed_rendered = cam.last_samples_rendered, resumed_done = cam.last_samples_done;

    cam.checkpoint_file = nullptr;
    cam.noise_target = std::atof(argv[7]);
    cam.image_name = noisy.c_str();
    cam.render(def.world, lights);
    std::printf("{\"prog_rendered\": %d, \"prog_done\": %d, \"prog_valid\": %d, \"resumed_rendered\": %d, \"resumed_done\": %d, "
                "\"noise_done\": %d, \"noise_rendered\": %d, \"noise_valid\": %d, \"noise_full_chunks\": %d, \"noise_mean_rel_se\": %.17g}\n",
                prog_rendered, prog_done, prog_valid, resumed_rendered, resumed_done, cam.last_samples_done, cam.last_samples_rendered,
                cam.last_noise.valid, cam.last_noise.full_chunks, cam.last_noise.mean_rel_se);
    return 0;
}
