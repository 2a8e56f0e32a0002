// GPU test helper: camera::projection of the drop-in C++ API (host/rtk_camera.h) on a library scene built exactly as
// librtk_host.so builds it.  Renders one equirect frame to <out.png> through camera::render(), then asks for temporal_history
// with the same projection, which render() must refuse: nothing is written to <refused.png>.
//   lens_camera_check <scene> <scene_file> <out.png> <refused.png> <real_mode>
// The size, samples, seed, frame and extents are the constants below, restated in tests/test_lens.py.
#include "camera.h"
#include "mesh.h"
#include "scenes/scene_library.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char** argv) {
    if (argc != 6) return 2;
    rtk::seed_scene_rng(0x5EED2025u);  // SCENE_SEED of the Python package
    rtk_scene_def def;
    if (!rtk_build_named_scene(argv[1], argv[2], def)) return 3;
    std::vector<point_light> lights;
    for (const auto& l : def.lights) lights.emplace_back(l.position, l.intensity, l.size);

    camera cam;
    cam.image_width = 24;
    cam.aspect_ratio = 1.5;            // 24 x 16
    cam.samples_per_pixel = 3;
    cam.max_depth = def.view.max_depth;
    cam.background = def.view.background;
    cam.lookfrom = point3(0, 0.25, 0.5);
    cam.lookat = point3(0, 0, -1);
    cam.vup = vec3(0, 1, 0);
    cam.projection = camera::equirect;
    cam.fov_h = 4.0;
    cam.fov_v = 2.0;
    cam.seed = 5;
    cam.real_mode = std::atoi(argv[5]);
    cam.order = camera::reference_order;
    cam.show_progress = false;
    cam.image_name = argv[3];
    cam.render(def.world, lights);
    if (FILE* f = std::fopen(argv[3], "rb")) std::fclose(f);
    else return 5;

    cam.temporal_history = 2;
    cam.image_name = argv[4];
    cam.render(def.world, lights);     // refused with a message on stderr
    if (FILE* f = std::fopen(argv[4], "rb")) {
        std::fclose(f);
        return 6;
    }
    cam.temporal_history = 0;
    cam.render_scale = 2;
    cam.render(def.world, lights);     // likewise
    if (FILE* f = std::fopen(argv[4], "rb")) {
        std::fclose(f);
        return 7;
    }
    std::printf("lens_camera_check: ok\n");
    return 0;
}
