// GPU test helper: camera::render() of the drop-in C++ API with the display transform, on a library scene built exactly as
// librtk_host.so builds it.  Writes into <out_dir>:
//   off.png              display = false: the one-shot image
//   on.png               display on the one-shot path: ACES, sRGB, bloom 0.5, metered
//   prog.png, den.png    display on the progressive path with denoise_image_name: REINHARD, metered; den.png takes prog.png's exposure
//   up.png               display on the upsampled path (render_scale = 2): a manual exposure of 0.5
//   t0.png .. t2.png     three calls with temporal_history = 8 and display_adapt = 0.5, lookfrom moved by <dx> along x, then
//   t3.png               one more after display_reset()
// and prints a one-line JSON verdict with last_exposure after each call.
//   display_camera_check <out_dir> <scene> <earth_texture> <width> <height> <spp> <depth> <dx>
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
    double exposure[8];
    int n = 0;
    auto render = [&](camera& cam, const std::string& name) {
        const std::string img = out + "/" + name;
        cam.image_name = img.c_str();
        cam.render(def.world, lights);
        exposure[n++] = cam.last_exposure;
    };

    camera off;
    configure(off, def, argv);
    render(off, "off.png");

    camera on;
    configure(on, def, argv);
    on.display = true;
    on.display_curve = RTK_DISPLAY_ACES;
    on.display_srgb = true;
    on.display_bloom = 0.5f;
    render(on, "on.png");

    camera prog;
    configure(prog, def, argv);
    const std::string den = out + "/den.png";
    prog.denoise_image_name = den.c_str();
    prog.display = true;
    prog.display_curve = RTK_DISPLAY_REINHARD;
    render(prog, "prog.png");

    camera up;
    configure(up, def, argv);
    up.render_scale = 2;
    up.display = true;
    up.display_exposure = 0.5f;
    render(up, "up.png");

    camera moving;
    configure(moving, def, argv);
    moving.temporal_history = 8;
    moving.display = true;
    moving.display_curve = RTK_DISPLAY_REINHARD;
    moving.display_adapt = 0.5f;
    for (int k = 0; k < 4; k++) {
        moving.lookfrom = def.view.lookfrom + vec3(dx * k, 0, 0);
        if (k == 3) moving.display_reset();
        render(moving, "t" + std::to_string(k) + ".png");
    }
    std::printf("{\"exposure\": [%.17g, %.17g, %.17g, %.17g, %.17g, %.17g, %.17g, %.17g]}\n", exposure[0], exposure[1], exposure[2], exposure[3], exposure[4],
                exposure[5], exposure[6], exposure[7]);
    return 0;
}
