// GPU test helper: rtk::light_probes of the drop-in C++ API (host/rtk_light_probes.h) on a library scene built exactly as
// librtk_host.so builds it.  Bakes a 2x2x2 grid and prints, with 17 significant digits, every coefficient and the irradiance at
// two points (single form for the first, batch form for both); the test compares them with what Python computes.
//   light_probes_check <scene> <scene_file> <rays> <max_depth> <samples> <real_mode> [<time>]
// The grid, the points and the normals are the constants below, restated in tests/test_light_probes.py.  With <time> the
// class's `time` is set to it and the grid is one around single_fog's moving ball (restated in tests/test_entry_options.py).
#include "camera.h"
#include "mesh.h"
#include "scenes/scene_library.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char** argv) {
    if (argc != 7 && argc != 8) return 2;
    rtk::seed_scene_rng(0x5EED2025u);  // SCENE_SEED of the Python package
    rtk_scene_def def;
    if (!rtk_build_named_scene(argv[1], argv[2], def)) return 3;
    std::vector<point_light> lights;
    for (const auto& l : def.lights) lights.emplace_back(l.position, l.intensity, l.size);
    const int rays = std::atoi(argv[3]), max_depth = std::atoi(argv[4]), samples = std::atoi(argv[5]), real_mode = std::atoi(argv[6]);

    rtk::light_probes probes(def.world, lights);
    if (!probes.ok()) {
        std::printf("light_probes_check: upload failed (%d): %s\n", probes.status(), rtk_last_error());
        return 5;
    }
    if (probes.irradiance(point3(0, 0, 0), vec3(0, 1, 0)).length_squared() != 0 || !probes.ok()) return 6;  // unbaked: black, and no failure
    probes.seed = 5;
    probes.real_mode = real_mode;
    probes.first_key = 11;
    const bool timed = argc == 8;
    if (timed) probes.time = std::atof(argv[7]);
    const rtk_probe_grid grid = timed ? rtk::light_probes::make_grid(point3(-1.5, -1.5, -4.5), vec3(3, 3, 3), 2, 2, 2)
                                      : rtk::light_probes::make_grid(point3(100, 350, 100), vec3(350, 100, 350), 2, 2, 2);
    if (!probes.bake(grid, rays, max_depth, def.view.background, samples)) {
        std::printf("light_probes_check: bake failed (%d): %s\n", probes.status(), rtk_last_error());
        return 5;
    }
    const std::vector<double>& sh = probes.coefficients();
    if (sh.size() != 8 * 27) return 6;
    for (size_t k = 0; k < sh.size(); k++) std::printf("sh %zu %.17g\n", k, sh[k]);
    const std::vector<point3> points = {point3(200, 400, 300), point3(500, 330, 90)};  // inside the grid; outside it on two axes (the first grid's)
    const std::vector<vec3> normals = {vec3(0, 1, 0), vec3(-0.6, 0, 0.8)};
    const color single = probes.irradiance(points[0], normals[0]);
    std::printf("single %.17g %.17g %.17g\n", single.x(), single.y(), single.z());
    std::vector<color> batch;
    if (!probes.irradiance(points, normals, batch) || batch.size() != 2) return 5;
    for (const color& c : batch) std::printf("batch %.17g %.17g %.17g\n", c.x(), c.y(), c.z());
    if (probes.bake(rtk::light_probes::make_grid(point3(0, 0, 0), vec3(1, 1, 1), 1, 1, 1), 100, max_depth, def.view.background) || probes.ok()) return 7;  // rays = 100: refused
    std::printf("refused %d %s\n", probes.status(), rtk_last_error());
    if (probes.bake(rtk::light_probes::make_grid(point3(0, 0, 0), vec3(1, 1, 1), 2, 0, 1), rays, max_depth, def.view.background)) return 7;  // a grid count of 0
    std::printf("refused-grid %s\n", rtk_last_error());
    if (probes.irradiance(points[0], normals[0]).length_squared() != 0) return 7;  // a refused bake leaves nothing baked
    std::printf("light_probes_check: ok\n");
    return 0;
}
