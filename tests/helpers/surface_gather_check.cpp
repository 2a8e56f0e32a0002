// GPU test helper: rtk::surface_gather of the drop-in C++ API (host/rtk_surface_gather.h) on a library scene built exactly as
// librtk_host.so builds it.  Gathers irradiance and occlusion at the 3 x 2 texels of the Cornell box's red wall and prints, with
// 17 significant digits, the texels, their normals and every result; the test compares them with what Python computes.
//   surface_gather_check <scene> <scene_file> <rays> <max_depth> <samples> <real_mode> [<time>]
// The quad, the grid, the reach and the keys are the constants below, restated in tests/test_surface_gather.py.  With <time>
// the class's `time` is set to it, the quad is one under single_fog's moving ball that faces it, and the background is the
// scene's (restated in tests/test_entry_options.py).
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

    rtk::surface_gather gather(def.world, lights);
    if (!gather.ok()) {
        std::printf("surface_gather_check: upload failed (%d): %s\n", gather.status(), rtk_last_error());
        return 5;
    }
    gather.seed = 5;
    gather.real_mode = real_mode;
    gather.first_key = 11;
    gather.samples = samples;
    const bool timed = argc == 8;
    if (timed) gather.time = std::atof(argv[7]);
    const color background = timed ? def.view.background : color(0, 0, 0);
    std::vector<point3> points;
    std::vector<vec3> normals;
    if (timed) rtk::surface_gather::quad_texels(point3(-1.5, -1.25, -1.5), vec3(3, 0, 0), vec3(0, 0, -3), 3, 2, points, normals);
    else rtk::surface_gather::quad_texels(point3(0, 0, 0), vec3(0, 555, 0), vec3(0, 0, 555), 3, 2, points, normals);
    if (points.size() != 6 || normals.size() != 6) return 6;
    for (const point3& p : points) std::printf("point %.17g %.17g %.17g\n", p.x(), p.y(), p.z());
    for (const vec3& n : normals) std::printf("normal %.17g %.17g %.17g\n", n.x(), n.y(), n.z());
    std::vector<color> e;
    if (!gather.irradiance(points, normals, rays, max_depth, background, e) || e.size() != 6) {
        std::printf("surface_gather_check: irradiance failed (%d): %s\n", gather.status(), rtk_last_error());
        return 5;
    }
    for (const color& c : e) std::printf("e %.17g %.17g %.17g\n", c.x(), c.y(), c.z());
    std::vector<double> open;
    std::vector<vec3> bent;
    if (!gather.occlusion(points, normals, rays, 200.0, open, bent) || open.size() != 6 || bent.size() != 6) {
        std::printf("surface_gather_check: occlusion failed (%d): %s\n", gather.status(), rtk_last_error());
        return 5;
    }
    for (double f : open) std::printf("open %.17g\n", f);
    for (const vec3& b : bent) std::printf("bent %.17g %.17g %.17g\n", b.x(), b.y(), b.z());
    std::vector<vec3> five(5, vec3(0, 1, 0));
    if (gather.irradiance(points, five, rays, max_depth, color(0, 0, 0), e) || !gather.ok()) return 7;  // lengths differ: false, and no failure
    if (!gather.irradiance({}, {}, rays, max_depth, color(0, 0, 0), e) || !e.empty() || !gather.ok()) return 7;  // no points: nothing to do
    if (gather.irradiance(points, normals, 100, max_depth, color(0, 0, 0), e) || gather.ok()) return 7;  // rays = 100: refused
    std::printf("refused %d %s\n", gather.status(), rtk_last_error());
    std::printf("surface_gather_check: ok\n");
    return 0;
}
