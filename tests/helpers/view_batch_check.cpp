// Compile check of host/rtk_view_batch.h against the drop-in headers (tests/test_view_batch.py): a reference-style program
// that collects a camera path and a cube capture into one rtk::view_batch.  Compiled, not linked or run.
#include "rtweekend.h"

#include "camera.h"
#include "hittable_list.h"
#include "material.h"
#include "sphere.h"
#include "rtk_view_batch.h"

#include <cstdio>
#include <vector>

int main() {
    hittable_list world;
    world.add(make_shared<sphere>(point3(0, -100.5, -1), 100, make_shared<lambertian>(color(0.8, 0.8, 0.0))));
    world.add(make_shared<sphere>(point3(0, 0, -1.2), 0.5, make_shared<lambertian>(color(0.1, 0.2, 0.5))));
    rtk::view_batch batch(world);
    camera cam;
    cam.aspect_ratio = 1.0;
    cam.image_width = 64;
    cam.samples_per_pixel = 16;
    cam.max_depth = 10;
    for (int k = 0; k < 4; k++) {
        cam.lookfrom = point3(0.5 * k, 0, 1);
        cam.lookat = point3(0, 0, -1);
        batch.add(cam, 7u + k);
    }
    for (const rtk_camera& face : rtk::view_batch::cube_faces(point3(0, 1, 0), 64, 16, 10, color(0.7, 0.8, 1.0))) batch.add(face);
    std::vector<double> linear;
    std::vector<uint8_t> rgb8;
    const bool done = batch.render(&linear, &rgb8);
    std::printf("%zu views of %d x %d: %s (%s)\n", batch.size(), batch.width(), batch.height(), done ? "ok" : rtk_last_error(), batch.kernel_name());
    return done ? 0 : 1;
}
