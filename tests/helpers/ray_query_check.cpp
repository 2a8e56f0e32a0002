// GPU test helper: rtk::ray_query of the drop-in C++ API (host/rtk_ray_query.h) on a library scene built exactly as
// librtk_host.so builds it.  The test computed, through Python, the answers for the rays of <case>; this program asks the
// same questions through the host API -- the batch forms for every ray, the single forms for each -- and exits 0 when every
// answer has the same bits.
//   ray_query_check <scene> <scene_file> <case>
// <case>: int32 n, max_depth, samples; double background[3]; rtk_ray[n]; rtk_ray_hit[n]; int32 occluded[n]; double radiance[n][3];
// double a[24][3], b[24][3] -- the end points of the last 24 rays, which are segments (tmin 0.001, tmax 1 - 0.001); the first
// n - 24 rays are on interval(0.001, inf).  Every ray has stream keys (0, 0, 0), the seed is 1.
#include "camera.h"
#include "mesh.h"
#include "scenes/scene_library.h"

#include <cstdio>
#include <cstring>
#include <vector>

template <typename T>
static bool read(FILE* f, T* dst, size_t count) { return std::fread(dst, sizeof(T), count, f) == count; }

static int fail(const char* what, int k) {
    std::printf("ray_query_check: %s differs at ray %d\n", what, k);
    return 1;
}

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    rtk::seed_scene_rng(0x5EED2025u);  // SCENE_SEED of the Python package
    rtk_scene_def def;
    if (!rtk_build_named_scene(argv[1], argv[2], def)) return 3;
    std::vector<point_light> lights;
    for (const auto& l : def.lights) lights.emplace_back(l.position, l.intensity, l.size);

    FILE* f = std::fopen(argv[3], "rb");
    if (!f) return 4;
    int32_t head[3];
    double bg[3];
    if (!read(f, head, 3) || !read(f, bg, 3) || head[0] < 24) return 4;
    const int n = head[0], max_depth = head[1], samples = head[2], n_segments = 24;
    std::vector<rtk_ray> rays(n);
    std::vector<rtk_ray_hit> want_hits(n);
    std::vector<int32_t> want_occluded(n);
    std::vector<double> want_radiance(size_t(n) * 3), ends(size_t(n_segments) * 6);
    if (!read(f, rays.data(), n) || !read(f, want_hits.data(), n) || !read(f, want_occluded.data(), n) || !read(f, want_radiance.data(), size_t(n) * 3) ||
        !read(f, ends.data(), ends.size()))
        return 4;
    std::fclose(f);
    const color background(bg[0], bg[1], bg[2]);

    rtk::ray_query q(def.world, lights);
    if (!q.ok()) {
        std::printf("ray_query_check: upload failed (%d): %s\n", q.status(), rtk_last_error());
        return 5;
    }
    std::vector<rtk_ray_hit> hits;
    std::vector<int32_t> occluded;
    std::vector<color> radiance;
    if (!q.hit(rays, hits) || !q.occluded(rays, occluded) || !q.radiance(rays, max_depth, background, samples, radiance)) {
        std::printf("ray_query_check: a batch query failed (%d): %s\n", q.status(), rtk_last_error());
        return 5;
    }
    for (int k = 0; k < n; k++) {
        if (std::memcmp(&hits[k], &want_hits[k], sizeof(rtk_ray_hit)) != 0) return fail("batch hit", k);
        if (occluded[k] != want_occluded[k]) return fail("batch occluded", k);
        const double rgb[3] = {radiance[k].x(), radiance[k].y(), radiance[k].z()};
        if (std::memcmp(rgb, &want_radiance[size_t(k) * 3], sizeof rgb) != 0) return fail("batch radiance", k);
    }
    for (int k = 0; k < n; k++) {
        const rtk_ray& r = rays[k];
        const ray ry(point3(r.origin[0], r.origin[1], r.origin[2]), vec3(r.direction[0], r.direction[1], r.direction[2]), r.time);
        rtk_ray_hit rec;
        const bool hit = q.hit(ry, interval(r.tmin, r.tmax), rec);
        if (hit != (want_hits[k].hit != 0) || std::memcmp(&rec, &want_hits[k], sizeof rec) != 0) return fail("hit", k);
        const color c = q.radiance(ry, max_depth, background, samples);
        const double rgb[3] = {c.x(), c.y(), c.z()};
        if (std::memcmp(rgb, &want_radiance[size_t(k) * 3], sizeof rgb) != 0) return fail("radiance", k);
    }
    for (int s = 0; s < n_segments; s++) {  // occluded(a, b): the segment from a to b
        const int k = n - n_segments + s;
        const double* a = &ends[size_t(s) * 3];
        const double* b = &ends[size_t(n_segments + s) * 3];
        if (q.occluded(point3(a[0], a[1], a[2]), point3(b[0], b[1], b[2])) != (want_occluded[k] != 0)) return fail("occluded", k);
    }
    if (!q.ok()) return 5;
    std::printf("ray_query_check: ok (%d rays)\n", n);
    return 0;
}
