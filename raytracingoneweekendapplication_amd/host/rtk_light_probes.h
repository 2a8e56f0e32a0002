// rtk_light_probes.h -- baked diffuse lighting from the drop-in C++ API.
//
// A grid of light probes over the scene (include/rtk.h "Light probes"): each probe looks along a fixed sphere of directions and
// keeps what it sees as nine spherical-harmonic coefficients per colour channel; irradiance at a point with a normal is looked
// up from the eight probes around it.  Like rtk::ray_query the object flattens and uploads the scene ONCE; bake() keeps the
// coefficients on the host, the lookups upload them with the points:
//
//     rtk::light_probes probes(world, lights);
//     probes.bake(rtk::light_probes::make_grid(point3(50, 50, 50), vec3(150, 150, 150), 4, 4, 4), 1024, 25, color(0, 0, 0));
//     color e = probes.irradiance(surface_point, surface_normal);      // E(n); times albedo / pi = the diffuse radiance
//
// Every call blocks.  The scene is uploaded in the reference's visiting order.  ok() / status() tell whether the upload and every
// library call so far succeeded (rtk_last_error() has the text of the latest failure); status() keeps the first failure.  A
// lookup on a failed object returns black.  Two misuses of the class itself never reach the library and leave status() alone:
// a lookup before any successful bake (black / false) and a batch lookup whose two vectors differ in length (false).
#ifndef RTK_LIGHT_PROBES_H
#define RTK_LIGHT_PROBES_H

#include <vector>

#include "rtk.h"
#include "rtk_scene_api.h"  // hittable, point_light, scene_builder, flatten; point3, vec3, color through rtk_math.h (it includes this file last)

namespace rtk {

class light_probes {
public:
    uint32_t seed = 1;              // the stream seed of the bake (rtk_probe_opts.seed)
    uint32_t first_key = 0;         // probe k draws from the streams of pixel key first_key + k
    double time = 0.0;              // the time of every probe ray
    int real_mode = RTK_REAL_F64;

    explicit light_probes(const hittable& world, const std::vector<point_light>& lights = {}, int device = 0) {
        scene_builder sb;
        const rtk_scene_desc desc = flatten(world, lights, sb);
        status_ = rtk_init(device, &ctx_);
        if (status_ == RTK_OK) status_ = rtk_scene_upload(ctx_, &desc);
    }
    light_probes(const light_probes&) = delete;
    light_probes& operator=(const light_probes&) = delete;
    ~light_probes() {
        if (ctx_) rtk_destroy(ctx_);
    }

    bool ok() const { return status_ == RTK_OK; }
    int status() const { return status_; }

    // nx x ny x nz probes, probe (ix, iy, iz) at origin + (ix, iy, iz) * spacing.
    static rtk_probe_grid make_grid(const point3& origin, const vec3& spacing, int nx, int ny, int nz) {
        rtk_probe_grid g{};
        g.origin = to_abi(origin);
        g.spacing = to_abi(spacing);
        g.counts[0] = nx;
        g.counts[1] = ny;
        g.counts[2] = nz;
        return g;
    }

    // Bake every probe of `grid`: `rays` rays per probe (a multiple of 256), `samples` paths per ray, ray_color to max_depth
    // against `background`.  Keeps the grid and its coefficients; false when the call failed (status()).
    bool bake(const rtk_probe_grid& grid, int rays, int max_depth, color background, int samples = 1) {
        baked_ = false;
        // the grid is refused by the entry point that will read it (counts, spacing, reserved; m = 0 launches nothing), so that
        // status() and rtk_last_error() say what a lookup would have said
        double none = 0.0;
        if (!call(rtk_probe_irradiance_host(ctx_, real_mode, &grid, &none, 0, &none, &none, &none))) return false;
        const size_t n = size_t(grid.counts[0]) * size_t(grid.counts[1]) * size_t(grid.counts[2]);
        std::vector<double> positions;
        positions.reserve(n * 3);
        for (int iz = 0; iz < grid.counts[2]; iz++)
            for (int iy = 0; iy < grid.counts[1]; iy++)
                for (int ix = 0; ix < grid.counts[0]; ix++) {
                    positions.push_back(grid.origin.x + double(ix) * grid.spacing.x);
                    positions.push_back(grid.origin.y + double(iy) * grid.spacing.y);
                    positions.push_back(grid.origin.z + double(iz) * grid.spacing.z);
                }
        rtk_probe_opts o{};
        o.seed = seed;
        o.real_mode = real_mode;
        o.max_depth = max_depth;
        o.samples = samples;
        o.rays = rays;
        o.first_key = first_key;
        o.background = to_abi(background);
        o.time = time;
        sh_.assign(n * 3 * RTK_PROBE_COEFFS, 0.0);
        grid_ = grid;
        baked_ = call(rtk_probe_bake_host(ctx_, &o, int64_t(n), positions.data(), sh_.data()));
        return baked_;
    }

    // The baked grid and its coefficients, [probe][9][3] (F32 results widened); empty before the first bake.
    const rtk_probe_grid& grid() const { return grid_; }
    const std::vector<double>& coefficients() const { return sh_; }

    // E(n) at `point` for the unit normal `normal`, interpolated between the eight probes around the point.
    color irradiance(const point3& point, const vec3& normal) {
        std::vector<color> out;
        irradiance(std::vector<point3>{point}, std::vector<vec3>{normal}, out);
        return out.empty() ? color(0, 0, 0) : out[0];
    }
    // The same for many points in one launch; false when the call failed (status()), nothing is baked or the lengths differ.
    bool irradiance(const std::vector<point3>& points, const std::vector<vec3>& normals, std::vector<color>& out) {
        out.assign(points.size(), color(0, 0, 0));
        if (!baked_ || normals.size() != points.size()) return false;
        if (points.empty()) return true;
        std::vector<double> p, n, e(points.size() * 3, 0.0);
        for (size_t k = 0; k < points.size(); k++)
            for (int a = 0; a < 3; a++) {
                p.push_back(points[k][a]);
                n.push_back(normals[k][a]);
            }
        if (!call(rtk_probe_irradiance_host(ctx_, real_mode, &grid_, sh_.data(), int64_t(points.size()), p.data(), n.data(), e.data()))) return false;
        for (size_t k = 0; k < points.size(); k++) out[k] = color(e[3 * k], e[3 * k + 1], e[3 * k + 2]);
        return true;
    }

private:
    rtk_ctx* ctx_ = nullptr;
    int status_ = RTK_OK;
    bool baked_ = false;
    rtk_probe_grid grid_{};
    std::vector<double> sh_;

    bool call(int rc) {
        if (rc != RTK_OK && status_ == RTK_OK) status_ = rc;
        return rc == RTK_OK;
    }
};

}  // namespace rtk

#endif  // RTK_LIGHT_PROBES_H
