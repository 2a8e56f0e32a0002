// rtk_surface_gather.h -- lightmaps and ambient occlusion from the drop-in C++ API.
//
// Irradiance and occlusion at points on surfaces (include/rtk.h "Surface gathers"): each point looks along a cosine-weighted set
// of directions around its own unit normal.  Like rtk::light_probes the object flattens and uploads the scene ONCE:
//
//     rtk::surface_gather gather(world, lights);
//     std::vector<point3> points; std::vector<vec3> normals;
//     rtk::surface_gather::quad_texels(point3(0, 0, 0), vec3(555, 0, 0), vec3(0, 0, 555), 64, 64, points, normals);   // a lightmap's texels
//     std::vector<color> e;
//     gather.irradiance(points, normals, 256, 25, color(0, 0, 0), e);     // E; times albedo / pi = the diffuse radiance
//     std::vector<double> open; std::vector<vec3> bent;
//     gather.occlusion(points, normals, 256, 100.0, open, bent);          // rays open within 100 units, and where they point
//
// Every call blocks.  The scene is uploaded in the reference's visiting order.  ok() / status() tell whether the upload and every
// library call so far succeeded (rtk_last_error() has the text of the latest failure); status() keeps the first failure.  One
// misuse of the class itself never reaches the library and leaves status() alone: vectors of points and normals that differ in
// length (false).
#ifndef RTK_SURFACE_GATHER_H
#define RTK_SURFACE_GATHER_H

#include <vector>

#include "rtk.h"
#include "rtk_scene_api.h"  // hittable, point_light, scene_builder, flatten; point3, vec3, color through rtk_math.h (it includes this file last)

namespace rtk {

class surface_gather {
public:
    uint32_t seed = 1;              // the stream seed (rtk_gather_opts.seed)
    uint32_t first_key = 0;         // point k draws from the streams of pixel key first_key + k
    bool rotate = true;             // each point its own rotation of the direction set
    int samples = 1;                // paths per ray
    double time = 0.0;              // the time of every ray
    int real_mode = RTK_REAL_F64;

    explicit surface_gather(const hittable& world, const std::vector<point_light>& lights = {}, int device = 0) {
        scene_builder sb;
        const rtk_scene_desc desc = flatten(world, lights, sb);
        status_ = rtk_init(device, &ctx_);
        if (status_ == RTK_OK) status_ = rtk_scene_upload(ctx_, &desc);
    }
    surface_gather(const surface_gather&) = delete;
    surface_gather& operator=(const surface_gather&) = delete;
    ~surface_gather() {
        if (ctx_) rtk_destroy(ctx_);
    }

    bool ok() const { return status_ == RTK_OK; }
    int status() const { return status_; }

    // The texel centres of the quad Q, u, v on an nu x nv grid -- texel (i, j) at index j * nu + i, Q + ((i + .5) / nu) u +
    // ((j + .5) / nv) v -- each with the quad's normal, unit_vector(cross(u, v)), as quad.h computes it.
    static void quad_texels(const point3& Q, const vec3& u, const vec3& v, int nu, int nv, std::vector<point3>& points, std::vector<vec3>& normals) {
        points.clear();
        normals.clear();
        const vec3 n = unit_vector(cross(u, v));
        for (int j = 0; j < nv; j++)
            for (int i = 0; i < nu; i++) {
                points.push_back(Q + ((i + 0.5) / nu) * u + ((j + 0.5) / nv) * v);
                normals.push_back(n);
            }
    }

    // E at every point: `rays` rays per point (a multiple of 64), ray_color to max_depth against `background`.
    bool irradiance(const std::vector<point3>& points, const std::vector<vec3>& normals, int rays, int max_depth, color background, std::vector<color>& out) {
        out.assign(points.size(), color(0, 0, 0));
        if (normals.size() != points.size()) return false;
        std::vector<double> p, n, e(points.size() * 3 + 1, 0.0);
        pack(points, normals, p, n);
        rtk_gather_opts o = options(rays);
        o.max_depth = max_depth;
        o.background = to_abi(background);
        if (!call(rtk_gather_irradiance_host(ctx_, &o, int64_t(points.size()), p.data(), n.data(), e.data()))) return false;
        for (size_t k = 0; k < points.size(); k++) out[k] = color(e[3 * k], e[3 * k + 1], e[3 * k + 2]);
        return true;
    }

    // The open fraction of every point's rays within max_distance (0 = any distance) and the bent normal: the mean over all
    // rays of the open rays' directions, not normalised.
    bool occlusion(const std::vector<point3>& points, const std::vector<vec3>& normals, int rays, double max_distance, std::vector<double>& open,
                   std::vector<vec3>& bent) {
        open.assign(points.size(), 0.0);
        bent.assign(points.size(), vec3(0, 0, 0));
        if (normals.size() != points.size()) return false;
        std::vector<double> p, n, f(points.size() + 1, 0.0), b(points.size() * 3 + 1, 0.0);
        pack(points, normals, p, n);
        rtk_gather_opts o = options(rays);
        o.max_distance = max_distance;
        if (!call(rtk_gather_occlusion_host(ctx_, &o, int64_t(points.size()), p.data(), n.data(), f.data(), b.data()))) return false;
        for (size_t k = 0; k < points.size(); k++) {
            open[k] = f[k];
            bent[k] = vec3(b[3 * k], b[3 * k + 1], b[3 * k + 2]);
        }
        return true;
    }

private:
    rtk_ctx* ctx_ = nullptr;
    int status_ = RTK_OK;

    rtk_gather_opts options(int rays) const {
        rtk_gather_opts o{};
        o.seed = seed;
        o.real_mode = real_mode;
        o.samples = samples;
        o.rays = rays;
        o.first_key = first_key;
        o.rotate = rotate ? 1 : 0;
        o.time = time;
        return o;
    }
    // (one spare element each: data() of an empty vector may be null, which the library refuses before it sees n == 0)
    static void pack(const std::vector<point3>& points, const std::vector<vec3>& normals, std::vector<double>& p, std::vector<double>& n) {
        p.assign(points.size() * 3 + 1, 0.0);
        n.assign(points.size() * 3 + 1, 0.0);
        for (size_t k = 0; k < points.size(); k++)
            for (int a = 0; a < 3; a++) {
                p[3 * k + a] = points[k][a];
                n[3 * k + a] = normals[k][a];
            }
    }
    bool call(int rc) {
        if (rc != RTK_OK && status_ == RTK_OK) status_ = rc;
        return rc == RTK_OK;
    }
};

}  // namespace rtk

#endif  // RTK_SURFACE_GATHER_H
