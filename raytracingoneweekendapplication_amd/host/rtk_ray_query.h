// rtk_ray_query.h -- asking the scene a question from the drop-in C++ API.
//
// The classes of rtk_scene_api.h are descriptions: none of them can intersect a ray on the host.  What the reference's users
// reach through world.hit(r, interval, rec) and ray_color (hittable.h:33, Camera.txt:203-238) is here an object that flattens
// and uploads the scene ONCE, as camera::render_to does, and then answers through the ray queries of include/rtk.h
// (rtk_query_hits / _occluded / _radiance) on the device:
//
//     rtk::ray_query q(world, lights);
//     rtk_ray_hit rec;
//     if (q.hit(ray(origin, direction), interval(0.001, infinity), rec)) ...
//     if (!q.occluded(surface_point, light_position)) ...
//     color c = q.radiance(ray(origin, direction), 50, color(0.7, 0.8, 1.0), 16);
//
// Every call blocks; the batch forms take many rays in one launch.  The scene is uploaded in the reference's visiting order.
// ok() / status() tell whether the upload succeeded (rtk_last_error() has the text); a query on a failed object returns false /
// black; status() keeps the first failure.
#ifndef RTK_RAY_QUERY_H
#define RTK_RAY_QUERY_H

#include <vector>

#include "rtk.h"
#include "rtk_scene_api.h"  // hittable, point_light, scene_builder, flatten; ray, interval, color through rtk_math.h (it includes this file last)

namespace rtk {

class ray_query {
public:
    uint32_t seed = 1;              // the stream seed of every query (rtk_query_opts.seed)
    int real_mode = RTK_REAL_F64;

    explicit ray_query(const hittable& world, const std::vector<point_light>& lights = {}, int device = 0) {
        scene_builder sb;
        const rtk_scene_desc desc = flatten(world, lights, sb);
        status_ = rtk_init(device, &ctx_);
        if (status_ == RTK_OK) status_ = rtk_scene_upload(ctx_, &desc);
    }
    ray_query(const ray_query&) = delete;
    ray_query& operator=(const ray_query&) = delete;
    ~ray_query() {
        if (ctx_) rtk_destroy(ctx_);
    }

    bool ok() const { return status_ == RTK_OK; }
    int status() const { return status_; }

    // A ray record with stream keys (pixel, sample); skip = uniforms of that stream already consumed.
    static rtk_ray make_ray(const ray& r, interval t = interval(0.001, infinity), uint32_t pixel = 0, uint32_t sample = 0, uint32_t skip = 0) {
        rtk_ray q{};
        for (int k = 0; k < 3; k++) {
            q.origin[k] = r.origin()[k];
            q.direction[k] = r.direction()[k];
        }
        q.time = r.time();
        q.tmin = t.min;
        q.tmax = t.max;
        q.pixel = pixel;
        q.sample = sample;
        q.skip = skip;
        return q;
    }

    // hittable::hit(r, ray_t, rec) of the world.
    bool hit(const ray& r, interval ray_t, rtk_ray_hit& rec) {
        rec = rtk_ray_hit{};
        const rtk_ray q = make_ray(r, ray_t);
        const rtk_query_opts o = opts();
        return call(rtk_query_hits_host(ctx_, &o, 1, &q, &rec)) && rec.hit != 0;
    }
    // Is anything between a and b?  The segment is the ray from a with direction b - a on interval(0.001, 1 - 0.001).
    bool occluded(const point3& a, const point3& b) {
        const rtk_ray q = make_ray(ray(a, b - a), interval(0.001, 1 - 0.001));
        const rtk_query_opts o = opts();
        int32_t flag = 0;
        return call(rtk_query_occluded_host(ctx_, &o, 1, &q, &flag)) && flag != 0;
    }
    // ray_color(r, max_depth, world, lights) against `background`, the mean of `samples` samples.
    color radiance(const ray& r, int max_depth, color background, int samples = 1) {
        const rtk_ray q = make_ray(r);
        double rgb[3] = {0, 0, 0};
        const rtk_query_opts o = opts(max_depth, background, samples);
        call(rtk_query_radiance_host(ctx_, &o, 1, &q, rgb, nullptr));
        return color(rgb[0], rgb[1], rgb[2]);
    }

    // The same for many rays in one launch each; false when the call failed (status()).
    bool hit(const std::vector<rtk_ray>& rays, std::vector<rtk_ray_hit>& recs) {
        recs.assign(rays.size(), rtk_ray_hit{});
        const rtk_query_opts o = opts();
        return rays.empty() || call(rtk_query_hits_host(ctx_, &o, int64_t(rays.size()), rays.data(), recs.data()));
    }
    bool occluded(const std::vector<rtk_ray>& rays, std::vector<int32_t>& flags) {
        flags.assign(rays.size(), 0);
        const rtk_query_opts o = opts();
        return rays.empty() || call(rtk_query_occluded_host(ctx_, &o, int64_t(rays.size()), rays.data(), flags.data()));
    }
    bool radiance(const std::vector<rtk_ray>& rays, int max_depth, color background, int samples, std::vector<color>& out) {
        std::vector<double> rgb(rays.size() * 3, 0.0);
        const rtk_query_opts o = opts(max_depth, background, samples);
        const bool done = rays.empty() || call(rtk_query_radiance_host(ctx_, &o, int64_t(rays.size()), rays.data(), rgb.data(), nullptr));
        out.clear();
        for (size_t k = 0; k < rays.size(); k++) out.emplace_back(rgb[3 * k], rgb[3 * k + 1], rgb[3 * k + 2]);
        return done;
    }

private:
    rtk_ctx* ctx_ = nullptr;
    int status_ = RTK_OK;

    rtk_query_opts opts(int max_depth = 0, color background = color(0, 0, 0), int samples = 1) const {
        rtk_query_opts o{};
        o.seed = seed;
        o.real_mode = real_mode;
        o.max_depth = max_depth;
        o.samples = samples;
        o.background = to_abi(background);
        return o;
    }
    bool call(int rc) {
        if (rc != RTK_OK && status_ == RTK_OK) status_ = rc;
        return rc == RTK_OK;
    }
};

}  // namespace rtk

#endif  // RTK_RAY_QUERY_H
