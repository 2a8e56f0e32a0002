// rtk_api.cpp -- implementation of the C ABI in include/rtk.h (host side of
// librtk_hip.so; compiled by hipcc).  It validates an rtk_scene_desc, compiles
// the scene graph into the linear traversal program of rtk_device_layout.h,
// uploads f64 and f32 images of it to HBM and owns the context's life (struct
// rtk_ctx: rtk_ctx.h); the frame entry points that enqueue the kernels are
// rtk_frame_host.cpp's.  There is no host rendering path: without a gfx950 device
// every compute entry point fails with RTK_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <string>
#include <vector>

#include "rtk.h"
#include "rtk_ctx.h"
#include "rtk_device_layout.h"
#include "rtk_internal.h"
#include "rtk_lds_plan.h"

namespace rtk {

thread_local std::string g_error;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_error = buf;
    return code;
}

}  // namespace rtk

namespace {

using rtk::fail;
using rtk::g_error;

using namespace rtk;

// ---------------------------------------------------------------------------
// Scene graph -> traversal program
// ---------------------------------------------------------------------------
struct ChainStep {
    bool rotate;
    int32_t index;  // into translates[] / rotates[]
    bool operator<(const ChainStep& o) const { return rotate != o.rotate ? rotate < o.rotate : index < o.index; }
};
using Chain = std::vector<ChainStep>;

struct Program {
    bool has_media_bracket = false;  // a constant_medium whose boundary is not one stationary sphere: OP_MED_BEGIN / MID / END records
    std::vector<Op> ops;
    std::vector<uint32_t> ranks;  // parallel to ops: rtk_node.c of a primitive op (1 + reference visiting rank; 0 = none)
    std::vector<uint32_t> extra;  // parallel to ops: OP_MED_SPHERE -> index of the boundary sphere
    std::vector<Chain> chains;
    std::map<Chain, uint32_t> chain_ids;
    size_t last_label = size_t(-1);  // op index some skip link points at
    uint32_t features = 0;
    int n_primitive_ops = 0;
    std::string error;
    int error_code = RTK_OK;
};

constexpr size_t kMaxOps = size_t(1) << 26;
constexpr int kMaxGraphDepth = 4096;

struct Compiler {
    const rtk_scene_desc& sc;
    Program& prog;

    bool bad(int code, const std::string& why) {
        if (prog.error_code == RTK_OK) {
            prog.error_code = code;
            prog.error = why;
        }
        return false;
    }
    uint32_t chain_id(const Chain& c) {
        auto it = prog.chain_ids.find(c);
        if (it != prog.chain_ids.end()) return it->second;
        uint32_t id = uint32_t(prog.chains.size());
        if (id > 255u) bad(RTK_ERR_UNSUPPORTED, "more than 255 distinct instance-transform chains");  // 8 bits of a record's aux word
        prog.chains.push_back(c);
        prog.chain_ids[c] = id;
        return id;
    }
    uint32_t push(uint32_t kind, uint32_t payload, uint32_t aux, uint32_t rank = 0) {
        prog.ops.push_back(Op{make_op(kind, payload), aux});
        prog.ranks.push_back(rank);
        prog.extra.push_back(0);
        return uint32_t(prog.ops.size()) - 1;
    }
    void label_here() { prog.last_label = prog.ops.size(); }
    // Consecutive chain switches collapse into one op unless a skip link lands
    // between them.
    void push_chain(uint32_t chain, uint32_t entries) {
        if (!prog.ops.empty() && (prog.ops.back().kind_payload & 15u) == OP_CHAIN && prog.last_label != prog.ops.size()) {
            Op& last = prog.ops.back();
            last.aux += entries;
            last.kind_payload = make_op(OP_CHAIN, chain);
            return;
        }
        push(OP_CHAIN, chain, entries);
    }

    bool emit(int32_t node, const Chain& chain, bool in_medium, int depth) {
        if (prog.error_code != RTK_OK) return false;
        if (node < 0 || node >= sc.n_nodes) return bad(RTK_ERR_INVALID, "node index out of range");
        if (depth > kMaxGraphDepth) return bad(RTK_ERR_INVALID, "scene graph too deep (cycle?)");
        if (prog.ops.size() > kMaxOps) return bad(RTK_ERR_UNSUPPORTED, "traversal program too large");
        const rtk_node& n = sc.nodes[node];
        const uint32_t cid = chain_id(chain);
        switch (n.kind) {
            case RTK_NODE_SPHERE:
                if (n.a < 0 || n.a >= sc.n_spheres) return bad(RTK_ERR_INVALID, "sphere index out of range");
                push(OP_SPHERE, uint32_t(n.a), cid, n.c > 0 ? uint32_t(n.c) : 0u);
                prog.n_primitive_ops++;
                return true;
            case RTK_NODE_QUAD:
                if (n.a < 0 || n.a >= sc.n_quads) return bad(RTK_ERR_INVALID, "quad index out of range");
                push(OP_QUAD, uint32_t(n.a), cid, n.c > 0 ? uint32_t(n.c) : 0u);
                prog.features |= F_QUAD;
                prog.n_primitive_ops++;
                return true;
            case RTK_NODE_TRIANGLE:
                if (n.a < 0 || n.a >= sc.n_triangles) return bad(RTK_ERR_INVALID, "triangle index out of range");
                push(OP_TRI, uint32_t(n.a), cid, n.c > 0 ? uint32_t(n.c) : 0u);
                prog.features |= F_TRI;
                prog.n_primitive_ops++;
                return true;
            case RTK_NODE_LIST:
                if (n.a < 0 || n.b < 0 || int64_t(n.a) + n.b > sc.n_list_children) return bad(RTK_ERR_INVALID, "list children out of range");
                for (int32_t k = 0; k < n.b; k++)
                    if (!emit(sc.list_children[n.a + k], chain, in_medium, depth + 1)) return false;
                return true;
            case RTK_NODE_BVH: {
                if (n.c < 0 || n.c >= sc.n_bvh_boxes) return bad(RTK_ERR_INVALID, "bvh box index out of range");
                uint32_t at = push(OP_BOX, uint32_t(n.c), 0);
                if (!emit(n.a, chain, in_medium, depth + 1)) return false;
                if (!emit(n.b, chain, in_medium, depth + 1)) return false;
                prog.ops[at].aux = uint32_t(prog.ops.size());
                label_here();
                return true;
            }
            case RTK_NODE_TRANSLATE:
            case RTK_NODE_ROTATE_Y: {
                const bool rot = n.kind == RTK_NODE_ROTATE_Y;
                if (n.a < 0 || n.a >= (rot ? sc.n_rotates : sc.n_translates)) return bad(RTK_ERR_INVALID, "transform index out of range");
                if (int(chain.size()) >= kMaxChain) return bad(RTK_ERR_UNSUPPORTED, "more than 4 nested instance transforms");
                Chain inner = chain;
                inner.push_back(ChainStep{rot, n.a});
                prog.features |= F_XFORM;
                push_chain(chain_id(inner), 1);
                if (!emit(n.b, inner, in_medium, depth + 1)) return false;
                push_chain(cid, 0);
                return true;
            }
            case RTK_NODE_MEDIUM: {
                if (n.a < 0 || n.a >= sc.n_media) return bad(RTK_ERR_INVALID, "medium index out of range");
                if (in_medium) return bad(RTK_ERR_UNSUPPORTED, "constant_medium inside the boundary of another constant_medium");
                prog.features |= F_MEDIA;
                if (n.b >= 0 && n.b < sc.n_nodes && sc.nodes[n.b].kind == RTK_NODE_SPHERE && sc.nodes[n.b].a >= 0 && sc.nodes[n.b].a < sc.n_spheres && !getenv("RTK_NO_MED_SPHERE")) {
                    const rtk_sphere& s = sc.spheres[sc.nodes[n.b].a];
                    if (s.center_dir.x == 0 && s.center_dir.y == 0 && s.center_dir.z == 0) {  // a stationary sphere as the boundary: the fused record
                        const uint32_t at = push(OP_MED_SPHERE, uint32_t(n.a), cid);
                        prog.extra[at] = uint32_t(sc.nodes[n.b].a);
                        prog.n_primitive_ops++;
                        return true;
                    }
                }
                prog.has_media_bracket = true;
                push(OP_MED_BEGIN, uint32_t(n.a), 0);
                if (!emit(n.b, chain, true, depth + 1)) return false;
                uint32_t mid = push(OP_MED_MID, uint32_t(n.a), 0);
                if (!emit(n.b, chain, true, depth + 1)) return false;
                push(OP_MED_END, uint32_t(n.a), cid);
                prog.ops[mid].aux = uint32_t(prog.ops.size());
                label_here();
                prog.n_primitive_ops++;
                return true;
            }
        }
        return bad(RTK_ERR_INVALID, "unknown node kind");
    }
};

bool texture_needs_uv(const rtk_scene_desc& sc, int32_t tex, int depth = 0) {
    if (tex < 0 || tex >= sc.n_textures || depth > 64) return false;
    const rtk_texture& t = sc.textures[tex];
    if (t.kind == RTK_TEX_IMAGE || t.kind == RTK_TEX_CHECKER_TRI) return true;
    if (t.kind == RTK_TEX_CHECKER) return texture_needs_uv(sc, t.even, depth + 1) || texture_needs_uv(sc, t.odd, depth + 1);
    return false;
}

int validate_tables(const rtk_scene_desc& sc) {
    if (sc.abi_version != RTK_ABI_VERSION) return fail(RTK_ERR_INVALID, "scene abi_version %d != %d", sc.abi_version, RTK_ABI_VERSION);
    if (sc.n_nodes <= 0 || !sc.nodes) return fail(RTK_ERR_INVALID, "scene has no nodes (the reference recurses forever on an empty world, bvh.h:38-43)");
    if (sc.n_materials >= (1 << 24)) return fail(RTK_ERR_UNSUPPORTED, "more than 2^24 materials");
    for (int32_t i = 0; i < sc.n_textures; i++) {
        const rtk_texture& t = sc.textures[i];
        switch (t.kind) {
            case RTK_TEX_SOLID: break;
            case RTK_TEX_CHECKER:
            case RTK_TEX_CHECKER_TRI:
                // children are emitted before their parent by every flattener, which also rules out cycles
                if (t.even < 0 || t.even >= i || t.odd < 0 || t.odd >= i) return fail(RTK_ERR_INVALID, "texture %d: child index must precede it", i);
                break;
            case RTK_TEX_IMAGE: {
                if (t.image < 0 || t.image >= sc.n_images) return fail(RTK_ERR_INVALID, "texture %d: image index out of range", i);
                const rtk_image& im = sc.images[t.image];
                if (im.width > 0 && im.height > 0 &&
                    (im.texel_offset < 0 || im.texel_offset + int64_t(im.width) * im.height * 3 > sc.n_texel_bytes))
                    return fail(RTK_ERR_INVALID, "image %d: texels out of range", t.image);
                break;
            }
            case RTK_TEX_NOISE:
                if (t.image < 0 || t.image >= sc.n_perlins) return fail(RTK_ERR_INVALID, "texture %d: perlin index out of range", i);
                break;
            default: return fail(RTK_ERR_INVALID, "texture %d: unknown kind %d", i, t.kind);
        }
    }
    for (int32_t i = 0; i < sc.n_materials; i++) {
        const rtk_material& m = sc.materials[i];
        const bool textured = m.kind == RTK_MAT_LAMBERTIAN || m.kind == RTK_MAT_DIFFUSE_LIGHT || m.kind == RTK_MAT_ISOTROPIC;
        if (m.kind < RTK_MAT_LAMBERTIAN || m.kind > RTK_MAT_SPECULAR) return fail(RTK_ERR_INVALID, "material %d: unknown kind %d", i, m.kind);
        if (textured && (m.texture < 0 || m.texture >= sc.n_textures)) return fail(RTK_ERR_INVALID, "material %d: texture index out of range", i);
    }
    auto mat_ok = [&](int32_t m) { return m >= 0 && m < sc.n_materials; };
    for (int32_t i = 0; i < sc.n_spheres; i++)
        if (!mat_ok(sc.spheres[i].material)) return fail(RTK_ERR_INVALID, "sphere %d: material out of range", i);
    for (int32_t i = 0; i < sc.n_quads; i++)
        if (!mat_ok(sc.quads[i].material)) return fail(RTK_ERR_INVALID, "quad %d: material out of range", i);
    for (int32_t i = 0; i < sc.n_triangles; i++)
        if (!mat_ok(sc.triangles[i].material)) return fail(RTK_ERR_INVALID, "triangle %d: material out of range", i);
    for (int32_t i = 0; i < sc.n_media; i++)
        if (!mat_ok(sc.media[i].material)) return fail(RTK_ERR_INVALID, "medium %d: material out of range", i);
    return RTK_OK;
}

template <typename real>
void store3(real* dst, const rtk_vec3& v) {
    dst[0] = real(v.x);
    dst[1] = real(v.y);
    dst[2] = real(v.z);
}

// Outward rounding of a box bound to float.
inline float round_down(double x) {
    float f = float(x);
    return double(f) > x ? std::nextafterf(f, -INFINITY) : f;
}
inline float round_up(double x) {
    float f = float(x);
    return double(f) < x ? std::nextafterf(f, INFINITY) : f;
}

// How far an f32 culling box is grown beyond its outward-rounded bounds.  The ray carries the error of its own origin
// term (a bracket of o/d, rtk_trace.hip begin_culling32), so a box answers only for the product b * rcp(d)
// -- float(d) 2^-24, v_rcp_f32 one ulp, the fused multiply-add's final rounding 2^-24 of it: < 2^-22 relative -- i.e. a
// plane displaced by < 2^-22 |b|; grown by 2^-21 of the box's largest coordinate (twice that).
static double box_margin(const rtk_aabb& b) {
    double big = 0.0;
    for (double v : {b.xmin, b.xmax, b.ymin, b.ymax, b.zmin, b.zmax}) big = std::max(big, std::fabs(v));
    return std::ldexp(big, -21) + 1e-300;
}

// The MIXED program of rtk_device_layout.h for a sphere-only scene whose boxes carry rtk_scene_optimize's margin:
// f32 culling boxes (rounded outward, then grown by 2^-19 of the largest coordinate in play), f64 spheres.
// Error budget of the f32 slab test t = fma(b, inv32, -(o32 * inv32)) with inv32 = rcp(float(d)) (1 ulp), o32 =
// float(o): |b*inv| 2^-22.4 + |o*inv| 2^-22 + |t| 2^-24, i.e. a plane displaced by less than 2^-21 (|b| + |o|)
// <= 2^-20 x extent -- half the margin.  The kernel sends rays whose origin leaves [-extent, extent]^3 through the
// exact test instead (they cannot come from a surface of the scene).
static void build_mixed_program(const rtk_scene_desc& sc, const Program& prog, double eye_extent, std::vector<MixedHead>& units, std::vector<uint32_t>& rank_of_unit,
                                float& extent_out) {
    auto kind_of = [&](const Op& op) -> uint32_t {
        uint32_t kind = op.kind_payload & 15u;
        if (kind == OP_SPHERE) {
            const rtk_sphere& s = sc.spheres[op.kind_payload >> 4];
            if (s.center_dir.x != 0 || s.center_dir.y != 0 || s.center_dir.z != 0) kind = OP_SPHERE_MOVING;
        }
        return kind;
    };
    std::vector<uint32_t> unit_of_op(prog.ops.size() + 1, 0);
    double extent = eye_extent;
    for (size_t i = 0; i < prog.ops.size(); i++) {
        const Op& op = prog.ops[i];
        unit_of_op[i + 1] = unit_of_op[i] + uint32_t(mixed_units(kind_of(op)));
        if ((op.kind_payload & 15u) == OP_BOX) {
            const rtk_aabb& b = sc.bvh_boxes[op.kind_payload >> 4];
            for (double v : {b.xmin, b.xmax, b.ymin, b.ymax, b.zmin, b.zmax}) extent = std::max(extent, std::fabs(v));
        } else if ((op.kind_payload & 15u) == OP_SPHERE) {
            const rtk_sphere& s = sc.spheres[op.kind_payload >> 4];
            for (double c : {s.center0.x, s.center0.y, s.center0.z, s.center0.x + s.center_dir.x, s.center0.y + s.center_dir.y, s.center0.z + s.center_dir.z})
                extent = std::max(extent, std::fabs(c) + s.radius);
        }
    }
    extent = double(round_up(extent * 1.0000001));
    units.assign(unit_of_op.back(), MixedHead{});
    std::memset(units.data(), 0, units.size() * sizeof(MixedHead));
    rank_of_unit.assign(unit_of_op.back(), 0u);
    for (size_t i = 0; i < prog.ops.size(); i++) {
        const Op& op = prog.ops[i];
        const uint32_t kind = kind_of(op), payload = op.kind_payload >> 4;
        MixedHead* rec = &units[unit_of_op[i]];
        rec->kind_payload = make_op(kind, payload);
        rec->aux = op.aux;
        rank_of_unit[unit_of_op[i]] = prog.ranks[i];
        if (kind == OP_BOX) {
            const rtk_aabb& b = sc.bvh_boxes[payload];
            // Centre / half-extent form.  The kernel computes, per axis, tc = fma(c, inv, -oi), near = fma(-h, |inv|, tc),
            // far = fma(h, |inv|, tc) with inv = v_rcp_f32(float(d)) (relative error <= 2^-24 + 2^-23) and oi = float(o) * inv
            // (<= 2^-24 + that + 2^-24).  Against the exact planes (c -/+ h - o) / d of the stored box the computed ones are off
            // by at most [(1.5 + 1) 2^-23 (|c| + h) + (2.5 + 1) 2^-23 |o|] / |d| -- the products' errors plus one final rounding
            // each of tc and of near / far, both bounded by (|c| + |o| + h) / |d| -- i.e. a plane displaced by less than
            // 2^-21 (|c| + h) + 2^-20 |o|.  |o| <= extent on every axis (a ray that starts outside never enters the float loop,
            // rtk_trace.hip begin_culling32), so the half-extent is grown by 2^-21 (|c| + h) + 2^-20 extent, plus the distance
            // the centre moved when it was rounded to float, and rounded up.
            const double lo[3] = {b.xmin, b.ymin, b.zmin}, hi[3] = {b.xmax, b.ymax, b.zmax};
            for (int ax = 0; ax < 3; ax++) {
                const double c = 0.5 * (lo[ax] + hi[ax]);
                const float cf = float(c);
                const double h = std::max(hi[ax] - double(cf), double(cf) - lo[ax]);  // covers [lo, hi] from the float centre
                const double grown = h + std::ldexp(std::fabs(double(cf)) + h, -21) + std::ldexp(extent, -20) + 1e-300;
                rec->set_f(ax, cf);
                rec->set_f(3 + ax, round_up(grown * (1.0 + 1e-7)));
            }
            rec->aux = unit_of_op[op.aux] * uint32_t(sizeof(MixedHead));  // the kernel's pcs count bytes
        } else if (kind == OP_SPHERE || kind == OP_SPHERE_MOVING) {
            const rtk_sphere& s = sc.spheres[payload];
            rec->set_d(0, s.center0.x); rec->set_d(1, s.center0.y); rec->set_d(2, s.center0.z);
            double* cont = reinterpret_cast<double*>(rec + 1);
            cont[0] = s.radius;
            cont[1] = 1.0 / s.radius;
            // radius * radius of sphere::hit (sphere.h:37): the same IEEE product the kernel formed in every sphere step, once
            if (kind == OP_SPHERE_MOVING) {
                cont[2] = s.center_dir.x;
                cont[3] = s.center_dir.y;
                cont[4] = s.center_dir.z;  // first double of the third unit
                cont[5] = s.radius * s.radius;
            } else {
                cont[2] = s.radius * s.radius;
            }
            rec->aux = (op.aux & 255u) | (uint32_t(s.material) << 8);
        }
    }
    extent_out = float(extent);
}

// The image of a MIXED program that the kernel which stages it copies into LDS (rtk_device_layout.h MixedImg): the same
// units and values with every head's words permuted, so that the first 16 bytes of any record tell its kind.
static void build_mixed_lds_image(const std::vector<MixedHead>& units, std::vector<MixedImg>& image) {
    image.assign(units.size(), MixedImg{});
    std::memcpy(image.data(), units.data(), units.size() * sizeof(MixedHead));  // continuation units stay as they are
    for (size_t u = 0; u < units.size();) {
        const MixedHead& src = units[u];
        MixedImg& dst = image[u];
        const uint32_t kind = src.kind_payload & 15u;
        if (kind == OP_BOX) {
            for (int k = 0; k < 3; k++) dst.w[k] = src.w[k], dst.w[4 + k] = src.w[3 + k];
            dst.w[3] = src.aux;  // the link: a multiple of 32, low nibble 0 = OP_BOX ^ kImageKindXor
            dst.w[7] = src.kind_payload;
        } else {
            dst.w[0] = src.w[0], dst.w[1] = src.w[1];
            dst.w[2] = src.aux;
            dst.w[3] = src.kind_payload ^ kImageKindXor;
            for (int k = 0; k < 4; k++) dst.w[4 + k] = src.w[2 + k];
        }
        u += size_t(mixed_units(kind));
    }
}

// Largest coordinate magnitude the f32 culling boxes of a scene have to cope with: every box bound and primitive
// extent (each in its own space), every instance offset, the eye.
static double scene_extent(const rtk_scene_desc& sc, double eye_extent) {
    double e = eye_extent;
    auto take = [&](double v) { e = std::max(e, std::fabs(v)); };
    for (int32_t i = 0; i < sc.n_bvh_boxes; i++) {
        const rtk_aabb& b = sc.bvh_boxes[i];
        for (double v : {b.xmin, b.xmax, b.ymin, b.ymax, b.zmin, b.zmax}) take(v);
    }
    for (int32_t i = 0; i < sc.n_spheres; i++) {
        const rtk_sphere& s = sc.spheres[i];
        for (double c : {s.center0.x, s.center0.y, s.center0.z, s.center0.x + s.center_dir.x, s.center0.y + s.center_dir.y, s.center0.z + s.center_dir.z})
            e = std::max(e, std::fabs(c) + std::fabs(s.radius));
    }
    for (int32_t i = 0; i < sc.n_quads; i++) {
        const rtk_quad& q = sc.quads[i];
        for (int k = 0; k < 4; k++) {
            const double a = (k & 1) ? 1.0 : 0.0, b = (k & 2) ? 1.0 : 0.0;
            take(q.Q.x + a * q.u.x + b * q.v.x); take(q.Q.y + a * q.u.y + b * q.v.y); take(q.Q.z + a * q.u.z + b * q.v.z);
        }
    }
    for (int32_t i = 0; i < sc.n_triangles; i++) {
        const rtk_triangle& t = sc.triangles[i];
        for (const rtk_vec3* p : {&t.p0, &t.p1, &t.p2}) { take(p->x); take(p->y); take(p->z); }
    }
    double offsets = 0;  // a ray's origin in an instance's space is at most this far beyond its world-space position
    for (int32_t i = 0; i < sc.n_translates; i++)
        offsets = std::max(offsets, std::max(std::fabs(sc.translates[i].offset.x), std::max(std::fabs(sc.translates[i].offset.y), std::fabs(sc.translates[i].offset.z))));
    return (e + offsets * double(kMaxChain)) * (sc.n_rotates > 0 ? 1.5 : 1.0);  // a rotation about y mixes x and z: sqrt(2) < 1.5
}

// The COMPACT program of rtk_device_layout.h for any scene whose boxes carry rtk_scene_optimize's margin: f32 culling
// boxes exactly as in build_mixed_program (rounded outward, grown by 2^-19 of the extent; same error budget -- under an
// instance transform the kernel applies it to the object-space ray and sends a ray whose object-space origin leaves
// [-extent, extent]^3 through the exact test), every primitive in f64, 16-byte units.
// One record of the COMPACT layout for op i (kind = its kind with moving spheres told apart) at `dst`; links (a box's or
// a MED_MID's `aux`) are translated through `unit_of_link`.
// COMPACT programs of the mesh family hold centre / half-extent box records (the rule of rtk_trace.hip kCompactChStatic)
static bool compact_ch_family(const Program& prog) {
    const uint32_t scene = prog.features & ~uint32_t(F_FMA_BOX | F_MATTE);
    return scene != kFeatLean && (scene & ~kFeatQuadBox) != 0 && (scene & ~kFeatMesh) == 0;
}

static void write_compact_record(const rtk_scene_desc& sc, const Program& prog, size_t i, uint32_t kind, Unit16* dst,
                                 const std::vector<uint32_t>& unit_of_link, bool ch_boxes = false) {
    const Op& op = prog.ops[i];
    const uint32_t payload = op.kind_payload >> 4;
    MixedHead* head = reinterpret_cast<MixedHead*>(dst);
    double* more = reinterpret_cast<double*>(dst) + 4;  // payload element 3 onwards (byte 32)
    head->kind_payload = make_op(kind, payload);
    head->aux = op.aux;
    auto with_material = [&](int32_t material) { head->aux = (op.aux & 255u) | (uint32_t(material) << 8); };
    switch (kind) {
        case OP_BOX: {
            const rtk_aabb& b = sc.bvh_boxes[payload];
            if (ch_boxes) {
            // centre / half-extent form, as in build_mixed_program, except that the origin's share of the error ((2.5 + 1) 2^-23
            // |o / d|) is not the box's to carry: the ray does (slab_test32_che's slack, 2^-20 max |o / d|), so that a box grows
            // by 2^-21 of its OWN coordinates whatever the scene's extent (the Cornell quads' boxes are 1e-4 thick, at 555)
            const double lo[3] = {b.xmin, b.ymin, b.zmin}, hi[3] = {b.xmax, b.ymax, b.zmax};
            for (int ax = 0; ax < 3; ax++) {
                const double c = 0.5 * (lo[ax] + hi[ax]);
                const float cf = float(c);
                const double h = std::max(hi[ax] - double(cf), double(cf) - lo[ax]);
                const double grown = h + std::ldexp(std::fabs(double(cf)) + h, -21) + 1e-300;
                head->set_f(ax, cf);
                head->set_f(3 + ax, round_up(grown * (1.0 + 1e-7)));
            }
            } else {
            const double m = box_margin(b);
            head->set_f(0, round_down(b.xmin - m)); head->set_f(1, round_up(b.xmax + m));
            head->set_f(2, round_down(b.ymin - m)); head->set_f(3, round_up(b.ymax + m));
            head->set_f(4, round_down(b.zmin - m)); head->set_f(5, round_up(b.zmax + m));
            }
            head->aux = unit_of_link[op.aux];
            break;
        }
        case OP_SPHERE:
        case OP_SPHERE_MOVING: {
            const rtk_sphere& s = sc.spheres[payload];
            head->set_d(0, s.center0.x); head->set_d(1, s.center0.y); head->set_d(2, s.center0.z);
            more[0] = s.radius;
            more[1] = 1.0 / s.radius;  // the factor of `(p - center) / radius` (vec3.h:91-93), once instead of per hit
            if (kind == OP_SPHERE_MOVING) { more[2] = s.center_dir.x; more[3] = s.center_dir.y; more[4] = s.center_dir.z; }
            with_material(s.material);
            break;
        }
        case OP_QUAD: {
            const rtk_quad& q = sc.quads[payload];
            const double vals[16] = {q.normal.x, q.normal.y, q.normal.z, q.D, q.Q.x, q.Q.y, q.Q.z, q.w.x, q.w.y, q.w.z,
                                     q.v.x, q.v.y, q.v.z, q.u.x, q.u.y, q.u.z};
            for (int e = 0; e < 3; e++) head->set_d(e, vals[e]);
            for (int e = 3; e < 16; e++) more[e - 3] = vals[e];
            with_material(q.material);
            break;
        }
        case OP_TRI: {
            const rtk_triangle& t = sc.triangles[payload];
            // v0v1 = p1 - p0, v0v2 = p2 - p0 (triangle.h:67-68) in double
            const double vals[9] = {t.p2.x - t.p0.x, t.p2.y - t.p0.y, t.p2.z - t.p0.z, t.p1.x - t.p0.x, t.p1.y - t.p0.y, t.p1.z - t.p0.z,
                                    t.p0.x, t.p0.y, t.p0.z};
            for (int e = 0; e < 3; e++) head->set_d(e, vals[e]);
            for (int e = 3; e < 9; e++) more[e - 3] = vals[e];
            with_material(t.material);
            break;
        }
        case OP_MED_MID: head->aux = unit_of_link[op.aux]; break;
        case OP_MED_END:
            head->set_d(0, sc.media[payload].neg_inv_density);
            with_material(sc.media[payload].material);
            break;
        case OP_MED_SPHERE: {
            const rtk_sphere& s = sc.spheres[prog.extra[i]];
            head->set_d(0, s.center0.x); head->set_d(1, s.center0.y); head->set_d(2, s.center0.z);
            more[0] = s.radius;
            more[1] = sc.media[payload].neg_inv_density;
            with_material(sc.media[payload].material);
            break;
        }
        default: break;
    }
}

static uint32_t compact_kind_of(const rtk_scene_desc& sc, const Op& op) {
    uint32_t kind = op.kind_payload & 15u;
    if (kind == OP_SPHERE) {
        const rtk_sphere& s = sc.spheres[op.kind_payload >> 4];
        if (s.center_dir.x != 0 || s.center_dir.y != 0 || s.center_dir.z != 0) kind = OP_SPHERE_MOVING;
    }
    return kind;
}

static void build_compact_program(const rtk_scene_desc& sc, const Program& prog, double eye_extent, std::vector<Unit16>& units, std::vector<uint32_t>& rank_of_unit,
                                  float& extent_out) {
    std::vector<uint32_t> unit_of_op(prog.ops.size() + 1, 0);
    for (size_t i = 0; i < prog.ops.size(); i++) unit_of_op[i + 1] = unit_of_op[i] + uint32_t(compact_units(compact_kind_of(sc, prog.ops[i])));
    const double extent = double(round_up(scene_extent(sc, eye_extent) * 1.0000001));
    units.assign(unit_of_op.back(), Unit16{{0u, 0u, 0u, 0u}});
    rank_of_unit.assign(unit_of_op.back(), 0u);
    for (size_t i = 0; i < prog.ops.size(); i++) {
        write_compact_record(sc, prog, i, compact_kind_of(sc, prog.ops[i]), &units[unit_of_op[i]], unit_of_op, compact_ch_family(prog));
        rank_of_unit[unit_of_op[i]] = prog.ranks[i];
    }
    extent_out = float(extent);
}

// The same program in two parts, for COMPACT programs that do not fit one CU's LDS (rtk_device_layout.h, SceneView::
// program_hot): quads and triangles -- the bulky records, tested a few times per sample -- go to `cold` in program order;
// `hot` is the program without them, each run of consecutive quads (or triangles) replaced by ONE two-unit record {kind,
// count; aux = first unit of the run in `cold`}.  A run ends where the kind changes, at 255 primitives, and in front of any
// record some box or medium links to (so that every link target is the start of a record of the hot program).
// rank_of_id[unit of a hot record, or hot.size() + unit of a cold one] = the primitive's reference rank.
static void build_hot_cold_program(const rtk_scene_desc& sc, const Program& prog, std::vector<Unit16>& hot, std::vector<Unit16>& cold,
                                   std::vector<uint32_t>& rank_of_id) {
    const size_t n = prog.ops.size();
    std::vector<uint32_t> kind(n);
    std::vector<char> is_target(n + 1, 0);
    for (size_t i = 0; i < n; i++) {
        kind[i] = compact_kind_of(sc, prog.ops[i]);
        if (kind[i] == OP_BOX || kind[i] == OP_MED_MID) is_target[prog.ops[i].aux] = 1;
    }
    auto is_cold = [&](size_t i) { return kind[i] == OP_QUAD || kind[i] == OP_TRI; };
    std::vector<uint32_t> hot_unit(n + 1, 0), cold_unit(n, 0), run_len(n, 0);
    uint32_t n_hot = 0, n_cold = 0;
    for (size_t i = 0; i < n;) {
        if (!is_cold(i)) {
            hot_unit[i] = n_hot;
            n_hot += uint32_t(compact_units(kind[i]));
            i++;
            continue;
        }
        size_t j = i;
        while (j < n && is_cold(j) && kind[j] == kind[i] && (j == i || !is_target[j]) && j - i < 255) {
            hot_unit[j] = n_hot;  // (only the run's first primitive can be a link target)
            cold_unit[j] = n_cold;
            n_cold += uint32_t(compact_units(kind[j]));
            j++;
        }
        run_len[i] = uint32_t(j - i);
        n_hot += 2;
        i = j;
    }
    hot_unit[n] = n_hot;
    hot.assign(n_hot, Unit16{{0u, 0u, 0u, 0u}});
    cold.assign(std::max<uint32_t>(n_cold, 1u), Unit16{{0u, 0u, 0u, 0u}});
    rank_of_id.assign(size_t(n_hot) + cold.size(), 0u);
    for (size_t i = 0; i < n; i++) {
        if (!is_cold(i)) {
            write_compact_record(sc, prog, i, kind[i], &hot[hot_unit[i]], hot_unit);
            rank_of_id[hot_unit[i]] = prog.ranks[i];
            continue;
        }
        if (run_len[i] > 0) {
            MixedHead* run = reinterpret_cast<MixedHead*>(&hot[hot_unit[i]]);
            run->kind_payload = make_op(kind[i], run_len[i]);
            run->aux = cold_unit[i];
        }
        write_compact_record(sc, prog, i, kind[i], &cold[cold_unit[i]], hot_unit);
        rank_of_id[size_t(n_hot) + cold_unit[i]] = prog.ranks[i];
    }
}

template <typename real>
int build_device_scene(const rtk_scene_desc& sc, const Program& prog, DeviceScene<real>& out, bool fast_order = false, bool want_mixed = false, double eye_extent = 0.0) {
    out.release();
    // ---- the fused traversal program: one or more slots per op, skip links
    // translated from op indices to slot indices
    std::vector<uint32_t> slot_of_op(prog.ops.size() + 1, 0);
    auto slot_kind = [&](const Op& op) -> uint32_t {
        uint32_t kind = op.kind_payload & 15u;
        if (kind == OP_SPHERE) {
            const rtk_sphere& s = sc.spheres[op.kind_payload >> 4];
            if (s.center_dir.x != 0 || s.center_dir.y != 0 || s.center_dir.z != 0) kind = OP_SPHERE_MOVING;
        }
        return kind;
    };
    for (size_t i = 0; i < prog.ops.size(); i++) slot_of_op[i + 1] = slot_of_op[i] + uint32_t(slots_of<real>(slot_kind(prog.ops[i])));
    std::vector<Slot<real>> slots(slot_of_op.back());
    std::memset(slots.data(), 0, slots.size() * sizeof(Slot<real>));
    auto pack = [&](Slot<real>* rec, const double* vals, int n) {
        for (int e = 0; e < n; e++) rec[e / Slot<real>::kReals].v[e % Slot<real>::kReals] = real(vals[e]);
    };
    // Float boxes: the slab test computes (b - o) * inv in float, which places a plane only to ~2^-24 (|b| + |o|).  A box
    // thinner than that on an axis -- the 1e-4 padding of an axis-aligned quad at z = 555 seen from z = -800 -- collapses to
    // near == far and culls every ray (the fast order tests such a box before the Cornell box's back wall: f32 lost 20 % of
    // its light there).  So every axis of a float box is at least 2^-20 x the scene's largest box coordinate thick, with its
    // bounds rounded outward; culling stays conservative and the primitive tests decide every hit, as in f64.
    double min_thick = 0.0;
    if constexpr (sizeof(real) == 4) {
        double coord = 1.0;
        for (int32_t k = 0; k < sc.n_bvh_boxes; k++) {
            const rtk_aabb& b = sc.bvh_boxes[k];
            for (double v : {b.xmin, b.xmax, b.ymin, b.ymax, b.zmin, b.zmax})
                if (std::isfinite(v)) coord = std::max(coord, std::fabs(v));
        }
        min_thick = std::ldexp(coord, -20);
    }
    auto float_box = [&](double* vals) {
        for (int a = 0; a < 3; a++) {
            double& lo = vals[2 * a];
            double& hi = vals[2 * a + 1];
            if (!(hi - lo >= min_thick)) {  // (also NaN-safe: an empty or degenerate box is padded like a thin one)
                const double mid = 0.5 * (lo + hi), half = 0.5 * min_thick;
                if (std::isfinite(mid)) lo = std::min(lo, mid - half), hi = std::max(hi, mid + half);
            }
            float flo = float(lo), fhi = float(hi);
            if (double(flo) > lo) flo = std::nextafter(flo, -INFINITY);
            if (double(fhi) < hi) fhi = std::nextafter(fhi, INFINITY);
            lo = flo;
            hi = fhi;
        }
    };
    for (size_t i = 0; i < prog.ops.size(); i++) {
        const Op& op = prog.ops[i];
        const uint32_t kind = slot_kind(op), payload = op.kind_payload >> 4;
        Slot<real>* rec = &slots[slot_of_op[i]];
        rec->kind_payload = make_op(kind, payload);
        rec->aux = op.aux;
        auto with_material = [&](int32_t material) { rec->aux = (op.aux & 255u) | (uint32_t(material) << 8); };
        switch (kind) {
            case OP_BOX: {
                const rtk_aabb& b = sc.bvh_boxes[payload];
                double vals[6] = {b.xmin, b.xmax, b.ymin, b.ymax, b.zmin, b.zmax};
                if constexpr (sizeof(real) == 4) float_box(vals);
                pack(rec, vals, 6);
                rec->aux = slot_of_op[op.aux];
                break;
            }
            case OP_SPHERE:
            case OP_SPHERE_MOVING: {
                const rtk_sphere& s = sc.spheres[payload];
                const double vals[4] = {s.center0.x, s.center0.y, s.center0.z, s.radius};
                pack(rec, vals, 4);
                rec->v[4] = real(1) / real(s.radius);  // the factor of `(p - center) / radius` (vec3.h:91-93), once instead of per hit
                with_material(s.material);
                if (kind == OP_SPHERE_MOVING) {
                    const double dir[3] = {s.center_dir.x, s.center_dir.y, s.center_dir.z};
                    pack(rec + 1, dir, 3);
                }
                break;
            }
            case OP_QUAD: {
                const rtk_quad& q = sc.quads[payload];
                const double vals[16] = {q.normal.x, q.normal.y, q.normal.z, q.D, q.Q.x, q.Q.y, q.Q.z, q.w.x, q.w.y, q.w.z,
                                         q.v.x, q.v.y, q.v.z, q.u.x, q.u.y, q.u.z};
                pack(rec, vals, 16);
                with_material(q.material);
                break;
            }
            case OP_TRI: {
                const rtk_triangle& t = sc.triangles[payload];
                // v0v1 = p1 - p0, v0v2 = p2 - p0 (triangle.h:67-68) in double, then to `real`
                const double vals[9] = {t.p2.x - t.p0.x, t.p2.y - t.p0.y, t.p2.z - t.p0.z, t.p1.x - t.p0.x, t.p1.y - t.p0.y, t.p1.z - t.p0.z,
                                        t.p0.x, t.p0.y, t.p0.z};
                pack(rec, vals, 9);
                with_material(t.material);
                break;
            }
            case OP_MED_MID: rec->aux = slot_of_op[op.aux]; break;
            case OP_MED_END:
                rec->v[0] = real(sc.media[payload].neg_inv_density);
                with_material(sc.media[payload].material);
                break;
            case OP_MED_SPHERE: {
                const rtk_sphere& s = sc.spheres[prog.extra[i]];
                const double vals[5] = {s.center0.x, s.center0.y, s.center0.z, s.radius, sc.media[payload].neg_inv_density};
                pack(rec, vals, 5);
                with_material(sc.media[payload].material);
                break;
            }
            default: break;
        }
    }
    // Sphere, quad and medium records live entirely in their program slots; only triangles keep a side record
    // (normal + UVs for the deferred hit record).
    std::vector<TriRec<real>> tris(sc.n_triangles);
    for (int32_t i = 0; i < sc.n_triangles; i++) {
        const rtk_triangle& t = sc.triangles[i];
        TriRec<real>& r = tris[i];
        // v0v1 = p1 - p0, v0v2 = p2 - p0 (triangle.h:67-68) in double, then to `real`
        store3(r.p0, t.p0);
        store3(r.e1, rtk_vec3{t.p1.x - t.p0.x, t.p1.y - t.p0.y, t.p1.z - t.p0.z});
        store3(r.e2, rtk_vec3{t.p2.x - t.p0.x, t.p2.y - t.p0.y, t.p2.z - t.p0.z});
        store3(r.n, t.normal);
        for (int k = 0; k < 2; k++) { r.uv0[k] = t.uv0[k]; r.uv1[k] = t.uv1[k]; r.uv2[k] = t.uv2[k]; }
        r.material = t.material;
        r._pad = 0;
    }

    std::vector<MaterialRec<real>> mats(sc.n_materials);
    for (int32_t i = 0; i < sc.n_materials; i++) {
        const rtk_material& m = sc.materials[i];
        MaterialRec<real>& r = mats[i];
        store3(r.albedo, m.albedo);
        r.param = real(m.param);
        if (m.kind == RTK_MAT_DIELECTRIC) {
            // a dielectric has no albedo (material.h:47-65): the slots carry its per-face constants instead, computed
            // in the kernel's arithmetic type exactly as scatter() does per call -- 1/ri (material.h:50) and Schlick's r0^2 for ri = 1/index
            // (front face) and ri = index (material.h:71-72)
            const real index = real(m.param), inv = real(1) / index;
            real r0f = (real(1) - inv) / (real(1) + inv), r0b = (real(1) - index) / (real(1) + index);
            r0f = r0f * r0f;
            r0b = r0b * r0b;
            r.albedo[0] = inv;
            r.albedo[1] = r0f;
            r.albedo[2] = r0b;
        }
        r.kind = m.kind;
        r.tex = -1;
        r.needs_uv = 0;
        r._pad = 0;
        const bool textured = m.kind == RTK_MAT_LAMBERTIAN || m.kind == RTK_MAT_DIFFUSE_LIGHT || m.kind == RTK_MAT_ISOTROPIC;
        if (textured) {
            const rtk_texture& t = sc.textures[m.texture];
            if (t.kind == RTK_TEX_SOLID) {
                store3(r.albedo, t.color);  // solid_color::value is the constant (texture.h:26): fold it in
            } else {
                r.tex = m.texture;
                r.needs_uv = texture_needs_uv(sc, m.texture) ? 1 : 0;
            }
        }
    }
    std::vector<TextureRec<real>> texs(sc.n_textures);
    for (int32_t i = 0; i < sc.n_textures; i++) {
        const rtk_texture& t = sc.textures[i];
        TextureRec<real>& r = texs[i];
        store3(r.color, t.color);
        r.param = real(t.param);
        r.kind = t.kind; r.even = t.even; r.odd = t.odd; r.image = t.image;
    }
    std::vector<ImageRec> images(sc.n_images);
    for (int32_t i = 0; i < sc.n_images; i++) images[i] = ImageRec{sc.images[i].width, sc.images[i].height, sc.images[i].texel_offset};
    std::vector<uint8_t> texels(sc.texels, sc.texels + sc.n_texel_bytes);
    std::vector<PerlinRec<real>> perlins(sc.n_perlins);
    for (int32_t i = 0; i < sc.n_perlins; i++) {
        for (int k = 0; k < 256; k++) {
            for (int c = 0; c < 3; c++) perlins[i].randvec[k][c] = real(sc.perlins[i].randvec[k][c]);
            perlins[i].perm_x[k] = sc.perlins[i].perm_x[k];
            perlins[i].perm_y[k] = sc.perlins[i].perm_y[k];
            perlins[i].perm_z[k] = sc.perlins[i].perm_z[k];
        }
    }
    std::vector<ChainRec<real>> chains(prog.chains.size());
    for (size_t i = 0; i < prog.chains.size(); i++) {
        ChainRec<real>& r = chains[i];
        std::memset(&r, 0, sizeof r);
        r.count = int32_t(prog.chains[i].size());
        for (int k = 0; k < r.count; k++) {
            const ChainStep& st = prog.chains[i][k];
            r.is_rotate[k] = st.rotate ? 1 : 0;
            if (st.rotate) {
                r.a[k] = real(sc.rotates[st.index].sin_theta);
                r.b[k] = real(sc.rotates[st.index].cos_theta);
            } else {
                r.a[k] = real(sc.translates[st.index].offset.x);
                r.b[k] = real(sc.translates[st.index].offset.y);
                r.c[k] = real(sc.translates[st.index].offset.z);
            }
        }
    }
    std::vector<LightRec<real>> lights(sc.n_lights);
    for (int32_t i = 0; i < sc.n_lights; i++) {
        store3(lights[i].position, sc.lights[i].position);
        store3(lights[i].intensity, sc.lights[i].intensity);
        lights[i].size = real(sc.lights[i].size);
    }
    int rc;
    if ((rc = out.upload(slots, &out.view.program)) != RTK_OK) return rc;
    if ((rc = out.upload(tris, &out.view.tris)) != RTK_OK) return rc;
    if ((rc = out.upload(mats, &out.view.materials)) != RTK_OK) return rc;
    if ((rc = out.upload(texs, &out.view.textures)) != RTK_OK) return rc;
    if ((rc = out.upload(images, &out.view.images)) != RTK_OK) return rc;
    if ((rc = out.upload(texels, &out.view.texels)) != RTK_OK) return rc;
    if ((rc = out.upload(perlins, &out.view.perlins)) != RTK_OK) return rc;
    if ((rc = out.upload(chains, &out.view.chains)) != RTK_OK) return rc;
    if ((rc = out.upload(lights, &out.view.lights)) != RTK_OK) return rc;
    out.view.n_slots = int32_t(slots.size());
    out.view.n_lights = sc.n_lights;
    out.view.n_materials = sc.n_materials;
    out.view.n_perlins = sc.n_perlins;
    out.view.n_chains = int32_t(chains.size());
    out.view.program_mixed = nullptr;
    out.view.program_mixed_lds = nullptr;
    out.view.n_units = 0;
    out.view.extent = 0.0f;
    // Programs that cannot be staged in LDS whole: the box slots alone, with the tables that find them (F_LDS_BOXES).
    out.view.box_cache = nullptr;
    out.view.kind_words = nullptr;
    out.view.box_rank = nullptr;
    out.view.n_cached_boxes = out.view.n_kind_words = out.view.n_rank_words = 0;
    if (lds_plan::wants_box_table(slots.size() * sizeof(Slot<real>), mats.size() * sizeof(MaterialRec<real>))) {
        std::vector<BoxRec<real>> boxes;
        std::vector<uint32_t> kind_words((slots.size() + 7) / 8, 0u);
        std::vector<uint2> rank((slots.size() + 31) / 32, uint2{0u, 0u});
        for (size_t pc = 0; pc < slots.size();) {
            const uint32_t kind = slots[pc].kind_payload & 15u;
            kind_words[pc >> 3] |= kind << ((pc & 7) * 4);
            if (kind == OP_BOX) {
                rank[pc >> 5].x |= 1u << (pc & 31);
                BoxRec<real> b{};
                for (int k = 0; k < 6; k++) b.v[k] = slots[pc].v[k];
                b.aux = slots[pc].aux;
                boxes.push_back(b);
            }
            pc += size_t(slots_of<real>(kind));
        }
        uint32_t before = 0;
        for (auto& r : rank) {
            r.y = before;
            before += uint32_t(__builtin_popcount(r.x));
        }
        const size_t bytes = lds_plan::box_table_bytes(boxes.size(), sizeof(BoxRec<real>), kind_words.size(), rank.size());
        if (getenv("RTK_DEBUG")) fprintf(stderr, "[rtk] %zu-byte reals: %zu slots, %zu box slots, boxes + tables %zu B\n", sizeof(real), slots.size(), boxes.size(), bytes);
        if (!boxes.empty() && lds_plan::box_table_fits(bytes)) {
            if ((rc = out.upload(boxes, &out.view.box_cache)) != RTK_OK) return rc;
            if ((rc = out.upload(kind_words, &out.view.kind_words)) != RTK_OK) return rc;
            if ((rc = out.upload(rank, &out.view.box_rank)) != RTK_OK) return rc;
            out.view.n_cached_boxes = int32_t(boxes.size());
            out.view.n_kind_words = int32_t(kind_words.size());
            out.view.n_rank_words = int32_t(rank.size());
        }
    }
    out.view.program_compact = nullptr;
    out.view.n_units16 = 0;
    out.view.compact_ch = 0;
    out.view.program_hot = nullptr;
    out.view.program_cold = nullptr;
    out.view.n_hot_units = out.view.n_cold_units = 0;
    out.view.tie_rank_hot = nullptr;
    out.view.tie_rank = nullptr;
    out.view.tie_rank_slot = nullptr;
    if (fast_order) {  // reference ranks of the primitive records, for exact ties (see SceneView::tie_rank)
        std::vector<uint32_t> rank_of_slot(slots.size(), 0u);
        bool any = false;
        for (size_t i = 0; i < prog.ops.size(); i++) {
            rank_of_slot[slot_of_op[i]] = prog.ranks[i];
            any = any || prog.ranks[i] != 0;
        }
        if (any && (rc = out.upload(rank_of_slot, &out.view.tie_rank_slot)) != RTK_OK) return rc;
    }
    if constexpr (sizeof(real) == 8) {
        if (fast_order && want_mixed) {
            std::vector<MixedHead> units;
            std::vector<uint32_t> ranks;
            build_mixed_program(sc, prog, eye_extent, units, ranks, out.view.extent);
            if ((rc = out.upload(units, &out.view.program_mixed)) != RTK_OK) return rc;
            std::vector<MixedImg> image;
            build_mixed_lds_image(units, image);
            if ((rc = out.upload(image, &out.view.program_mixed_lds)) != RTK_OK) return rc;
            if ((rc = out.upload(ranks, &out.view.tie_rank)) != RTK_OK) return rc;
            out.view.n_units = int32_t(units.size());
        } else if (fast_order) {
            std::vector<Unit16> units;
            std::vector<uint32_t> ranks;
            build_compact_program(sc, prog, eye_extent, units, ranks, out.view.extent);
            if ((rc = out.upload(units, &out.view.program_compact)) != RTK_OK) return rc;
            if ((rc = out.upload(ranks, &out.view.tie_rank)) != RTK_OK) return rc;
            out.view.n_units16 = int32_t(units.size());
            out.view.compact_ch = compact_ch_family(prog) ? 1 : 0;
            // the same program in its hot/cold form: for programs too large for LDS -- and, through variant bit 23, for tests
            // of that form on scenes small enough for the oracle (only the full-feature kernel family has it)
            if ((prog.features & ~kFeatQuadBox) != 0 && (prog.features & ~kFeatMesh) != 0) {
                std::vector<Unit16> hot, cold;
                std::vector<uint32_t> ranks_by_id;
                build_hot_cold_program(sc, prog, hot, cold, ranks_by_id);
                if (getenv("RTK_DEBUG")) fprintf(stderr, "[rtk] COMPACT program %zu B; hot part %zu B, cold part %zu B\n", units.size() * 16, hot.size() * 16, cold.size() * 16);
                if (lds_plan::hot_fits(hot.size() * sizeof(Unit16), mats.size() * sizeof(MaterialRec<real>)) && hot.size() < (size_t(1) << 24)) {
                    if ((rc = out.upload(hot, &out.view.program_hot)) != RTK_OK) return rc;
                    if ((rc = out.upload(cold, &out.view.program_cold)) != RTK_OK) return rc;
                    if ((rc = out.upload(ranks_by_id, &out.view.tie_rank_hot)) != RTK_OK) return rc;
                    out.view.n_hot_units = int32_t(hot.size());
                    out.view.n_cold_units = int32_t(cold.size());
                }
            }
        }
    }
    return RTK_OK;
}

template <typename real>
CameraRec<real> to_device_camera(const rtk_camera& c) {
    CameraRec<real> r;
    store3(r.background, c.background);
    store3(r.center, c.center);
    store3(r.pixel00, c.pixel00_loc);
    store3(r.du, c.pixel_delta_u);
    store3(r.dv, c.pixel_delta_v);
    store3(r.disk_u, c.defocus_disk_u);
    store3(r.disk_v, c.defocus_disk_v);
    r.defocus_angle = real(c.defocus_angle);
    r.samples_scale = real(c.pixel_samples_scale);
    r.width = c.image_width;
    r.height = c.image_height;
    r.spp = c.samples_per_pixel;
    r.max_depth = c.max_depth;
    return r;
}

}  // namespace

namespace rtk {

constexpr unsigned int kCounterRing = 256;  // (rtk_ctx.h: slots of the rings rtk_init allocates)

int ctx_device(const rtk_ctx* ctx) { return ctx->device; }

}  // namespace rtk

extern "C" {

int rtk_abi_version(void) { return RTK_ABI_VERSION; }

const char* rtk_last_error(void) { return g_error.c_str(); }

int rtk_init(int device, rtk_ctx** out_ctx) {
    if (!out_ctx) return fail(RTK_ERR_INVALID, "rtk_init: out_ctx is null");
    *out_ctx = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(RTK_ERR_NO_DEVICE, "no HIP device available (%s); this library has no CPU path", e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    if (device < 0 || device >= count) return fail(RTK_ERR_INVALID, "rtk_init: device %d out of range (0..%d)", device, count - 1);
    hipDeviceProp_t prop;
    RTK_HIP(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(RTK_ERR_NO_DEVICE, "device %d is %s; the kernels are built for gfx950 (MI355X) only", device, prop.gcnArchName);
    RTK_HIP(hipSetDevice(device));
    auto* ctx = new rtk_ctx;
    ctx->device = device;
    hipError_t me = hipMalloc(reinterpret_cast<void**>(&ctx->tile_counters), kCounterRing * sizeof(unsigned int));
    if (me == hipSuccess) me = hipMalloc(reinterpret_cast<void**>(&ctx->d_cameras), kCounterRing * kCameraStride);
    if (me != hipSuccess) {
        if (ctx->tile_counters) (void)hipFree(ctx->tile_counters);
        delete ctx;
        return fail(RTK_ERR_HIP, "hipMalloc(launch state) failed: %s", hipGetErrorString(me));
    }
    ctx->h_cameras.resize(kCounterRing * kCameraStride);
    *out_ctx = ctx;
    return RTK_OK;
}

int rtk_destroy(rtk_ctx* ctx) {
    if (!ctx) return RTK_OK;
    (void)hipSetDevice(ctx->device);
    ctx->scene64.release();
    ctx->scene32.release();
    if (ctx->tile_counters) (void)hipFree(ctx->tile_counters);
    if (ctx->d_cameras) (void)hipFree(ctx->d_cameras);
    if (ctx->d_partial) (void)hipFree(ctx->d_partial);
    if (ctx->d_denoise) (void)hipFree(ctx->d_denoise);
    if (ctx->d_gather) (void)hipFree(ctx->d_gather);
    if (ctx->d_tile_cost) (void)hipFree(ctx->d_tile_cost);
    if (ctx->d_tile_order) (void)hipFree(ctx->d_tile_order);
    if (ctx->d_tile_list) (void)hipFree(ctx->d_tile_list);
    if (ctx->d_views) (void)hipFree(ctx->d_views);
    for (auto& st : ctx->view_stage) {
        if (st.done) (void)hipEventDestroy(st.done);
        if (st.host) (void)hipHostFree(st.host);
    }
    if (ctx->progress_stream) (void)hipStreamDestroy(ctx->progress_stream);
    if (ctx->progress_word) (void)hipHostFree(ctx->progress_word);
    delete ctx;
    return RTK_OK;
}

int rtk_set_progress_callback(rtk_ctx* ctx, rtk_progress_fn fn, void* user, int interval_ms) {
    if (!ctx) return fail(RTK_ERR_INVALID, "rtk_set_progress_callback: null context");
    ctx->progress_fn = fn;
    ctx->progress_user = user;
    ctx->progress_interval_ms = interval_ms > 0 ? interval_ms : 100;
    return RTK_OK;
}

// How a description's hierarchy was made, which decides the slab tests the kernels may use on it.
enum UploadOrder {
    kOrderReference,  // the caller's own boxes: aabb::hit as written (aabb.h:61-85)
    kOrderFast,       // rtk_scene_optimize output, every box grown by the pass's margin: fused / f32 culling tests
};
static int upload_scene(rtk_ctx* ctx, const rtk_scene_desc* scene, UploadOrder order, double eye_extent = 0.0);

int rtk_scene_upload(rtk_ctx* ctx, const rtk_scene_desc* scene) {
    if (!ctx || !scene) return fail(RTK_ERR_INVALID, "rtk_scene_upload: null argument");
    return upload_scene(ctx, scene, kOrderReference);
}

int rtk_scene_upload_fast(rtk_ctx* ctx, const rtk_scene_desc* scene, const rtk_optimize_opts* opts, rtk_optimize_info* info) {
    if (!ctx || !scene) return fail(RTK_ERR_INVALID, "rtk_scene_upload_fast: null argument");
    rtk_scene_desc* fast = nullptr;
    int rc = rtk_scene_optimize(scene, opts, &fast, info);
    if (rc != RTK_OK) return fail(rc, "rtk_scene_upload_fast: rtk_scene_optimize rejected the scene description");
    // every box of `fast` was grown by rtk_scene_optimize's margin: the kernels may use the fused slab test
    double eye_extent = 0.0;
    if (opts && opts->has_eye) eye_extent = std::max(std::fabs(opts->eye.x), std::max(std::fabs(opts->eye.y), std::fabs(opts->eye.z)));
    rc = upload_scene(ctx, fast, kOrderFast, eye_extent);
    rtk_scene_optimized_free(fast);
    return rc;
}

int rtk_scene_upload_optimized(rtk_ctx* ctx, const rtk_scene_desc* optimized, const rtk_optimize_opts* opts) {
    if (!ctx || !optimized) return fail(RTK_ERR_INVALID, "rtk_scene_upload_optimized: null argument");
    double eye_extent = 0.0;
    if (opts && opts->has_eye) eye_extent = std::max(std::fabs(opts->eye.x), std::max(std::fabs(opts->eye.y), std::fabs(opts->eye.z)));
    return upload_scene(ctx, optimized, kOrderFast, eye_extent);
}

// Everything that can be decided without a device: table validation and the compilation of the traversal program.
static int compile_scene(const rtk_scene_desc* scene, Program& prog) {
    int rc = validate_tables(*scene);
    if (rc != RTK_OK) return rc;
    Compiler comp{*scene, prog};
    comp.chain_id(Chain{});  // chain 0 = world space
    comp.emit(scene->root, Chain{}, false, 0);
    if (prog.error_code != RTK_OK) return fail(prog.error_code, "rtk_scene_upload: %s", prog.error.c_str());
    if (prog.n_primitive_ops == 0) return fail(RTK_ERR_INVALID, "rtk_scene_upload: no primitive reachable from the root");
    // A switch back to world space that is the program's last record serves nobody: what follows is OP_END, the shade step works
    // from the world ray and the hit record's own chain, and begin_segment sets the object ray anew.  It is a scheduler step of
    // its own for every ray that entered the last instance (the Cornell box: a fifth of its chain steps), so it is dropped and
    // the skip links that pointed behind it are moved up.  (RTK_KEEP_LAST_CHAIN=1 keeps it: tools/, A/B.)
    if (prog.ops.size() > 1 && (prog.ops.back().kind_payload & 15u) == OP_CHAIN && (prog.ops.back().kind_payload >> 4) == 0u && prog.ops.back().aux == 0u &&
        !getenv("RTK_KEEP_LAST_CHAIN")) {
        const uint32_t behind = uint32_t(prog.ops.size());
        prog.ops.pop_back();
        prog.ranks.pop_back();
        prog.extra.pop_back();
        for (Op& op : prog.ops) {
            const uint32_t kind = op.kind_payload & 15u;
            if ((kind == OP_BOX || kind == OP_MED_MID) && op.aux == behind) op.aux = behind - 1;
        }
    }
    prog.ops.push_back(Op{make_op(OP_END, 0), 0});
    prog.ranks.push_back(0);
    prog.extra.push_back(0);
    return RTK_OK;
}

int rtk_scene_validate(const rtk_scene_desc* scene, int32_t* n_program_ops) {
    if (!scene) return fail(RTK_ERR_INVALID, "rtk_scene_validate: null argument");
    try {
        Program prog;
        const int rc = compile_scene(scene, prog);
        if (rc == RTK_OK && n_program_ops) *n_program_ops = int32_t(prog.ops.size());
        return rc;
    } catch (const std::bad_alloc&) {
        return fail(RTK_ERR_UNSUPPORTED, "rtk_scene_validate: out of memory while compiling the traversal program");
    }
}


// What a frame depends on besides the camera and the seed: the compiled program (ops, tie ranks, chains), every table of the
// description, the kernel features and the visiting order with its culling margin.
static uint64_t scene_digest(const rtk_scene_desc& sc, const Program& prog, uint32_t features, bool fast_order, double eye_extent) {
    Fnv64 f;
    f.add_pod(features);
    f.add_pod(fast_order);
    f.add_pod(eye_extent);
    f.add(prog.ops.data(), prog.ops.size() * sizeof(Op));
    f.add(prog.ranks.data(), prog.ranks.size() * sizeof(uint32_t));
    f.add(prog.extra.data(), prog.extra.size() * sizeof(uint32_t));
    for (const Chain& ch : prog.chains) {
        f.add_pod(uint64_t(ch.size()));
        for (const ChainStep& st : ch) {
            f.add_pod(st.rotate);
            f.add_pod(st.index);
        }
    }
    f.add_pod(sc.root);
    f.add_table(sc.nodes, sc.n_nodes);
    f.add_table(sc.list_children, sc.n_list_children);
    f.add_table(sc.spheres, sc.n_spheres);
    f.add_table(sc.quads, sc.n_quads);
    f.add_table(sc.triangles, sc.n_triangles);
    f.add_table(sc.bvh_boxes, sc.n_bvh_boxes);
    f.add_table(sc.translates, sc.n_translates);
    f.add_table(sc.rotates, sc.n_rotates);
    f.add_table(sc.media, sc.n_media);
    f.add_table(sc.materials, sc.n_materials);
    f.add_table(sc.textures, sc.n_textures);
    f.add_table(sc.images, sc.n_images);
    f.add_table(sc.texels, sc.n_texel_bytes);
    f.add_table(sc.perlins, sc.n_perlins);
    f.add_table(sc.lights, sc.n_lights);
    return f.h;
}

static int upload_scene(rtk_ctx* ctx, const rtk_scene_desc* scene, UploadOrder order, double eye_extent) {
    Program prog;
    int rc = compile_scene(scene, prog);
    if (rc != RTK_OK) return rc;
    // (Media scenes included: rtk_scene_optimize keeps a medium's POSITION in the reference's order; the boxes around it may
    // be as conservative as any other -- a medium the reference would have skipped returns false before it draws.)
    const bool fast_order = order == kOrderFast;
    uint32_t hierarchy_flags = fast_order ? uint32_t(F_FMA_BOX) : 0u;
    for (int32_t i = 0; i < scene->n_materials; i++) {
        const rtk_material& m = scene->materials[i];
        if (m.kind == RTK_MAT_DIFFUSE_LIGHT || m.kind == RTK_MAT_ISOTROPIC || m.kind == RTK_MAT_SPECULAR) prog.features |= F_EXOTIC_MAT;
        const bool textured = m.kind == RTK_MAT_LAMBERTIAN || m.kind == RTK_MAT_DIFFUSE_LIGHT || m.kind == RTK_MAT_ISOTROPIC;
        if (textured && scene->textures[m.texture].kind != RTK_TEX_SOLID) prog.features |= F_TEXTURE;
    }
    if (scene->n_lights > 0) prog.features |= F_LIGHTS;
    bool matte = true;  // only lambertians and lights: the quad/box subset kernel drops its glossy branches (F_MATTE)
    for (int32_t i = 0; i < scene->n_materials; i++)
        if (scene->materials[i].kind != RTK_MAT_LAMBERTIAN && scene->materials[i].kind != RTK_MAT_DIFFUSE_LIGHT) matte = false;
    if (matte) hierarchy_flags |= F_MATTE;
    if ((prog.features & F_MEDIA) != 0 && !prog.has_media_bracket) hierarchy_flags |= F_SPHERE_MEDIA_ONLY;

    RTK_HIP(hipSetDevice(ctx->device));
    ctx->has_scene = false;
    ctx->order_valid = false;  // a new scene: tile costs measured on the old one mean nothing
    // sphere-only scenes in the fast order additionally get the MIXED program (f32 culling boxes) for the f64 kernels
    // ... every other scene of the fast order the COMPACT program (f32 culling boxes, f64 primitives, 16-byte units)
    const bool want_mixed = fast_order && prog.features == kFeatLean && prog.chains.size() <= 1;
    if ((rc = build_device_scene<double>(*scene, prog, ctx->scene64, fast_order, want_mixed, eye_extent)) != RTK_OK) return rc;
    if ((rc = build_device_scene<float>(*scene, prog, ctx->scene32, fast_order)) != RTK_OK) return rc;
    ctx->features = prog.features | hierarchy_flags;
    ctx->n_ops = int32_t(prog.ops.size());
    ctx->n_materials = scene->n_materials;
    ctx->n_textures = scene->n_textures;
    ctx->scene_digest = scene_digest(*scene, prog, ctx->features, fast_order, eye_extent);
    ctx->has_scene = true;
    return RTK_OK;
}

int rtk_debug_mixed_program(const rtk_scene_desc* optimized, double eye_extent, int32_t capacity_units, int32_t* n_units, float* extent, void* h_units,
                            void* h_image) {
    if (!optimized || !n_units) return fail(RTK_ERR_INVALID, "rtk_debug_mixed_program: null argument");
    try {
        Program prog;
        const int rc = compile_scene(optimized, prog);
        if (rc != RTK_OK) return rc;
        if (prog.features != kFeatLean || prog.chains.size() > 1) return fail(RTK_ERR_INVALID, "rtk_debug_mixed_program: not a sphere-only scene");
        std::vector<MixedHead> units;
        std::vector<uint32_t> ranks;
        float ext = 0.0f;
        build_mixed_program(*optimized, prog, eye_extent, units, ranks, ext);
        *n_units = int32_t(units.size());
        if (extent) *extent = ext;
        if (size_t(capacity_units < 0 ? 0 : capacity_units) < units.size() && (h_units || h_image))
            return fail(RTK_ERR_INVALID, "rtk_debug_mixed_program: %zu units, room for %d", units.size(), capacity_units);
        if (h_units) std::memcpy(h_units, units.data(), units.size() * sizeof(MixedHead));
        if (h_image) {
            std::vector<MixedImg> image;
            build_mixed_lds_image(units, image);
            std::memcpy(h_image, image.data(), image.size() * sizeof(MixedImg));
        }
        return RTK_OK;
    } catch (const std::bad_alloc&) {
        return fail(RTK_ERR_INVALID, "rtk_debug_mixed_program: out of memory");
    }
}

int rtk_scene_info(rtk_ctx* ctx, int32_t* n_program_ops, int64_t* bytes_f64, int64_t* bytes_f32) {
    if (!ctx || !ctx->has_scene) return fail(RTK_ERR_NO_SCENE, "rtk_scene_info: no scene uploaded");
    if (n_program_ops) *n_program_ops = ctx->scene64.view.n_slots;
    if (bytes_f64) *bytes_f64 = ctx->scene64.bytes;
    if (bytes_f32) *bytes_f32 = ctx->scene32.bytes;
    return RTK_OK;
}

}  // extern "C"

namespace rtk {

// What the hot part of `scene`'s COMPACT program takes in LDS, materials included (build_hot_cold_program; exact: the
// program is compiled).  For rtk_scene_optimize's choice of the primitive cost (rtk_optimize.cpp); 0 when the
// description does not compile.
size_t hot_program_lds_bytes(const rtk_scene_desc* scene) {
    if (!scene) return 0;
    try {
        Program prog;
        if (compile_scene(scene, prog) != RTK_OK) return 0;
        std::vector<Unit16> hot, cold;
        std::vector<uint32_t> ranks;
        build_hot_cold_program(*scene, prog, hot, cold, ranks);
        return hot.size() * sizeof(Unit16) + size_t(scene->n_materials) * sizeof(MaterialRec<double>);
    } catch (const std::bad_alloc&) {
        return 0;
    }
}

}  // namespace rtk

// ------------------------------------------------------------------------------------------------ progressive sessions --
// What csrc/rtk_progressive.cpp needs of a context (rtk_internal.h).
namespace rtk {

int ctx_scene(const rtk_ctx* ctx, uint64_t* digest) {
    *digest = ctx->scene_digest;
    return ctx->has_scene ? 1 : 0;
}

uint32_t ctx_features(const rtk_ctx* ctx) { return ctx->features; }

int32_t ctx_n_materials(const rtk_ctx* ctx) { return ctx->n_materials; }

int32_t ctx_n_textures(const rtk_ctx* ctx) { return ctx->n_textures; }

size_t camera_record_bytes() { return kCameraStride; }

template <typename real>
const SceneView<real>& ctx_view(const rtk_ctx* ctx) {
    if constexpr (std::is_same_v<real, double>) return ctx->scene64.view;
    else return ctx->scene32.view;
}
template const SceneView<double>& ctx_view<double>(const rtk_ctx*);
template const SceneView<float>& ctx_view<float>(const rtk_ctx*);

template <typename real>
CameraRec<real> device_camera(const rtk_camera& cam) { return to_device_camera<real>(cam); }
template CameraRec<double> device_camera<double>(const rtk_camera&);
template CameraRec<float> device_camera<float>(const rtk_camera&);

}  // namespace rtk
