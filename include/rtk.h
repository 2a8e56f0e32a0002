/*
 * rtk.h -- C ABI of the MI355X path-tracing kernel library (librtk_hip.so).
 *
 * This is the drop-in boundary for ONE hot path of the reference: the per-pixel
 * sample loop behind camera::render() (Camera.txt:54-119 -> get_ray :177-191 ->
 * ray_color :203-238 -> hittable::hit / material::scatter / texture::value).
 * The reference has no FFI of its own; the only boundary it
 * offers is the header-level C++ scene API that main.cpp programs against.
 * The build keeps that API (raytracingoneweekendapplication_amd/host/) and its
 * camera::render() calls the functions below instead of spawning std::async
 * row workers (Camera.txt:59-61,96-100).
 *
 * Conventions
 *   - plain C, no torch / C++ types; every function returns 0 on success or a
 *     negative rtk_status; rtk_last_error() gives the text of the last failure
 *     on the calling thread.  Nothing throws across the boundary.
 *   - the caller owns every host buffer it passes; rtk_ctx owns device memory.
 *   - "device pointer" arguments are raw HIP device addresses (e.g. a torch
 *     tensor's data_ptr()); "stream" is a hipStream_t passed as void* (NULL =
 *     the default stream).
 *   - all scene reals are IEEE double, exactly the values the reference's
 *     constructors compute (vec3.h:7 `double e[3]`); rtk_scene_upload converts
 *     to float for the RTK_REAL_F32 kernels.
 *   - there is no CPU fallback: every entry point that computes fails with
 *     RTK_ERR_NO_DEVICE when no gfx950 device is usable.
 */
#ifndef RTK_H
#define RTK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: rtk_optimize_opts grew by free_media_order (40 -> 48 bytes; the entry points that take it copy it by value, so a
 * caller built against version 1 must be rebuilt), rtk_optimize_info.exact became three-valued, new entry points
 * (rtk_multi_*, rtk_render_multi_enqueue / rtk_multi_wait, rtk_debug_*).  Every rtk_scene_desc carries the version it was
 * built against and is refused when it differs (rtk_scene_upload, rtk_scene_optimize). */
#define RTK_ABI_VERSION 2

typedef enum rtk_status {
    RTK_OK = 0,
    RTK_ERR_INVALID = -1,      /* bad argument / malformed scene description     */
    RTK_ERR_NO_DEVICE = -2,    /* no usable HIP device (product never falls back) */
    RTK_ERR_HIP = -3,          /* a HIP runtime call failed                       */
    RTK_ERR_UNSUPPORTED = -4,  /* scene uses a construct the kernel does not run  */
    RTK_ERR_NO_SCENE = -5      /* render requested before rtk_scene_upload        */
} rtk_status;

typedef struct rtk_vec3 { double x, y, z; } rtk_vec3;

/* ------------------------------------------------------------------------
 * Scene description: an index-based copy of the reference's pointer graph.
 * One rtk_node per `hittable` object (hittable.h:29-36); shared_ptr edges
 * become node indices, so a DAG (e.g. the fog boundary that is also in the
 * world, main.cpp:305-307) stays a DAG.
 * ---------------------------------------------------------------------- */
typedef enum rtk_node_kind {
    RTK_NODE_SPHERE = 1,     /* sphere.h:12-28        a = index into spheres[]          */
    RTK_NODE_QUAD = 2,       /* quad.h:10-19          a = index into quads[]            */
    RTK_NODE_TRIANGLE = 3,   /* triangle.h:17-45      a = index into triangles[]        */
    RTK_NODE_LIST = 4,       /* hittable_list.h:9-41  a = first slot in list_children[], b = count */
    RTK_NODE_BVH = 5,        /* bvh.h:11-79           a = left node, b = right node, c = index into bvh_boxes[] */
    RTK_NODE_TRANSLATE = 6,  /* hittable.h:39-65      a = index into translates[], b = child node */
    RTK_NODE_ROTATE_Y = 7,   /* hittable.h:67-146     a = index into rotates[],    b = child node */
    RTK_NODE_MEDIUM = 8      /* constant_medium.h:8-60 a = index into media[],     b = boundary node */
} rtk_node_kind;

/* For primitive nodes (sphere, quad, triangle) `c` is 0 or 1 + the primitive's rank in the reference's visiting
 * order: rtk_scene_optimize fills it in so that, in its re-grouped hierarchy, two primitives hit at exactly the same
 * distance are resolved the way the reference's left-then-right traversal resolves them. */
typedef struct rtk_node { int32_t kind, a, b, c; } rtk_node;

/* sphere.h:60-64: `ray center` (origin = center1, direction = center2-center1),
 * radius = fmax(0, r).  A stationary sphere has center_dir = 0. */
typedef struct rtk_sphere {
    rtk_vec3 center0, center_dir;
    double radius;
    int32_t material, _pad;
} rtk_sphere;

/* quad.h:76-83: Q, u, v, w = n/dot(n,n), normal = unit(n), D = dot(normal,Q). */
typedef struct rtk_quad {
    rtk_vec3 Q, u, v, w, normal;
    double D;
    int32_t material, _pad;
} rtk_quad;

/* triangle.h:124-143: vertices, unit normal, raw (un-wrapped) float UVs. */
typedef struct rtk_triangle {
    rtk_vec3 p0, p1, p2, normal;
    float uv0[2], uv1[2], uv2[2];
    int32_t material, _pad;
} rtk_triangle;

typedef struct rtk_aabb { double xmin, xmax, ymin, ymax, zmin, zmax; } rtk_aabb; /* aabb.h:12 */
typedef struct rtk_translate { rtk_vec3 offset; } rtk_translate;                /* hittable.h:62 */
typedef struct rtk_rotate_y { double sin_theta, cos_theta; } rtk_rotate_y;      /* hittable.h:142-143 */
typedef struct rtk_medium {                                                     /* constant_medium.h:57-59 */
    double neg_inv_density;
    int32_t material, _pad;  /* the isotropic phase function.  Its texture is evaluated at the scatter POINT with u = v = 0:
                              * constant_medium::hit leaves rec.u / rec.v as the record held them (constant_medium.h:45-50), so in
                              * the reference an image or uv-checker texture there reads whatever an earlier hit() wrote -- not
                              * reproduced (solid colours, checkers over the point and noise textures are exact). */
} rtk_medium;

typedef enum rtk_material_kind {
    RTK_MAT_LAMBERTIAN = 1,    /* material.h:22-41   tex                       */
    RTK_MAT_METAL = 2,         /* material.h:78-92   albedo, param = fuzz (<=1) */
    RTK_MAT_DIELECTRIC = 3,    /* material.h:43-76   param = refraction index  */
    RTK_MAT_DIFFUSE_LIGHT = 4, /* material.h:94-122  tex (emissive_light is the same behaviour) */
    RTK_MAT_ISOTROPIC = 5,     /* material.h:124-138 tex                       */
    RTK_MAT_SPECULAR = 6       /* material.h:140-172 albedo, param = shininess */
} rtk_material_kind;

typedef struct rtk_material {
    int32_t kind, texture;     /* texture = -1 when the material has none */
    rtk_vec3 albedo;
    double param;
} rtk_material;

typedef enum rtk_texture_kind {
    RTK_TEX_SOLID = 1,         /* texture.h:20-32   color                                    */
    RTK_TEX_CHECKER = 2,       /* texture.h:34-56   param = inv_scale, even/odd = texture ids */
    RTK_TEX_CHECKER_TRI = 3,   /* texture.h:58-84   param = inv_scale, even/odd              */
    RTK_TEX_IMAGE = 4,         /* texture.h:86-108  image = index into images[]              */
    RTK_TEX_NOISE = 5          /* texture.h:110-120 param = scale, image = index into perlins[] */
} rtk_texture_kind;

typedef struct rtk_texture {
    int32_t kind, even, odd, image;
    rtk_vec3 color;
    double param;
} rtk_texture;

/* rtw_stb_image.h:71-81: 8-bit RGB, row-major, 3 bytes per texel.  width == 0
 * means "no data": image_texture::value returns cyan (texture.h:92). */
typedef struct rtk_image {
    int32_t width, height;
    int64_t texel_offset;      /* byte offset of texel (0,0) in rtk_scene_desc.texels */
} rtk_image;

/* perlin.h:52-57: gradient table and the three permutation tables.  They are
 * INPUTS to the device: the reference fills them from its global RNG at
 * construction (perlin.h:6-13), which is host-side scene setup. */
typedef struct rtk_perlin {
    double randvec[256][3];
    int32_t perm_x[256], perm_y[256], perm_z[256];
} rtk_perlin;

typedef struct rtk_point_light { rtk_vec3 position, intensity; double size; } rtk_point_light; /* point_light.h:24-27 */

typedef struct rtk_scene_desc {
    int32_t abi_version;       /* RTK_ABI_VERSION */
    int32_t root;              /* node index `camera::render` is handed as `world` */
    int32_t n_nodes, n_list_children, n_spheres, n_quads, n_triangles, n_bvh_boxes;
    int32_t n_translates, n_rotates, n_media, n_materials, n_textures, n_images, n_perlins, n_lights;
    int64_t n_texel_bytes;
    const rtk_node* nodes;
    const int32_t* list_children;
    const rtk_sphere* spheres;
    const rtk_quad* quads;
    const rtk_triangle* triangles;
    const rtk_aabb* bvh_boxes;
    const rtk_translate* translates;
    const rtk_rotate_y* rotates;
    const rtk_medium* media;
    const rtk_material* materials;
    const rtk_texture* textures;
    const rtk_image* images;
    const uint8_t* texels;
    const rtk_perlin* perlins;
    const rtk_point_light* lights;  /* the `lights` argument of camera::render (Camera.txt:54) */
} rtk_scene_desc;

/* ------------------------------------------------------------------------
 * Camera: the values camera::initialize() derives (Camera.txt:136-175).  The
 * host computes them in double exactly as the reference does (tan/sin/cos stay
 * on the host); the kernel only consumes them in get_ray (Camera.txt:177-200).
 * ---------------------------------------------------------------------- */
typedef struct rtk_camera {
    int32_t image_width, image_height;   /* Camera.txt:39,137-138 */
    int32_t samples_per_pixel, max_depth; /* Camera.txt:42-43     */
    rtk_vec3 background;                  /* Camera.txt:44        */
    rtk_vec3 center, pixel00_loc, pixel_delta_u, pixel_delta_v; /* Camera.txt:125-128 */
    rtk_vec3 defocus_disk_u, defocus_disk_v;                    /* Camera.txt:130-131 */
    double defocus_angle;                 /* Camera.txt:51        */
    double pixel_samples_scale;           /* Camera.txt:124,140   */
} rtk_camera;

typedef enum rtk_real_mode {
    RTK_REAL_F64 = 0,   /* the reference's arithmetic type; the parity mode        */
    RTK_REAL_F32 = 1    /* throughput mode: images agree statistically;
                         * hit / scatter / texture / get_ray match the reference's
                         * known answers within f32 rounding, case by case        */
} rtk_real_mode;

/* Image tiles: one 8x8-pixel tile per 64-lane wavefront.  Tile t (row-major
 * over ceil(W/8) x ceil(H/8)) belongs to rank (t % n_ranks) and is that rank's
 * local tile (t / n_ranks).  n_ranks = 1 renders the whole image. */
#define RTK_TILE_W 8
#define RTK_TILE_H 8
#define RTK_TILE_PIXELS 64

typedef struct rtk_render_opts {
    uint32_t seed;          /* render seed; per-sample stream = f(seed, pixel, sample) */
    int32_t real_mode;      /* rtk_real_mode */
    int32_t rank, n_ranks;  /* tile ownership; (0,1) = whole image */
    int32_t count_work;     /* != 0: also accumulate rtk_work_counters (slower; not for timing) */
    int32_t variant;        /* 0 = default.  Bit flags for A/B measurements and tests; none of them changes what is
                             * computed: 1 = keep the traversal program in global memory (no LDS staging);
                             * 2 = one sample chunk per pixel; 4 = fixed row-major tile order (no cost-ordered
                             * hand-out); bits 3-4 = chunk size (0: 8 samples, 1: 4, 2: 2, 3: 16);
                             * bits 5-7 = grid cap k, read by the host only (tests, tools): 0 = none, k = 1..7 = the launch has at
                             * most 2^(k-1) waves (1, 2, 4, ... 64), so that a small frame's waves each take many work items;
                             * the kernel chosen, its name and rtk_frame_launches do not depend on it; progressive sessions ignore it;
                             * bits 8-13 = scheduler loop-exit thresholds, bits 14-16 = refill batch size, bits 17-19 = lanes needed
                             * for a sphere step inside the box loop, bit 20 = f64 boxes instead of the MIXED program, bit 21 = no boxes-in-LDS
                             * kernel for programs larger than LDS (see csrc/rtk_trace.hip); bit 22 = write the compact tile
                             * buffer [tiles][3][64] also when n_ranks == 1 (rtk_multi's one-device RCCL path; d_rgb8 NULL);
                             * bit 23 = the hot/cold form of a COMPACT program (quads and triangles in memory, the rest in
                             * LDS) although the whole program would fit (tests); bit 24 = render every sample chunk in ONE
                             * launch with a partial-sum plane per chunk (up to 64) instead of passes over as many chunks as the 1.1 GB workspace budget holds planes for, whose running
                             * sum the resolve kernel carries (tests: the same additions in the same order, the same image) */
    void* stream;           /* hipStream_t, NULL = default stream */
} rtk_render_opts;

/* Exact per-render work counters (sums over all samples this rank traced);
 * the "algorithmic bytes" model of SURVEY.md 8(d) is a linear form in them. */
typedef struct rtk_work_counters {
    uint64_t samples;        /* primary samples traced                         */
    uint64_t segments;       /* ray segments = world.hit calls (Camera.txt:211) */
    uint64_t box_tests;      /* aabb::hit calls (bvh.h:65)                V    */
    uint64_t sphere_tests;   /* sphere::hit calls                        T_sphere */
    uint64_t quad_tests;     /* quad::hit calls                          T_quad */
    uint64_t triangle_tests; /* triangle::hit calls                      T_tri */
    uint64_t xform_enters;   /* translate::hit + rotate_y::hit calls     X     */
    uint64_t medium_tests;   /* constant_medium::hit calls               M     */
    uint64_t surface_hits;   /* material interactions (Camera.txt:216-223) H   */
    uint64_t noise_calls;    /* perlin::noise calls (perlin.h:14)        P     */
    uint64_t texel_fetches;  /* rtw_image::pixel_data calls              I     */
    uint64_t rng_draws;      /* random_double() calls (rtweekend.h:26)         */
} rtk_work_counters;

typedef struct rtk_ctx rtk_ctx;

/* Version / diagnostics --------------------------------------------------- */
int rtk_abi_version(void);
const char* rtk_last_error(void);

/* Lifetime ---------------------------------------------------------------- */
/* Binds a context to HIP device `device` (ordinal as seen by this process). */
int rtk_init(int device, rtk_ctx** out_ctx);
int rtk_destroy(rtk_ctx* ctx);

/* Scene --------------------------------------------------------------------
 * Validates the description (>= 1 primitive reachable from root -- the
 * reference recurses forever on an empty world, bvh.h:38-43 / SURVEY Q6),
 * linearises the graph into the kernel's traversal program in the
 * reference's visiting order (bvh.h:64-72: left, then right, both always)
 * and uploads f64 and f32 copies.  Replaces any previously uploaded scene. */
int rtk_scene_upload(rtk_ctx* ctx, const rtk_scene_desc* scene);

/* Host-only: everything rtk_scene_upload checks before it touches the device --
 * table indices, texture/material references, node kinds, nesting limits, at
 * least one primitive reachable from the root -- and the compilation of the
 * traversal program, without a device (works where there is no GPU).  Returns
 * the status rtk_scene_upload would return for a malformed description;
 * *n_program_ops (may be NULL) receives the program length in ops. */
int rtk_scene_validate(const rtk_scene_desc* scene, int32_t* n_program_ops);

/* Fast visiting order -----------------------------------
 * Host-only pass, no device needed.  Re-groups the SAME primitives of `scene`
 * into a surface-area-heuristic hierarchy with a fixed near-child-first order
 * (near = closer to opts->eye) and returns it as a new description made of
 * RTK_NODE_BVH / RTK_NODE_LIST nodes; upload that instead of `scene` to render
 * with fewer aabb::hit calls per ray.  The reference's own order (bvh.h:13-45
 * median split, bvh.h:64-72 left then right) stays the default everywhere else.
 * The closest hit of every ray is preserved and exact ties go to the primitive
 * the reference would have kept (rtk_node.c ranks), so the image is bit-identical
 * (info->exact = 2: proven; 1 for scenes with triangles: measured, not provable).  A constant_medium draws a random number inside hit()
 * (constant_medium.h:40), so it must be called with the interval the reference
 * calls it with: media (and instances holding one) keep their position in the
 * reference's visiting order and only the runs of objects between them are
 * re-grouped -- the bvh_nodes above a medium need not be kept, because a medium
 * the reference skips there returns false before it draws anyway (see
 * opts->free_media_order).  With triangles see rtk_optimize_info.has_triangles.
 * The work counters differ by design.  *out_scene borrows every table of `scene` except nodes,
 * list_children and bvh_boxes: keep `scene` alive while it is in use, release it
 * with rtk_scene_optimized_free. */
typedef struct rtk_optimize_opts {
    int32_t has_eye;        /* != 0: order children by distance to `eye` (camera::center, Camera.txt:125) */
    int32_t max_leaf;       /* most primitives tested in a row without a box of their own (0 = 4) */
    rtk_vec3 eye;
    double prim_cost_scale; /* scales the cost of a primitive test relative to a slab test in the SAH.  0 = automatic: the
                             * largest of a short list of scales (from 1.5 without quads, 2.0 with) whose program the f64
                             * kernels can keep in one CU's LDS -- whole, or at least its hot part (everything but quads
                             * and triangles), or at least the box records (see rtk_optimize.cpp) */
    int32_t free_media_order; /* 0 (default): a constant_medium keeps its position in the reference's visiting order -- it is
                               * called after exactly the objects that precede it there -- so it meets the same interval
                               * and draws the same random numbers as in the reference: the image stays bit-identical
                               * (info->exact >= 1).  != 0: media are re-grouped like any other object; the order of the
                               * draws inside constant_medium::hit changes and parity becomes statistical */
    int32_t _pad;
} rtk_optimize_opts;

typedef struct rtk_optimize_info {
    int32_t exact;              /* 2: images are PROVEN bit-identical to the reference order (closest hits preserved, ties by
                                 * reference rank, media at their reference positions).  1: EMPIRICALLY identical -- the scene
                                 * has triangles (see has_triangles): identical in every measurement, not provable; verify
                                 * (render both orders) or opt in before relying on it.  0: statistical parity only
                                 * (opts->free_media_order) */
    int32_t has_media;          /* a constant_medium draws inside hit(): exact only while opts->free_media_order == 0 */
    int32_t has_triangles;      /* triangle::hit's float determinant (triangle.h:72,77): identical except where the
                                 * reference's own boxes cull a hit that triangle::hit accepts (order-dependent);
                                 * caps `exact` at 1 */
    int32_t n_bvh_nodes_in, n_bvh_nodes_out;
    int32_t n_ordered_items;    /* media, and instances holding one, that kept their position in the reference's order */
    double expected_cost;       /* SAH estimate, in slab tests, of one closest-hit query */
    double box_margin;          /* every new box is grown by this much (2^-40 of the scene extent) */
} rtk_optimize_info;

int rtk_scene_optimize(const rtk_scene_desc* scene, const rtk_optimize_opts* opts,
                       rtk_scene_desc** out_scene, rtk_optimize_info* info /* may be NULL */);
void rtk_scene_optimized_free(rtk_scene_desc* scene);

/* rtk_scene_optimize + rtk_scene_upload in one call.  Because every box of the
 * optimised hierarchy carries the pass's margin, the kernels additionally use a
 * fused multiply-add slab test (18 instead of 24 f64 operations per aabb::hit)
 * that is conservative with respect to aabb.h:61-85 on such boxes: no hit is
 * lost, the image is the same as rendering rtk_scene_optimize's output through
 * rtk_scene_upload.  `scene` is not needed after the call returns. */
int rtk_scene_upload_fast(rtk_ctx* ctx, const rtk_scene_desc* scene, const rtk_optimize_opts* opts,
                          rtk_optimize_info* info /* may be NULL */);

/* Upload a description RETURNED BY rtk_scene_optimize (its boxes carry the pass's margin) with the fused / f32
 * culling slab tests enabled -- the second half of rtk_scene_upload_fast, for callers that optimise once and
 * upload to several contexts (rtk_multi_scene_upload_fast does).  `opts` = the options the pass was given
 * (its eye sizes the f32 culling margin); may be NULL. */
int rtk_scene_upload_optimized(rtk_ctx* ctx, const rtk_scene_desc* optimized, const rtk_optimize_opts* opts);

/* Number of tiles rank `rank` of `n_ranks` owns for a W x H image, and the
 * element count of its compact tile buffer (tiles * 3 * 64 reals). */
int64_t rtk_tiles_per_rank(int image_width, int image_height, int n_ranks);

/* Render -------------------------------------------------------------------
 * The replacement for the body of camera::render (Camera.txt:65-93), device
 * resident and asynchronous on opts->stream.
 *   n_ranks == 1:  d_linear = row-major H*W*3 reals (double for F64, float for
 *                  F32), the pixel colour AFTER the 1/spp scale and BEFORE
 *                  gamma (Camera.txt:74); d_rgb8 = row-major H*W*3 bytes as
 *                  Camera.txt:77-89 writes them.  Either may be NULL.
 *   n_ranks  > 1:  d_linear = this rank's compact tile buffer
 *                  [tiles_per_rank][3][64] reals; d_rgb8 must be NULL (bytes
 *                  are produced by rtk_tiles_unpermute on the gathering rank).
 * d_counters (device, sizeof(rtk_work_counters), zeroed by the caller) is
 * required iff opts->count_work != 0.
 *
 * Streams (this holds for every entry point that is "asynchronous on" a stream:
 * rtk_render_device, rtk_tiles_unpermute, rtk_progressive_step, rtk_render_aovs,
 * rtk_denoise, rtk_progressive_denoise, rtk_render_guides, rtk_denoise_guided, rtk_progressive_denoise_guided,
 * rtk_temporal_accumulate, rtk_query_hits / _occluded / _radiance, rtk_probe_*, rtk_lens_*, rtk_gather_*):
 *   - all work of a call -- kernels, memsets, the upload of the camera record --
 *     is enqueued on the stream it is given and on no other; the call reads its
 *     host arguments (cam, opts) before it returns and never waits for the
 *     device, except to grow a workspace the first time a larger frame is seen.
 *   - a context is driven from ONE stream at a time: its launches share the
 *     partial-sum workspace, the tile order and the per-launch rings, and what
 *     orders them is that stream.  Sessions of the context count: a session
 *     steps on the stream it was created with.
 *   - moving a context (or a session and the one-shot renders between its steps)
 *     to another stream needs an event the new stream waits for, or a host wait.
 *     Two streams on one context without such ordering are a data race.
 *   - any number of frames may be in flight on the stream; the rings behind a
 *     launch (work-item counters, camera records) are reused in stream order.
 *   - rtk_progressive_create, rtk_progressive_set_adaptive and
 *     rtk_progressive_resume may be called while the stream is busy: they touch
 *     only the session's own, new memory.  create and set_adaptive set it up on
 *     the session's stream and do not wait for it; resume copies the caller's
 *     checkpoint with blocking calls, which may wait for work queued ahead of
 *     them on the device, and for an adaptive checkpoint waits for the stream.
 *   - for overlap use two contexts on two streams. */
int rtk_render_device(rtk_ctx* ctx, const rtk_camera* cam, const rtk_render_opts* opts,
                      void* d_linear, uint8_t* d_rgb8, rtk_work_counters* d_counters);

/* After gathering every rank's compact buffer into
 * d_gathered[n_ranks][tiles_per_rank][3][64] (rank-major, as ncclGather /
 * torch.distributed.gather lays them out): scatter to the row-major image
 * and apply gamma/clamp/quantise.  Asynchronous on `stream`. */
int rtk_tiles_unpermute(rtk_ctx* ctx, int image_width, int image_height, int n_ranks,
                        int real_mode, const void* d_gathered,
                        void* d_linear, uint8_t* d_rgb8, void* stream);

/* Convenience for host callers (camera::render): allocates device buffers,
 * renders the whole image, synchronises and copies back.  h_linear is
 * H*W*3 doubles (F32 results are widened), h_rgb8 is H*W*3 bytes; either may
 * be NULL.  counters may be NULL. */
int rtk_render_host(rtk_ctx* ctx, const rtk_camera* cam, const rtk_render_opts* opts,
                    double* h_linear, uint8_t* h_rgb8, rtk_work_counters* counters);

/* Several GPUs behind one call --------------------------------------------------
 * camera::render owns all parallelism in the reference (std::async row blocks,
 * Camera.txt:59-61,96-100); rtk_multi is that on the GPUs of one node, driven by
 * ONE host thread: the scene is replicated, device i renders the interleaved tiles
 * (t % n == i) into its compact tile buffer on its own stream, ONE gather brings
 * the buffers to the first device -- a single RCCL ncclGather over xGMI
 * (rccl.h:745; librccl is loaded on demand) or, when a device is listed more than
 * once or RCCL is unavailable, one peer copy per device issued on the producing
 * device's stream -- and rtk_tiles_unpermute there writes the row-major image.
 * No other exchange exists: every (pixel, sample) is independent.  The image is
 * bit-identical for any device count (per-sample RNG streams, fixed sample
 * chunks).  `devices` are HIP ordinals; an ordinal may repeat (two ranks then share
 * a GPU: used by tests on one-GPU boxes). */
typedef struct rtk_multi rtk_multi;

typedef enum rtk_gather_mode {
    RTK_GATHER_AUTO = 0,   /* RCCL when every device is distinct and librccl loads, else peer copies */
    RTK_GATHER_PEER = 1,   /* hipMemcpyPeerAsync from each device's stream */
    RTK_GATHER_RCCL = 2    /* ncclGather; rtk_init_multi fails if RCCL cannot be set up */
} rtk_gather_mode;

int rtk_init_multi(int n_devices, const int* devices, int gather_mode, rtk_multi** out_multi);
int rtk_multi_destroy(rtk_multi* multi);
int rtk_multi_device_count(const rtk_multi* multi);
/* 1 when the gather runs through RCCL, 0 for peer copies. */
int rtk_multi_uses_rccl(const rtk_multi* multi);
/* The context bound to device slot i (owned by `multi`; for rtk_scene_info / rtk_kernel_name). */
rtk_ctx* rtk_multi_ctx(rtk_multi* multi, int i);
/* Replicated upload.  The _fast form runs rtk_scene_optimize ONCE on the host and uploads
 * its output to every device. */
int rtk_multi_scene_upload(rtk_multi* multi, const rtk_scene_desc* scene);
int rtk_multi_scene_upload_fast(rtk_multi* multi, const rtk_scene_desc* scene, const rtk_optimize_opts* opts,
                                rtk_optimize_info* info /* may be NULL */);
/* Render one frame on all devices; the result (row-major H*W*3 reals of opts->real_mode
 * and/or H*W*3 bytes, either may be NULL) is resident on the FIRST device when the call
 * returns (blocking).  opts->rank / n_ranks / stream are ignored (the call owns the split). */
int rtk_render_multi_device(rtk_multi* multi, const rtk_camera* cam, const rtk_render_opts* opts,
                            void* d_linear, uint8_t* d_rgb8);
/* The asynchronous form: returns when the frame's work has been enqueued -- the renders on each device's stream, the
 * gather and the un-permute on per-device transfer streams -- with up to two frames in flight: frame k + 1 renders into a
 * second set of tile buffers while frame k is gathered and un-permuted (frame k + 2 waits on the device for frame k's
 * release; the host never blocks here).  d_linear / d_rgb8 (on the first device, either may be NULL) must stay valid
 * until rtk_multi_wait returns; frames that name the same buffers overwrite them in order.  rtk_multi_wait blocks until
 * every enqueued frame is complete (progress callbacks run from it).  rtk_render_multi_device = enqueue + wait. */
int rtk_render_multi_enqueue(rtk_multi* multi, const rtk_camera* cam, const rtk_render_opts* opts,
                             void* d_linear, uint8_t* d_rgb8);
int rtk_multi_wait(rtk_multi* multi);
/* Host-only, no device needed: the buffer-set rule rtk_render_multi_enqueue follows for frame number `frame`
 * (0, 1, 2, ...): out[0] = buffer set, out[1] = 1 when the renders first wait for that set's release by frame - 2. */
int rtk_multi_frame_plan(int64_t frame, int32_t out[2]);
/* The same into host buffers (h_linear: H*W*3 doubles, F32 results widened), as rtk_render_host. */
int rtk_render_multi(rtk_multi* multi, const rtk_camera* cam, const rtk_render_opts* opts,
                     double* h_linear, uint8_t* h_rgb8);

/* Progress ----------------------------------------------------------------------
 * The reference prints "Scanlines remaining" from an atomic the row workers bump
 * (Camera.txt:63,91,102-106).  Here the render kernel's work-item counter plays
 * that role: while a blocking render (rtk_render_host, rtk_render_multi*) runs,
 * the calling thread samples it off the kernel's path -- a 4-byte device-to-host
 * hipMemcpyAsync of the counter into a pinned word, on a stream of its own (the
 * copy engine; the persistent kernel does no extra work, and a sample that has not
 * landed by the next tick is skipped) -- and calls `fn(done, total, user)` with
 * done/total in work items (8x8 tile x sample chunk), at most every `interval_ms`
 * (<= 0: 100 ms).  fn == NULL switches it off.  Never called from another thread. */
typedef void (*rtk_progress_fn)(int64_t done, int64_t total, void* user);
int rtk_set_progress_callback(rtk_ctx* ctx, rtk_progress_fn fn, void* user, int interval_ms);

/* Progressive, resumable rendering ------------------------------------------------
 * A session (rtk_progressive) owns the running sums of ONE frame -- this rank's [local tile][3][64] reals, the layout of the
 * resolve's running sum -- and renders it in steps: a step adds samples [done, done + n) of every pixel.  The target spp is
 * cam->samples_per_pixel at creation, and the frame is cut into the chunks a one-shot render of the target uses
 * (rtk_progressive_chunk_size: 8 samples up to 512 spp).  Because every sample's random stream is f(seed, pixel, absolute
 * sample) and the chunks are added in the one-shot order (c0, + c1, + c2, ...), the finished session's image is BIT-IDENTICAL
 * to rtk_render_device's for the same scene, camera, seed and real mode, whatever the steps; and after each step the preview is
 * bit-identical to a one-shot render with samples_per_pixel = samples_done (and pixel_samples_scale = 1.0 / samples_done) as
 * long as that render uses the same chunk size (target <= 512).  One device, one rank's tiles; not through rtk_multi.
 *
 * Rules:
 *   - n_samples must be a multiple of the chunk size, except for the step that ends exactly at the target.  A step that would
 *     pass the target, a step on a finished session and n_samples <= 0 return RTK_ERR_INVALID and change nothing.
 *   - the session records a 64-bit digest of the program uploaded when it was created; a step after the context's scene changed
 *     (another scene, or the same one in the other visiting order) fails with RTK_ERR_INVALID.
 *   - a step that fails in a HIP call poisons the session: every later call on it fails (rtk_progressive_destroy excepted).
 *   - the session's sums are its own device memory: one-shot renders may be enqueued on the same context between steps.
 *
 * Noise estimate (batch means over chunks): for every full chunk k of a pixel, y_k = (s.x + s.y + s.z) / (3 c) (c = chunk
 * size, s = the chunk's sample sum); the session keeps S1 = sum y_k and S2 = sum y_k^2 in double.  With K >= 2 full chunks:
 * m = S1 / K, v = max(0, (S2 - K m^2) / (K - 1)), se = sqrt(v / K), rel = se / max(m, 1e-3).  A final partial chunk is in the
 * image, not in the estimate.  rtk_noise_stats reduces se / rel over this rank's in-image pixels in a fixed order (the same
 * inputs give the same bits); valid = 0 while K < 2. */
typedef struct rtk_progressive rtk_progressive;

typedef struct rtk_noise_stats {
    int64_t samples_done;
    int32_t full_chunks;     /* K */
    int32_t valid;           /* K >= 2 */
    double mean_se;          /* mean over in-image pixels of se */
    double max_se;
    double mean_rel_se;      /* mean over in-image pixels of se / max(m, 1e-3) */
} rtk_noise_stats;

/* Checkpoint (rtk_progressive_save): a little-endian byte string, version 1:
 *   offset  0  char[8]     magic "RTKPROG\0"
 *           8  int32       version (1)
 *          12  int32 x 8   width, height, rank, n_ranks, real_mode, target_spp, chunk_size, samples_done
 *          44  uint32      seed
 *          48  uint64      scene_digest
 *          56  rtk_camera  the session's camera (200 bytes)
 *         256  real  [tiles_per_rank][3][64]   running sum (8-byte reals for F64, 4-byte for F32)
 *              double[tiles_per_rank][64]      S1, then S2
 *              uint64      FNV-1a 64 of every byte before it
 * (tiles_per_rank = rtk_tiles_per_rank(width, height, n_ranks)). */
#define RTK_CHECKPOINT_VERSION 1
typedef struct rtk_checkpoint_info {
    int32_t version, width, height, rank, n_ranks, real_mode, target_spp, chunk_size, samples_done;
    uint32_t seed;
    uint64_t scene_digest;
} rtk_checkpoint_info;

/* A session for cam (samples_per_pixel = target) and opts (seed, real_mode, rank / n_ranks, stream; count_work and variant
 * are ignored: a step counts work when it is given counters).  Needs an uploaded scene. */
int rtk_progressive_create(rtk_ctx* ctx, const rtk_camera* cam, const rtk_render_opts* opts, rtk_progressive** out);
/* Enqueue the next n_samples of every pixel on opts->stream and write the preview (scaled by 1 / samples_done): n_ranks == 1:
 * d_linear row-major H*W*3 reals, d_rgb8 H*W*3 bytes, d_noise H*W floats (se); n_ranks > 1: d_linear this rank's compact tile
 * buffer, d_rgb8 NULL, d_noise [tiles_per_rank][64].  Any output may be NULL.  d_counters (zeroed by the caller) receives this
 * step's work counters when given. */
int rtk_progressive_step(rtk_progressive* p, int32_t n_samples, void* d_linear, uint8_t* d_rgb8, float* d_noise, rtk_work_counters* d_counters);
/* The same into host buffers (h_linear doubles -- F32 widened -- of the layout above); blocking.  counters may be NULL. */
int rtk_progressive_step_host(rtk_progressive* p, int32_t n_samples, double* h_linear, uint8_t* h_rgb8, float* h_noise, rtk_work_counters* counters);
int rtk_progressive_samples_done(const rtk_progressive* p);
int rtk_progressive_chunk_size(const rtk_progressive* p);
/* Frame noise statistics of the samples done so far (synchronises the session's stream). */
int rtk_progressive_noise(rtk_progressive* p, rtk_noise_stats* out);
int64_t rtk_progressive_checkpoint_bytes(const rtk_progressive* p);
/* Write the checkpoint into h_buf (n >= rtk_progressive_checkpoint_bytes); synchronises the session's stream. */
int rtk_progressive_save(rtk_progressive* p, void* h_buf, int64_t n);
/* A session that continues a checkpoint.  Refused (RTK_ERR_INVALID, reason in rtk_last_error) when the checkpoint is truncated or
 * corrupted, or its camera, seed, real mode, rank / n_ranks, target or scene digest differ from the call's / the context's. */
int rtk_progressive_resume(rtk_ctx* ctx, const rtk_camera* cam, const rtk_render_opts* opts, const void* h_buf, int64_t n, rtk_progressive** out);
/* Host-only (no context, no device): parse and check a checkpoint (magic, version, sizes, checksum). */
int rtk_checkpoint_read_info(const void* h_buf, int64_t n, rtk_checkpoint_info* out);
int rtk_progressive_destroy(rtk_progressive* p);

/* Tile-adaptive sampling ------------------------------------------------------------
 * An adaptive session puts its samples where the noise is, one 8x8 tile (the work of one wave) at a time.  Every tile of the
 * rank is ACTIVE -- it holds samples_done samples -- or RETIRED: it keeps the tile_spp[t] samples it had when it retired and
 * never renders again.  A step renders the next n samples of the active tiles only (the step rules above are unchanged).  At
 * the end of a step, an active tile with min_samples <= samples_done < target retires when its metric -- the maximum over its
 * in-image pixels of se / max(m, 1e-3), K = samples_done / chunk (the noise estimate above) -- is <= rel_target.  Padding
 * tiles of a rank (outside the image) are never rendered and count as neither (tile_spp 0).
 *   - previews scale each pixel by 1 / tile_spp[t] and its se uses the tile's own K; rtk_progressive_noise uses per-tile K.
 *   - every pixel of tile t is BIT-IDENTICAL to a one-shot render of the same scene, camera, seed and real mode with
 *     samples_per_pixel = tile_spp[t], as long as that render uses the same chunk size (target <= 512).  With a rel_target no
 *     tile reaches, the finished image is the one-shot frame.
 *   - a step when no tile is active is valid: it changes no pixel (the previews are still written) and stays asynchronous.
 *   - checkpoints of an adaptive session are version 2 (see above: the version-1 layout, then double rel_target, int32
 *     min_samples, int32 0, int32 tile_spp[tiles_per_rank], then the checksum); resume restores the adaptive state.
 *     Non-adaptive sessions still write version 1.
 *   - one rank or several, like progressive sessions; not through rtk_multi. */
typedef struct rtk_adaptive_opts {
    double rel_target;     /* > 0 */
    int32_t min_samples;   /* a multiple of the chunk size, >= 2 chunks, <= the target */
    int32_t reserved;      /* 0 */
} rtk_adaptive_opts;

typedef struct rtk_adaptive_state {
    int32_t active_tiles;      /* this rank's tiles that still render */
    int32_t retired_tiles;
    int64_t pixel_samples;     /* sum over in-image pixels of their tile's sample count */
    double mean_spp;           /* pixel_samples / in-image pixels of this rank */
} rtk_adaptive_state;

/* Make a session adaptive: only before its first step (RTK_ERR_INVALID afterwards, or for bad options). */
int rtk_progressive_set_adaptive(rtk_progressive* p, const rtk_adaptive_opts* opts);
/* Synchronises the session's stream.  A non-adaptive session reports every in-image tile active. */
int rtk_adaptive_status(rtk_progressive* p, rtk_adaptive_state* out);
/* tile_spp of this rank's tiles: h_out[rtk_tiles_per_rank(...)], local tile order; synchronises. */
int rtk_adaptive_tile_samples(rtk_progressive* p, int32_t* h_out);
/* Host-only: the adaptive part of a checkpoint (checked like rtk_checkpoint_read_info).  Version 1: *out = {0, 0, 0} and
 * h_tile_spp is left alone.  Version 2: the options and, when h_tile_spp is given, tile_spp[tiles_per_rank]. */
int rtk_checkpoint_read_adaptive(const void* h_buf, int64_t n, rtk_adaptive_opts* out, int32_t* h_tile_spp);

/* Denoising ------------------------------------------------------------------------
 * First-hit guide buffers (AOVs): rtk_render_aovs renders, for samples s = 0 .. n_samples-1 of every pixel, the render's primary
 * ray (get_ray with opts->seed: sample s of the render, bit for bit) and the closest hit of the scene root on interval(0.001, inf)
 * (Camera.txt:211), a constant medium drawing from the stream of keys (seed, j*W+i, s + 2^31) -- rtk_debug_get_ray then
 * rtk_debug_closest_hit reproduce every sample.  d_aov[(j*W+i)*8 + k] (float32; sums in the real mode's type in sample order,
 * each divided by its count once, then rounded to float):
 *   k 0-2  albedo, mean over the n samples: a miss gives the camera background clamped to [0, 1]; a hit, by material kind:
 *          lambertian / isotropic texture::value(u, v, p), metal / specular albedo, dielectric (1, 1, 1), diffuse_light
 *          min(1, texture::value) per channel
 *   k 3    hit fraction: hits / n (medium hits count)
 *   k 4-6  the hit record's normal summed over hits (isotropic hits add 0), divided by n
 *   k 7    depth: the mean over hits of t * |rd|; 0 when no sample hits
 * Whole images only: n_ranks != 1, n_samples <= 0 or a null buffer give RTK_ERR_INVALID; no scene gives RTK_ERR_NO_SCENE.
 * Alignment: d_aov is written and read 16 bytes at a time and must be 16-byte aligned -- rtk_render_aovs and rtk_denoise refuse
 * another pointer with RTK_ERR_INVALID (the text names d_aov) before anything is launched or written.  Every other device
 * buffer of this section needs only the alignment of its element type (8 for F64 reals, 4 for floats, 1 for bytes).
 * rtk_render_aovs is asynchronous on opts->stream; rtk_render_aovs_host blocks (count_work and variant are ignored).
 *
 * Denoiser: an edge-avoiding a-trous filter (Dammertz et al. 2010) with the luminance weight of SVGF (Schied et al. 2017),
 * spatial part (the temporal part is "Temporal accumulation" below), guided by the AOVs and by the per-pixel variance se^2
 * of the noise estimate (d_noise, as a progressive step writes it).  Iteration k = 0 .. iterations-1 takes the 5x5 taps q = p + 2^k (dx, dy), dy outer, dx inner, skipping
 * taps outside the image, with weight h[dx] h[dy] w_l w_n w_z w_a, h = (1/16, 1/4, 3/8, 1/4, 1/16):
 *   w_l = exp(-|y_p - y_q| / (sigma_l sqrt(max(gv_p, 0)) + 1e-6)), y = (r + g + b) / 3, gv_p = the 3x3 binomial (1 2 1)/4 of
 *         the variance around p (edges clamped)
 *   w_n = 1 if both mean normals are 0, 0 if one is, else max(0, cos(n_p, n_q))^sigma_n
 *   w_z = 1 if either hit fraction is 0, else exp(-|z_p - z_q| / (sigma_z (g_p |o| + 1e-3 z_p) + 1e-6)), g_p = half the
 *         larger central difference of depth at p (edges clamped), |o| = 2^k sqrt(dx^2 + dy^2)
 *   w_a = exp(-|a_p - a_q| / sigma_a)
 * c'_p = sum w c_q / sum w, var'_p = sum w^2 var_q / (sum w)^2.  The filter computes in float32 with no atomics and a fixed tap
 * order: the same inputs give the same bits.  Its ping-pong buffers are context-owned device memory, grown on demand.
 *   d_linear  H*W*3 reals of real_mode (read as such, then rounded to float); d_aov as above; d_noise H*W floats (se; required)
 *   outputs   d_out_linear H*W*3 reals of real_mode and / or d_out_rgb8 H*W*3 bytes (the resolve's gamma / clamp / quantise in
 *             double); either may alias d_linear or d_noise (read once, before the first iteration), but not d_aov: the last
 *             iteration reads the neighbours' guides from d_aov while it writes the outputs.
 * Options: a field that is 0 takes its default -- iterations 5 (1..8), sigma_l 4, sigma_n 128, sigma_z 1, sigma_a 0.1; negative
 * or non-finite sigmas, other iteration counts and reserved != 0 give RTK_ERR_INVALID.  opts may be NULL (all defaults).
 * rtk_denoise is asynchronous on `stream`; rtk_denoise_host (h_linear doubles, F32 rounded; h_out_linear widened) blocks. */
typedef struct rtk_denoise_opts {
    int32_t iterations;
    float sigma_l, sigma_n, sigma_z, sigma_a;
    int32_t reserved;   /* 0 */
} rtk_denoise_opts;

int rtk_render_aovs(rtk_ctx* ctx, const rtk_camera* cam, const rtk_render_opts* opts, int32_t n_samples, float* d_aov);
int rtk_render_aovs_host(rtk_ctx* ctx, const rtk_camera* cam, const rtk_render_opts* opts, int32_t n_samples, float* h_aov);
int rtk_denoise(rtk_ctx* ctx, int32_t width, int32_t height, int32_t real_mode, const void* d_linear, const float* d_aov, const float* d_noise,
                const rtk_denoise_opts* opts, void* d_out_linear, uint8_t* d_out_rgb8, void* stream);
int rtk_denoise_host(rtk_ctx* ctx, int32_t width, int32_t height, int32_t real_mode, const double* h_linear, const float* h_aov, const float* h_noise,
                     const rtk_denoise_opts* opts, double* h_out_linear, uint8_t* h_out_rgb8);
/* The session's current preview denoised with its own se (per-tile scale and K in adaptive sessions), on the session's stream.
 * The AOVs of the session's camera and seed are rendered on first use and kept per aov_samples on the session (not in
 * checkpoints).  Needs n_ranks == 1 and at least 2 full chunks (RTK_ERR_INVALID otherwise).  The session is not changed: later
 * steps, checkpoints, noise statistics and the finished image are what they would have been.  The _host form blocks and
 * returns the linear image as doubles. */
int rtk_progressive_denoise(rtk_progressive* p, int32_t aov_samples, const rtk_denoise_opts* opts, void* d_out_linear, uint8_t* d_out_rgb8);
int rtk_progressive_denoise_host(rtk_progressive* p, int32_t aov_samples, const rtk_denoise_opts* opts, double* h_out_linear, uint8_t* h_out_rgb8);

/* Guides that follow mirrors ---------------------------------------------------------
 * First-hit guides give everything seen in a mirror one albedo, one smooth normal and one smooth depth.  rtk_render_guides
 * writes 16 floats per pixel, d_guides[(j*W+i)*16 + k]:
 *   k 0-7   set 1: exactly what rtk_render_aovs writes for the same camera, seed, real mode and n_samples (bit-identical)
 *   k 8-10  seen albedo, mean over the n samples      k 11     end-hit fraction
 *   k 12-14 end normal summed over end hits, / n      k 15     mean over end hits of the path length
 * Per sample s of pixel (i, j), in the real mode's type:  ray_0 = the render's primary ray, T = (1, 1, 1), len = 0;  for
 * b = 0, 1, ...: hit_b = the closest hit of ray_b on interval(0.001, inf), a constant medium drawing from the stream of keys
 * (seed, j*W+i, 2^31 + ((2b) << 20) + s) (b = 0 is rtk_render_aovs' key).  A miss adds T * clamp01(background) to the seen
 * albedo and ends the sample without an end hit.  Otherwise len += t_b |rd_b|; the hit material is FOLLOWED when
 * (follow & RTK_GUIDE_FOLLOW_MIRROR and it is a metal with fuzz 0) or (follow & RTK_GUIDE_FOLLOW_DIELECTRIC and it is a
 * dielectric).  A followed hit with b < max_bounces runs material::scatter (as rtk_debug_scatter does) with the stream of keys
 * (seed, j*W+i, 2^31 + ((2b+1) << 20) + s); if it scatters, T = T * attenuation, ray_{b+1} = the scattered ray (time kept)
 * and the chain goes on.  Every other hit is the END HIT: seen albedo += T * (rtk_render_aovs' albedo rule at hit_b), end
 * normal += the record's normal (isotropic: 0), path length += len.  Sums run in sample order and are divided once (k 15 by
 * the end hits), then rounded to float.  Where nothing is followed, k 8-15 equal k 0-7 bit for bit.
 * Options (NULL = defaults): follow 0 = RTK_GUIDE_FOLLOW_MIRROR, other bits RTK_ERR_INVALID (glass is followed by the
 * render's own reflect / refract lottery: noisy at few samples, hence opt-in); max_bounces 0 = 4, else 1..8.
 * n_samples 1 .. 2^20.  Otherwise the rules of rtk_render_aovs: whole images only, asynchronous on opts->stream, _host blocks.
 * Alignment: d_guides must be 16-byte aligned, as d_aov must -- rtk_render_guides and rtk_denoise_guided refuse another pointer
 * with RTK_ERR_INVALID (the text names d_guides), nothing launched or written; every other device buffer needs only the
 * alignment of its element type.
 *
 * rtk_denoise_guided is rtk_denoise's iteration (taps, h, tap order, w_l, variance propagation, output conversion) with
 *   w_n = min(w_n of set 1, w_n of set 2), w_z = min(w_z of set 1, w_z of set 2) -- each w_z with its own set's hit fraction,
 *   depth and depth gradient (k 3 / 7 and k 11 / 15) -- and w_a on the SEEN albedo (k 8-10).
 * With set 2 == set 1 every weight is rtk_denoise's and the output is bit-identical to it.
 * flags & RTK_DENOISE_DEMODULATE: the filter runs on irradiance.  Before the first iteration A = max(seen albedo, 0.02) per
 * channel, c' = c / A, var' = var / ((A.x + A.y + A.z) / 3)^2; w_a = 1 (sigma_a is ignored); after the last iteration
 * out = c' * A, then the usual conversion.  It keeps textures sharp where the guide albedo matches the colour (a textured wall:
 * the error falls by half) and loses where few-pixel objects give a 4-sample albedo that does not (book1_final): off by default.
 * Other flag bits give RTK_ERR_INVALID.  Outputs may alias d_linear or d_noise but not d_guides. */
#define RTK_GUIDE_FOLLOW_MIRROR 1
#define RTK_GUIDE_FOLLOW_DIELECTRIC 2
#define RTK_DENOISE_DEMODULATE 1
typedef struct rtk_guide_opts {
    int32_t follow;       /* RTK_GUIDE_FOLLOW_* bits; 0 = RTK_GUIDE_FOLLOW_MIRROR */
    int32_t max_bounces;  /* 0 = 4, else 1..8 */
} rtk_guide_opts;

int rtk_render_guides(rtk_ctx* ctx, const rtk_camera* cam, const rtk_render_opts* opts, int32_t n_samples, const rtk_guide_opts* gopts, float* d_guides);
int rtk_render_guides_host(rtk_ctx* ctx, const rtk_camera* cam, const rtk_render_opts* opts, int32_t n_samples, const rtk_guide_opts* gopts, float* h_guides);
int rtk_denoise_guided(rtk_ctx* ctx, int32_t width, int32_t height, int32_t real_mode, const void* d_linear, const float* d_guides, const float* d_noise,
                       const rtk_denoise_opts* opts, int32_t flags, void* d_out_linear, uint8_t* d_out_rgb8, void* stream);
int rtk_denoise_guided_host(rtk_ctx* ctx, int32_t width, int32_t height, int32_t real_mode, const double* h_linear, const float* h_guides,
                            const float* h_noise, const rtk_denoise_opts* opts, int32_t flags, double* h_out_linear, uint8_t* h_out_rgb8);
/* rtk_progressive_denoise with followed guides: the guides of the session's camera and seed are rendered on first use and kept
 * per (aov_samples, follow, max_bounces) on the session (not in checkpoints); the session is otherwise unchanged. */
int rtk_progressive_denoise_guided(rtk_progressive* p, int32_t aov_samples, const rtk_guide_opts* gopts, const rtk_denoise_opts* opts, int32_t flags,
                                   void* d_out_linear, uint8_t* d_out_rgb8);
int rtk_progressive_denoise_guided_host(rtk_progressive* p, int32_t aov_samples, const rtk_guide_opts* gopts, const rtk_denoise_opts* opts, int32_t flags,
                                        double* h_out_linear, uint8_t* h_out_rgb8);

/* Temporal accumulation ---------------------------------------------------------------
 * The temporal half of SVGF (Schied et al. 2017): an rtk_temporal object carries the frames of a MOVING camera along.  Per frame
 * the caller renders a noisy frame with its se (a progressive step of at least two full chunks), the guides of the same camera
 * (rtk_render_guides) and calls rtk_temporal_accumulate; the object reprojects the frame it returned last time into the new
 * camera, rejects history that belongs to another surface, blends, and carries the variance along, so rtk_denoise_guided on the
 * outputs keeps working on honest numbers.  The object owns its history (ping-pong, 52 bytes per pixel each) in device memory,
 * apart from the render workspace and the denoiser's buffers; it is bound to the stream given at creation (the stream rules of
 * rtk_render_device: every launch goes there, the call reads cam / opts before it returns and never waits for the device;
 * create and reset do not touch the device's queues at all).
 *   d_linear  H*W*3 reals of real_mode (read as such, then rounded to float); d_guides H*W*16 floats from rtk_render_guides of
 *             `cam`; d_noise H*W floats (se; required)
 *   outputs   d_out_linear H*W*3 reals of real_mode, d_out_noise H*W floats, d_out_rgb8 H*W*3 bytes, d_out_history H*W floats;
 *             any may be NULL; they may alias d_linear / d_noise (a pixel's inputs are read before its outputs are written and
 *             the taps read the object's own memory), but not d_guides.  Whole images only.
 *   alignment d_guides must be 16-byte aligned (read 16 bytes at a time); every other device buffer needs only the alignment of
 *             its element type.
 * The rule, per pixel (i, j) with colour c (float), se and guides g[0..15]; primes mark the previous frame's values:
 *   1. Start of a history: the first frame after create / reset, and any pixel whose first-hit fraction g[3] == 0 (the
 *      background is a constant): out = c, var_out = se^2, n_out = 1.
 *   2. Reprojection, in double for both real modes: d = pixel00_loc + i du + j dv - center, P = center + g[7] d / |d|,
 *      q = P - center', (u, v, w) = M'^-1 q with M'^-1 = rtk_temporal_reproject_matrix(previous camera), computed once per frame
 *      on the host.  w <= 0: no history (a start).  x = u / w, y = v / w, z_exp = |q|.
 *   3. Taps (x0 + a, y0 + b), a, b in {0, 1}, b outer: x0 = floor(x), fx = x - x0 (the same in y), bilinear weight
 *      omega = (a ? fx : 1 - fx)(b ? fy : 1 - fy) rounded to float.  A tap is valid iff it lies in the image, its g'[3] > 0,
 *      |g'[7] - z_exp| <= depth_tol z_exp (in double), the normals g[4..6] and g'[4..6] are both zero or neither is and their
 *      cosine >= normal_cos, and -- with RTK_TEMPORAL_CHECK_ALBEDO -- max over channels |g[8..10] - g'[8..10]| <= albedo_tol.
 *   4. Over the valid taps Omega = sum omega; Omega < 1e-3 is a start.  Otherwise c_h = sum omega c' / Omega,
 *      var_h = sum omega^2 var' / Omega^2, n_h = sum omega n' / Omega, n_out = min(n_h + 1, max_history), alpha = 1 / n_out,
 *      out = (1 - alpha) c_h + alpha c, var_out = (1 - alpha)^2 var_h + alpha^2 se^2.  c', var' and n' are the previous frame's
 *      OUTPUTS as float32: the history is what was returned, before any spatial filter.
 *   5. d_out_linear = out, d_out_noise = sqrt(var_out), d_out_history = n_out, d_out_rgb8 = the resolve's gamma / clamp /
 *      quantise of out, in double.  Colour arithmetic is float32, no atomics, a fixed tap order: the same inputs give the same
 *      bits.
 * Options (NULL = defaults; a 0 field takes its default): max_history 32 (1..1024), depth_tol 0.02, normal_cos 0.9, albedo_tol
 * 0.25.  RTK_ERR_INVALID, with nothing written and the history and frame count untouched: a camera whose size is not the
 * object's, negative or non-finite tolerances, normal_cos > 1, unknown flags, reserved != 0, max_history out of range, a null
 * object, camera or input, a d_guides that is not 16-byte aligned (the text names it).  Options are checked first (they need no object).
 * Limits: geometry is taken as static -- moving spheres are time-averaged within every frame and accumulate like anything else;
 * what a mirror shows is reprojected with the mirror's own surface: the opt-in check on the SEEN albedo is the available guard
 * and max_history bounds the lag.
 * rtk_temporal_accumulate is asynchronous on the object's stream; the _host form (h_linear / h_out_linear doubles, F32 rounded /
 * widened) blocks.  rtk_temporal_reset makes the next frame start a new history.  rtk_temporal_frames = frames accumulated since
 * create / reset (negative rtk_status for a null object). */
#define RTK_TEMPORAL_CHECK_ALBEDO 1
typedef struct rtk_temporal rtk_temporal;
typedef struct rtk_temporal_opts {
    int32_t max_history;   /* 0 = 32; else 1..1024 */
    float depth_tol;       /* 0 = 0.02 */
    float normal_cos;      /* 0 = 0.9  */
    float albedo_tol;      /* 0 = 0.25; used only with RTK_TEMPORAL_CHECK_ALBEDO */
    int32_t flags;         /* RTK_TEMPORAL_CHECK_ALBEDO; other bits RTK_ERR_INVALID */
    int32_t reserved;      /* 0 */
} rtk_temporal_opts;

int rtk_temporal_create(rtk_ctx* ctx, int32_t width, int32_t height, int32_t real_mode, void* stream, rtk_temporal** out);
int rtk_temporal_accumulate(rtk_temporal* t, const rtk_camera* cam, const void* d_linear, const float* d_guides, const float* d_noise,
                            const rtk_temporal_opts* opts, void* d_out_linear, float* d_out_noise, uint8_t* d_out_rgb8, float* d_out_history);
int rtk_temporal_accumulate_host(rtk_temporal* t, const rtk_camera* cam, const double* h_linear, const float* h_guides, const float* h_noise,
                                 const rtk_temporal_opts* opts, double* h_out_linear, float* h_out_noise, uint8_t* h_out_rgb8, float* h_out_history);
int rtk_temporal_reset(rtk_temporal* t);
int rtk_temporal_frames(const rtk_temporal* t);
int rtk_temporal_destroy(rtk_temporal* t);
/* Host-only, no device: out[0..8] = the inverse (row-major) of the matrix whose COLUMNS are pixel_delta_u, pixel_delta_v and
 * pixel00_loc - center; out[9..11] = center.  A point center + q is seen at pixel (u / w, v / w), (u, v, w) = out[0..8] q, when
 * w > 0.  RTK_ERR_INVALID for a singular camera. */
int rtk_temporal_reproject_matrix(const rtk_camera* cam, double out[12]);

/* Guided upsampling -------------------------------------------------------------------
 * Joint-bilateral upsampling (Kopf et al. 2007): the noisy frame is rendered at 1/f of the width and height -- with f^2 times the
 * samples per pixel for the same budget, or the same samples in 1/f^2 of the time -- the guides at both resolutions
 * (rtk_render_guides costs a fraction of a frame), and rtk_upsample rebuilds the full-resolution frame from the low-resolution
 * colour, steered by both guide sets: edges, normals, depth and -- demodulated -- textures come back at full resolution.
 *
 * rtk_upsample_camera (host-only, no device): the low camera of `full` for factor f = 2..4.  With W, H the full size:
 * image_width = ceil(W / f), image_height = ceil(H / f), pixel_delta_u / v = f * full's, pixel00_loc = full.pixel00_loc +
 * ((f - 1) / 2)(du + dv), in double; every other field is copied.  The centre of low pixel (I, J) is then the mean of the centres
 * of full pixels fI .. fI+f-1 by fJ .. fJ+f-1, and the low pixel's sample square is exactly those f x f full pixels' squares.
 * RTK_ERR_INVALID, with out_low untouched, for a null pointer, a factor outside 2..4 or a camera with non-positive size.
 *
 * rtk_upsample, with W x H = full's size, LW x LH = the low camera's:
 *   d_low_linear  LH*LW*3 reals of real_mode (read as such, then rounded to float); d_low_noise LH*LW floats (se);
 *                 d_low_guides LH*LW*16 floats from rtk_render_guides of the low camera; d_guides H*W*16 floats from
 *                 rtk_render_guides of `full`.  All four are required.
 *   outputs       d_out_linear H*W*3 reals of real_mode, d_out_noise H*W floats, d_out_rgb8 H*W*3 bytes, d_out_support H*W
 *                 floats; any may be NULL, not all.  They may not alias an input.  Whole images only.
 *   alignment     d_low_guides and d_guides must be 16-byte aligned (read 16 bytes at a time); every other device buffer needs
 *                 only the alignment of its element type.
 * The rule, per full pixel (i, j) with guides g[0..15]; a low pixel has guides G[0..15], colour c (float) and standard error se:
 *   1. Position, in integers: n = 2i - (f - 1), x0 = floor(n / 2f), fx = float(n - 2f x0) / float(2f); the same in j for y0, fy.
 *      Taps (x0 + a, y0 + b), a, b in {0, 1}, b outer; a tap outside the low image is skipped.  Bilinear weight
 *      beta = (a ? fx : 1 - fx)(b ? fy : 1 - fy) in float.  The taps inside the image always carry sum beta >= 0.39: no pixel
 *      is without taps.
 *   2. Weight w = w_n w_z w_a with rtk_denoise_guided's expressions, p = the full pixel, q = the tap:
 *      w_n = min over the two guide sets (k 4-6 / k 12-14) of: 1 if both normals are 0, 0 if one is, else max(0, cos)^sigma_n;
 *      w_z = min over the two sets (hit fraction k 3 / 11, depth k 7 / 15) of: 1 if either hit fraction is 0, else
 *            exp(-|z_p - z_q| / (sigma_z (grad_p o + 1e-3 z_p) + 1e-6)), grad_p = half the larger central difference of the
 *            FULL-resolution depth at p (edges clamped), o = f sqrt((fx - a)^2 + (fy - b)^2), the tap's distance in full pixels;
 *      w_a = exp(-|g[8..10] - G[8..10]| / sigma_a) (Euclidean), or 1 with RTK_UPSAMPLE_DEMODULATE.
 *   3. Blend: omega = beta (w + 1e-3); Omega = sum omega; out = sum omega c_q / Omega; var_out = sum omega^2 se_q^2 / Omega^2;
 *      support = sum beta w / sum beta, the share of the bilinear weight the guides accepted.  The floor 1e-3 makes a pixel
 *      whose taps are all rejected fall back smoothly to the (edge-renormalised) bilinear interpolation; there is no threshold.
 *      A caller can re-render pixels with low support (whole tiles with the render kernel: "Tile lists" below; single pixels
 *      with rtk_query_radiance and the frame's own streams: INTEGRATION 4g).
 *   4. RTK_UPSAMPLE_DEMODULATE: per tap A_q = max(G[8..10], 0.02) per channel, c_q <- c_q / A_q, se_q^2 <- se_q^2 /
 *      ((A_q.x + A_q.y + A_q.z) / 3)^2; after the blend out <- out * A_p, var_out <- var_out * mean(A_p)^2, A_p from g[8..10].
 *   5. d_out_linear = out, d_out_noise = sqrt(var_out), d_out_support = support, d_out_rgb8 = the resolve's gamma / clamp /
 *      quantise of out, in double.  Arithmetic is float32, no atomics, a fixed tap order: the same inputs give the same bits.
 *      Neighbouring output pixels share taps: d_out_noise is a per-pixel marginal, the errors of neighbours are correlated.
 * Options (NULL = defaults; a 0 field takes its default): factor 2 (2..4), sigma_n 128, sigma_z 1, sigma_a 0.1 (the denoiser's).
 * RTK_ERR_INVALID, with nothing written: a factor outside 2..4, unknown flags, reserved != 0, negative or non-finite sigmas
 * (these are checked first and need no context or device), a null context, camera or input, all outputs null, a camera with
 * non-positive size, an unknown real_mode, a d_low_guides or d_guides that is not 16-byte aligned (the text names the argument).
 * rtk_upsample is asynchronous on `stream` under the stream rules of rtk_render_device: its one launch goes there, `full` and
 * opts are read before it returns, it allocates nothing, uses no context workspace and never waits for the device.
 * rtk_upsample_host (h_low_linear / h_out_linear doubles, F32 rounded / widened) blocks.
 * Limits: geometry thinner than a low pixel's footprint may be missed by every low sample that could colour it; a low pixel that
 * straddles the border of an emitter has a colour no full pixel has, and only w_a tells a light from the wall it lies in (none
 * with RTK_UPSAMPLE_DEMODULATE); a 4-sample albedo at a texture edge demodulates with a value the colour does not have; what a
 * mirror shows is steered by the second guide set only as far as the guides follow it (rtk_guide_opts), as for the filter. */
#define RTK_UPSAMPLE_DEMODULATE 1
typedef struct rtk_upsample_opts {
    int32_t factor;        /* 0 = 2; else 2..4 */
    float sigma_n, sigma_z, sigma_a;   /* 0 = the denoiser's defaults: 128, 1, 0.1 */
    int32_t flags;         /* RTK_UPSAMPLE_DEMODULATE; other bits RTK_ERR_INVALID */
    int32_t reserved;      /* 0 */
} rtk_upsample_opts;

int rtk_upsample_camera(const rtk_camera* full, int32_t factor, rtk_camera* out_low);
int rtk_upsample(rtk_ctx* ctx, const rtk_camera* full, int32_t real_mode, const void* d_low_linear, const float* d_low_noise, const float* d_low_guides,
                 const float* d_guides, const rtk_upsample_opts* opts, void* d_out_linear, float* d_out_noise, uint8_t* d_out_rgb8, float* d_out_support,
                 void* stream);
int rtk_upsample_host(rtk_ctx* ctx, const rtk_camera* full, int32_t real_mode, const double* h_low_linear, const float* h_low_noise, const float* h_low_guides,
                      const float* h_guides, const rtk_upsample_opts* opts, double* h_out_linear, float* h_out_noise, uint8_t* h_out_rgb8, float* h_out_support);

/* Display transform -------------------------------------------------------------------
 * Between a linear frame and its pixels: every other rgb8 output of this header is the reference's conversion (sqrt, clamp to
 * 0.999, quantise), which clips wherever a light of radiance 7..15 or its first bounce is seen.  An rtk_display object meters
 * the frame, adapts an exposure over the frames of a moving camera, optionally adds bloom, and applies a tone curve and an
 * encoding.  It is bound to a context, a size, a real mode and a stream at creation (the stream rules of rtk_render_device:
 * every launch goes there, opts are read before the call returns, the call never waits for the device); it owns its device
 * memory (the exposure, two histograms; with bloom a pyramid of about 9.3 bytes per pixel, allocated by the first call that
 * asks for bloom).  The exposure goes from the metering kernel to the kernels that use it through device memory: there is no
 * host round trip.  No other rgb8 output changes.
 *   d_linear  H*W*3 reals of real_mode; outputs d_out_linear H*W*3 reals of real_mode, d_out_rgb8 H*W*3 bytes; either may be
 *             NULL, not both; they may alias d_linear.  Whole images only.
 * The rule, for the W x H image with colour c in the real mode's type:
 *   1. Sanitise, per channel: NaN and values <= 0 become 0, values > 65504 become 65504.
 *   2. Luminance for metering, in float32: the sanitised channels rounded to float32, y = (0.2126f r + 0.7152f g) + 0.0722f b,
 *      each product and sum rounded on its own (no fma).
 *   3. Histogram, in integers: a pixel with y < 2^-20 is black and not counted; any other is counted in bin
 *      min(bits(y) >> 20, 1175) - 856: 320 bins, 8 per octave from 2^-20 to 2^20, from the exponent and the top three mantissa
 *      bits.  Counts are uint32 and do not depend on the order of arrival.
 *   4. Metering, in double: N = the sum of the counts, lo = meter_low N, hi = meter_high N.  Over the bins in index order with
 *      the running count C_k, bin k has the mass m_k = max(0, min(C_k, hi) - max(C_{k-1}, lo)); L = sum m_k lambda_k / sum m_k
 *      with lambda_k = e + log2(1 + (m + 0.5) / 8), e = floor(k / 8) - 20 the bin's octave and m = k mod 8 its sub-bin;
 *      E_target = clamp(key / 2^L, min_exposure, max_exposure).  N = 0: E_target = the previous E, or 1 on a first frame.
 *   5. Adaptation: on the first frame after create / reset, or with adapt = 1, E = E_target; otherwise
 *      E = E_prev (E_target / E_prev)^adapt, a blend in the log domain.  With a manual exposure (opts.exposure > 0) steps 2-4
 *      are skipped, E = E_target = that value, and it becomes E_prev.
 *   6. Scale: s = E x in the real mode's type (E rounded to it).  E = 1 leaves the bits alone.
 *   7. Bloom, in float32, only when bloom > 0, with n = bloom_levels: T_0 = max(s - bloom_threshold, 0) per channel.  For
 *      k = 1..n level k has ceil(half) the previous size in each axis; D_k(i, j) = ((a + b) + (c + d)) / 4 over the 2x2 block
 *      of T_{k-1} at columns 2i, 2i+1 (a, b: row 2j; c, d: row 2j+1), indices clamped to the edge; T_k = D_k under the
 *      separable tent ((l + 2 m) + r) / 4, horizontal then vertical, edges clamped.  Upwards U_n = T_n,
 *      U_k = T_k + bilinear(U_{k+1}); the bloom image is B = bilinear(U_1) / n.  bilinear samples a half-size level at centred
 *      pixels: for the target index i, m = 2i - 1, x0 = floor(m / 4), fx = (m - 4 x0) / 4, taps x0 and x0 + 1 clamped to the
 *      level, value (1 - fx) p + fx q; the same in y, y outer.  s' = s + bloom B.  A constant bright image blooms to the same
 *      constant (B = T_0).
 *   8. Curve, in the real mode's type: RTK_DISPLAY_CLAMP t = s'; RTK_DISPLAY_REINHARD t = s' (1 + Y / white^2) / (1 + Y) with
 *      Y = (0.2126 r + 0.7152 g) + 0.0722 b of s'; RTK_DISPLAY_ACES (Narkowicz 2015) per channel
 *      t = clamp(x (2.51 x + 0.03) / (x (2.43 x + 0.59) + 0.14), 0, 1).
 *   9. Encode: d_out_linear = t.  RTK_DISPLAY_GAMMA2 bytes are the resolve's gamma / clamp / quantise of double(t);
 *      RTK_DISPLAY_SRGB: g = t <= 0.0031308 ? 12.92 t : 1.055 t^(1/2.4) - 0.055 in double, clamped to [0, 0.999], byte =
 *      uint8(int(255.999 g)).
 * The anchor: with exposure = 1, CLAMP, GAMMA2 and no bloom, d_out_rgb8 is the resolve's own rgb8 of the same linear image,
 * byte for byte, in both real modes.  No float atomics, fixed orders: the same inputs give the same bits.
 * Options (NULL = defaults; a 0 field takes its default): exposure 0 = metered, key 0.18, meter_low 0.10 and meter_high 0.90
 * (0 < low < high <= 1), min_exposure 2^-10, max_exposure 2^10, adapt 1 (0 < adapt <= 1), curve CLAMP, white 4 (REINHARD),
 * encode GAMMA2, bloom 0 = off, bloom_threshold 1, bloom_levels 4 (1..6).  RTK_ERR_INVALID, naming the field, with nothing
 * written and the object's state and frame count untouched: a negative or non-finite field, meter_low >= meter_high,
 * meter_high > 1, min_exposure > max_exposure, adapt > 1, an unknown curve or encode, bloom_levels out of range,
 * reserved != 0 (these are checked first and need no object), a null object or input, both outputs null.
 * rtk_display_apply is asynchronous on the object's stream; the _host form (doubles, F32 rounded / widened) blocks.
 * rtk_display_exposure blocks: out = {E, E_target} of the last apply ({1, 1} before the first apply after create / reset).
 * rtk_display_histogram blocks: the histogram of the last metered apply (zeros before one).  rtk_display_reset makes the next
 * frame a first frame; rtk_display_frames = applies since create / reset (negative rtk_status for a null object). */
#define RTK_DISPLAY_CLAMP 0
#define RTK_DISPLAY_REINHARD 1
#define RTK_DISPLAY_ACES 2
#define RTK_DISPLAY_GAMMA2 0
#define RTK_DISPLAY_SRGB 1
#define RTK_DISPLAY_BINS 320
typedef struct rtk_display rtk_display;
typedef struct rtk_display_opts {
    float exposure;                     /* 0 = metered; > 0 sets E and skips the metering pass */
    float key;                          /* 0 = 0.18 */
    float meter_low, meter_high;        /* 0 = 0.10, 0.90; 0 < low < high <= 1 */
    float min_exposure, max_exposure;   /* 0 = 2^-10, 2^10 */
    float adapt;                        /* 0 = 1; else (0, 1] */
    int32_t curve;                      /* RTK_DISPLAY_CLAMP / REINHARD / ACES */
    float white;                        /* 0 = 4; REINHARD only */
    int32_t encode;                     /* RTK_DISPLAY_GAMMA2 / SRGB */
    float bloom;                        /* 0 = off; strength */
    float bloom_threshold;              /* 0 = 1 */
    int32_t bloom_levels;               /* 0 = 4; else 1..6 */
    int32_t reserved;                   /* 0 */
} rtk_display_opts;

int rtk_display_create(rtk_ctx* ctx, int32_t width, int32_t height, int32_t real_mode, void* stream, rtk_display** out);
int rtk_display_apply(rtk_display* d, const void* d_linear, const rtk_display_opts* opts, void* d_out_linear, uint8_t* d_out_rgb8);
int rtk_display_apply_host(rtk_display* d, const double* h_linear, const rtk_display_opts* opts, double* h_out_linear, uint8_t* h_out_rgb8);
int rtk_display_exposure(rtk_display* d, double out[2]);
int rtk_display_histogram(rtk_display* d, uint32_t out[320]);
int rtk_display_reset(rtk_display* d);
int rtk_display_frames(const rtk_display* d);
int rtk_display_destroy(rtk_display* d);

/* Ray queries -------------------------------------------------------------------------
 * Hits, occlusion and radiance for rays the CALLER chooses -- light probes, lightmaps, picking, line-of-sight tests, other
 * projections, re-rendering chosen pixels: what the reference offers as world.hit(r, interval, rec) and ray_color (hittable.h:33,
 * Camera.txt:203-238).  Device resident and asynchronous on opts->stream, on the uploaded scene in either visiting order and both
 * real modes; one rank only (not through rtk_multi).  The kernels walk the slot program one lane per ray, with every record
 * kind, through the device functions the render kernel runs.
 *
 * Streams of random numbers: a ray's stream is keyed (opts->seed, ray.pixel, ray.sample) -- state pcg_hash(pixel +
 * pcg_hash(sample + pcg_hash(seed))), the keying of the rtk_debug_* entry points and of the render's samples -- and then
 * advanced by ray.skip draws (a jump of at most 32 squarings of the generator's step: any skip costs the same).  skip lets a
 * path continue where the caller's ray generation left the stream: for a camera ray, skip = rtk_debug_get_ray's h_draws, and
 * the query continues the render's own stream of that pixel and sample.
 *
 * rtk_query_hits      hittable::hit(r, interval(ray.tmin, ray.tmax), rec) of the scene root; a constant medium draws from the
 *                     ray's stream.  With skip = 0 it is rtk_debug_closest_hit, bit for bit.  prim_kind / prim_index name the
 *                     primitive in the tables of the rtk_scene_desc that was uploaded (rtk_scene_optimize borrows them unchanged,
 *                     so both visiting orders report the same; a primitive reached through several instances reports one index).
 *                     A constant medium's record has u = v = 0 (the reference leaves them as the record held them); an
 *                     empty interval, tmin > tmax, is a miss.
 * rtk_query_occluded  d_occluded[k] = the hit flag rtk_query_hits returns for the same ray, keys and skip, exactly.  In a scene
 *                     without a constant_medium the walk stops at the first accepted hit; with one it is the closest-hit walk.
 * rtk_query_radiance  ray_color(r, opts->max_depth, world, lights) with opts->background: world.hit on interval(0.001, inf)
 *                     and the shading of the render kernels, point lights included, until the path ends; ray.tmin / tmax are
 *                     ignored, as ray_color ignores them.  Sample s = 0 .. samples-1 of ray k draws from the stream (seed,
 *                     pixel, sample + s) advanced by skip; d_radiance[k] = the sum in sample order, divided once by the number
 *                     of samples, [n][3] reals of real_mode.  d_draws (may be NULL) [n]: the uniforms the paths of ray k drew,
 *                     skip not counted; giving it selects a counting build of the kernel.
 * Buffers: every buffer needs the alignment of its element type -- 8 bytes for rtk_ray, rtk_ray_hit and F64 reals, 4 otherwise;
 * a misaligned pointer is refused (the text names the argument) and nothing is launched.  Outputs may not alias d_rays: an
 * output whose range overlaps the rays' is refused likewise.  rtk_ray.reserved is not read today; set it to 0.
 * n == 0 is valid and launches nothing.  RTK_ERR_INVALID, checked first and without a device: a null context, opts, rays or
 * output; n < 0 or n > 2^31 - 1; an unknown real_mode; negative max_depth or samples; reserved != 0.  RTK_ERR_NO_SCENE
 * without an uploaded scene.  The stream rules of rtk_render_device hold: every launch goes to opts->stream, opts is read before
 * the call returns, the call allocates nothing and never waits for the device.  The _host forms take host buffers (h_radiance
 * doubles, F32 widened) and block. */
typedef struct rtk_ray {                 /* 88 bytes, 8-byte aligned */
    double origin[3], direction[3], time, tmin, tmax;
    uint32_t pixel, sample;              /* stream keys: the ray's random stream is (opts.seed, pixel, sample) */
    uint32_t skip;                       /* uniforms of that stream the caller has already consumed */
    uint32_t reserved;                   /* 0 */
} rtk_ray;

typedef struct rtk_ray_hit {             /* 96 bytes */
    double t, p[3], normal[3], u, v;     /* the hit record; F32 results widened; all 0 on a miss */
    int32_t hit, front_face, material;   /* material -1 on a miss */
    int32_t prim_kind, prim_index;       /* RTK_NODE_SPHERE / QUAD / TRIANGLE / MEDIUM and the index into spheres[] / quads[] /
                                          * triangles[] / media[]; 0, -1 on a miss */
    int32_t draws;                       /* random_double() calls inside hit() (skip not counted) */
} rtk_ray_hit;

typedef struct rtk_query_opts {          /* 56 bytes */
    uint32_t seed; int32_t real_mode;
    int32_t max_depth;                   /* radiance only; >= 0, as rtk_camera.max_depth (0 = black) */
    int32_t samples;                     /* radiance only; 0 = 1 */
    rtk_vec3 background;                 /* radiance only */
    void* stream;
    int32_t reserved[2];                 /* 0 */
} rtk_query_opts;

int rtk_query_hits(rtk_ctx* ctx, const rtk_query_opts* opts, int64_t n, const rtk_ray* d_rays, rtk_ray_hit* d_hits);
int rtk_query_occluded(rtk_ctx* ctx, const rtk_query_opts* opts, int64_t n, const rtk_ray* d_rays, int32_t* d_occluded);
int rtk_query_radiance(rtk_ctx* ctx, const rtk_query_opts* opts, int64_t n, const rtk_ray* d_rays, void* d_radiance, uint32_t* d_draws);
int rtk_query_hits_host(rtk_ctx* ctx, const rtk_query_opts* opts, int64_t n, const rtk_ray* h_rays, rtk_ray_hit* h_hits);
int rtk_query_occluded_host(rtk_ctx* ctx, const rtk_query_opts* opts, int64_t n, const rtk_ray* h_rays, int32_t* h_occluded);
int rtk_query_radiance_host(rtk_ctx* ctx, const rtk_query_opts* opts, int64_t n, const rtk_ray* h_rays, double* h_radiance, uint32_t* h_draws);

/* Light probes ------------------------------------------------------------------------
 * Baked diffuse lighting on top of the radiance query: a probe is a point that looks along a fixed sphere of directions, and
 * what it sees is kept as nine spherical-harmonic coefficients per colour channel.  rtk_probe_bake makes the rays where they are
 * used and reduces them where they land (one workgroup per probe); rtk_probe_irradiance turns a grid of probes into irradiance
 * at points with normals.  Device resident and asynchronous, on the uploaded scene in either visiting order and both real modes.
 *
 * Basis: the real spherical harmonics up to l = 2 of a unit direction (x, y, z), in this order and with these constants:
 *   Y0 = 0.28209479177387814          Y1 = 0.4886025119029199 y          Y2 = 0.4886025119029199 z
 *   Y3 = 0.4886025119029199 x         Y4 = 1.0925484305920792 x y        Y5 = 1.0925484305920792 y z
 *   Y6 = 0.31539156525252005 (3 z^2 - 1)   Y7 = 1.0925484305920792 x z   Y8 = 0.5462742152960396 (x^2 - y^2)
 * Directions: a probe with R = opts->rays rays looks along d_j, j = 0 .. R-1, the same for every probe, computed in double with
 * no fused operation and not renormalised:  z_j = 1 - (2j + 1) / R;  u_j = (j * 2654435769) mod 2^32;  phi_j = double(u_j) *
 * (2 pi 2^-32);  r_j = sqrt(1 - z_j z_j);  d_j = (r_j cos phi_j, r_j sin phi_j, z_j)  (a spherical Fibonacci set).
 * Rays and streams: with S = samples per ray, ray j of probe k is the record { origin = the probe's position, direction = d_j,
 * time = opts->time, tmin = 0.001, tmax = +inf, pixel = first_key + k (32-bit wrap), sample = j * S, skip = 0 } -- what
 * rtk_probe_rays writes, [n * rays] records, probe-major -- and its radiance L_kj is what rtk_query_radiance returns for that
 * record with samples = S and the call's seed, max_depth and background.
 * Coefficients (of radiance): c[k][i][ch] = (4 pi / R) sum_j L_kj[ch] Y_i(d_j), accumulated in double in both real modes and
 * written as [n][9][3] reals of real_mode.  The sum has a fixed order -- each pass of 256 rays by a fixed tree inside each of the
 * four waves, the passes in increasing j, then the four waves in wave order -- so the same call gives the same bits, and a
 * probe's coefficients do not depend on the other probes of the call.
 * Irradiance at a unit normal n (Ramamoorthi & Hanrahan 2001): E(n)[ch] = sum_i A_i c[i][ch] Y_i(n), A = pi for i = 0, 2 pi / 3
 * for i = 1..3, pi / 4 for i = 4..8.  rtk_probe_irradiance interpolates the coefficients of the eight probes around each point
 * trilinearly (a point outside the grid is clamped to it, an axis with one probe has weight 1) and evaluates E for the normal as
 * given: no normalisation, nothing clamped at zero, no visibility term.  d_sh, d_points, d_normals and d_irradiance hold reals of
 * real_mode; the arithmetic is in that type.
 * Buffers: d_positions [n][3] doubles in both modes, 8-byte aligned; d_rays 8-byte aligned; reals need the alignment of their
 * type (8 bytes in F64, 4 in F32).  A misaligned pointer is refused (the text names the argument) and nothing is launched.
 * n == 0 / m == 0 is valid and launches nothing.  RTK_ERR_INVALID, checked first and without a device: null opts, grid,
 * positions, points, normals or outputs; n or m < 0; n * rays, m or the grid's number of probes over 2^31 - 1; rays not a multiple
 * of 256 in 256 .. 65536; negative max_depth or samples; reserved != 0 (opts and grid); an unknown real_mode; a grid count < 1; a
 * spacing that is not > 0 as a real of real_mode (in F32 a positive double that rounds to 0 is refused); then a null context; then
 * (rtk_probe_bake only) RTK_ERR_NO_SCENE.  rtk_probe_rays and rtk_probe_irradiance need a context for its device but no scene.
 * The stream rules of rtk_render_device hold: every launch goes to the given stream, the call allocates nothing and never waits.
 * The _host forms take host buffers (reals as doubles, F32 widened) and block. */
#define RTK_PROBE_COEFFS 9
typedef struct rtk_probe_opts {          /* 72 bytes */
    uint32_t seed; int32_t real_mode;
    int32_t max_depth;                   /* >= 0 */
    int32_t samples;                     /* paths per ray; 0 = 1 */
    int32_t rays;                        /* per probe; 0 = 1024; a multiple of 256 in 256 .. 65536 */
    uint32_t first_key;                  /* probe k draws from the streams of pixel key first_key + k */
    rtk_vec3 background;
    double time;
    void* stream;
    int32_t reserved[2];                 /* 0 */
} rtk_probe_opts;
typedef struct rtk_probe_grid {          /* 64 bytes: probe (ix, iy, iz) sits at origin + (ix, iy, iz) * spacing,  */
    rtk_vec3 origin, spacing;            /* its coefficients at index (iz * ny + iy) * nx + ix; spacing > 0 per axis */
    int32_t counts[3]; int32_t reserved; /* nx, ny, nz >= 1 */
} rtk_probe_grid;

int rtk_probe_rays(rtk_ctx* ctx, const rtk_probe_opts* opts, int64_t n, const double* d_positions, rtk_ray* d_rays);
int rtk_probe_bake(rtk_ctx* ctx, const rtk_probe_opts* opts, int64_t n, const double* d_positions, void* d_sh);
int rtk_probe_irradiance(rtk_ctx* ctx, int real_mode, const rtk_probe_grid* grid, const void* d_sh, int64_t m, const void* d_points, const void* d_normals,
                         void* d_irradiance, void* stream);
int rtk_probe_rays_host(rtk_ctx* ctx, const rtk_probe_opts* opts, int64_t n, const double* h_positions, rtk_ray* h_rays);
int rtk_probe_bake_host(rtk_ctx* ctx, const rtk_probe_opts* opts, int64_t n, const double* h_positions, double* h_sh);
int rtk_probe_irradiance_host(rtk_ctx* ctx, int real_mode, const rtk_probe_grid* grid, const double* h_sh, int64_t m, const double* h_points,
                              const double* h_normals, double* h_irradiance);

/* Lens models ---------------------------------------------------------------------------
 * Whole frames through other projections than get_ray's pinhole / thin lens: a 360-degree panorama from a point (also an
 * environment map or reflection capture), an equidistant fisheye for domes, an orthographic view for plans and elevations.  The
 * rays are made on the device, one lane per pixel, and traced by the radiance query's path loop; the frame comes with the noise
 * estimate and the guide buffers the denoiser and the display transform take.  Device resident and asynchronous on opts->stream,
 * on the uploaded scene in either visiting order and both real modes; one rank only.  rtk_render_kernel, the scheduler and
 * every other output are untouched.
 *
 * The sample rule.  Sample s = 0 .. S-1 of pixel (i, j) of a W x H frame draws from the stream keyed (seed, j*W+i,
 * first_sample+s) (the keying of the ray queries).
 *   RTK_LENS_PERSPECTIVE is begin_sample -- get_ray, Camera.txt:177-200 -- on lens->cam, unchanged: in the real mode's type, with
 *   the defocus rejection loop, so skip is what rtk_debug_get_ray reports as h_draws.  It reads all of lens->cam and none of the
 *   other fields (model and reserved excepted).
 *   The other three models make three draws and then compute in double in both real modes, with no fused operation and no
 *   renormalisation.  A draw is v * 2^-24 for a 24-bit v, exact in either type.  In order:
 *       oy = draw - 0.5;   ox = draw - 0.5  (y first, as get_ray);   time = draw;   skip = 3
 *   Film coordinates:      x = 2 * ((i + ox) + 0.5) / W - 1        y = 1 - 2 * ((j + oy) + 0.5) / H
 *   EQUIRECT      lon = x * (fov_h / 2), lat = y * (fov_v / 2), c = cos(lat); local direction (c * sin(lon), sin(lat),
 *                 -(c * cos(lon))); origin = cam.center.
 *   FISHEYE       yy = y * (double(H) / double(W)), r = sqrt(x * x + yy * yy), theta = r * (fov_h / 2); local direction
 *                 (sin(theta) * (x / r), sin(theta) * (yy / r), -cos(theta)), or (0, 0, -1) when r == 0; origin = cam.center.
 *                 There is no mask: beyond r = 1 the mapping simply continues, and the caller may mask.
 *   ORTHOGRAPHIC  local direction (0, 0, -1); origin = (center + (x * (ortho_width / 2)) * u) + (y * (ortho_height / 2)) * v,
 *                 per component.
 *   World direction, per component: (lx * u + ly * v) + lz * w, with u, v, w as given (not normalised, not orthogonalised).
 * A record is { origin, direction, time, tmin = 0.001, tmax = +inf, pixel = j*W+i, sample = first_sample+s, skip, reserved = 0 }
 * (rtk_ray).  In RTK_REAL_F32 the ray a lane traces is the record rounded to float, as the ray queries round a caller's record.
 * One device function computes the record; rtk_lens_rays stores it, rtk_lens_render and rtk_lens_aovs / _guides trace it
 * from registers: the bits are the same in all of them.
 *
 * rtk_lens_rays    d_rays[(j*W+i) * n_samples + s] = the record of sample first_sample+s: pixel-major, samples inner.  Needs a
 *                  context but no scene; 8-byte aligned.
 * rtk_lens_render  S = cam.samples_per_pixel samples per pixel.  L_s = what rtk_query_radiance returns for the record of sample
 *                  first_sample+s with samples = 1 and cam.max_depth / cam.background.  d_linear[j][i][0..2] = (the sum of L_s
 *                  in sample order, in the real mode's type) * cam.pixel_samples_scale, reals of real_mode (set the scale to
 *                  1 / S for a mean, as the helpers do).  d_noise (may be NULL) [H][W] floats: with y_s = ((r + g) + b) / 3, the
 *                  channels of L_s widened to double first, S1 = sum y_s and S2 = sum y_s^2 in double in sample order, m = S1 / S,
 *                  v = max(0, (S2 - S m^2) / (S - 1)), se = float(sqrt(v / S)); se = 0 when S < 2 -- the session estimate's
 *                  form, over samples instead of chunks.  No atomics: the result does not depend on the launch geometry.
 * rtk_lens_aovs    the 8 floats per pixel of rtk_render_aovs, and
 * rtk_lens_guides  the 16 floats per pixel of rtk_render_guides, by their rules, with the lens's record for samples
 *                  0 .. n_samples-1 as the primary ray (the same kernel with another sample generator; the first-hit walks draw
 *                  from the keys 2^31 + ... as there).  With RTK_LENS_PERSPECTIVE they are rtk_render_aovs / _guides of lens->cam,
 *                  bit for bit.  d_aov / d_guides must be 16-byte aligned.
 * opts supplies seed, real_mode and stream; n_ranks other than 1 is refused; rank, count_work and variant are ignored.
 * RTK_ERR_INVALID, checked first and without a device, the text naming the argument: a null lens, opts or output; an unknown
 * model; reserved != 0; a camera size outside 1 .. 65536; negative samples_per_pixel (rtk_lens_render needs >= 1) or max_depth;
 * n_samples < 0 (rtk_lens_rays; 0 launches nothing) or < 1 (_aovs, _guides; _guides at most 2^20); first_sample < 0;
 * H * W * n_samples over 2^31 - 1 (rtk_lens_render: H * W * samples_per_pixel); an unknown real_mode; n_ranks != 1; a non-finite
 * real anywhere in the lens, whatever the model; fov_h outside (0, 2 pi] (0 = the default), for EQUIRECT fov_v outside (0, pi]
 * (0 = the default), for ORTHOGRAPHIC ortho_width or ortho_height <= 0; a misaligned buffer; bad rtk_guide_opts.  Then a null context, then (all but rtk_lens_rays) RTK_ERR_NO_SCENE.  The stream rules of rtk_render_device
 * hold: every launch goes to opts->stream, lens and opts are read before the call returns, the call allocates nothing and never
 * waits for the device.  The _host forms take host buffers (h_linear doubles, F32 widened) and block.
 * rtk_lens_look_at (host-only): cam.center = lookfrom, w = unit_vector(lookfrom - lookat), u = unit_vector(cross(vup, w)),
 * v = cross(w, u) (Camera.txt:147-149, the operations of vec3.h in their order); RTK_ERR_INVALID for a null lens. */
#define RTK_LENS_PERSPECTIVE  0   /* get_ray itself (Camera.txt:177-200): the anchor the tests hold the rest to */
#define RTK_LENS_EQUIRECT     1   /* longitude x latitude */
#define RTK_LENS_FISHEYE      2   /* equidistant: angle from the axis proportional to the radius on the film */
#define RTK_LENS_ORTHOGRAPHIC 3
typedef struct rtk_lens {          /* 312 bytes */
    rtk_camera cam;                /* size, samples_per_pixel, max_depth, background, center, pixel_samples_scale; PERSPECTIVE reads all of it */
    int32_t model, reserved;       /* reserved = 0 */
    rtk_vec3 u, v, w;              /* camera frame as Camera.txt:147-149: right, up, back (the view direction is -w); used as given */
    double fov_h, fov_v;           /* radians.  EQUIRECT: extents, 0 = 2 pi and pi.  FISHEYE: fov_h = full angle across the image width, 0 = pi */
    double ortho_width, ortho_height; /* ORTHOGRAPHIC: the window in world units, > 0 */
} rtk_lens;

int rtk_lens_look_at(rtk_lens* lens, rtk_vec3 lookfrom, rtk_vec3 lookat, rtk_vec3 vup);
int rtk_lens_rays(rtk_ctx* ctx, const rtk_lens* lens, const rtk_render_opts* opts, int32_t first_sample, int32_t n_samples, rtk_ray* d_rays);
int rtk_lens_render(rtk_ctx* ctx, const rtk_lens* lens, const rtk_render_opts* opts, int32_t first_sample, void* d_linear, float* d_noise);
int rtk_lens_aovs(rtk_ctx* ctx, const rtk_lens* lens, const rtk_render_opts* opts, int32_t n_samples, float* d_aov);
int rtk_lens_guides(rtk_ctx* ctx, const rtk_lens* lens, const rtk_render_opts* opts, int32_t n_samples, const rtk_guide_opts* gopts, float* d_guides);
int rtk_lens_rays_host(rtk_ctx* ctx, const rtk_lens* lens, const rtk_render_opts* opts, int32_t first_sample, int32_t n_samples, rtk_ray* h_rays);
int rtk_lens_render_host(rtk_ctx* ctx, const rtk_lens* lens, const rtk_render_opts* opts, int32_t first_sample, double* h_linear, float* h_noise);
int rtk_lens_aovs_host(rtk_ctx* ctx, const rtk_lens* lens, const rtk_render_opts* opts, int32_t n_samples, float* h_aov);
int rtk_lens_guides_host(rtk_ctx* ctx, const rtk_lens* lens, const rtk_render_opts* opts, int32_t n_samples, const rtk_guide_opts* gopts, float* h_guides);

/* Tile lists --------------------------------------------------------------------------
 * Render a chosen set of the frame's 8x8 tiles with the render kernel itself: the pixels of the chosen tiles come out with the
 * bits rtk_render_device gives them, at a cost that follows the number of tiles, and every other pixel of the caller's buffers
 * is left alone.  A tile set is an array of rtk_tiles_per_rank(width, height, 1) int32 flags, row-major over the tiles (tile t
 * covers pixels x in 8 (t % tiles_x) .. + 7, y in 8 (t / tiles_x) .. + 7, clipped to the image); a tile is chosen when its flag
 * is non-zero.  One rank only.  New entry points; RTK_ABI_VERSION stays 2.
 *
 * rtk_tiles_select makes a tile set from per-pixel maps (W*H floats each, row-major) -- the support map of rtk_upsample, a
 * noise map, any per-pixel score.  The rule, in integers after two float comparisons per pixel:
 *   1. Raw flags.  An in-image pixel q is raw-flagged when d_below_map is given and !(below_map[q] >= opts->below), or when
 *      d_above_map is given and !(above_map[q] <= opts->above).  A NaN flags; a value equal to its threshold does not; with
 *      both maps the two tests are OR-ed.  Either map may be NULL, not both.
 *   2. Dilation.  With r = opts->dilate (0..8) tile t is flagged -- d_tile_flags[t] = 1, otherwise 0 -- iff some raw-flagged
 *      in-image pixel q lies within r of an in-image pixel p of the tile in both x and y (Chebyshev distance): with the tile's
 *      in-image pixels x0 .. x1, y0 .. y1, iff a raw-flagged q has x0 - r <= q.x <= x1 + r and y0 - r <= q.y <= y1 + r.
 * Every one of the flags is written.  One wave per tile tests the (8 + 2r)^2 window and one ballot decides: no atomics, the
 * same result on every run.  RTK_ERR_INVALID, checked first and without a device, nothing written, the text naming the
 * argument: a width or height outside 1..65536, both maps null, null d_tile_flags or opts, dilate outside 0..8, a non-finite
 * `below` (`above`) when its map is given, reserved != 0, a map or d_tile_flags that is not 4-byte aligned; then a null
 * context.  The stream rules are rtk_upsample's: the one launch goes to `stream`, opts are read before the call returns, it
 * allocates nothing, needs a context for its device but no scene, and never waits for the device.  rtk_tiles_select_host takes
 * host maps, returns host flags and blocks.  sizeof(rtk_tile_select_opts) = 16.
 *
 * rtk_render_tiles renders the flagged tiles of `cam`'s frame.  For every in-image pixel of every tile whose flag is non-zero:
 *   d_linear  (H*W*3 reals of opts->real_mode) and d_rgb8 (H*W*3 bytes) get the values rtk_render_device writes for the same
 *             scene, camera, seed, real mode and variant, bit for bit and byte for byte, in both real modes and both visiting
 *             orders;
 *   d_noise   (H*W floats) gets the standard error a progressive session of the same camera, seed and mode writes after one
 *             step of all samples_per_pixel samples: batch means over the full chunks of the frame's chunk size (the session's
 *             chunk size when samples_per_pixel <= 512, where the two agree), 0 with fewer than two full chunks;
 *   d_support (H*W floats) gets 1.0f -- the pixel is rendered, not interpolated (rtk_upsample's support map).
 * Pixels of unflagged tiles are not written in any buffer.  Any of the four may be NULL, not all.  max_tiles = 0 is no limit;
 * otherwise, when more tiles are flagged than max_tiles, nothing is rendered and nothing is written -- decided on the device,
 * without a host round trip.  d_info (2 int32, may be NULL) = {tiles flagged, tiles rendered}.  The flags are compacted on the
 * device, in ascending tile index, into a list the context owns; the render kernel hands out that list up to its device-side
 * length, and a resolve over the list's positions performs rtk_render_device's additions in its order.  The context's learned
 * tile order is neither used nor changed: a tile render does not change the next full frame's hand-out.
 * RTK_ERR_INVALID, checked without a device and with nothing written or launched: rtk_render_device's own checks of camera and
 * opts (count_work is ignored), null d_tile_flags, max_tiles < 0, all four outputs null, a buffer without the alignment of its
 * element type (the text names it), n_ranks != 1 (or the tile-buffer layout, variant bit 22), and a camera and opts for which
 * rtk_frame_launches() > 1 (more chunks than the workspace holds planes for: 1920x1080 f64 above 168 samples per pixel);
 * then a null context; then RTK_ERR_NO_SCENE.  Allocation and stream behaviour are rtk_render_device's: it may grow context
 * workspace (the partial sums, the list), and every launch goes to opts->stream.
 * rtk_render_tiles_host takes host flags (required) and blocks; h_linear (doubles; F32 rounded / widened), h_rgb8, h_noise and
 * h_support are in-out -- their contents on entry are what unflagged pixels keep -- and any may be NULL, not all; h_info [2]. */
typedef struct rtk_tile_select_opts {
    float below;       /* with d_below_map: pixel q is raw-flagged when !(map[q] >= below) */
    float above;       /* with d_above_map: pixel q is raw-flagged when !(map[q] <= above) */
    int32_t dilate;    /* 0..8 pixels, Chebyshev */
    int32_t reserved;  /* 0 */
} rtk_tile_select_opts;

int rtk_tiles_select(rtk_ctx* ctx, int32_t width, int32_t height, const float* d_below_map, const float* d_above_map, const rtk_tile_select_opts* opts,
                     int32_t* d_tile_flags, void* stream);
int rtk_tiles_select_host(rtk_ctx* ctx, int32_t width, int32_t height, const float* h_below_map, const float* h_above_map, const rtk_tile_select_opts* opts,
                          int32_t* h_tile_flags);
int rtk_render_tiles(rtk_ctx* ctx, const rtk_camera* cam, const rtk_render_opts* opts, const int32_t* d_tile_flags, int32_t max_tiles, void* d_linear,
                     uint8_t* d_rgb8, float* d_noise, float* d_support, int32_t* d_info);
int rtk_render_tiles_host(rtk_ctx* ctx, const rtk_camera* cam, const rtk_render_opts* opts, const int32_t* h_tile_flags, int32_t max_tiles, double* h_linear,
                          uint8_t* h_rgb8, float* h_noise, float* h_support, int32_t* h_info);

/* Surface gathers ---------------------------------------------------------------------
 * Lighting that arrives at points ON surfaces -- the texels of a lightmap, the vertices of a mesh -- and how open each point is:
 * irradiance over the cosine-weighted hemisphere around the point's own normal, and ambient occlusion with the bent normal.
 * The rays are made on the device where they are used; a point's rays are cut into passes of 64 that run as separate waves
 * anywhere on the chip, and a second stage adds the passes in order.  Device resident and asynchronous, on the uploaded scene in
 * either visiting order and both real modes; one rank only.  New entry points; RTK_ABI_VERSION stays 2.
 *
 * Everything below is computed in double with no fused operation, every sum and product left to right as written, and nothing
 * is renormalised.  The normals are used as given: the caller supplies unit normals.
 * Local directions: a cosine-weighted Fibonacci set (Malley's construction over a Fibonacci disc).  For point k and ray
 * j = 0 .. R-1, R = opts->rays:  u_j = (2j + 1) / (2R);  r_j = sqrt(u_j);  z_j = sqrt(1 - u_j);  a_j = (j * 2654435769 + rot_k)
 * mod 2^32;  phi_j = double(a_j) * (2 pi 2^-32);  local direction (x, y, z) = (r_j cos phi_j, r_j sin phi_j, z_j).
 * rot_k = 0 when opts->rotate == 0, else ((first_key + k) mod 2^32) * 0x85EBCA6B mod 2^32, in integers: each point has its own
 * rotation of the set, so neighbouring points do not alias alike.
 * Frame: the branch-free basis of Duff et al. 2017 ("Building an Orthonormal Basis, Revisited").  With normal n:
 *   s = copysign(1, n.z);  a = -1 / (s + n.z);  b = n.x n.y a;
 *   t = (1 + s n.x n.x a, s b, -s n.x);  bt = (b, s + n.y n.y a, -n.y);  world direction d = x t + y bt + z n.
 * Rays and streams: with S = samples per ray, ray j of point k is the record { origin = the point as given (no offset: tmin
 * does that job), direction = d, time = opts->time, tmin = 0.001, tmax = max_distance or +inf, pixel = first_key + k (32-bit
 * wrap), sample = j * S, skip = 0 } -- what rtk_gather_rays writes, [n * R] records, point-major.  L_kj is what
 * rtk_query_radiance returns for that record with samples = S and the call's seed, max_depth and background.
 * Irradiance: E[k][ch] = (pi / R) sum_j L_kj[ch], accumulated in double in both real modes, [n][3] reals of real_mode.
 * rtk_gather_irradiance checks max_distance and then ignores it, as rtk_query_radiance ignores a record's tmax: E is the same
 * for every valid value.
 * Occlusion: ray j is open when the flag rtk_query_occluded returns for its record is 0 (in a scene with a constant medium the
 * walk draws from the record's stream, as the query's does).  open[k] = (open rays) / R, [n] reals; bent[k] = (the sum of the
 * world directions d -- the doubles of the record -- of the open rays) / R, [n][3] reals, not normalised, zero when none is
 * open.  Either of d_open and d_bent may be NULL, not both.
 * Order of the sums: rays 64q .. 64q + 63 of a point form pass q; a pass is reduced by a butterfly across its wave (offsets
 * 32, 16, .. 1); the passes are added in increasing q; the result is scaled (by pi / R) or divided (by R) once and stored once.
 * The same call gives the same bits, and a point's result does not depend on n, on its place in the call or on batch_points.
 * Workspace: the passes' sums, 32 bytes per pass, live in a buffer the context owns, grown on demand up to
 * RTK_GATHER_WORKSPACE_BYTES; a call that needs more, or sets batch_points, runs consecutive batches of points on the stream.
 * Allocation and stream behaviour are rtk_render_device's: growing the buffer allocates and waits for the device, every launch
 * goes to opts->stream, opts is read before the call returns, and one context serves one stream at a time.
 * Buffers: d_points and d_normals [n][3] doubles in both modes, 8-byte aligned; d_rays 8-byte aligned; reals need the alignment
 * of their type.  A misaligned pointer is refused (the text names the argument); so is an output whose range overlaps d_points
 * or d_normals.  n == 0 is valid and launches nothing.  RTK_ERR_INVALID, checked first and without a device: null opts; n < 0;
 * an unknown real_mode; negative max_depth or samples; reserved != 0; rays not a multiple of 64 in 64 .. 16384; n * rays over
 * 2^31 - 1; rotate not 0 or 1; negative batch_points; max_distance negative or NaN; null points, normals or outputs; then
 * alignment, then overlap, then a null context, then (not rtk_gather_rays, which needs a context for its device but no scene)
 * RTK_ERR_NO_SCENE.  The _host forms take host buffers (reals as doubles, F32 widened) and block.
 * sizeof(rtk_gather_opts) = 96. */
#define RTK_GATHER_WORKSPACE_BYTES (64u << 20)
typedef struct rtk_gather_opts {         /* 96 bytes */
    uint32_t seed; int32_t real_mode;
    int32_t max_depth;                   /* irradiance only; >= 0 */
    int32_t samples;                     /* paths per ray; 0 = 1 (occlusion: only the stream key j * samples) */
    int32_t rays;                        /* R per point; 0 = 256; a multiple of 64 in 64 .. 16384 */
    uint32_t first_key;                  /* point k draws from the streams of pixel key first_key + k */
    int32_t rotate;                      /* 0: every point uses the same set; 1: each point's own rotation of it */
    int32_t batch_points;                /* 0 = as many points per launch as the workspace budget holds; else that many */
    rtk_vec3 background;                 /* irradiance only */
    double time;
    double max_distance;                 /* the records' tmax, so occlusion's reach; 0 = +inf.  Irradiance ignores it, as the
                                          * radiance query ignores tmax */
    void* stream;
    int32_t reserved[4];                 /* 0 */
} rtk_gather_opts;

int rtk_gather_rays(rtk_ctx* ctx, const rtk_gather_opts* opts, int64_t n, const double* d_points, const double* d_normals, rtk_ray* d_rays);
int rtk_gather_irradiance(rtk_ctx* ctx, const rtk_gather_opts* opts, int64_t n, const double* d_points, const double* d_normals, void* d_irradiance);
int rtk_gather_occlusion(rtk_ctx* ctx, const rtk_gather_opts* opts, int64_t n, const double* d_points, const double* d_normals, void* d_open, void* d_bent);
int rtk_gather_rays_host(rtk_ctx* ctx, const rtk_gather_opts* opts, int64_t n, const double* h_points, const double* h_normals, rtk_ray* h_rays);
int rtk_gather_irradiance_host(rtk_ctx* ctx, const rtk_gather_opts* opts, int64_t n, const double* h_points, const double* h_normals, double* h_irradiance);
int rtk_gather_occlusion_host(rtk_ctx* ctx, const rtk_gather_opts* opts, int64_t n, const double* h_points, const double* h_normals, double* h_open,
                              double* h_bent);

/* Known-answer / diagnostic entry point: hittable::hit(r, interval(tmin, tmax), rec) of the uploaded
 * scene's root (hittable.h:33) for n caller-supplied rays, run through the same device traversal and
 * hit-record code as the render kernel.  Host buffers:
 *   h_rays [n][9] = origin(3), direction(3), time, tmin, tmax
 *   h_keys [n][3] = seed, pixel, sample of the RNG stream a constant_medium draws from (constant_medium.h:40)
 *   h_out  [n][12] = hit(0/1), t, p(3), normal(3), front_face, u, v, material index (-1 on a miss)
 *   h_draws[n]     = random_double() calls consumed
 * real_mode is RTK_REAL_F64 or RTK_REAL_F32; any other value is refused with RTK_ERR_INVALID, as by the entry points below.
 * Blocking; not a rendering path. */
int rtk_debug_closest_hit(rtk_ctx* ctx, int real_mode, int n, const double* h_rays, const uint32_t* h_keys,
                          double* h_out, uint64_t* h_draws);

/* The same for the shading side, on the device functions the render kernel itself executes (blocking; not rendering paths):
 *   rtk_debug_scatter   material::scatter + emitted (material.h:22-172) of materials[h_materials[k]] for a caller-supplied
 *                       hit record:  h_rays[n][7] = origin(3), direction(3), time;  h_records[n][11] = t, p(3), normal(3),
 *                       front_face, u, v, (unused);  h_keys[n][3] = seed, pixel, sample of the RNG stream scatter() draws from;
 *                       h_out[n][14] = scattered (0/1), scattered ray origin(3) direction(3), attenuation(3), time, emitted(3);
 *                       h_draws[n] = random_double() calls consumed
 *   rtk_debug_texture   texture::value(u, v, p) (texture.h:20-120, perlin.h:14-50) of textures[h_textures[k]]:
 *                       h_uvp[n][5] = u, v, p(3);  h_out[n][3] = colour;  h_work[n][2] = perlin::noise calls, texel fetches
 *   rtk_debug_get_ray   camera::get_ray (Camera.txt:177-200) of `cam` for h_pixel_sample[n][3] = i, j, sample:
 *                       h_out[n][7] = origin(3), direction(3), time;  h_draws[n] = random_double() calls consumed */
int rtk_debug_scatter(rtk_ctx* ctx, int real_mode, int n, const int32_t* h_materials, const double* h_rays, const double* h_records,
                      const uint32_t* h_keys, double* h_out, uint64_t* h_draws);
int rtk_debug_texture(rtk_ctx* ctx, int real_mode, int n, const int32_t* h_textures, const double* h_uvp, double* h_out, uint64_t* h_work);
int rtk_debug_get_ray(rtk_ctx* ctx, int real_mode, const rtk_camera* cam, uint32_t seed, int n, const int32_t* h_pixel_sample,
                      double* h_out, uint64_t* h_draws);

/* Introspection of the uploaded scene's traversal program (for tests and
 * for the byte model): number of program slots (fused records) and device bytes per mode. */
int rtk_scene_info(rtk_ctx* ctx, int32_t* n_program_ops, int64_t* bytes_f64, int64_t* bytes_f32);

/* The MIXED traversal program of a sphere-only description in the fast order, as rtk_scene_upload_optimized would build it
 * (host-only, no device; for tests): its 32-byte units as they lie in memory (h_units) and the image of them that the kernel
 * which stages the program copies into LDS (h_image).  eye_extent: the largest |coordinate| of the eye (0: none).  Each
 * buffer is null or holds capacity_units x 32 bytes; *n_units is set even when the buffers are too small (RTK_ERR_INVALID
 * then).  RTK_ERR_INVALID for a description with anything but spheres. */
int rtk_debug_mixed_program(const rtk_scene_desc* optimized, double eye_extent, int32_t capacity_units, int32_t* n_units, float* extent, void* h_units,
                            void* h_image);

/* Render-kernel launches one frame takes (host-only): a pixel's samples are split into chunks of 8 (at most 64 chunks); the
 * partial-sum workspace is budgeted at 1.095 GB per context (22 planes of a 1920x1080 f64 frame), and a frame with more
 * chunks than the budget holds planes for is rendered in consecutive passes over the chunks whose running sums the resolve
 * kernel carries -- the image is the same for any number of passes.  1920x1080 f64: 1 launch up to 168 samples per pixel,
 * 3 at 1000; 800x800, or an eighth of the 1920x1080 tiles: 1 at 1000.  (opts: real_mode, rank / n_ranks, variant.) */
int rtk_frame_launches(const rtk_camera* cam, const rtk_render_opts* opts);

/* Names of the kernel symbols rtk_render_device launches for (real_mode,
 * variant) on the uploaded scene -- used to find the dispatch in rocprofv3
 * traces.  Returns a static string. */
const char* rtk_kernel_name(rtk_ctx* ctx, int real_mode, int variant);

/* View batches --------------------------------------------------------------------------
 * Many cameras' frames of one size in one launch: cube faces, a camera path, thumbnails, a light field.  Device resident and
 * asynchronous on opts->stream, on the uploaded scene in either visiting order and both real modes; one rank only.  New entry
 * points; RTK_ABI_VERSION stays 2.
 *
 * The rule.  View v of the batch is, bit for bit, the frame that
 *     rtk_render_device(ctx, &h_cams[v], opts with seed = h_seeds ? h_seeds[v] : opts->seed, ...)
 * writes, linear and rgb8: d_linear = [n_views][H][W][3] reals (double for F64, float for F32), d_rgb8 = [n_views][H][W][3]
 * bytes; either may be NULL.  A sample's random stream is keyed (seed of its view, j * W + i, s) with (i, j) the pixel INSIDE
 * its view, as in the single frame.  A pixel's samples are cut into the single frame's chunks -- their boundaries depend on
 * samples_per_pixel only -- and a pixel's chunk sums are added in the single frame's order, through the same code.
 *
 * Shared by all views, and checked: image_width, image_height, samples_per_pixel, and therefore pixel_samples_scale.  Free
 * per view: everything else in rtk_camera -- the pose (center, pixel00_loc, pixel_delta_u / _v), background, max_depth (0
 * included), the defocus disk -- and the seed.
 *
 * What runs.  Work items are (view, tile, chunk), handed out from one counter to the persistent waves of ONE launch per pass
 * of rtk_view_batch_kernel<real, FEAT, IN_LDS>, the render kernel's body with a camera per lane read from a table of view
 * records.  It exists for the instantiations that stage the traversal program, its hot part or its boxes in LDS (DESIGN.md
 * "View batches" has the table).  For every other choice -- variant bit 0, programs too large for any LDS form -- and whenever
 * opts->count_work != 0, the call renders the batch as n_views plain frames, one rtk_render_kernel launch (per pass) each
 * into the view's plane: the same bits by construction, and d_counters (zeroed by the caller) receives the sum over the views.
 * rtk_view_kernel_name returns the symbol a batch would dispatch for (real_mode, variant) without work counters, as
 * rtk_kernel_name does for a frame: the view kernel's, or the plain kernel's where the per-view form runs.  Passes follow
 * rtk_frame_launches' budget with the batch's n_views * tiles in place of a frame's tiles.
 *
 * Refusals (RTK_ERR_INVALID, rtk_last_error names the cause): null ctx / h_cams / opts; n_views < 1 or > 65536; a view whose
 * shared fields differ from view 0's (the message names the view), or with max_depth < 0; bad dimensions (as
 * rtk_render_device); opts->n_ranks != 1 (or rank != 0); variant bit 22; opts->count_work without d_counters; n_views * tiles *
 * sample chunks beyond 2^31 - 1.  RTK_ERR_NO_SCENE without an uploaded scene.
 *
 * Streams: the rules of rtk_render_device.  h_cams, h_seeds and opts are read before the call returns; any number of batches
 * may be in flight on the stream.  The view records travel through a ring of four context-owned pinned buffers into a
 * context-owned device table (grown on demand like the partial-sum workspace, reused in stream order); with more than four
 * batches in flight the call waits until the upload of the fourth-last batch's records has run, and for nothing else.
 * Context state: a batch neither reads nor changes the tile order the context learned from its frames (per-view form
 * included: its frames are handed out row-major and measure nothing).  A progress callback sees the batch's work items like a
 * frame's (per-view form: those of its last view).
 *
 * rtk_render_views_host allocates, renders, waits and copies back: h_linear [n_views][H][W][3] doubles (F32 widened), h_rgb8
 * bytes, either may be NULL; counters != NULL selects count_work. */
int rtk_render_views(rtk_ctx* ctx, int32_t n_views, const rtk_camera* h_cams, const uint32_t* h_seeds /* NULL: opts->seed for all */,
                     const rtk_render_opts* opts, void* d_linear, uint8_t* d_rgb8, rtk_work_counters* d_counters);
int rtk_render_views_host(rtk_ctx* ctx, int32_t n_views, const rtk_camera* h_cams, const uint32_t* h_seeds, const rtk_render_opts* opts,
                          double* h_linear, uint8_t* h_rgb8, rtk_work_counters* counters);
const char* rtk_view_kernel_name(rtk_ctx* ctx, int real_mode, int variant);

#ifdef __cplusplus
}
#endif
#endif /* RTK_H */
