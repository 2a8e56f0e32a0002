// rtk_trace.h -- launch entry points of the device code for the C-ABI layer: the render kernel and the lane-per-ray kernels
// (known-answer, AOV / guide, ray query, light probes) of rtk_trace.hip and the frame-assembly kernels of rtk_frame.hip (tile order, resolve, accumulate, preview, noise statistics,
// adaptive state, un-permute).
#ifndef RTK_TRACE_H
#define RTK_TRACE_H

#include <hip/hip_runtime.h>

#include "rtk_device_layout.h"

namespace rtk {

// Enqueue the render kernel for one rank's tiles.  `features` selects the
// kernel instantiation (kFeatLean or kFeatAll); `count` selects the
// work-counting instantiation (the full-feature kernel, or -- for a scene with a
// MIXED program -- the counting build of the F_F32_BOX kernel itself).  tile_counter is
// a device word the persistent waves pull tile indices from (zeroed on `stream`
// before the launch); d_cam points at the camera record in device memory.  `diag`
// bits 8..13 select scheduler thresholds for A/B runs from tools/ (images are unaffected).
template <typename real>
hipError_t launch_render(const SceneView<real>& sc, const CameraRec<real>* d_cam, const TileMap& tmap, uint32_t seed, uint32_t features, bool count,
                         bool allow_lds, uint32_t diag, void* partial, unsigned long long* counters, unsigned int* tile_counter,
                         const int32_t* tile_order, unsigned int* tile_cost, hipStream_t stream);
// A view batch (rtk_render_views): the view kernel of the instantiation launch_render would choose (count = false), over tmap's
// local tiles [view][tile of a view's tiles_x x tiles_y grid] (rank 0 of 1), cameras and hashed seeds from the table d_views --
// hipErrorInvalidValue where that instantiation has no view kernel, which view_kernel_name tells beforehand (*is_view_kernel;
// its return value is the symbol a batch dispatches: the view kernel's, or else the plain kernel's).
template <typename real>
hipError_t launch_view_batch(const SceneView<real>& sc, const ViewRec<real>* d_views, const TileMap& tmap, uint32_t features, bool allow_lds, uint32_t diag,
                             void* partial, unsigned int* tile_counter, hipStream_t stream);
template <typename real>
const char* view_kernel_name(const SceneView<real>& sc, uint32_t features, bool allow_lds, uint32_t diag, bool* is_view_kernel);
// The resolve of a view batch (rtk_views.hip): launch_resolve's fold, carry and outputs over tmap's [view][tile] tiles, written
// to the planes [view][H][W][3] of out_linear / out_rgb8 (either may be null).
template <typename real>
hipError_t launch_resolve_views(const void* partial, const TileMap& tmap, int width, int height, double samples_scale, void* out_linear, uint8_t* out_rgb8,
                                void* acc, bool first_pass, bool last_pass, hipStream_t stream);

// cost[n] (segments per local tile, measured by the frame just rendered) -> order[n], most expensive first; clears cost.
hipError_t launch_tile_order(unsigned int* cost, int n, int32_t* order, hipStream_t stream);

// Partial sums [item][3][64] -> the row-major image (+ bytes) or this rank's compact tile buffer.  A frame rendered in several
// passes over consecutive chunk ranges carries its running sum in `acc` [local tile][3][64] (read unless first_pass, written
// unless last_pass); only the last pass writes the outputs.
template <typename real>
hipError_t launch_resolve(const void* partial, const TileMap& tmap, int width, int height, double samples_scale, void* out_linear, uint8_t* out_rgb8,
                          void* acc, bool first_pass, bool last_pass, hipStream_t stream);

// Progressive sessions: fold this launch's chunk planes into the session's running sum `acc` [local tile][3][64] (the resolve's
// additions in the resolve's order; `init` = plane 0 is the session's first chunk and becomes the sum) and every full chunk
// (chunk_size samples) into the noise sums s1 / s2 [local tile][64] (double).  write_out: also write the preview scaled by
// samples_scale (the resolve's outputs) and, when out_noise is given, the per-pixel standard error over k_full chunks.
template <typename real>
hipError_t launch_accumulate(const void* partial, const TileMap& tmap, int width, int height, int chunk_size, bool init, void* acc, double* s1, double* s2,
                             bool write_out, double samples_scale, int k_full, void* out_linear, uint8_t* out_rgb8, float* out_noise, hipStream_t stream);

// Frame noise statistics over this rank's in-image pixels: out3 = {sum se, max se, sum se / max(mean, 1e-3)}, reduced in a fixed
// order (per-block partials -- noise_partial_blocks(tmap) x 3 doubles -- then one single-block tree).
int noise_partial_blocks(const TileMap& tmap);
hipError_t launch_noise_stats(const double* s1, const double* s2, const TileMap& tmap, int width, int height, int k_full, double* partials, double* out3,
                              hipStream_t stream);

// Adaptive sessions (per-tile state: active[t] 1 / 0, tile_spp[t] = the tile's sample count).  launch_accumulate with the state:
// folds only the tiles active in this launch; on the last launch (`last`) writes the preview (per-tile scale and K), sets
// tile_spp = s_end of the active tiles and, when retire_ok, retires those whose metric is <= rel_target.
template <typename real>
hipError_t launch_accumulate_adaptive(const void* partial, const TileMap& tmap, int width, int height, int chunk_size, bool init, void* acc, double* s1,
                                      double* s2, int32_t* active, int32_t* tile_spp, bool last, int s_end, bool retire_ok, double rel_target,
                                      void* out_linear, uint8_t* out_rgb8, float* out_noise, hipStream_t stream);
// Resume: active[t] from tile_spp, done and the retire test of the step that ended at `done`.
hipError_t launch_adaptive_restore(const double* s1, const double* s2, const TileMap& tmap, int width, int height, int chunk_size, const int32_t* tile_spp,
                                   int done, bool retire_ok, double rel_target, int32_t* active, hipStream_t stream);
// list = the positions of `order` (identity when null; n entries) whose tile is active, in order; *count = their number.
hipError_t launch_adaptive_compact(const int32_t* active, const int32_t* order, int n, int32_t* list, int32_t* count, hipStream_t stream);
// Tile lists (rtk_render_tiles).  launch_tile_gate: *count tiles are listed; more than max_tiles (> 0) of them makes *count 0;
// info (may be null) = {listed, *count afterwards}.  launch_resolve_tiles: launch_resolve of a one-launch frame for the tiles
// list[0 .. *count - 1] only (one rank, row-major outputs), plus the session's standard error over the full chunks of chunk_size
// samples (out_noise) and 1.0f (out_support); pixels of other tiles are not written.
hipError_t launch_tile_gate(int32_t* count, int max_tiles, int32_t* info, hipStream_t stream);
template <typename real>
hipError_t launch_resolve_tiles(const void* partial, const TileMap& tmap, int width, int height, int chunk_size, double samples_scale, const int32_t* list,
                                const int32_t* count, void* out_linear, uint8_t* out_rgb8, float* out_noise, float* out_support, hipStream_t stream);
// Session set-up on the session's stream: a record of up to 256 bytes (a multiple of 4) stored from a kernel argument; the
// state of a fresh adaptive session (in-image tiles active, no samples).
hipError_t launch_store_record(const void* h_record, size_t bytes, void* d_dst, hipStream_t stream);
hipError_t launch_adaptive_init(const TileMap& tmap, int32_t* active, int32_t* tile_spp, hipStream_t stream);
// launch_noise_stats with per-tile K = tile_spp[t] / chunk_size (the same kernel, given tile_spp).
hipError_t launch_noise_stats_adaptive(const double* s1, const double* s2, const TileMap& tmap, int width, int height, int chunk_size, const int32_t* tile_spp,
                                       double* partials, double* out3, hipStream_t stream);

// Known-answer helper: closest hit of the scene root for n caller-supplied rays (device buffers), keys[n][3] = seed, pixel,
// sample of each ray's stream: launch_query_hits' walk with a seed per ray and no skip.
template <typename real>
hipError_t launch_debug_hit(const SceneView<real>& sc, int n, const double* d_rays, const uint32_t* d_keys, double* d_out, unsigned long long* d_draws,
                            hipStream_t stream);

// Known-answer helpers for the shading side: shade_surface, texture_value and begin_sample on caller-supplied inputs.
template <typename real>
hipError_t launch_debug_scatter(const SceneView<real>& sc, int n, const int32_t* d_mat, const double* d_ray, const double* d_rec, const uint32_t* d_keys, double* d_out,
                                unsigned long long* d_draws, hipStream_t stream);
template <typename real>
hipError_t launch_debug_texture(const SceneView<real>& sc, int n, const int32_t* d_tex, const double* d_uvp, double* d_out, unsigned long long* d_work, hipStream_t stream);
template <typename real>
hipError_t launch_debug_get_ray(const CameraRec<real>& cam, uint32_t seed, int n, const int32_t* d_ijs, double* d_out, unsigned long long* d_draws, hipStream_t stream);

// Guide buffers of the denoiser: aov[(j * W + i) * 8 + k] over samples 0 .. n_samples - 1 of every pixel (rtk_render_aovs):
// rtk_guide_kernel compiled without the chain.
template <typename real>
hipError_t launch_aov(const SceneView<real>& sc, const CameraRec<real>& cam, uint32_t seed, int n_samples, float* d_aov, hipStream_t stream);

// The same kernel with the surface seen through followed mirrors / glass: guides[(j * W + i) * 16 + k], k 0-7 = launch_aov's
// values (rtk_render_guides).  follow = RTK_GUIDE_FOLLOW_* bits, max_bounces 1..8 (both resolved by the caller).
template <typename real>
hipError_t launch_guides(const SceneView<real>& sc, const CameraRec<real>& cam, uint32_t seed, int n_samples, int follow, int max_bounces, float* d_guides,
                         hipStream_t stream);

// Ray queries (rtk_query_hits / _occluded / _radiance): n caller-supplied rtk_ray records in device memory, one lane each.
// any_hit = the program holds no medium, so occlusion may stop at the first accepted hit.  cam carries the radiance query's
// background, max_depth and spp = samples per ray; d_draws selects the counting instantiation.
template <typename real>
hipError_t launch_query_hits(const SceneView<real>& sc, uint32_t seed, long long n, const void* d_rays, void* d_hits, hipStream_t stream);
template <typename real>
hipError_t launch_query_occluded(const SceneView<real>& sc, uint32_t seed, bool any_hit, long long n, const void* d_rays, int32_t* d_occluded, hipStream_t stream);
template <typename real>
hipError_t launch_query_radiance(const SceneView<real>& sc, const CameraRec<real>& cam, uint32_t seed, long long n, const void* d_rays, void* d_radiance,
                                 uint32_t* d_draws, hipStream_t stream);

// Light probes (rtk_probe_rays / rtk_probe_bake): n probes at d_positions [n][3] doubles, `rays` rays each (a multiple of 256).
// launch_probe_rays writes the n * rays ray records, one lane each; launch_probe_bake runs one workgroup per probe and writes
// [n][9][3] reals.  cam carries background, max_depth and spp = samples per ray, as for launch_query_radiance.
hipError_t launch_probe_rays(long long n, int rays, int samples, uint32_t first_key, double time, const double* d_positions, void* d_rays, hipStream_t stream);
template <typename real>
hipError_t launch_probe_bake(const SceneView<real>& sc, const CameraRec<real>& cam, uint32_t seed, uint32_t first_key, int rays, double time, long long n,
                             const double* d_positions, void* d_sh, hipStream_t stream);

// Surface gathers (rtk_gather_irradiance / _occlusion), stage 1: n points of one batch at d_points / d_normals [n][3] doubles,
// `rays` rays each (a multiple of 64), one wave per 64 rays; first_key is the key of the batch's first point.  d_partial gets
// [n * rays / 64][4] doubles -- the sums of each unit's radiance (three words), or its open rays and their directions (four) --
// for launch_gather_reduce (rtk_gather.hip).  cam as for launch_query_radiance, any_hit as for launch_query_occluded.
template <typename real>
hipError_t launch_gather_irradiance(const SceneView<real>& sc, const CameraRec<real>& cam, uint32_t seed, uint32_t first_key, int rays, uint32_t rotate, double time,
                                    long long n, const double* d_points, const double* d_normals, double* d_partial, hipStream_t stream);
template <typename real>
hipError_t launch_gather_occlusion(const SceneView<real>& sc, uint32_t seed, bool any_hit, uint32_t first_key, int rays, int samples, uint32_t rotate, double time,
                                   double tmax, long long n, const double* d_points, const double* d_normals, double* d_partial, hipStream_t stream);
// ... and what rtk_gather.hip holds: the n * rays ray records of rtk_gather_rays, one lane each, and stage 2, one lane per
// (point, channel): a point's rays / 64 partial sums added in order, scaled once by pi / rays (irradiance, [n][3] reals) or divided
// once by rays (occlusion: d_open [n], d_bent [n][3] reals, either may be null).
hipError_t launch_gather_rays(long long n, int rays, int samples, uint32_t first_key, uint32_t rotate, double time, double tmax, const double* d_points,
                              const double* d_normals, void* d_rays, hipStream_t stream);
template <typename real>
hipError_t launch_gather_irradiance_reduce(long long n, int rays, const double* d_partial, void* d_irradiance, hipStream_t stream);
template <typename real>
hipError_t launch_gather_occlusion_reduce(long long n, int rays, const double* d_partial, void* d_open, void* d_bent, hipStream_t stream);

// Lens models (rtk_lens_*): what the kernels read of an rtk_lens besides its camera record, in double in both real modes.
// half_h / half_v = fov_h / 2, fov_v / 2 with the defaults resolved (EQUIRECT, FISHEYE) or ortho_width / 2, ortho_height / 2
// (ORTHOGRAPHIC): halving is exact, so the rule's x * (fov_h / 2) is x * half_h.
struct LensRec {
    double center[3], u[3], v[3], w[3];
    double half_h, half_v;
    int32_t model, reserved;
};
// launch_lens_rays: the records of samples first_sample .. + n_samples - 1 of every pixel, one lane each, [H * W * n_samples].
// launch_lens_render: cam.spp samples per pixel, a pixel's samples spread over up to 16 lanes and summed in sample order;
// d_linear [H][W][3] reals, d_noise [H][W] or null.
// launch_lens_aov / _guides: launch_aov / launch_guides with the lens's record as the primary ray.
template <typename real>
hipError_t launch_lens_rays(const LensRec& lens, const CameraRec<real>& cam, uint32_t seed, uint32_t first_sample, int n_samples, void* d_rays, hipStream_t stream);
template <typename real>
hipError_t launch_lens_render(const SceneView<real>& sc, const LensRec& lens, const CameraRec<real>& cam, uint32_t seed, uint32_t first_sample, void* d_linear,
                              float* d_noise, hipStream_t stream);
template <typename real>
hipError_t launch_lens_aov(const SceneView<real>& sc, const LensRec& lens, const CameraRec<real>& cam, uint32_t seed, int n_samples, float* d_aov, hipStream_t stream);
template <typename real>
hipError_t launch_lens_guides(const SceneView<real>& sc, const LensRec& lens, const CameraRec<real>& cam, uint32_t seed, int n_samples, int follow, int max_bounces,
                              float* d_guides, hipStream_t stream);

// A one-rank progressive session's preview and se (row-major) from its running sum and noise sums; tile_spp null = every tile
// holds `done` samples.  Reads the state only.
template <typename real>
hipError_t launch_preview(const void* acc, const double* s1, const double* s2, const TileMap& tmap, int width, int height, int chunk_size, int done,
                          const int32_t* tile_spp, void* out_linear, float* out_noise, hipStream_t stream);

template <typename real>
hipError_t launch_unpermute(const void* gathered, int width, int height, int n_ranks, long long tiles_per_rank, void* out_linear, uint8_t* out_rgb8,
                            hipStream_t stream);

// Symbol name of the render kernel launch_render would launch for these arguments (the one decision function serves both).
template <typename real>
const char* render_kernel_name(const SceneView<real>& sc, uint32_t features, bool count, bool allow_lds, uint32_t diag);

}  // namespace rtk

#endif  // RTK_TRACE_H
