// rtk_frame.hip -- frame assembly: the kernels that turn the render kernel's partial-sum planes
// (partial[chunk][local tile][3][64], rtk_trace.hip) into images and into the state of a progressive session, and their
// launchers (declared in rtk_trace.h).  Nothing here traces a ray; what it shares with the traversal is rtk_device_math.h.
//
// Bit-exactness of a stepped, resumed or adaptive frame against the one-shot frame rests on every kernel performing the
// same additions in the same order.  That holds by construction: the slot -> pixel addressing (pixel_slot), the fold of a
// launch's planes (fold_planes) and the output of a pixel (write_pixel) each exist once (rtk_frame_steps.h), and every kernel uses them.
// One thread per (local tile, pixel); a wave64 is one 8x8 tile, a 256-thread block four of them.
#include <hip/hip_runtime.h>

#include "rtk.h"
#include "rtk_device_layout.h"
#include "rtk_device_math.h"
#include "rtk_frame_steps.h"
#include "rtk_trace.h"

namespace rtk {

// Batch means over k >= 2 chunk means: the standard error of the pixel mean, and the same relative to max(mean, 1e-3).
RTK_DEV double noise_se(double s1, double s2, int k) {
    if (k < 2) return 0.0;
    const double m = s1 / double(k);
    double v = (s2 - double(k) * m * m) / double(k - 1);
    v = v > 0.0 ? v : 0.0;
    return __builtin_sqrt(v / double(k));
}
RTK_DEV double noise_rel(double se, double s1, int k) {
    const double m = s1 / double(k);
    return se / (m > 1e-3 ? m : 1e-3);
}

RTK_DEV double wave_max(double v) {
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(v, off);
        v = o > v ? o : v;
    }
    return v;
}
RTK_DEV void wave_reduce3(double& a, double& b, double& c) {  // wave64 butterfly: a and c summed, b maximised
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_xor(a, off);
        const double bo = __shfl_xor(b, off);
        b = bo > b ? bo : b;
        c += __shfl_xor(c, off);
    }
}

// ------------------------------------------------------------------ tile order --
// Tile order for the NEXT frame: local tiles sorted by the cost measured in this frame, most expensive first
// (64 buckets on a scale relative to the maximum: a counting sort, one workgroup).  A frame cannot end before its
// slowest sample -- a 50-bounce path inside a glass sphere is one sequential ~2-3 ms chain on one lane -- so the
// expensive tiles must START early; otherwise every GPU idles ~2.5 ms at the end of its share of the frame.
// Clears the cost array for the next measurement.
__global__ __launch_bounds__(1024) void rtk_tile_order_kernel(unsigned int* __restrict__ cost, int n, int32_t* __restrict__ order) {
    __shared__ unsigned int s_max;
    __shared__ unsigned int s_count[64], s_base[64];
    const int tid = threadIdx.x;
    if (tid == 0) s_max = 0;
    if (tid < 64) s_count[tid] = 0;
    __syncthreads();
    unsigned int local_max = 0;
    for (int k = tid; k < n; k += 1024) local_max = cost[k] > local_max ? cost[k] : local_max;
    atomicMax(&s_max, local_max);
    __syncthreads();
    const unsigned long long top = (unsigned long long)s_max + 1ull;
    for (int k = tid; k < n; k += 1024) atomicAdd(&s_count[63 - int((unsigned long long)cost[k] * 64ull / top)], 1u);  // bucket 0 = most expensive
    __syncthreads();
    if (tid == 0) {
        unsigned int run = 0;
        for (int b = 0; b < 64; b++) {
            s_base[b] = run;
            run += s_count[b];
        }
    }
    __syncthreads();
    for (int k = tid; k < n; k += 1024) {
        const int b = 63 - int((unsigned long long)cost[k] * 64ull / top);
        order[atomicAdd(&s_base[b], 1u)] = k;
    }
    __syncthreads();
    for (int k = tid; k < n; k += 1024) cost[k] = 0;
}

hipError_t launch_tile_order(unsigned int* cost, int n, int32_t* order, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    rtk_tile_order_kernel<<<dim3(1), dim3(1024), 0, stream>>>(cost, n, order);
    return hipGetLastError();
}

// ------------------------------------------------------------------ one-shot frames --
// Partial sums -> pixels.  For every pixel of this rank: fold its chunks, scale by 1/spp (Camera.txt:74) and write either
// the row-major image (+ bytes) or this rank's compact tile buffer.
// A frame with more sample chunks than the workspace has planes (kMaxPlanesPerPass) is rendered in several passes over
// consecutive chunk ranges; `acc` [local tile][3][64] carries the running sum from pass to pass, so the image does not
// depend on the number of passes (fold_planes).
template <typename real>
__global__ __launch_bounds__(256) void rtk_resolve_kernel(const real* __restrict__ partial, TileMap tmap, int width, int height, real samples_scale,
                                                           real* __restrict__ out_linear, uint8_t* __restrict__ out_rgb8, real* __restrict__ acc, int first_pass,
                                                           int last_pass) {
    const PixelSlot p = pixel_slot(tmap, width, height);
    if (p.local_tile >= tmap.n_tiles_local) return;
    V3<real> sum = mk(real(0), real(0), real(0));
    if (p.inside) {
        sum = fold_planes<false>(partial, tmap, p, first_pass != 0, acc);
        if (!last_pass) store3(acc + p.plane(), sum);
        sum = scale(samples_scale, sum);
    }
    if (last_pass) write_pixel<real>(p, tmap.compact != 0, width, sum, 0.0, out_linear, out_rgb8, nullptr);
}

template <typename real>
hipError_t launch_resolve(const void* partial, const TileMap& tmap, int width, int height, double samples_scale, void* out_linear, uint8_t* out_rgb8,
                          void* acc, bool first_pass, bool last_pass, hipStream_t stream) {
    if (tmap.n_tiles_local <= 0) return hipSuccess;
    rtk_resolve_kernel<real><<<dim3(pixel_slot_blocks(tmap)), dim3(256), 0, stream>>>(static_cast<const real*>(partial), tmap, width, height, real(samples_scale),
                                                                                     static_cast<real*>(out_linear), out_rgb8, static_cast<real*>(acc),
                                                                                     first_pass ? 1 : 0, last_pass ? 1 : 0);
    return hipGetLastError();
}
template hipError_t launch_resolve<double>(const void*, const TileMap&, int, int, double, void*, uint8_t*, void*, bool, bool, hipStream_t);
template hipError_t launch_resolve<float>(const void*, const TileMap&, int, int, double, void*, uint8_t*, void*, bool, bool, hipStream_t);

// Gathered compact tiles of all ranks -> row-major image (+ bytes).  `whole` maps the whole image as one rank's tiles.
template <typename real>
__global__ __launch_bounds__(256) void rtk_unpermute_kernel(const real* __restrict__ gathered, TileMap whole, int width, int height, int n_ranks,
                                                             long long tiles_per_rank, real* __restrict__ out_linear, uint8_t* __restrict__ out_rgb8) {
    const PixelSlot p = pixel_slot(whole, width, height);
    if (!p.inside) return;
    const long long rank = p.local_tile % n_ranks, local_tile = p.local_tile / n_ranks;
    write_pixel<real>(p, false, width, load3(gathered + (rank * tiles_per_rank + local_tile) * 192 + p.pix), 0.0, out_linear, out_rgb8, nullptr);
}

template <typename real>
hipError_t launch_unpermute(const void* gathered, int width, int height, int n_ranks, long long tiles_per_rank, void* out_linear, uint8_t* out_rgb8,
                            hipStream_t stream) {
    TileMap whole{};
    whole.tiles_x = (width + 7) / 8;
    whole.tiles_y = (height + 7) / 8;
    whole.n_tiles_local = whole.tiles_x * whole.tiles_y;
    whole.n_ranks = 1;
    rtk_unpermute_kernel<real><<<dim3(pixel_slot_blocks(whole)), dim3(256), 0, stream>>>(static_cast<const real*>(gathered), whole, width, height, n_ranks,
                                                                                        tiles_per_rank, static_cast<real*>(out_linear), out_rgb8);
    return hipGetLastError();
}
template hipError_t launch_unpermute<double>(const void*, int, int, int, long long, void*, uint8_t*, hipStream_t);
template hipError_t launch_unpermute<float>(const void*, int, int, int, long long, void*, uint8_t*, hipStream_t);

// ------------------------------------------------------------------ progressive sessions --
// A step renders an absolute range of sample chunks into the partial-sum planes and this kernel folds them into the session's
// own running sum [local tile][3][64] and noise sums S1 / S2 [local tile][64] (fold_planes: the resolve's additions in the
// resolve's order, so a frame rendered in steps is the one-shot frame bit for bit).  On the step's last launch (`scale_out`
// != 0) the preview is written like the resolve's output: scaled by 1 / samples_done, plus the per-pixel standard error over
// k_full chunks (float) when out_noise is given.
template <typename real>
__global__ __launch_bounds__(256) void rtk_accumulate_kernel(const real* __restrict__ partial, TileMap tmap, int width, int height, int chunk_size, int init,
                                                              real* __restrict__ acc, double* __restrict__ s1, double* __restrict__ s2, int scale_out,
                                                              real samples_scale, int k_full, real* __restrict__ out_linear, uint8_t* __restrict__ out_rgb8,
                                                              float* __restrict__ out_noise) {
    const PixelSlot p = pixel_slot(tmap, width, height);
    if (p.local_tile >= tmap.n_tiles_local) return;
    V3<real> sum = mk(real(0), real(0), real(0));
    double se = 0.0;
    if (p.inside) {
        double n1 = s1[p.word()], n2 = s2[p.word()];
        sum = fold_planes<true>(partial, tmap, p, init != 0, acc, chunk_size, &n1, &n2);
        store3(acc + p.plane(), sum);
        s1[p.word()] = n1;
        s2[p.word()] = n2;
        sum = scale(samples_scale, sum);
        se = noise_se(n1, n2, k_full);
    }
    if (scale_out) write_pixel(p, tmap.compact != 0, width, sum, se, out_linear, out_rgb8, out_noise);
}

template <typename real>
hipError_t launch_accumulate(const void* partial, const TileMap& tmap, int width, int height, int chunk_size, bool init, void* acc, double* s1, double* s2,
                             bool write_out, double samples_scale, int k_full, void* out_linear, uint8_t* out_rgb8, float* out_noise, hipStream_t stream) {
    if (tmap.n_tiles_local <= 0) return hipSuccess;
    rtk_accumulate_kernel<real><<<dim3(pixel_slot_blocks(tmap)), dim3(256), 0, stream>>>(
        static_cast<const real*>(partial), tmap, width, height, chunk_size, init ? 1 : 0, static_cast<real*>(acc), s1, s2, write_out ? 1 : 0,
        real(samples_scale), k_full, static_cast<real*>(out_linear), out_rgb8, out_noise);
    return hipGetLastError();
}
template hipError_t launch_accumulate<double>(const void*, const TileMap&, int, int, int, bool, void*, double*, double*, bool, double, int, void*, uint8_t*,
                                              float*, hipStream_t);
template hipError_t launch_accumulate<float>(const void*, const TileMap&, int, int, int, bool, void*, double*, double*, bool, double, int, void*, uint8_t*,
                                             float*, hipStream_t);

// A session's current preview, rebuilt from its state without changing it (rtk_progressive_denoise): the accumulate kernels'
// outputs -- the running sum scaled by 1 / the tile's sample count (`done`, or tile_spp[t] of an adaptive session) and se over
// that count's full chunks -- row-major, for one rank that renders the whole image.
template <typename real>
__global__ __launch_bounds__(256) void rtk_preview_kernel(const real* __restrict__ acc, const double* __restrict__ s1, const double* __restrict__ s2,
                                                           TileMap tmap, int width, int height, int chunk_size, int done, const int32_t* __restrict__ tile_spp,
                                                           real* __restrict__ out_linear, float* __restrict__ out_noise) {
    const PixelSlot p = pixel_slot(tmap, width, height);
    if (!p.inside) return;
    const int spp = tile_spp ? tile_spp[p.local_tile] : done;
    const V3<real> sum = scale(real(1.0 / double(spp)), load3(acc + p.plane()));
    write_pixel<real>(p, false, width, sum, noise_se(s1[p.word()], s2[p.word()], spp / chunk_size), out_linear, nullptr, out_noise);
}

template <typename real>
hipError_t launch_preview(const void* acc, const double* s1, const double* s2, const TileMap& tmap, int width, int height, int chunk_size, int done,
                          const int32_t* tile_spp, void* out_linear, float* out_noise, hipStream_t stream) {
    rtk_preview_kernel<real><<<dim3(pixel_slot_blocks(tmap)), dim3(256), 0, stream>>>(static_cast<const real*>(acc), s1, s2, tmap, width, height, chunk_size, done,
                                                                                     tile_spp, static_cast<real*>(out_linear), out_noise);
    return hipGetLastError();
}
template hipError_t launch_preview<double>(const void*, const double*, const double*, const TileMap&, int, int, int, int, const int32_t*, void*, float*, hipStream_t);
template hipError_t launch_preview<float>(const void*, const double*, const double*, const TileMap&, int, int, int, int, const int32_t*, void*, float*, hipStream_t);

// Frame noise statistics, deterministic (no float atomics): every block reduces its pixels' (se, max se, se / max(mean, 1e-3))
// -- a wave64 butterfly, then the four waves in a fixed order -- into partials[block][3]; one single-block kernel reduces the
// partials in a fixed tree.  The same inputs give the same bits on every run.  K is the tile's own, tile_spp[t] / chunk_size,
// when tile_spp is given (adaptive sessions), the frame's k_full otherwise.
__global__ __launch_bounds__(256) void rtk_noise_partial_kernel(const double* __restrict__ s1, const double* __restrict__ s2, TileMap tmap, int width, int height,
                                                                 int chunk_size, int k_full, const int32_t* __restrict__ tile_spp,
                                                                 double* __restrict__ partials) {
    __shared__ double s_w[4][3];
    const PixelSlot p = pixel_slot(tmap, width, height);
    double se = 0.0, rel = 0.0;
    if (p.inside) {
        const int k = tile_spp ? tile_spp[p.local_tile] / chunk_size : k_full;
        if (k >= 2) {
            se = noise_se(s1[p.word()], s2[p.word()], k);
            rel = noise_rel(se, s1[p.word()], k);
        }
    }
    double sum_se = se, max_se = se, sum_rel = rel;
    wave_reduce3(sum_se, max_se, sum_rel);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_w[wave][0] = sum_se;
        s_w[wave][1] = max_se;
        s_w[wave][2] = sum_rel;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double a = (s_w[0][0] + s_w[1][0]) + (s_w[2][0] + s_w[3][0]);
        const double b01 = s_w[0][1] > s_w[1][1] ? s_w[0][1] : s_w[1][1], b23 = s_w[2][1] > s_w[3][1] ? s_w[2][1] : s_w[3][1];
        const double c = (s_w[0][2] + s_w[1][2]) + (s_w[2][2] + s_w[3][2]);
        partials[size_t(blockIdx.x) * 3] = a;
        partials[size_t(blockIdx.x) * 3 + 1] = b01 > b23 ? b01 : b23;
        partials[size_t(blockIdx.x) * 3 + 2] = c;
    }
}

__global__ __launch_bounds__(256) void rtk_noise_final_kernel(const double* __restrict__ partials, int n, double* __restrict__ out) {
    __shared__ double s_v[3][256];
    const int t = threadIdx.x;
    double a = 0.0, b = 0.0, c = 0.0;
    for (int k = t; k < n; k += 256) {  // each thread walks its strided slice in index order
        a += partials[size_t(k) * 3];
        b = partials[size_t(k) * 3 + 1] > b ? partials[size_t(k) * 3 + 1] : b;
        c += partials[size_t(k) * 3 + 2];
    }
    s_v[0][t] = a;
    s_v[1][t] = b;
    s_v[2][t] = c;
    __syncthreads();
    for (int half = 128; half > 0; half >>= 1) {  // fixed pairwise tree
        if (t < half) {
            s_v[0][t] = s_v[0][t] + s_v[0][t + half];
            s_v[1][t] = s_v[1][t + half] > s_v[1][t] ? s_v[1][t + half] : s_v[1][t];
            s_v[2][t] = s_v[2][t] + s_v[2][t + half];
        }
        __syncthreads();
    }
    if (t == 0) {
        out[0] = s_v[0][0];
        out[1] = s_v[1][0];
        out[2] = s_v[2][0];
    }
}

int noise_partial_blocks(const TileMap& tmap) { return pixel_slot_blocks(tmap); }

static hipError_t noise_stats(const double* s1, const double* s2, const TileMap& tmap, int width, int height, int chunk_size, int k_full, const int32_t* tile_spp,
                              double* partials, double* out3, hipStream_t stream) {
    const int blocks = noise_partial_blocks(tmap);
    if (blocks <= 0) return hipErrorInvalidValue;
    rtk_noise_partial_kernel<<<dim3(blocks), dim3(256), 0, stream>>>(s1, s2, tmap, width, height, chunk_size, k_full, tile_spp, partials);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    rtk_noise_final_kernel<<<dim3(1), dim3(256), 0, stream>>>(partials, blocks, out3);
    return hipGetLastError();
}
hipError_t launch_noise_stats(const double* s1, const double* s2, const TileMap& tmap, int width, int height, int k_full, double* partials, double* out3,
                              hipStream_t stream) {
    return noise_stats(s1, s2, tmap, width, height, 1, k_full, nullptr, partials, out3, stream);
}
hipError_t launch_noise_stats_adaptive(const double* s1, const double* s2, const TileMap& tmap, int width, int height, int chunk_size, const int32_t* tile_spp,
                                       double* partials, double* out3, hipStream_t stream) {
    return noise_stats(s1, s2, tmap, width, height, chunk_size, 0, tile_spp, partials, out3, stream);
}

// ------------------------------------------------------------------ adaptive sessions --
// (include/rtk.h, "Tile-adaptive sampling"): every local tile is active (it holds the session's samples_done samples) or
// retired (it keeps tile_spp[t] samples for good).  A step renders the active tiles only -- the render kernel hands out the
// compacted list `tile_order` up to the device word `active_count` -- and the kernels below keep the per-tile state.  The
// retire metric of a tile is the maximum over its in-image pixels of se / max(m, 1e-3) over K chunks.

// rtk_accumulate_kernel with per-tile state: folds this launch's planes only into the tiles that were active in it and leaves
// retired tiles' sums and S1 / S2 alone.  On the step's last launch (`last`) it writes the preview -- each tile scaled by
// 1 / its own sample count, se over its own K -- and fuses the retire test: one wave64 per tile, the wave max of the metric
// through __shfl_xor, lane 0 writes the tile's new state.
template <typename real>
__global__ __launch_bounds__(256) void rtk_accumulate_adaptive_kernel(const real* __restrict__ partial, TileMap tmap, int width, int height, int chunk_size,
                                                                       int init, real* __restrict__ acc, double* __restrict__ s1, double* __restrict__ s2,
                                                                       int32_t* __restrict__ active, int32_t* __restrict__ tile_spp, int last, int s_end,
                                                                       int retire_ok, double rel_target, real samples_scale, real* __restrict__ out_linear,
                                                                       uint8_t* __restrict__ out_rgb8, float* __restrict__ out_noise) {
    const PixelSlot p = pixel_slot(tmap, width, height);
    if (p.local_tile >= tmap.n_tiles_local) return;  // (wave-uniform: one wave is one tile)
    const bool is_active = active[p.local_tile] != 0;
    V3<real> sum = mk(real(0), real(0), real(0));
    double n1 = 0.0, n2 = 0.0;
    if (p.inside && is_active) {
        n1 = s1[p.word()];
        n2 = s2[p.word()];
        sum = fold_planes<true>(partial, tmap, p, init != 0, acc, chunk_size, &n1, &n2);
        store3(acc + p.plane(), sum);
        s1[p.word()] = n1;
        s2[p.word()] = n2;
    } else if (p.inside && last) {
        sum = load3(acc + p.plane());
        n1 = s1[p.word()];
        n2 = s2[p.word()];
    }
    if (!last) return;
    const int spp = is_active ? s_end : tile_spp[p.local_tile];
    const int k_full = spp / chunk_size;
    double se = 0.0, rel = 0.0;
    if (p.inside) {
        sum = scale(is_active ? samples_scale : real(1.0 / double(spp)), sum);
        se = noise_se(n1, n2, k_full);
        if (k_full >= 2) rel = noise_rel(se, n1, k_full);
    }
    if (is_active) {  // the retire test: wave-uniform branch, every lane of the tile takes part in the reduction
        const double metric = wave_max(rel);
        if (p.pix == 0) {
            tile_spp[p.local_tile] = s_end;
            if (retire_ok && metric <= rel_target) active[p.local_tile] = 0;
        }
    }
    write_pixel(p, tmap.compact != 0, width, sum, se, out_linear, out_rgb8, out_noise);
}

template <typename real>
hipError_t launch_accumulate_adaptive(const void* partial, const TileMap& tmap, int width, int height, int chunk_size, bool init, void* acc, double* s1,
                                      double* s2, int32_t* active, int32_t* tile_spp, bool last, int s_end, bool retire_ok, double rel_target,
                                      void* out_linear, uint8_t* out_rgb8, float* out_noise, hipStream_t stream) {
    if (tmap.n_tiles_local <= 0) return hipSuccess;
    rtk_accumulate_adaptive_kernel<real><<<dim3(pixel_slot_blocks(tmap)), dim3(256), 0, stream>>>(
        static_cast<const real*>(partial), tmap, width, height, chunk_size, init ? 1 : 0, static_cast<real*>(acc), s1, s2, active, tile_spp, last ? 1 : 0,
        s_end, retire_ok ? 1 : 0, rel_target, real(1.0 / double(s_end)), static_cast<real*>(out_linear), out_rgb8, out_noise);
    return hipGetLastError();
}
template hipError_t launch_accumulate_adaptive<double>(const void*, const TileMap&, int, int, int, bool, void*, double*, double*, int32_t*, int32_t*, bool, int,
                                                       bool, double, void*, uint8_t*, float*, hipStream_t);
template hipError_t launch_accumulate_adaptive<float>(const void*, const TileMap&, int, int, int, bool, void*, double*, double*, int32_t*, int32_t*, bool, int,
                                                      bool, double, void*, uint8_t*, float*, hipStream_t);

// Resume of an adaptive checkpoint: the retired state is not stored, it is recomputed -- a tile is active when it holds
// samples_done samples and the retire test of the step that ended there (the same metric, from the same S1 / S2) did not
// retire it.  One wave64 per tile, as in the accumulate pass.
__global__ __launch_bounds__(256) void rtk_adaptive_restore_kernel(const double* __restrict__ s1, const double* __restrict__ s2, TileMap tmap, int width,
                                                                    int height, int chunk_size, const int32_t* __restrict__ tile_spp, int done,
                                                                    int retire_ok, double rel_target, int32_t* __restrict__ active) {
    const PixelSlot p = pixel_slot(tmap, width, height);
    if (p.local_tile >= tmap.n_tiles_local) return;
    const int k_full = done / chunk_size;
    double rel = 0.0;
    if (p.inside && k_full >= 2) rel = noise_rel(noise_se(s1[p.word()], s2[p.word()], k_full), s1[p.word()], k_full);
    const double metric = wave_max(rel);
    if (p.pix == 0) active[p.local_tile] = (p.in_grid && tile_spp[p.local_tile] == done && !(retire_ok && metric <= rel_target)) ? 1 : 0;
}

hipError_t launch_adaptive_restore(const double* s1, const double* s2, const TileMap& tmap, int width, int height, int chunk_size, const int32_t* tile_spp,
                                   int done, bool retire_ok, double rel_target, int32_t* active, hipStream_t stream) {
    if (tmap.n_tiles_local <= 0) return hipSuccess;
    rtk_adaptive_restore_kernel<<<dim3(pixel_slot_blocks(tmap)), dim3(256), 0, stream>>>(s1, s2, tmap, width, height, chunk_size, tile_spp, done,
                                                                                        retire_ok ? 1 : 0, rel_target, active);
    return hipGetLastError();
}

// The next step's hand-out list: a stable filter of `order` (identity when null) keeping the active tiles, and its length.
// One block walks the positions 1024 at a time: a 64-bit ballot per wave, the waves' counts summed in wave order -- the same
// list on every run.
__global__ __launch_bounds__(1024) void rtk_adaptive_compact_kernel(const int32_t* __restrict__ active, const int32_t* __restrict__ order, int n,
                                                                     int32_t* __restrict__ list, int32_t* __restrict__ count) {
    __shared__ int s_wave[16];
    __shared__ int s_base;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (int base = 0; base < n; base += 1024) {
        const int pos = base + tid;
        int t = 0;
        bool keep = false;
        if (pos < n) {
            t = order ? order[pos] : pos;
            keep = active[t] != 0;
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int at = s_base;
        for (int w = 0; w < wave; w++) at += s_wave[w];
        if (keep) list[at + __popcll(m & ((1ull << lane) - 1ull))] = t;
        __syncthreads();
        if (tid == 0) {
            int total = 0;
            for (int w = 0; w < 16; w++) total += s_wave[w];
            s_base += total;
        }
        __syncthreads();
    }
    if (tid == 0) *count = s_base;
}

hipError_t launch_adaptive_compact(const int32_t* active, const int32_t* order, int n, int32_t* list, int32_t* count, hipStream_t stream) {
    if (n <= 0) return hipErrorInvalidValue;
    rtk_adaptive_compact_kernel<<<dim3(1), dim3(1024), 0, stream>>>(active, order, n, list, count);
    return hipGetLastError();
}

// ------------------------------------------------------------------ tile lists --
// (include/rtk.h, "Tile lists"): rtk_render_tiles renders the tiles of a compacted list -- rtk_adaptive_compact_kernel's output
// over the caller's flags, in ascending tile index -- and the kernels below decide its length and turn its tiles into pixels.

// After the compaction: count[0] tiles are flagged.  More than max_tiles (> 0) of them: the list's length becomes 0, so the
// render hands out nothing and the resolve writes nothing.  info = {flagged, rendered}.  One lane.
__global__ __launch_bounds__(64) void rtk_tile_gate_kernel(int32_t* __restrict__ count, int max_tiles, int32_t* __restrict__ info) {
    if (threadIdx.x != 0) return;
    const int flagged = *count;
    const int rendered = (max_tiles > 0 && flagged > max_tiles) ? 0 : flagged;
    *count = rendered;
    if (info) {
        info[0] = flagged;
        info[1] = rendered;
    }
}

hipError_t launch_tile_gate(int32_t* count, int max_tiles, int32_t* info, hipStream_t stream) {
    rtk_tile_gate_kernel<<<dim3(1), dim3(64), 0, stream>>>(count, max_tiles, info);
    return hipGetLastError();
}

// pixel_slot over list positions: wave w takes tile list[w] (one rank: the local tile is the tile); false at positions >= count.
RTK_DEV bool list_slot(const TileMap& tmap, const int32_t* __restrict__ list, const int32_t* __restrict__ count, int width, int height, PixelSlot& p) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long pos = gid >> 6;
    if (pos >= tmap.n_tiles_local || pos >= *count) return false;
    const int tile = list[pos];
    p.pix = int(gid & 63);
    p.local_tile = tile;
    p.i = (tile % tmap.tiles_x) * 8 + (p.pix & 7);
    p.j = (tile / tmap.tiles_x) * 8 + (p.pix >> 3);
    p.in_grid = tile >= 0 && tile < tmap.n_tiles_local;
    p.inside = p.in_grid && p.i < width && p.j < height;
    return true;
}

// The resolve of a one-launch frame for the listed tiles only: the resolve's fold and output (fold_planes, write_pixel), the
// session's noise (batch means over the full chunks, noise_se) and support 1 -- rendered, not interpolated.  Row-major outputs.
template <typename real>
__global__ __launch_bounds__(256) void rtk_resolve_tiles_kernel(const real* __restrict__ partial, TileMap tmap, int width, int height, int chunk_size, int k_full,
                                                                 real samples_scale, const int32_t* __restrict__ list, const int32_t* __restrict__ count,
                                                                 real* __restrict__ out_linear, uint8_t* __restrict__ out_rgb8, float* __restrict__ out_noise,
                                                                 float* __restrict__ out_support) {
    PixelSlot p;
    if (!list_slot(tmap, list, count, width, height, p) || !p.inside) return;
    double n1 = 0.0, n2 = 0.0;
    const V3<real> sum = scale(samples_scale, fold_planes<true>(partial, tmap, p, true, static_cast<const real*>(nullptr), chunk_size, &n1, &n2));
    write_pixel<real>(p, false, width, sum, noise_se(n1, n2, k_full), out_linear, out_rgb8, out_noise);
    if (out_support) out_support[size_t(p.j) * width + p.i] = 1.0f;
}

template <typename real>
hipError_t launch_resolve_tiles(const void* partial, const TileMap& tmap, int width, int height, int chunk_size, double samples_scale, const int32_t* list,
                                const int32_t* count, void* out_linear, uint8_t* out_rgb8, float* out_noise, float* out_support, hipStream_t stream) {
    if (tmap.n_tiles_local <= 0) return hipSuccess;
    const int k_full = int(tmap.chunk_start[tmap.n_chunks]) / chunk_size;
    rtk_resolve_tiles_kernel<real><<<dim3(pixel_slot_blocks(tmap)), dim3(256), 0, stream>>>(static_cast<const real*>(partial), tmap, width, height, chunk_size, k_full,
                                                                                           real(samples_scale), list, count, static_cast<real*>(out_linear), out_rgb8,
                                                                                           out_noise, out_support);
    return hipGetLastError();
}
template hipError_t launch_resolve_tiles<double>(const void*, const TileMap&, int, int, int, double, const int32_t*, const int32_t*, void*, uint8_t*, float*, float*,
                                                 hipStream_t);
template hipError_t launch_resolve_tiles<float>(const void*, const TileMap&, int, int, int, double, const int32_t*, const int32_t*, void*, uint8_t*, float*, float*,
                                                hipStream_t);

// ------------------------------------------------------------------ session set-up --
// A session is set up on ITS stream by kernels and asynchronous memsets: a blocking call on the NULL stream can be queued
// behind another stream's backlog (streams share the hardware queues), and rtk_progressive_create would then wait for the
// very stream it is documented not to wait for.  The camera record travels as a kernel argument, so no host memory has to
// outlive the call.
struct RecordWords {
    unsigned int w[64];
};
__global__ __launch_bounds__(64) void rtk_store_record_kernel(RecordWords rec, unsigned int n_words, unsigned int* __restrict__ dst) {
    if (threadIdx.x < n_words) dst[threadIdx.x] = rec.w[threadIdx.x];
}

hipError_t launch_store_record(const void* h_record, size_t bytes, void* d_dst, hipStream_t stream) {
    RecordWords rec{};
    if (bytes > sizeof rec || bytes % sizeof(unsigned int) != 0) return hipErrorInvalidValue;
    __builtin_memcpy(rec.w, h_record, bytes);
    rtk_store_record_kernel<<<dim3(1), dim3(64), 0, stream>>>(rec, static_cast<unsigned int>(bytes / sizeof(unsigned int)), static_cast<unsigned int*>(d_dst));
    return hipGetLastError();
}

// A fresh adaptive session: every tile of the rank that lies in the image is active, and none holds a sample.
__global__ __launch_bounds__(256) void rtk_adaptive_init_kernel(TileMap tmap, int32_t* __restrict__ active, int32_t* __restrict__ tile_spp) {
    const long long lt = (long long)blockIdx.x * 256 + threadIdx.x;
    if (lt >= tmap.n_tiles_local) return;
    active[lt] = lt * tmap.n_ranks + tmap.rank < (long long)tmap.tiles_x * tmap.tiles_y ? 1 : 0;
    tile_spp[lt] = 0;
}

hipError_t launch_adaptive_init(const TileMap& tmap, int32_t* active, int32_t* tile_spp, hipStream_t stream) {
    if (tmap.n_tiles_local <= 0) return hipSuccess;
    rtk_adaptive_init_kernel<<<dim3((tmap.n_tiles_local + 255) / 256), dim3(256), 0, stream>>>(tmap, active, tile_spp);
    return hipGetLastError();
}

}  // namespace rtk
