// rtk_frame_steps.h -- the steps every frame-assembly kernel shares (rtk_frame.hip, rtk_views.hip): the slot -> pixel
// addressing, the fold of a launch's partial-sum planes and the output of a pixel.  Each exists once, here: that a stepped, resumed,
// adaptive or batched frame is the one-shot frame bit for bit rests on every kernel performing these additions in this order.
#ifndef RTK_FRAME_STEPS_H
#define RTK_FRAME_STEPS_H

#include <hip/hip_runtime.h>

#include "rtk_device_layout.h"
#include "rtk_device_math.h"

namespace rtk {

// ------------------------------------------------------------------ shared steps --
// Thread -> (local tile, pixel of the tile, image coordinates).  in_grid: the tile exists (a rank's last local tile may lie
// beyond the image's tile grid); inside: its pixel (i, j) lies in the image as well.
struct PixelSlot {
    long long local_tile;
    int pix, i, j;
    bool in_grid, inside;
    RTK_DEV size_t plane() const { return size_t(local_tile) * 192 + pix; }  // this pixel in a [local tile][3][64] buffer
    RTK_DEV size_t word() const { return size_t(local_tile) * 64 + pix; }    // ... and in a [local tile][64] one
};
RTK_DEV PixelSlot pixel_slot(const TileMap& tmap, int width, int height) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const int pix = int(gid & 63);
    PixelSlot p;
    p.pix = pix;
    p.local_tile = gid >> 6;
    const long long tile = p.local_tile * tmap.n_ranks + tmap.rank;
    p.i = int(tile % tmap.tiles_x) * 8 + (pix & 7);
    p.j = int(tile / tmap.tiles_x) * 8 + (pix >> 3);
    p.in_grid = p.local_tile < tmap.n_tiles_local && tile < (long long)tmap.tiles_x * tmap.tiles_y;
    p.inside = p.in_grid && p.i < width && p.j < height;
    return p;
}
static int pixel_slot_blocks(const TileMap& tmap) { return int(((long long)tmap.n_tiles_local * 64 + 255) / 256); }

template <typename real>
RTK_DEV V3<real> load3(const real* p) { return mk(p[0], p[64], p[128]); }  // one pixel of a [3][64] tile
template <typename real>
RTK_DEV void store3(real* p, V3<real> v) {
    p[0] = v.x;
    p[64] = v.y;
    p[128] = v.z;
}

// Fold this launch's planes of pixel `p` into its running sum, the only place where partial sums are added.  The contract:
//   * `first` (plane 0 is the frame's or the session's first chunk): plane 0 BECOMES the sum -- 0.0 + (-0.0) is not -0.0 --
//     otherwise the sum so far is read from `acc`; then + c1, + c2, ... in index order.  A frame folded in several launches
//     over consecutive chunk ranges therefore performs the additions of one launch over all chunks.
//   * NOISE: every FULL chunk (chunk_size samples; a final partial chunk goes into the image only) also feeds the
//     batch-means sums S1 += y, S2 += y * y with y = ((x + y) + z) / (3 c) of that chunk's plane, in double.
template <bool NOISE, typename real>
RTK_DEV V3<real> fold_planes(const real* __restrict__ partial, const TileMap& tmap, const PixelSlot& p, bool first, const real* acc,
                             int chunk_size = 0, double* n1 = nullptr, double* n2 = nullptr) {
    const real* src = partial + p.plane();
    const size_t chunk_stride = size_t(tmap.n_tiles_local) * 192;
    const int c = first ? 1 : 0;
    V3<real> sum = first ? load3(src) : load3(acc + p.plane());
    [[maybe_unused]] const double three_c = 3.0 * double(chunk_size);
    for (int k = NOISE ? 0 : c; k < tmap.n_chunks; k++) {
        const V3<real> part = load3(src + size_t(k) * chunk_stride);
        if (k >= c) sum = sum + part;
        if constexpr (NOISE) {
            if (tmap.chunk_start[k + 1] - tmap.chunk_start[k] == chunk_size) {
                const double y = ((double(part.x) + double(part.y)) + double(part.z)) / three_c;
                *n1 = *n1 + y;
                *n2 = *n2 + y * y;
            }
        }
    }
    return sum;
}

// Write one pixel's outputs: the linear colour, its bytes (gamma / clamp / quantise, Camera.txt:77-89; row-major only) and the
// standard error -- into this rank's compact buffers ([local tile][3][64], [local tile][64]: every slot of the tile, so the
// gather moves whole tiles) or at (i, j) of the row-major image.  Null outputs are skipped.
template <typename real>
RTK_DEV void write_pixel(const PixelSlot& p, bool compact, int width, V3<real> colour, double se, real* __restrict__ out_linear,
                         uint8_t* __restrict__ out_rgb8, float* __restrict__ out_noise) {
    if (compact) {
        if (out_linear) store3(out_linear + p.plane(), colour);
        if (out_noise) out_noise[p.word()] = float(se);
    } else if (p.inside) {
        const size_t px = size_t(p.j) * width + p.i, idx = px * 3;
        if (out_linear) {
            out_linear[idx] = colour.x;
            out_linear[idx + 1] = colour.y;
            out_linear[idx + 2] = colour.z;
        }
        if (out_rgb8) {
            out_rgb8[idx] = to_byte(double(colour.x));
            out_rgb8[idx + 1] = to_byte(double(colour.y));
            out_rgb8[idx + 2] = to_byte(double(colour.z));
        }
        if (out_noise) out_noise[px] = float(se);
    }
}

}  // namespace rtk

#endif  // RTK_FRAME_STEPS_H
