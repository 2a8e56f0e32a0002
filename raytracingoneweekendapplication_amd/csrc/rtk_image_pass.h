// rtk_image_pass.h -- what the image passes (rtk_denoise.hip, rtk_temporal.hip, rtk_upsample.hip, rtk_display.hip) share on the
// device side and at the launch: the tile grid every one-lane-per-pixel kernel runs on, its lane -> pixel mapping, the small
// integer and guide predicates, and the choice of a launch function per arithmetic type and demodulation.  The byte conversion
// is rtk_device_math.h's to_byte; the host side of a pass (shared checks, the _host staging) is in rtk_internal.h.
#ifndef RTK_IMAGE_PASS_H
#define RTK_IMAGE_PASS_H

#include <hip/hip_runtime.h>

#include <type_traits>

#include "rtk_device_math.h"

namespace rtk {

// The 8x8 tiles over an image (the render's tile convention): one wave per tile, one lane per pixel, four tiles per 256-thread
// block.  The first member of a pass's kernel parameters.
struct TileGrid {
    int width, height, tiles_x, n_tiles;
};

inline TileGrid tile_grid(int width, int height) {
    const int tiles_x = (width + 7) / 8;
    return TileGrid{width, height, tiles_x, tiles_x * ((height + 7) / 8)};
}

// Lane -> pixel: wave w of the grid is tile w (row-major over tiles_x), lane l its pixel (l & 7, l >> 3).  False outside.
RTK_DEV bool lane_pixel(const TileGrid& G, int& i, int& j) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const int tile = int(gid >> 6), pix = int(gid & 63);
    if (tile >= G.n_tiles) return false;
    i = (tile % G.tiles_x) * 8 + (pix & 7);
    j = (tile / G.tiles_x) * 8 + (pix >> 3);
    return i < G.width && j < G.height;
}

RTK_DEV int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

RTK_DEV bool zero3(float4 v) { return v.x == 0.0f && v.y == 0.0f && v.z == 0.0f; }

// f(real{}, std::bool_constant<DEMOD>{}) for the arithmetic type and the demodulation asked for at run time: a pass writes its
// launch once, as a generic lambda over the two tags.
template <typename F>
auto with_real_demod(bool f64, bool demod, F&& f) {
    if (demod) return f64 ? f(double{}, std::true_type{}) : f(float{}, std::true_type{});
    return f64 ? f(double{}, std::false_type{}) : f(float{}, std::false_type{});
}

}  // namespace rtk

#endif  // RTK_IMAGE_PASS_H
