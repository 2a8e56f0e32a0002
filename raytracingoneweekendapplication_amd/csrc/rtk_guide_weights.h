// rtk_guide_weights.h -- the device expressions the guided a-trous filter (rtk_denoise.hip) and the guided upsampling pass
// (rtk_upsample.hip) share: the weights between two pixels' guides as include/rtk.h states them ("Denoiser", "Guides that
// follow mirrors").  Guides are the four float4s rtk_render_guides writes per pixel: {first albedo, hit}, {normal, depth},
// {seen albedo, end hit}, {end normal, path length}.  Every function is inlined into its caller.
#ifndef RTK_GUIDE_WEIGHTS_H
#define RTK_GUIDE_WEIGHTS_H

#include <hip/hip_runtime.h>

#include "rtk_image_pass.h"

namespace rtk {

#define RTK_GW static __device__ __forceinline__

// Depth gradient of guide float4 `slot` (1 = first hit, 3 = end hit): half the larger central difference, edges clamped.
RTK_GW float guide_depth_gradient(const float4* __restrict__ g, int slot, int i, int j, int W, int H) {
    const float zx = fabsf(g[(size_t(j) * W + clampi(i + 1, 0, W - 1)) * 4 + slot].w - g[(size_t(j) * W + clampi(i - 1, 0, W - 1)) * 4 + slot].w);
    const float zy = fabsf(g[(size_t(clampi(j + 1, 0, H - 1)) * W + i) * 4 + slot].w - g[(size_t(clampi(j - 1, 0, H - 1)) * W + i) * 4 + slot].w);
    return (zx > zy ? zx : zy) / 2.0f;
}

RTK_GW float normal_weight(float4 gp, bool np_zero, float np_len, float4 gq, float sigma_n) {
    const bool nq_zero = zero3(gq);
    if (np_zero || nq_zero) return np_zero && nq_zero ? 1.0f : 0.0f;
    const float c = (gp.x * gq.x + gp.y * gq.y + gp.z * gq.z) / (np_len * sqrtf(gq.x * gq.x + gq.y * gq.y + gq.z * gq.z));
    return c > 0.0f ? __powf(c, sigma_n) : 0.0f;
}

RTK_GW float depth_weight(float hit_p, float hit_q, float zp, float zq, float grad, float o, float sigma_z) {
    if (hit_p == 0.0f || hit_q == 0.0f) return 1.0f;
    return __expf(-fabsf(zp - zq) / (sigma_z * (grad * o + 1e-3f * zp) + 1e-6f));
}

// The albedo a demodulating pass divides by and multiplies back: max(seen albedo, 0.02) per channel.
RTK_GW float4 demodulation_albedo(float4 seen) {
    return make_float4(seen.x > 0.02f ? seen.x : 0.02f, seen.y > 0.02f ? seen.y : 0.02f, seen.z > 0.02f ? seen.z : 0.02f, 0.0f);
}

#undef RTK_GW

}  // namespace rtk

#endif  // RTK_GUIDE_WEIGHTS_H
