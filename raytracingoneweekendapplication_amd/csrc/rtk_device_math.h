// rtk_device_math.h -- the few device helpers the traversal (rtk_trace.hip) and the frame-assembly kernels
// (rtk_frame.hip) both use: the three-component vector and the byte conversion of the reference's image writer.
#ifndef RTK_DEVICE_MATH_H
#define RTK_DEVICE_MATH_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rtk {

template <typename real>
struct V3 {
    real x, y, z;
};
#define RTK_DEV __device__ __forceinline__

template <typename real> RTK_DEV V3<real> mk(real a, real b, real c) { return V3<real>{a, b, c}; }
template <typename real> RTK_DEV V3<real> operator+(V3<real> a, V3<real> b) { return V3<real>{a.x + b.x, a.y + b.y, a.z + b.z}; }
template <typename real> RTK_DEV V3<real> scale(real t, V3<real> a) { return V3<real>{t * a.x, t * a.y, t * a.z}; }

RTK_DEV uint8_t to_byte(double x) {  // Camera.txt:29-34,77-83
    double g = x > 0 ? __builtin_sqrt(x) : 0.0;
    g = g < 0.000 ? 0.000 : (g > 0.999 ? 0.999 : g);
    return uint8_t(int(255.999 * g));
}

}  // namespace rtk

#endif  // RTK_DEVICE_MATH_H
