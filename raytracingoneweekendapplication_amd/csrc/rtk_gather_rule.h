// rtk_gather_rule.h -- the direction rule of the surface gathers (include/rtk.h "Surface gathers"), shared by the kernel that
// writes the ray records (rtk_gather.hip) and the two that trace them (rtk_trace.hip), so that the three agree bit for bit.
#ifndef RTK_GATHER_RULE_H
#define RTK_GATHER_RULE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rtk_device_math.h"

namespace rtk {

// The rotation of point key `pixel` (= first_key + k, wrapped): 0 without rotation, else the key times 0x85EBCA6B mod 2^32.
RTK_DEV uint32_t gather_rotation(uint32_t rotate, uint32_t pixel) { return rotate ? pixel * 0x85EBCA6Bu : 0u; }

// World direction j of a point with `rays` rays, rotation `rot` and normal n: the cosine-weighted Fibonacci set (Malley's
// construction over a Fibonacci disc) in the branch-free frame of Duff et al. 2017.  In double, not renormalised, and with
// contraction off whatever the flags of the kernel it is inlined into; every product and sum left to right as written.
RTK_DEV void gather_direction(uint32_t j, int rays, uint32_t rot, const double* __restrict__ n, double d[3]) {
#pragma clang fp contract(off)
    const double u = double(2u * j + 1u) / double(2 * rays);
    const double r = __builtin_sqrt(u), z = __builtin_sqrt(1.0 - u);
    const uint32_t a32 = j * 2654435769u + rot;                    // the golden ratio in 32-bit fixed point
    const double phi = double(a32) * (6.283185307179586476925286766559 * 0x1p-32);
    const double x = r * cos(phi), y = r * sin(phi);
    const double nx = n[0], ny = n[1], nz = n[2];
    const double s = __builtin_copysign(1.0, nz);
    const double a = -1.0 / (s + nz);
    const double b = nx * ny * a;
    const double t[3] = {1.0 + s * nx * nx * a, s * b, -s * nx};
    const double bt[3] = {b, s + ny * ny * a, -ny};
    d[0] = x * t[0] + y * bt[0] + z * nx;
    d[1] = x * t[1] + y * bt[1] + z * ny;
    d[2] = x * t[2] + y * bt[2] + z * nz;
}

}  // namespace rtk

#endif  // RTK_GATHER_RULE_H
