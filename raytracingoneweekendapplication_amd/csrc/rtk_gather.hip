// rtk_gather.hip -- the surface gathers' kernels that trace nothing (include/rtk.h "Surface gathers"): the ray records of
// rtk_gather_rays, one lane each, and stage 2 of the two gathers, which adds the partial sums stage 1 left in the workspace -- one
// lane per (point, channel), the passes of a point in increasing order, one scale, one store.  Stage 1 (rtk_gather_irradiance_kernel,
// rtk_gather_occlusion_kernel) is rtk_trace.hip's, next to the path loop and the walk it runs; the C-ABI half is rtk_gather.cpp.
#include <hip/hip_runtime.h>

#include "rtk.h"
#include "rtk_gather_rule.h"
#include "rtk_trace.h"

namespace rtk {
namespace {

// The ray records of n points, point-major: lane gid writes ray gid % rays of point gid / rays as eleven 8-byte words.
__global__ __launch_bounds__(256) void rtk_gather_rays_kernel(long long n_rays, int rays, int spr, uint32_t first_key, uint32_t rotate, double time, double tmax,
                                                               const double* __restrict__ points, const double* __restrict__ normals, double* __restrict__ out) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= n_rays) return;
    const long long k = gid / rays;
    const uint32_t j = uint32_t(gid - k * rays), pixel = first_key + uint32_t(k);
    double d[3];
    gather_direction(j, rays, gather_rotation(rotate, pixel), normals + k * 3, d);
    const double* p = points + k * 3;
    double* o = out + gid * 11;
    o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
    o[3] = d[0]; o[4] = d[1]; o[5] = d[2];
    o[6] = time;
    o[7] = 0.001;
    o[8] = tmax;
    uint2* keys = reinterpret_cast<uint2*>(o + 9);
    keys[0] = make_uint2(pixel, j * uint32_t(spr));
    keys[1] = make_uint2(0u, 0u);
}

// Stage 2.  partial holds [n * passes][4] doubles, a point's passes consecutive.  Lane gid takes channel gid % channels of point
// gid / channels and adds its passes in increasing order.
// Irradiance (3 channels): out[k][ch] = (pi / rays) * sum.
template <typename real>
__global__ __launch_bounds__(256) void rtk_gather_irradiance_reduce_kernel(long long n, int rays, const double* __restrict__ partial, real* __restrict__ out) {
#pragma clang fp contract(off)
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= n * 3) return;
    const long long k = gid / 3;
    const int ch = int(gid - k * 3), passes = rays >> 6;
    const double* u = partial + k * passes * 4 + ch;
    double total = 0.0;
    for (int q = 0; q < passes; q++) total += u[(long long)q * 4];
    out[gid] = real(total * (3.14159265358979323846 / double(rays)));
}

// Occlusion (4 channels): open[k] = count / rays, bent[k][c] = sum_c / rays; either output may be null.
template <typename real>
__global__ __launch_bounds__(256) void rtk_gather_occlusion_reduce_kernel(long long n, int rays, const double* __restrict__ partial, real* __restrict__ open,
                                                                           real* __restrict__ bent) {
#pragma clang fp contract(off)
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= n * 4) return;
    const long long k = gid >> 2;
    const int c = int(gid & 3), passes = rays >> 6;
    const double* u = partial + k * passes * 4 + c;
    double total = 0.0;
    for (int q = 0; q < passes; q++) total += u[(long long)q * 4];
    const real v = real(total / double(rays));
    if (c == 0) {
        if (open) open[k] = v;
    } else if (bent) {
        bent[k * 3 + (c - 1)] = v;
    }
}

dim3 lanes(long long n) { return dim3((unsigned int)((n + 255) / 256)); }

}  // namespace

hipError_t launch_gather_rays(long long n, int rays, int samples, uint32_t first_key, uint32_t rotate, double time, double tmax, const double* d_points,
                              const double* d_normals, void* d_rays, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    rtk_gather_rays_kernel<<<lanes(n * rays), dim3(256), 0, stream>>>(n * rays, rays, samples, first_key, rotate, time, tmax, d_points, d_normals,
                                                                        static_cast<double*>(d_rays));
    return hipGetLastError();
}

template <typename real>
hipError_t launch_gather_irradiance_reduce(long long n, int rays, const double* d_partial, void* d_irradiance, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    rtk_gather_irradiance_reduce_kernel<real><<<lanes(n * 3), dim3(256), 0, stream>>>(n, rays, d_partial, static_cast<real*>(d_irradiance));
    return hipGetLastError();
}
template hipError_t launch_gather_irradiance_reduce<double>(long long, int, const double*, void*, hipStream_t);
template hipError_t launch_gather_irradiance_reduce<float>(long long, int, const double*, void*, hipStream_t);

template <typename real>
hipError_t launch_gather_occlusion_reduce(long long n, int rays, const double* d_partial, void* d_open, void* d_bent, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    rtk_gather_occlusion_reduce_kernel<real><<<lanes(n * 4), dim3(256), 0, stream>>>(n, rays, d_partial, static_cast<real*>(d_open), static_cast<real*>(d_bent));
    return hipGetLastError();
}
template hipError_t launch_gather_occlusion_reduce<double>(long long, int, const double*, void*, void*, hipStream_t);
template hipError_t launch_gather_occlusion_reduce<float>(long long, int, const double*, void*, void*, hipStream_t);

}  // namespace rtk
