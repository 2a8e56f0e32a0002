// rtk_probe.hip -- the light probes' lookup (include/rtk.h "Light probes"): irradiance at points with normals from a grid of
// baked SH coefficients.  One lane per point: the trilinear weights of the eight probes around the point, eight weighted reads of
// 27 reals, then E(n) = sum_i A_i c_i Y_i(n) -- all in `real`.  A few hundred bytes read per point against a few hundred
// operations: HBM/L2-bound, no LDS.  The bake (rtk_probe_bake_kernel) is rtk_trace.hip's, its C-ABI half rtk_probe.cpp.
#include <hip/hip_runtime.h>

#include "rtk.h"
#include "rtk_device_math.h"
#include "rtk_internal.h"

namespace rtk {
namespace {

template <typename real>
struct ProbeGridRec {
    real origin[3], spacing[3];
    int counts[3];
};

// Along one axis with n probes: the lower probe i of the pair around coordinate g (in probe units, clamped to the grid; a NaN
// goes to probe 0) and the weight f of the upper one.  n == 1: probe 0 with f = 0, so the pair's upper index is never used with
// a weight.  The last probe is reached as i = n - 2, f = 1.
template <typename real>
RTK_DEV void probe_cell(real p, real origin, real spacing, int n, int& i, real& f) {
    real g = (p - origin) / spacing;
    const real last = real(n - 1);
    g = g > real(0) ? g : real(0);
    g = g < last ? g : last;
    i = int(g);
    if (i > n - 2) i = n - 2;
    if (i < 0) i = 0;
    f = g - real(i);
}

template <typename real>
__global__ __launch_bounds__(256) void rtk_probe_irradiance_kernel(ProbeGridRec<real> G, const real* __restrict__ sh, long long m, const real* __restrict__ points,
                                                                    const real* __restrict__ normals, real* __restrict__ out) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= m) return;
    const real* p = points + gid * 3;
    int i0[3];
    real f[3];
    for (int a = 0; a < 3; a++) probe_cell(p[a], G.origin[a], G.spacing[a], G.counts[a], i0[a], f[a]);
    real c[27];
    for (int q = 0; q < 27; q++) c[q] = real(0);
    for (int corner = 0; corner < 8; corner++) {                   // x fastest, as the coefficients are stored
        const int dx = corner & 1, dy = (corner >> 1) & 1, dz = corner >> 2;
        const int ix = min(i0[0] + dx, G.counts[0] - 1), iy = min(i0[1] + dy, G.counts[1] - 1), iz = min(i0[2] + dz, G.counts[2] - 1);
        const real w = ((dx ? f[0] : real(1) - f[0]) * (dy ? f[1] : real(1) - f[1])) * (dz ? f[2] : real(1) - f[2]);
        const real* s = sh + ((long long)(iz * G.counts[1] + iy) * G.counts[0] + ix) * 27;
        for (int q = 0; q < 27; q++) c[q] = c[q] + w * s[q];
    }
    const real* nrm = normals + gid * 3;
    const real x = nrm[0], y = nrm[1], z = nrm[2];
    const real pi = real(3.14159265358979323846), a0 = pi, a1 = real(2) * pi / real(3), a2 = pi / real(4);
    const real AY[9] = {a0 * real(0.28209479177387814),
                        a1 * (real(0.4886025119029199) * y),
                        a1 * (real(0.4886025119029199) * z),
                        a1 * (real(0.4886025119029199) * x),
                        a2 * (real(1.0925484305920792) * (x * y)),
                        a2 * (real(1.0925484305920792) * (y * z)),
                        a2 * (real(0.31539156525252005) * (real(3) * (z * z) - real(1))),
                        a2 * (real(1.0925484305920792) * (x * z)),
                        a2 * (real(0.5462742152960396) * (x * x - y * y))};
    real* o = out + gid * 3;
    for (int ch = 0; ch < 3; ch++) {
        real e = real(0);
        for (int i = 0; i < 9; i++) e = e + c[i * 3 + ch] * AY[i];
        o[ch] = e;
    }
}

template <typename real>
hipError_t launch_probe_irradiance(const rtk_probe_grid& grid, const void* d_sh, long long m, const void* d_points, const void* d_normals, void* d_out,
                                   hipStream_t stream) {
    ProbeGridRec<real> G;
    const double origin[3] = {grid.origin.x, grid.origin.y, grid.origin.z}, spacing[3] = {grid.spacing.x, grid.spacing.y, grid.spacing.z};
    for (int a = 0; a < 3; a++) {
        G.origin[a] = real(origin[a]);
        G.spacing[a] = real(spacing[a]);
        G.counts[a] = grid.counts[a];
    }
    rtk_probe_irradiance_kernel<real><<<dim3((unsigned int)((m + 255) / 256)), dim3(256), 0, stream>>>(
        G, static_cast<const real*>(d_sh), m, static_cast<const real*>(d_points), static_cast<const real*>(d_normals), static_cast<real*>(d_out));
    return hipGetLastError();
}

// What both forms check first, without a device; the context comes afterwards (no scene is read).
int check_irradiance_args(const char* who, int real_mode, const rtk_probe_grid* grid, const void* sh, const char* sh_name, int64_t m,
                          const void* points, const char* points_name, const void* normals, const char* normals_name, const void* out, const char* out_name) {
    if (check_real_mode(who, real_mode) != RTK_OK) return RTK_ERR_INVALID;
    if (!grid) return fail(RTK_ERR_INVALID, "%s: null grid", who);
    int64_t probes = 1;
    for (int a = 0; a < 3; a++) {
        if (grid->counts[a] < 1) return fail(RTK_ERR_INVALID, "%s: grid counts must be at least 1 (counts[%d] = %d)", who, a, grid->counts[a]);
        probes *= grid->counts[a];
        if (probes > int64_t(0x7FFFFFFF)) return fail(RTK_ERR_INVALID, "%s: grid counts: more than 2^31 - 1 probes", who);
    }
    const double spacing[3] = {grid->spacing.x, grid->spacing.y, grid->spacing.z};
    for (int a = 0; a < 3; a++) {  // ... as the kernel sees it: in F32 mode a spacing that rounds to 0 as a float is no spacing
        const double seen = real_mode == RTK_REAL_F64 ? spacing[a] : double(float(spacing[a]));
        if (!(seen > 0.0)) return fail(RTK_ERR_INVALID, "%s: grid spacing must be positive in the real type (spacing[%d] = %g)", who, a, spacing[a]);
    }
    if (grid->reserved != 0) return fail(RTK_ERR_INVALID, "%s: grid reserved must be 0", who);
    if (m < 0 || m > int64_t(0x7FFFFFFF)) return fail(RTK_ERR_INVALID, "%s: m must be 0 .. 2^31 - 1 (%lld)", who, (long long)m);
    if (!sh) return fail(RTK_ERR_INVALID, "%s: null %s", who, sh_name);
    if (!points) return fail(RTK_ERR_INVALID, "%s: null %s", who, points_name);
    if (!normals) return fail(RTK_ERR_INVALID, "%s: null %s", who, normals_name);
    if (!out) return fail(RTK_ERR_INVALID, "%s: null %s", who, out_name);
    return RTK_OK;
}

}  // namespace
}  // namespace rtk

using namespace rtk;

extern "C" {

int rtk_probe_irradiance(rtk_ctx* ctx, int real_mode, const rtk_probe_grid* grid, const void* d_sh, int64_t m, const void* d_points, const void* d_normals,
                         void* d_irradiance, void* stream) {
    const char* who = "rtk_probe_irradiance";
    if (check_irradiance_args(who, real_mode, grid, d_sh, "d_sh", m, d_points, "d_points", d_normals, "d_normals", d_irradiance, "d_irradiance") != RTK_OK)
        return RTK_ERR_INVALID;
    const size_t real_bytes = real_mode == RTK_REAL_F64 ? sizeof(double) : sizeof(float);
    if (check_aligned(d_sh, real_bytes, who, "d_sh") != RTK_OK || check_aligned(d_points, real_bytes, who, "d_points") != RTK_OK ||
        check_aligned(d_normals, real_bytes, who, "d_normals") != RTK_OK || check_aligned(d_irradiance, real_bytes, who, "d_irradiance") != RTK_OK)
        return RTK_ERR_INVALID;
    const int rc = check_ctx(who, ctx, false);
    if (rc != RTK_OK || m == 0) return rc;
    hipError_t e = hipSetDevice(ctx_device(ctx));
    if (e == hipSuccess) {
        const hipStream_t st = static_cast<hipStream_t>(stream);
        e = with_real(real_mode, [&](auto real) { return launch_probe_irradiance<decltype(real)>(*grid, d_sh, m, d_points, d_normals, d_irradiance, st); });
    }
    return launched(who, e);
}

int rtk_probe_irradiance_host(rtk_ctx* ctx, int real_mode, const rtk_probe_grid* grid, const double* h_sh, int64_t m, const double* h_points,
                              const double* h_normals, double* h_irradiance) {
    const char* who = "rtk_probe_irradiance_host";
    int rc = check_irradiance_args(who, real_mode, grid, h_sh, "h_sh", m, h_points, "h_points", h_normals, "h_normals", h_irradiance, "h_irradiance");
    if (rc != RTK_OK) return rc;
    rc = check_ctx(who, ctx, false);
    if (rc != RTK_OK || m == 0) return rc;
    rc = launched(who, hipSetDevice(ctx_device(ctx)));
    if (rc != RTK_OK) return rc;
    const size_t probes = size_t(grid->counts[0]) * grid->counts[1] * grid->counts[2];
    HostStaging s(real_mode == RTK_REAL_F64);
    const int sh = s.linear(probes * 3 * RTK_PROBE_COEFFS), points = s.linear(size_t(m) * 3), normals = s.linear(size_t(m) * 3), out = s.linear(size_t(m) * 3);
    return run_host_form(who, nullptr, s, {{sh, h_sh, true}, {points, h_points, true}, {normals, h_normals, true}},
                         [&] { return rtk_probe_irradiance(ctx, real_mode, grid, s.ptr(sh), m, s.ptr(points), s.ptr(normals), s.ptr(out), nullptr); },
                         {{out, h_irradiance, true}});
}

}  // extern "C"
