// Heights of the tau = 1 surface of an emergent spectrum (write_tau_unity, src/plot_utils.jl:434-576), on the device.
//
// Per wavelength and interior column (ix, iy) the march starts at the top plane with s = 0, tau = 0 and follows the
// characteristic of the up solve traced back downward (the upwind direction of xy_up_ray, src/characteristics.jl:
// 209-221): at plane iz the point is (z[iz], x[ix] + s k_x, y[iy] + s k_y), s = (z_top - z[iz]) / |k_z|.  alpha there
// is the bilinear value of the plane, periodic in x and y with period nx dx and ny dy.  tau accumulates by the
// trapezoid of cumtrapz (src/functions.jl:507-519) over the path steps r = |dz / k_z|, and the height is the z of the
// FIRST argmin |tau - 1| (Julia's argmin), top plane first.
//
// At k = (+-1, 0, 0) the lateral offsets are exactly zero, every alpha is a grid value and the steps are |dz|: the
// result is write_tau_unity(DATA) (:434-490) bit for bit, non-finite alpha included: the first plane whose tau is NaN
// is the minimum (Julia's argmin), and a zero fraction does not read the neighbouring column.  The inclined reference
// (:492-576) is NOT reproduced in three respects, all defects there: its lateral offset uses the step r of the current
// plane instead of the path s accumulated from the top, its horizontal sign (x - r k_x) is opposite to the solver's
// upwind point (x + s k_x), and its upper wrap assigns to misspelled variables (x_mrx, y_mrx), so a point past the
// upper edge is never wrapped.
//
// One thread per (wavelength, column); alpha in the ghosted layout of vrt_synth_opacity_dev (nlam, ny + 2, nx + 2, nz)
// numpy order, z fastest: a thread walks its own column downward, and the neighbouring columns of the bilinear
// interpolation are those of the neighbouring threads (shared through the caches).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "vrt_internal.h"

namespace vrt {

struct TauArgs {
    int64_t nz, nx, ny, nlam;                // interior raster
    double kz, kx, ky, dx, dy;               // direction; the uniform spacings of x and y
    const double *z;                         // [nz] device
    const double *alpha;                     // (nlam, ny + 2, nx + 2, nz)
    double *height;                          // (nlam, ny, nx)
};

__device__ __forceinline__ int64_t tau_wrap(int64_t i, int64_t n)
{
    i %= n;
    return i < 0 ? i + n : i;
}

// the plane's cell of an offset of u cells from column i (u = s k / d): first node and fraction in [0, 1)
__device__ __forceinline__ void tau_cell(double u, int64_t i, int64_t n, int64_t &i0, int64_t &i1, double &t)
{
    const double f = floor(u);
    t = u - f;
    i0 = tau_wrap(i + (int64_t)fmod(f, (double)n), n);
    i1 = i0 + 1 == n ? 0 : i0 + 1;
}

__global__ void __launch_bounds__(256)
k_tau_unity(TauArgs ta)
{
    const int64_t nz = ta.nz, nx = ta.nx, ny = ta.ny, ncol = nx * ny;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ncol * ta.nlam) return;
    const int64_t ix = t % nx, iy = (t / nx) % ny, l = t / ncol;
    const int64_t nxg = nx + 2;
    const double *__restrict__ A = ta.alpha + l * nz * nxg * (ny + 2);
    const double *__restrict__ z = ta.z;
    auto node = [&](int64_t i, int64_t j, int64_t iz) { return A[iz + nz * ((i + 1) + nxg * (j + 1))]; };
    const double z_top = z[nz - 1], akz = fabs(ta.kz);
    double prev = node(ix, iy, nz - 1);                          // s = 0: the column's own top value
    double tau = 0.0, best = 1.0;                                // |tau - 1| of the top plane
    int64_t arg = nz - 1;
    for (int64_t iz = nz - 2; iz >= 0; iz--) {
        const double s = (z_top - z[iz]) / akz;
        int64_t i0, i1, j0, j1;
        double tx, ty;
        tau_cell(s * ta.kx / ta.dx, ix, nx, i0, i1, tx);
        tau_cell(s * ta.ky / ta.dy, iy, ny, j0, j1, ty);
        // a zero fraction takes the grid value and does not read the other node: q + 0 (q' - q) is q for finite q',
        // but NaN for a NaN or Inf q' that the algorithm never uses (at k = (+-1, 0, 0): the neighbouring column)
        auto along_x = [&](int64_t j) {
            const double q0 = node(i0, j, iz);
            return tx != 0.0 ? q0 + tx * (node(i1, j, iz) - q0) : q0;
        };
        const double f0 = along_x(j0);
        double a = f0;
        if (ty != 0.0) a = f0 + ty * (along_x(j1) - f0);
        const double r = fabs((z[iz + 1] - z[iz]) / ta.kz);
        tau = tau + 0.5 * r * (a + prev);                        // cumtrapz: 0.5*abs(X[i] - X[i-1])*(Y[i] + Y[i-1])
        const double d = fabs(tau - 1.0);
        if (d != d) {                                            // Julia's argmin: the first NaN is the minimum
            arg = iz;
            break;
        }
        if (d < best) {
            best = d;
            arg = iz;
        }
        prev = a;
    }
    ta.height[t] = z[arg];
}

}  // namespace vrt

using namespace vrt;

// the uniform spacing of an ascending axis of n >= 2 points, or 0 (not uniform to a relative 1e-9)
static double uniform_spacing(const double *a, int64_t n)
{
    const double d = (a[n - 1] - a[0]) / (double)(n - 1);
    if (!(d > 0.0) || !std::isfinite(d)) return 0.0;
    for (int64_t i = 0; i + 1 < n; i++)
        if (!(std::fabs((a[i + 1] - a[i]) - d) <= 1e-9 * d)) return 0.0;
    return d;
}

static int tau_checks(int64_t nz, int64_t nx, int64_t ny, const double *z, const double *x, const double *y,
                      const double *k, int64_t nlam, const void *alpha, const void *height, double *dx, double *dy)
{
    if (!z || !x || !y || !k || !alpha || !height) return fail(VRT_EINVAL, "NULL argument");
    if (nz < 2 || nx < 2 || ny < 2) return fail(VRT_EINVAL, "need nz, nx, ny >= 2");
    if (nlam < 1) return fail(VRT_EINVAL, "nlam must be >= 1");
    const double nrm = std::sqrt(k[0] * k[0] + k[1] * k[1] + k[2] * k[2]);
    if (!(std::fabs(nrm - 1.0) < 1e-6)) return fail(VRT_EINVAL, "k is not a unit vector");
    if (k[0] == 0.0) return fail(VRT_EINVAL, "horizontal ray (k_z = 0) never leaves its plane");
    for (int64_t i = 0; i + 1 < nz; i++)
        if (!(z[i + 1] > z[i])) return fail(VRT_EINVAL, "z must be strictly ascending");
    *dx = uniform_spacing(x, nx);
    *dy = uniform_spacing(y, ny);
    if (*dx == 0.0 || *dy == 0.0) return fail(VRT_EINVAL, "x and y must be uniform and ascending");
    return VRT_OK;
}

static int tau_launch(int64_t nz, int64_t nx, int64_t ny, const double *z, const double *k, int64_t nlam, double dx,
                      double dy, const double *d_alpha, double *d_height, hipStream_t st)
{
    DevBuf<double> d_z;
    int rc = d_z.alloc((size_t)nz);
    if (rc) return rc;
    TauArgs ta;
    ta.nz = nz; ta.nx = nx; ta.ny = ny; ta.nlam = nlam;
    ta.kz = k[0]; ta.kx = k[1]; ta.ky = k[2]; ta.dx = dx; ta.dy = dy;
    ta.z = d_z; ta.alpha = d_alpha; ta.height = d_height;
    const int64_t n = nx * ny * nlam;
    hipError_t e = hipMemcpyAsync(d_z, z, sizeof(double) * (size_t)nz, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_tau_unity, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ta);
        e = hipGetLastError();
    }
    const hipError_t e2 = hipStreamSynchronize(st);       // (d_z is freed on return)
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) return fail(VRT_ENODEVICE, std::string("vrt_tau_unity: ") + hipGetErrorString(e));
    return VRT_OK;
}

// d_alpha, d_height: device pointers; runs on the calling thread's current HIP device and synchronises `stream`
extern "C" int vrt_tau_unity_dev(int64_t nz, int64_t nx, int64_t ny, const double *z, const double *x, const double *y,
                                 const double *k, int64_t nlam, const double *d_alpha, double *d_height, void *stream)
{
    return guarded([&] {
        double dx = 0, dy = 0;
        int rc = tau_checks(nz, nx, ny, z, x, y, k, nlam, d_alpha, d_height, &dx, &dy);
        if (!rc) rc = use_current_device();
        return rc ? rc : tau_launch(nz, nx, ny, z, k, nlam, dx, dy, d_alpha, d_height, (hipStream_t)stream);
    });
}

extern "C" int vrt_tau_unity(int64_t nz, int64_t nx, int64_t ny, const double *z, const double *x, const double *y,
                             const double *k, int64_t nlam, const double *alpha, int device, double *height)
{
    return guarded([&] {
        double dx = 0, dy = 0;
        int rc = tau_checks(nz, nx, ny, z, x, y, k, nlam, alpha, height, &dx, &dy);
        if (rc || (rc = use_device(device))) return rc;
        const size_t na = (size_t)(nz * (nx + 2) * (ny + 2)) * (size_t)nlam, nh = (size_t)(nx * ny) * (size_t)nlam;
        DevBuf<double> d;
        if ((rc = d.alloc(na + nh))) return rc;
        hipError_t e;
        if ((e = hipMemcpy(d, alpha, sizeof(double) * na, hipMemcpyHostToDevice)) != hipSuccess)
            return fail(VRT_ENODEVICE, std::string("vrt_tau_unity: ") + hipGetErrorString(e));
        if ((rc = tau_launch(nz, nx, ny, z, k, nlam, dx, dy, d, d + na, nullptr))) return rc;
        if ((e = hipMemcpy(height, d + na, sizeof(double) * nh, hipMemcpyDeviceToHost)) != hipSuccess)
            return fail(VRT_ENODEVICE, std::string("vrt_tau_unity: ") + hipGetErrorString(e));
        return VRT_OK;
    });
}
