// The line Λ-iteration on the regular grid, on the device: J_λ_regular's line method (src/lambda_iteration.jl:1-58) and
// Λ_regular's loop (:116-205), the regular half of the reference's Voronoi-versus-regular comparison (compare_line.jl).
//
//   vrt_regular_execute_line   J = Σ_a w_a I_a of every (angle, wavelength) solve from host arrays, α_tot made on the device
//   vrt_regular_lambda_*       the loop with library-owned device state: per iteration only the criterion's scalar comes back
//
// Layout.  The points are the raster's, ghost border included, n = nz nx ny.  The caller's arrays are in Julia order
// (point i = iz + nz (ix + nx iy), wavelength fastest: S[i nlam + l]); the solver works plane-major
// ([l][iz][iy][ix]).  A session keeps S, J and B_0 in the caller's layout for the pointwise steps (the update and
// the rates kernels of the Voronoi session, unchanged) and one plane-major copy of S for the solves; J is reduced
// plane-major and transposed once per iteration, S_new once (32 x 32 LDS tiles: four passes over nλ n doubles).  S and J
// in both layouts, and the order of those steps, are RasterStore's (vrt_raster_store.h).
//
// Chunking.  Solve g = a nλ + l runs over the active angles a (dirs != 0) with the wavelength fastest.  The solves go
// through in chunks whose workspace (α_tot and I of the chunk, the row-march coefficients) stays under
// VRT_REG_LAMBDA_BYTES; per chunk: α_tot straight into the solver's plane-major workspace (k_reg_line_opacity), the
// solves (regular_solve_planes: no transposes, I_0 per solve = B_0's bottom plane or zeros), and the reduction of
// the chunk's I into J (k_reg_reduce_J).  J[l] is summed angle after angle in quadrature order (J_λ .+= weights[i]
// .* I, :39, :47), each element by one thread, so that J is bit-identical for any chunking.  I never leaves the device.
//
// The diagonal operator (vrt_regular_lambda_use_operator).  With it on, every chunk also adds its solves' share
// of Λ* = Σ_a w_a c_a(p; α_a[l]) right after its opacity, from the α the chunk's solves read
// (launch_regular_line_lambda_diagonal, vrt_regular.hip: the same one-thread-per-element order, so Λ* is bit-identical
// for any chunking too), and the update is the ALI one of the Voronoi line session.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "vrt_device.h"
#include "vrt_line_case.h"
#include "vrt_raster_store.h"
#include "vrt_voigt.h"

namespace vrt {
namespace {

constexpr double kPiL = 3.14159265358979323846;

// Julia point index of plane-major position p = ix + nx (iy + ny iz)
__device__ __forceinline__ int64_t julia_of_plane(int64_t p, int nz, int nx, int ny)
{
    const int64_t ix = p % nx, t = p / nx;
    const int64_t iy = t % ny, iz = t / ny;
    return iz + (int64_t)nz * (ix + (int64_t)nx * iy);
}

// (n, nlam) wavelength-fastest in Julia point order -> [l][iz][iy][ix], through a 32 x 32 LDS tile (256 threads)
__global__ void __launch_bounds__(256)
k_reg_lam_to_planes(int nz, int nx, int ny, int nlam, const double *__restrict__ in, double *__restrict__ out)
{
    __shared__ double t[32][33];
    const int64_t vol = (int64_t)nz * nx * ny;
    const int64_t p0 = (int64_t)blockIdx.x * 32;
    const int l0 = (int)blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8) {                         // point p0 + r, wavelength l0 + tx: contiguous in l
        const int64_t p = p0 + r;
        const int l = l0 + tx;
        if (p < vol && l < nlam) t[r][tx] = in[julia_of_plane(p, nz, nx, ny) * nlam + l];
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {                         // wavelength l0 + r, point p0 + tx: contiguous in p
        const int64_t p = p0 + tx;
        const int l = l0 + r;
        if (p < vol && l < nlam) out[(int64_t)l * vol + p] = t[tx][r];
    }
}

// the inverse
__global__ void __launch_bounds__(256)
k_reg_lam_from_planes(int nz, int nx, int ny, int nlam, const double *__restrict__ in, double *__restrict__ out)
{
    __shared__ double t[32][33];
    const int64_t vol = (int64_t)nz * nx * ny;
    const int64_t p0 = (int64_t)blockIdx.x * 32;
    const int l0 = (int)blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8) {                         // wavelength l0 + r, point p0 + tx
        const int64_t p = p0 + tx;
        const int l = l0 + r;
        if (p < vol && l < nlam) t[r][tx] = in[(int64_t)l * vol + p];
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {                         // point p0 + r, wavelength l0 + tx
        const int64_t p = p0 + r;
        const int l = l0 + tx;
        if (p < vol && l < nlam) out[julia_of_plane(p, nz, nx, ny) * nlam + l] = t[tx][r];
    }
}

// out[l][q] = B0[nz q][l] for the nx ny points q = ix + nx iy of the bottom plane: B_λ(λ_l, T[1, :, :]) (:38), the I_0
// planes of the up solves, from B_0 (nlam, n)
__global__ void __launch_bounds__(256)
k_reg_bottom_planes(int64_t plane, int nz, int nlam, const double *__restrict__ B0, double *__restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= plane * nlam) return;
    const int64_t l = t / plane, q = t - l * plane;
    out[t] = B0[q * nz * nlam + l];
}

struct LinePoint {                      // per-point line inputs, device, Julia point order
    const double *lambda;               // [nlam]
    const double *velocity;             // (3, n): z, x, y per point
    const double *doppler, *gamma, *strength, *alpha_cont;
    double lambda0, c0;
};

// α_tot = strength H(a, v) / (√π ΔλD) + α_cont of the chunk's solves [g0, g0 + cnt) into the solver's plane-major
// workspace out[g - g0][iz][iy][ix], with v_los = dot(velocity, -k): the expressions of k_line_opacity (vrt_physics.hip,
// lambda_iteration.jl:28-35) with the same Voigt function.  One thread per point and angle (grid.y: the chunk's
// angles from a0), walking that angle's wavelengths of the chunk: the point's inputs are read once, every store is
// coalesced.
__global__ void __launch_bounds__(256)
k_reg_line_opacity(int nz, int nx, int ny, int nlam, int64_t g0, int64_t cnt, int64_t a0, int64_t na,
                   const double *__restrict__ ka, LinePoint lp, double *__restrict__ out)
{
    exp2_table_fill();
    __syncthreads();
    const int64_t vol = (int64_t)nz * nx * ny;
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= vol) return;
    const int64_t i = julia_of_plane(p, nz, nx, ny);
    const double dD = lp.doppler[i], ac = lp.alpha_cont[i];
    const double r_dD = 1.0 / dD;
    const double ga = lp.gamma[i] / (4.0 * kPiL * lp.c0 * dD);            // broadening.jl:87-89
    const double sp = lp.strength[i] / (sqrt(kPiL) * dD);                  // line.jl:133, :219-225
    const double vz = lp.velocity[3 * i], vx = lp.velocity[3 * i + 1], vy = lp.velocity[3 * i + 2];
    for (int64_t a = a0 + blockIdx.y; a < a0 + na; a += gridDim.y) {
        const double v_los = vz * (-ka[3 * a]) + vx * (-ka[3 * a + 1]) + vy * (-ka[3 * a + 2]);   // line.jl:126, :205
        const double shift = lp.lambda0 * v_los / lp.c0;
        const int64_t lo = g0 > a * nlam ? g0 : a * nlam;
        const int64_t hi = g0 + cnt < (a + 1) * nlam ? g0 + cnt : (a + 1) * nlam;
        for (int64_t g = lo; g < hi; g++) {
            const double lam = lp.lambda[g - a * nlam];
            const double av = ga * (lam * lam);
            const double v = (lam - lp.lambda0 + shift) * r_dD;                   // line.jl:132
            out[(g - g0) * vol + p] = fma(sp, humlicek_w4_re(v, av), ac);
        }
    }
}

// J[l][p] += w_a I[g - g0][p] over the chunk's solves g = a nlam + l, angle after angle (J_λ .+= weights[i] .* I): one
// thread per point and wavelength of the chunk (grid.y), so that every element is summed in quadrature order
__global__ void __launch_bounds__(256)
k_reg_reduce_J(int64_t vol, int nlam, int64_t g0, int64_t cnt, int64_t nl, const double *__restrict__ w,
               const double *__restrict__ I, double *__restrict__ J)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= vol) return;
    for (int64_t y = blockIdx.y; y < nl; y += gridDim.y) {
        const int64_t g1 = g0 + y;                               // the chunk's first solve of wavelength g1 % nlam
        double *Jl = J + (g1 % nlam) * vol + p;
        double acc = *Jl;
        for (int64_t g = g1; g < g0 + cnt; g += nlam) acc = acc + w[g / nlam] * I[(g - g0) * vol + p];
        *Jl = acc;
    }
}

}  // namespace

// ---- host side (the launchers and the solve list are shared with vrt_continuum.hip: vrt_regular.h) -------------------------

int launch_to_planes(const vrt_regular *r, int64_t nlam, const double *in, double *out, hipStream_t st)
{
    const int64_t vol = r->nz * r->nx * r->ny;
    hipLaunchKernelGGL(k_reg_lam_to_planes, dim3((unsigned)((vol + 31) / 32), (unsigned)((nlam + 31) / 32)), dim3(256), 0, st,
                       (int)r->nz, (int)r->nx, (int)r->ny, (int)nlam, in, out);
    VRT_HIP_TRY(hipGetLastError());
    return VRT_OK;
}

int launch_from_planes(const vrt_regular *r, int64_t nlam, const double *in, double *out, hipStream_t st)
{
    const int64_t vol = r->nz * r->nx * r->ny;
    hipLaunchKernelGGL(k_reg_lam_from_planes, dim3((unsigned)((vol + 31) / 32), (unsigned)((nlam + 31) / 32)), dim3(256), 0, st,
                       (int)r->nz, (int)r->nx, (int)r->ny, (int)nlam, in, out);
    VRT_HIP_TRY(hipGetLastError());
    return VRT_OK;
}

int launch_bottom_planes(const vrt_regular *r, int64_t nlam, const double *B0, double *out, hipStream_t st)
{
    const int64_t plane = r->nx * r->ny;
    hipLaunchKernelGGL(k_reg_bottom_planes, dim3((unsigned)((plane * nlam + 255) / 256)), dim3(256), 0, st, plane, (int)r->nz,
                       (int)nlam, B0, out);
    VRT_HIP_TRY(hipGetLastError());
    return VRT_OK;
}

// the checks of a direction set, before the device is touched
int check_angles(int64_t n_angles, const double *k, const int *dirs)
{
    if (n_angles < 1) return fail(VRT_EINVAL, "n_angles must be >= 1");
    for (int64_t a = 0; a < n_angles; a++) {
        if (dirs[a] < -1 || dirs[a] > 1) return fail(VRT_EINVAL, "dirs must be 1 (up), -1 (down) or 0 (skipped)");
        if (dirs[a] != 0) {
            const int rc = regular_check_k(1, k + 3 * a);
            if (rc) return rc;
        }
    }
    return VRT_OK;
}

int line_solves_init(LineSolves &ls, const vrt_regular *r, int64_t n_angles, const double *k, const int *dirs,
                     const double *weights, int64_t nlam)
{
    std::vector<double> ka, w;
    std::vector<int> up1;
    for (int64_t a = 0; a < n_angles; a++) {
        if (dirs[a] == 0) continue;                          // θ = 90: the reference adds nothing
        for (int j = 0; j < 3; j++) ka.push_back(k[3 * a + j]);
        w.push_back(weights[a]);
        up1.push_back(dirs[a] > 0 ? 1 : 0);
    }
    ls.A = (int64_t)w.size();
    ls.nlam = nlam;
    const int64_t n_solve = ls.A * nlam;
    ls.hk.resize(3 * (size_t)n_solve);
    std::vector<int> ups((size_t)n_solve);
    for (int64_t a = 0; a < ls.A; a++)
        for (int64_t l = 0; l < nlam; l++) {
            const size_t g = (size_t)(a * nlam + l);
            for (int j = 0; j < 3; j++) ls.hk[3 * g + (size_t)j] = ka[3 * (size_t)a + (size_t)j];
            ups[g] = up1[(size_t)a];
        }
    int rc;
    if ((rc = ls.d_ka.alloc(ka.size())) || (rc = ls.d_w.alloc(w.size())) || (rc = ls.d_ks.alloc(ls.hk.size())) ||
        (rc = ls.d_up.alloc(ups.size())))
        return rc;
    if (ls.A > 0) {
        VRT_HIP_TRY(hipMemcpy(ls.d_ka, ka.data(), sizeof(double) * ka.size(), hipMemcpyHostToDevice));
        VRT_HIP_TRY(hipMemcpy(ls.d_w, w.data(), sizeof(double) * w.size(), hipMemcpyHostToDevice));
        VRT_HIP_TRY(hipMemcpy(ls.d_ks, ls.hk.data(), sizeof(double) * ls.hk.size(), hipMemcpyHostToDevice));
        VRT_HIP_TRY(hipMemcpy(ls.d_up, ups.data(), sizeof(int) * ups.size(), hipMemcpyHostToDevice));
    }
    // workspace of a solve: α_tot and I (vol each) and the row-march coefficients (5 per point of a plane); the split
    // path's coefficients are chunked under 2 GiB inside regular_solve_planes
    const int64_t vol = r->nz * r->nx * r->ny, plane = r->nx * r->ny;
    const int64_t per_solve = (int64_t)sizeof(double) * (2 * vol + 5 * plane);
    const int64_t cap = std::max<int64_t>(1, std::min<int64_t>(std::max<int64_t>(n_solve, 1), r->lambda_bytes / per_solve));
    const int64_t nchunk = (std::max<int64_t>(n_solve, 1) + cap - 1) / cap;        // chunks of equal size under the cap
    ls.chunk = (std::max<int64_t>(n_solve, 1) + nchunk - 1) / nchunk;
    return VRT_OK;
}

int launch_reduce_J_planes(const vrt_regular *r, const LineSolves &ls, int64_t g0, int64_t cnt, double *dJ_pl, hipStream_t st)
{
    const int64_t vol = r->nz * r->nx * r->ny, nl = std::min(cnt, ls.nlam);
    hipLaunchKernelGGL(k_reg_reduce_J, dim3((unsigned)((vol + 255) / 256), (unsigned)std::min<int64_t>(nl, 65535)), dim3(256), 0, st,
                       vol, (int)ls.nlam, g0, cnt, nl, (const double *)ls.d_w, (const double *)r->d_I, dJ_pl);
    VRT_HIP_TRY(hipGetLastError());
    return VRT_OK;
}

namespace {

// dJ_pl ([l][iz][iy][ix]) = Σ_a w_a I_a over every solve, from the plane-major S and up-solve I_0 planes.  d_diag_pl, if
// not NULL: also Λ* of this pass's per-angle α_tot into those planes (launch_regular_line_lambda_diagonal), chunk after
// chunk while the chunk's α stands in the workspace; NULL: no launch more than without it
int line_J_pass(vrt_regular *r, const LineSolves &ls, const LinePoint &lp, const double *dS_pl, const double *dI0_pl,
                const double *dI0_zero, int n_sweeps, double *dJ_pl, hipStream_t st, double *d_diag_pl = nullptr)
{
    const int64_t nz = r->nz, nx = r->nx, ny = r->ny, vol = nz * nx * ny, nlam = ls.nlam;
    VRT_HIP_TRY(hipMemsetAsync(dJ_pl, 0, sizeof(double) * (size_t)(nlam * vol), st));
    if (d_diag_pl) VRT_HIP_TRY(hipMemsetAsync(d_diag_pl, 0, sizeof(double) * (size_t)(nlam * vol), st));
    const int64_t n_solve = ls.A * nlam;
    const unsigned bx = (unsigned)((vol + 255) / 256);
    int rc;
    for (int64_t g0 = 0; g0 < n_solve; g0 += ls.chunk) {
        const int64_t cnt = std::min(ls.chunk, n_solve - g0);
        if ((rc = r->d_A.grow((size_t)(cnt * vol)))) return rc;
        const int64_t a0 = g0 / nlam, na = (g0 + cnt - 1) / nlam - a0 + 1;
        hipLaunchKernelGGL(k_reg_line_opacity, dim3(bx, (unsigned)std::min<int64_t>(na, 65535)), dim3(256), 0, st, (int)nz,
                           (int)nx, (int)ny, (int)nlam, g0, cnt, a0, na, (const double *)ls.d_ka, lp, r->d_A);
        VRT_HIP_TRY(hipGetLastError());
        if (d_diag_pl && (rc = launch_regular_line_lambda_diagonal(r, ls, g0, cnt, r->d_A, d_diag_pl, st))) return rc;
        if ((rc = regular_solve_planes(r, cnt, ls.hk.data() + 3 * g0, ls.d_ks + 3 * g0, ls.d_up + g0, dS_pl, nlam, g0, r->d_A,
                                       dI0_pl, dI0_zero, n_sweeps, st)))
            return rc;
        if ((rc = launch_reduce_J_planes(r, ls, g0, cnt, dJ_pl, st))) return rc;
    }
    return VRT_OK;
}

}  // namespace
}  // namespace vrt

using namespace vrt;

struct vrt_regular_lambda {
    vrt_regular *r = nullptr;           // borrowed
    int device = 0, n_sweeps = 3;
    int64_t n = 0, nlam = 0;
    LineSolves ls;
    Stream st;
    // per point, Julia order
    LineCaseDev line;                   // the uploaded case, γ, the line strength and R (vrt_line_case.h)
    RasterStore sj;                     // S and J, rows and planes, and what the solves start from (vrt_raster_store.h)
    DevBuf<double> d_B0;
    DevBuf<double> d_pops[2];           // [pc]: the current populations
    int pc = 0;
    DevBuf<unsigned long long> d_scalars;
    int64_t iterations = 0;
    NgState ng;                         // vrt_regular_lambda_set_acceleration (off: nothing allocated, nothing run)
    // vrt_regular_lambda_use_operator (0: nothing allocated, nothing run): Λ* of the current iterate's α, plane-major as
    // the chunks leave it and as (n, nlam) rows for the update; nothing of it survives an iterate
    int op = 0;
    DevBuf<double> d_diag_pl, d_diag;
    int64_t fallback_last = 0;          // entries of the last iterate that took the plain update (den not > 0)
};

extern "C" {

int vrt_regular_execute_line(vrt_regular *r, int64_t n_angles, const double *k, const int *dirs, const double *weights,
                             int64_t nlam, const double *lambda, double lambda0, double c0, const double *velocity,
                             const double *doppler_width, const double *gamma, const double *line_strength,
                             const double *alpha_cont, const double *S, const double *I0_up, int n_sweeps, double *J)
{
    if (!r || !k || !dirs || !weights || !lambda || !velocity || !doppler_width || !gamma || !line_strength || !alpha_cont ||
        !S || !J)
        return fail(VRT_EINVAL, "NULL argument");
    if (nlam < 1 || n_sweeps < 1) return fail(VRT_EINVAL, "need nlam >= 1 and n_sweeps >= 1");
    if (!(lambda0 > 0) || !(c0 > 0)) return fail(VRT_EINVAL, "lambda0 and c0 must be positive");
    int rc = check_angles(n_angles, k, dirs);
    if (rc) return rc;
    return guarded([&] {
        if ((rc = use_device(r->device))) return rc;
        const int64_t vol = r->nz * r->nx * r->ny, plane = r->nx * r->ny;
        const size_t n = (size_t)vol, nS = n * (size_t)nlam, nP = (size_t)(plane * nlam);
        LineSolves ls;
        if ((rc = line_solves_init(ls, r, n_angles, k, dirs, weights, nlam))) return rc;
        DevBuf<double> d_vec, d_S, d_S_pl, d_J_pl, d_I0, d_zero;
        if ((rc = d_vec.alloc(7 * n + (size_t)nlam)) || (rc = d_S.alloc(nS)) || (rc = d_S_pl.alloc(nS)) ||
            (rc = d_J_pl.alloc(nS)) || (rc = d_I0.alloc(nP)) || (rc = d_zero.alloc((size_t)plane)))
            return rc;
        double *dv = d_vec;
        LinePoint lp;
        lp.velocity = dv; lp.doppler = dv + 3 * n; lp.gamma = dv + 4 * n; lp.strength = dv + 5 * n; lp.alpha_cont = dv + 6 * n;
        lp.lambda = dv + 7 * n; lp.lambda0 = lambda0; lp.c0 = c0;
        VRT_HIP_TRY(hipMemcpy(dv, velocity, sizeof(double) * 3 * n, hipMemcpyHostToDevice));
        VRT_HIP_TRY(hipMemcpy(dv + 3 * n, doppler_width, sizeof(double) * n, hipMemcpyHostToDevice));
        VRT_HIP_TRY(hipMemcpy(dv + 4 * n, gamma, sizeof(double) * n, hipMemcpyHostToDevice));
        VRT_HIP_TRY(hipMemcpy(dv + 5 * n, line_strength, sizeof(double) * n, hipMemcpyHostToDevice));
        VRT_HIP_TRY(hipMemcpy(dv + 6 * n, alpha_cont, sizeof(double) * n, hipMemcpyHostToDevice));
        VRT_HIP_TRY(hipMemcpy(dv + 7 * n, lambda, sizeof(double) * (size_t)nlam, hipMemcpyHostToDevice));
        VRT_HIP_TRY(hipMemcpy(d_S, S, sizeof(double) * nS, hipMemcpyHostToDevice));
        hipStream_t st = nullptr;
        VRT_HIP_TRY(hipMemsetAsync(d_zero, 0, sizeof(double) * (size_t)plane, st));
        if (I0_up)                                           // (nx, ny, nlam) Julia order is [l][iy][ix]: the solver's planes
            VRT_HIP_TRY(hipMemcpy(d_I0, I0_up, sizeof(double) * nP, hipMemcpyHostToDevice));
        else
            VRT_HIP_TRY(hipMemsetAsync(d_I0, 0, sizeof(double) * nP, st));
        if ((rc = launch_to_planes(r, nlam, d_S, d_S_pl, st))) return rc;
        if ((rc = line_J_pass(r, ls, lp, d_S_pl, d_I0, d_zero, n_sweeps, d_J_pl, st))) return rc;
        if ((rc = launch_from_planes(r, nlam, d_J_pl, d_S, st))) return rc;
        VRT_HIP_TRY(hipStreamSynchronize(st));
        VRT_HIP_TRY(hipMemcpy(J, d_S, sizeof(double) * nS, hipMemcpyDeviceToHost));
        r->timed = false;                                    // (the handle's events saw only the last chunk)
        regular_release_workspace(r);                        // (tens of GB at a user's size: not kept on the handle)
        return VRT_OK;
    });
}

int vrt_regular_lambda_create(vrt_regular *r, int64_t n_angles, const double *k, const int *dirs, const double *weights,
                              const vrt_line_case *lc, int n_sweeps, vrt_regular_lambda **out)
{
    if (!out) return fail(VRT_EINVAL, "out is NULL");
    *out = nullptr;
    if (!r || !k || !dirs || !weights || !lc) return fail(VRT_EINVAL, "NULL argument");
    const int64_t nlam = lc->nlam;
    // (n_sweeps is reported after nlam and before the rest of the case, as it always was)
    if (nlam >= 2 && n_sweeps < 1) return fail(VRT_EINVAL, "n_sweeps must be >= 1");
    int rc = check_line_case(lc);
    if (rc || (rc = check_angles(n_angles, k, dirs))) return rc;
    return guarded([&] {
        if ((rc = use_device(r->device))) return rc;
        std::unique_ptr<vrt_regular_lambda> s(new vrt_regular_lambda());
        s->r = r;
        s->device = r->device;
        s->n_sweeps = n_sweeps;
        const int64_t vol = r->nz * r->nx * r->ny;
        s->n = vol;
        s->nlam = nlam;
        if ((rc = line_solves_init(s->ls, r, n_angles, k, dirs, weights, nlam))) return rc;
        if ((rc = s->st.create())) return rc;
        const size_t n = (size_t)vol, nS = n * (size_t)nlam;
        hipStream_t st = s->st;
#define VRT_S(expr) do { if ((rc = (expr))) return rc; } while (0)
        VRT_S(s->line.create(lc, vol, st));
        VRT_S(upload(s->d_B0, lc->B0, nS, st));
        VRT_S(upload(s->d_pops[0], lc->lte_populations, 3 * n, st));        // populations = copy(LTE_pops), :127
        VRT_S(s->sj.create(r, nlam, s->d_B0, st));           // S_new = B_0, :150; I_0 = B_λ(λ_l, T[1, :, :]), :38
        VRT_S(s->d_pops[1].alloc(3 * n));
        VRT_S(s->d_scalars.alloc(kUpdateWords));
        // (R and γ, like the store's J, are those of "no iteration yet": zeros)
        VRT_HIP_TRY(hipMemsetAsync(s->line.d_R, 0, sizeof(double) * 9 * n, st));
        VRT_HIP_TRY(hipMemsetAsync(s->line.d_gamma, 0, sizeof(double) * n, st));
#undef VRT_S
        VRT_HIP_TRY(hipStreamSynchronize(st));               // the host arrays may go after return
        *out = s.release();
        return VRT_OK;
    });
}

int vrt_regular_lambda_iterate(vrt_regular_lambda *s, double *max_rel_change)
{
    if (!s || !max_rel_change) return fail(VRT_EINVAL, "NULL argument");
    return guarded([&] {
        int rc = use_device(s->device);
        if (rc) return rc;
        hipStream_t st = s->st;
        const int64_t n = s->n, nlam = s->nlam;
        RasterStore &sj = s->sj;
        // γ and the line strength of the current populations (:13-16, line.jl:219-225)
        LineCaseDev &line = s->line;
        if ((rc = line.terms(s->d_pops[s->pc], st))) return rc;
        // α_tot of every angle, J_λ (:22-55) from S_old = the last S_new (:165-167)
        LinePoint lp;
        lp.lambda = small_view(line.d_small, nlam, line.k.blocks).lambda; lp.velocity = line.d_velocity; lp.doppler = line.d_doppler;
        lp.gamma = line.d_gamma; lp.strength = line.d_strength; lp.alpha_cont = line.d_alpha_cont; lp.lambda0 = line.k.lambda0;
        lp.c0 = line.k.c0;
        // (with the operator on also Λ* of that α, formed beside the solves that read the same workspace)
        if ((rc = line_J_pass(s->r, s->ls, lp, sj.S_planes(), sj.I0_planes(), sj.zero_plane(), s->n_sweeps, sj.J_planes(), st,
                              s->op ? s->d_diag_pl.get() : nullptr)))
            return rc;
        if ((rc = sj.J_home(st))) return rc;
        if (s->op && (rc = sj.rows_from_planes(s->d_diag_pl, s->d_diag, st))) return rc;
        // S_new = (1 - ε) J + ε B_0 (:169-171) and the criterion's scalar; S_new also plane-major for the next solves.  With
        // the operator on (d_diag is NULL otherwise): the ALI update
        if ((rc = launch_lambda_update(n, nlam, nlam, sj.J_rows(), s->d_B0, line.d_eps, sj.S_rows(), sj.S_next(), s->d_scalars, st,
                                       s->op ? s->d_diag.get() : nullptr)))
            return rc;
        if ((rc = sj.S_written(st))) return rc;
        // R, populations (:176, :181)
        if ((rc = launch_rates_populations(line.rates_in(), RatesJ::from_rows(sj.J_rows(), nlam), line.d_R, s->d_pops[s->pc ^ 1], st)))
            return rc;
        s->pc ^= 1;
        // (the third word: the ALI update's, in the same copy; with the operator off fallback_last is 0 and stays)
        if ((rc = read_criterion(s->d_scalars, s->op ? 3 : 2, st, max_rel_change, &s->fallback_last))) return rc;
        s->r->timed = false;                                 // (the handle's events saw only the last chunk)
        s->iterations++;
        // history copy or Ng step on the S of the plain update; an accepted x_acc becomes the store's S, and the plane-major
        // copy the next solves read is made again from it
        return ng_after_update(s->ng, s->iterations, sj, st);
    });
}

int vrt_regular_lambda_set_acceleration(vrt_regular_lambda *s, int order, int start, int period)
{
    if (!s) return fail(VRT_EINVAL, "NULL session");
    int rc = ng_check_settings(order, start, period);
    if (rc) return rc;
    return guarded([&] {
        if ((rc = use_device(s->device))) return rc;
        VRT_HIP_TRY(hipStreamSynchronize(s->st));
        return ng_configure(s->ng, order, start, period, s->sj.ng_count());
    });
}

int vrt_regular_lambda_use_operator(vrt_regular_lambda *s, int op)
{
    if (!s) return fail(VRT_EINVAL, "NULL session");
    if (op != 0 && op != 1) return fail(VRT_EINVAL, "operator must be 0 (plain) or 1 (diagonal)");
    return guarded([&] {
        int rc = use_device(s->device);
        if (rc) return rc;
        if (op == s->op) return (int)VRT_OK;
        VRT_HIP_TRY(hipStreamSynchronize(s->st));
        if (op) {
            // both arrays beside the session: it is untouched unless both exist
            const size_t nS = (size_t)s->n * (size_t)s->nlam;
            DevBuf<double> pl, rows;
            if ((rc = pl.alloc(nS)) || (rc = rows.alloc(nS))) return rc;
            s->d_diag_pl = std::move(pl);
            s->d_diag = std::move(rows);
        } else {
            s->d_diag_pl = DevBuf<double>();
            s->d_diag = DevBuf<double>();
        }
        s->op = op;
        s->fallback_last = 0;
        s->ng.have = 0;                                      // iterates of another fixed-point map are no history of this one
        return (int)VRT_OK;
    });
}

int vrt_regular_lambda_get_operator(const vrt_regular_lambda *s, int *op, int64_t *fallback_entries_last_iterate)
{
    if (!s || !op) return fail(VRT_EINVAL, "NULL argument");
    *op = s->op;
    if (fallback_entries_last_iterate) *fallback_entries_last_iterate = s->fallback_last;
    return VRT_OK;
}

// Λ* of per-angle α planes [a][l][iz][iy][ix] (active angles in order) into d_diag_pl [l][iz][iy][ix]: the session's kernel
// on the whole solve list as one chunk
static int line_diagonal_planes(vrt_regular *r, int64_t n_angles, const double *k, const int *dirs, const double *weights,
                                int64_t nlam, const double *d_alpha_pl, double *d_diag_pl, hipStream_t st)
{
    LineSolves ls;
    int rc = line_solves_init(ls, r, n_angles, k, dirs, weights, nlam);
    if (rc) return rc;
    const int64_t vol = r->nz * r->nx * r->ny;
    VRT_HIP_TRY(hipMemsetAsync(d_diag_pl, 0, sizeof(double) * (size_t)(nlam * vol), st));
    if (ls.A > 0 && (rc = launch_regular_line_lambda_diagonal(r, ls, 0, ls.A * nlam, d_alpha_pl, d_diag_pl, st))) return rc;
    VRT_HIP_TRY(hipStreamSynchronize(st));                   // (the solve list goes here)
    return VRT_OK;
}

int vrt_regular_line_lambda_diagonal_dev(vrt_regular *r, int64_t n_angles, const double *k, const int *dirs, const double *weights,
                                         int64_t nlam, const double *d_alpha_pl, double *d_diag_pl, void *stream)
{
    if (!r || !k || !dirs || !weights || !d_alpha_pl || !d_diag_pl) return fail(VRT_EINVAL, "NULL argument");
    if (nlam < 1) return fail(VRT_EINVAL, "need nlam >= 1");
    int rc = check_angles(n_angles, k, dirs);
    if (rc) return rc;
    return guarded([&] {
        if ((rc = use_device(r->device))) return rc;
        return line_diagonal_planes(r, n_angles, k, dirs, weights, nlam, d_alpha_pl, d_diag_pl, (hipStream_t)stream);
    });
}

int vrt_regular_line_lambda_diagonal(vrt_regular *r, int64_t n_angles, const double *k, const int *dirs, const double *weights,
                                     int64_t nlam, int64_t ld, const double *alpha, double *diag)
{
    if (!r || !k || !dirs || !weights || !alpha || !diag) return fail(VRT_EINVAL, "NULL argument");
    if (nlam < 1 || ld < nlam) return fail(VRT_EINVAL, "need nlam >= 1 and ld >= nlam");
    int rc = check_angles(n_angles, k, dirs);
    if (rc) return rc;
    return guarded([&] {
        const int64_t n = r->nz * r->nx * r->ny;
        int64_t A = 0;
        for (int64_t a = 0; a < n_angles; a++) {
            if (dirs[a] == 0) continue;                      // (never read)
            A++;
            for (int64_t i = 0; i < n; i++)
                for (int64_t l = 0; l < nlam; l++) {
                    const double v = alpha[(a * n + i) * ld + l];
                    if (!std::isfinite(v) || !(v > 0.0)) return fail(VRT_EINVAL, "alpha must be finite and > 0 everywhere");
                }
        }
        if ((rc = use_device(r->device))) return rc;
        const size_t nS = (size_t)n * (size_t)nlam, row = sizeof(double) * (size_t)nlam, pitch = sizeof(double) * (size_t)ld;
        DevBuf<double> d_rows, d_alpha_pl, d_diag_pl;
        if ((rc = d_rows.alloc(nS)) || (rc = d_alpha_pl.alloc(nS * (size_t)std::max<int64_t>(A, 1))) || (rc = d_diag_pl.alloc(nS)))
            return rc;
        hipStream_t st = nullptr;
        int64_t b = 0;
        for (int64_t a = 0; a < n_angles; a++) {             // the active angles' rows, one after the other, into planes
            if (dirs[a] == 0) continue;
            VRT_HIP_TRY(hipMemcpy2DAsync(d_rows, row, alpha + a * n * ld, pitch, row, (size_t)n, hipMemcpyHostToDevice, st));
            if ((rc = launch_to_planes(r, nlam, d_rows, d_alpha_pl + (size_t)b * nS, st))) return rc;
            b++;
        }
        if ((rc = line_diagonal_planes(r, n_angles, k, dirs, weights, nlam, d_alpha_pl, d_diag_pl, st))) return rc;
        if ((rc = launch_from_planes(r, nlam, d_diag_pl, d_rows, st))) return rc;
        VRT_HIP_TRY(hipStreamSynchronize(st));
        // (the padding columns of diag stay as they came)
        VRT_HIP_TRY(hipMemcpy2D(diag, pitch, d_rows, row, row, (size_t)n, hipMemcpyDeviceToHost));
        return VRT_OK;
    });
}

int vrt_regular_lambda_last_acceleration(const vrt_regular_lambda *s, int *applied, double sums[5], double coeffs[2])
{
    if (!s || !applied) return fail(VRT_EINVAL, "NULL argument");
    return ng_report(s->ng, applied, sums, coeffs);
}

int vrt_regular_lambda_get(vrt_regular_lambda *s, double *J, double *S, double *populations, double *R, double *gamma)
{
    if (!s) return fail(VRT_EINVAL, "NULL session");
    return guarded([&] {
        int rc = use_device(s->device);
        if (rc) return rc;
        const size_t n = (size_t)s->n;
        if ((rc = s->sj.download(J, S, s->st))) return rc;   // (synchronises the stream)
        if (populations) VRT_HIP_TRY(hipMemcpy(populations, s->d_pops[s->pc], sizeof(double) * 3 * n, hipMemcpyDeviceToHost));
        if (R) VRT_HIP_TRY(hipMemcpy(R, s->line.d_R, sizeof(double) * 9 * n, hipMemcpyDeviceToHost));
        if (gamma) VRT_HIP_TRY(hipMemcpy(gamma, s->line.d_gamma, sizeof(double) * n, hipMemcpyDeviceToHost));
        return VRT_OK;
    });
}

int vrt_regular_lambda_set_state(vrt_regular_lambda *s, const double *S, const double *populations)
{
    int rc = check_state_pointers(s, S, populations);
    if (rc || (rc = check_state(s->n, s->nlam, S, populations))) return rc;
    return guarded([&] {
        if ((rc = use_device(s->device))) return rc;
        hipStream_t st = s->st;
        const size_t n = (size_t)s->n;
        // staged copies beside the session: it is untouched until every one of them is complete
        RasterStore::Staged staged;
        DevBuf<double> pops;
        if (S && (rc = s->sj.stage(S, staged, st))) return rc;
        if (populations) {
            if ((rc = pops.alloc(3 * n))) return rc;
            VRT_HIP_TRY(hipMemcpyAsync(pops, populations, sizeof(double) * 3 * n, hipMemcpyHostToDevice, st));
        }
        VRT_HIP_TRY(hipStreamSynchronize(st));               // the host arrays may go after return
        if (S) s->sj.adopt(staged);
        if (populations) std::swap(s->d_pops[s->pc], pops);
        s->ng.have = 0;                                      // iterates of another state are no history of this one
        s->ng.last_applied = 0;
        return VRT_OK;
    });
}

void vrt_regular_lambda_destroy(vrt_regular_lambda *s)
{
    DeviceScope scope;
    if (!s) return;
    (void)hipSetDevice(s->device);
    (void)hipStreamSynchronize(s->st);
    regular_release_workspace(s->r);                         // the chunk workspace goes with the session
    delete s;
}

}  // extern "C"
