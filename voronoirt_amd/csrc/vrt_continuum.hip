// The continuum scattering Λ-iteration on the device, on both grids: Λ_voronoi and Λ_regular of src/lambda_continuum.jl
// (:109-160, :58-107; J_λ_voronoi :27-56, J_λ_regular :1-24; criterion :162-198), the loop of the reference's production
// run (src/compare_continuum.jl).  Coherent scattering at nlam independent wavelengths (the reference: one, 500 nm):
//   J = Σ_a w_a I_a(S_old)          I_0 of the up solves = B_0 of the bottom layer / plane, down solves from zeros
//   S_new = (1 - ε) J + ε B_0       at EVERY entry, ε per (point, wavelength)
//   diff = max |1 - S_old / S_new|  over the THICK entries only (ε > eps_thick; the reference: ε_λ .> 1e-4)
//
//   vrt_continuum_update_dev       the masked update alone, caller layout (k_continuum_update)
//   vrt_continuum_*                the loop on a vrt_plan with library-owned device state: S and J in a SourceStore
//                                  (vrt_source_store.h), B_0, ε and α beside them in its order -- sweep order
//                                  (vrt_plan_execute_native_dev's plane sets, α as VRT_ALPHA_SITE_LAM_NATIVE; the update is
//                                  k_continuum_update_native), or -- VRT_LAMBDA_NATIVE=0, a plan without a sweep-order
//                                  form -- the caller's layout through k_continuum_update; S, J and the scalar are the
//                                  same bits either way
//   vrt_regular_continuum_*        the loop on a vrt_regular: the chunked solve of vrt_regular_lambda.hip with one α array
//                                  per wavelength shared by all angles, J reduced in quadrature order, the masked update
//                                  on the raster in the caller's layout
// The update's operations and their order are those of k_lambda_update (vrt_kernels.hip); Ng acceleration is that of
// vrt_accel.hip (ng_after_iterate), over all n nlam physical entries, thin ones included.
//
// Accelerated Λ-iteration (Olson, Auer & Buchler 1986) on the Voronoi session, vrt_continuum_set_operator(s, 1): the local
// operator Λ*[i,l] = Σ_a w_a upd(a,i) ((w_1 b(Δτ_1)) + (w_2 b(Δτ_2))) is the coefficient of a site's own S in the last
// Gauss-Seidel visit of every angle (k_lambda_diagonal, once per session: α does not change), and the update becomes
//   S_new = ((1 - ε) (J - Λ* S_old) + ε B_0) / (1 - (1 - ε) Λ*)
// in both layouts (the ALI instantiations of the two update kernels; Λ* of the sweep-order one is an up-order plane set).
// On the raster session, vrt_regular_continuum_select_operator(s, 1): Λ* is the diagonal of one sweep of the raster's Λ
// (k_regular_lambda_diagonal, vrt_regular.hip, from the session's plane-major α), exactly 0 on the ghost border, and the
// update is the same k_continuum_update<true> in the caller's layout.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "vrt_device.h"
#include "vrt_raster_store.h"
#include "vrt_source_store.h"

namespace vrt {
namespace {

// the criterion of one thread: maximum and NaN flag over its thick entries, and how many those were
struct Crit {
    double d = 0.0;
    bool nan_ = false;
    unsigned thick = 0;
};

// Julia indexes with `thick` BEFORE it takes the maximum (lambda_continuum.jl:169, :188): a thin entry is not seen at all,
// a NaN at a thick one makes the maximum NaN
__device__ __forceinline__ void crit_entry(Crit &c, double e, double eps_thick, double s_old, double s_new)
{
    if (!(e > eps_thick)) return;
    c.thick++;
    const double dd = fabs(1.0 - s_old / s_new);
    if (!(dd == dd)) c.nan_ = true;
    else c.d = fmax(c.d, dd);
}

// per wave with shuffles, then ONE integer atomic per workgroup and word (256 threads): the maximum on the IEEE bits
// (all candidates are >= 0), the NaN flag, the thick count
__device__ __forceinline__ void crit_reduce(const Crit &c, unsigned long long *__restrict__ result)
{
    __shared__ double wmax[4];
    __shared__ int wnan[4];
    __shared__ unsigned wcnt[4];
    double d = c.d;
    unsigned cnt = c.thick;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        d = fmax(d, __shfl_xor(d, off, 64));
        cnt += (unsigned)__shfl_xor((int)cnt, off, 64);
    }
    const unsigned long long any_nan = __ballot(c.nan_);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { wmax[wave] = d; wnan[wave] = any_nan != 0ull; wcnt[wave] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double m = fmax(fmax(wmax[0], wmax[1]), fmax(wmax[2], wmax[3]));
        atomicMax(&result[0], (unsigned long long)__double_as_longlong(m));
        if (wnan[0] | wnan[1] | wnan[2] | wnan[3]) atomicMax(&result[1], 1ull);
        atomicAdd(&result[2], (unsigned long long)wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3]);
    }
}

// one entry of the update: plain Λ-iteration, or -- ALI -- with the local operator L = Λ*.  The ALI form is
// S_old + (S_fs - S_old) / den written so that num >= 0: every coefficient of Λ is >= 0 and Λ* <= Λ_ii
template <bool ALI>
__device__ __forceinline__ double update_entry(double e, double J, double B, double L, double s_old)
{
    if (!ALI) return (1.0 - e) * J + e * B;
    const double t = 1.0 - e;
    const double num = t * (J - L * s_old) + e * B;
    const double den = 1.0 - t * L;
    return num / den;
}

// caller layout: J, B, eps, S (and Λ*) (n, ld) rows, wavelength fastest; grid-stride over the n nlam entries
template <bool ALI>
__global__ void __launch_bounds__(256)
k_continuum_update(int64_t n, int64_t nlam, int64_t ld, const double *__restrict__ J, const double *__restrict__ B,
                   const double *__restrict__ eps, const double *__restrict__ diag, double eps_thick,
                   const double *__restrict__ S_old, double *__restrict__ S_new,
                   unsigned long long *__restrict__ result /* max bits, NaN flag, thick count */)
{
    const int64_t total = n * nlam;
    Crit c;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t site = t / nlam, l = t - site * nlam;
        const size_t o = (size_t)site * ld + l;
        const double e = eps[o], s_old = S_old[o];
        const double s_new = update_entry<ALI>(e, J[o], B[o], ALI ? diag[o] : 0.0, s_old);
        S_new[o] = s_new;
        crit_entry(c, e, eps_thick, s_old, s_new);
    }
    crit_reduce(c, result);
}

// Sweep-order plane sets ([pair][pos][2] per direction): one thread per UP position walks the wavelength pairs.  J = J_up +
// J_down as k_combine_J forms it, B and ε from the up plane set, the old S read from the up plane it is written back to,
// the down-order copy of S_new written beside it: the operations of k_continuum_update on the same values.  An odd nlam
// carries its padding wavelength as zeros, outside both the criterion and the thick count.  ALI: Λ* from its up-order
// plane set Lu, one more load per pair.
template <bool ALI>
__global__ void __launch_bounds__(256)
k_continuum_update_native(int64_t n, int npair, int nlam, const int32_t *__restrict__ store_up,
                          const int32_t *__restrict__ rank_down, const double2 *__restrict__ Ju,
                          const double2 *__restrict__ Jd, const double2 *__restrict__ Bu, const double2 *__restrict__ Eu,
                          const double2 *__restrict__ Lu, double eps_thick, double2 *__restrict__ Su,
                          double2 *__restrict__ Sd, unsigned long long *__restrict__ result)
{
    Crit c;
    for (int64_t pos = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; pos < n; pos += (int64_t)gridDim.x * blockDim.x) {
        const size_t pd = (size_t)rank_down[store_up[pos]];
        constexpr int U = 2;                                // (five loads per pair: two pairs in flight; the continuum has few)
        for (int q0 = 0; q0 < npair; q0 += U) {
            double2 J[U], B[U], E[U], So[U], L[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int q = q0 + u < npair ? q0 + u : npair - 1;
                const size_t t = (size_t)q * (size_t)n + (size_t)pos;
                const double2 jd = Jd[(size_t)q * (size_t)n + pd];
                J[u] = Ju[t];
                J[u].x = J[u].x + jd.x; J[u].y = J[u].y + jd.y;
                B[u] = Bu[t];
                E[u] = Eu[t];
                So[u] = Su[t];
                L[u] = ALI ? Lu[t] : make_double2(0.0, 0.0);
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int q = q0 + u;
                if (q >= npair) break;
                const size_t t = (size_t)q * (size_t)n + (size_t)pos;
                double2 Sn;
                Sn.x = update_entry<ALI>(E[u].x, J[u].x, B[u].x, L[u].x, So[u].x);
                Sn.y = update_entry<ALI>(E[u].y, J[u].y, B[u].y, L[u].y, So[u].y);
                const bool second = 2 * q + 1 < nlam;
                if (!second) Sn.y = 0.0;
                Su[t] = Sn;
                Sd[(size_t)q * (size_t)n + pd] = Sn;
                crit_entry(c, E[u].x, eps_thick, So[u].x, Sn.x);
                if (second) crit_entry(c, E[u].y, eps_thick, So[u].y, Sn.y);
            }
        }
    }
    crit_reduce(c, result);
}

// d_diag: Λ* in the layout of the other arrays, or NULL for the plain update
int launch_continuum_update(int64_t n, int64_t nlam, int64_t ld, const double *dJ, const double *dB, const double *deps,
                            const double *d_diag, double eps_thick, const double *dS_old, double *dS_new,
                            unsigned long long *d_result, hipStream_t st)
{
    VRT_HIP_TRY(hipMemsetAsync(d_result, 0, 3 * sizeof(unsigned long long), st));
    const int64_t blocks = std::min<int64_t>((n * nlam + 255) / 256, 256 * 16);
    const dim3 grid((unsigned)std::max<int64_t>(blocks, 1));
    if (d_diag)
        hipLaunchKernelGGL(k_continuum_update<true>, grid, dim3(256), 0, st, n, nlam, ld, dJ, dB, deps, d_diag, eps_thick,
                           dS_old, dS_new, d_result);
    else
        hipLaunchKernelGGL(k_continuum_update<false>, grid, dim3(256), 0, st, n, nlam, ld, dJ, dB, deps, d_diag, eps_thick,
                           dS_old, dS_new, d_result);
    VRT_HIP_TRY(hipGetLastError());
    return VRT_OK;
}

int launch_continuum_update_native(vrt_grid *g, int64_t nlam, const double *dJ_up, const double *dJ_down, const double *dB_up,
                                   const double *dE_up, const double *dL_up, double eps_thick, double *dS_up,
                                   double *dS_down, unsigned long long *d_result, hipStream_t st)
{
    VRT_HIP_TRY(hipMemsetAsync(d_result, 0, 3 * sizeof(unsigned long long), st));
    const int npair = (int)((nlam + 1) / 2);
    const int64_t blocks = std::min<int64_t>((g->n + 255) / 256, 256 * 16);
    const dim3 grid((unsigned)std::max<int64_t>(blocks, 1));
#define VRT_UPDATE_NATIVE(ALI)                                                                                             \
    hipLaunchKernelGGL(k_continuum_update_native<ALI>, grid, dim3(256), 0, st, g->n, npair, (int)nlam, g->up.d_store,      \
                       g->down.d_srank, reinterpret_cast<const double2 *>(dJ_up),                                          \
                       reinterpret_cast<const double2 *>(dJ_down), reinterpret_cast<const double2 *>(dB_up),               \
                       reinterpret_cast<const double2 *>(dE_up), reinterpret_cast<const double2 *>(dL_up), eps_thick,      \
                       reinterpret_cast<double2 *>(dS_up), reinterpret_cast<double2 *>(dS_down), d_result)
    if (dL_up) VRT_UPDATE_NATIVE(true);
    else VRT_UPDATE_NATIVE(false);
#undef VRT_UPDATE_NATIVE
    VRT_HIP_TRY(hipGetLastError());
    return VRT_OK;
}

// ---- the local operator Λ* (DiagAngles: vrt_device.h) ------------------------------------------------------------------
// Λ*[i,l] = Σ_a w_a upd(a,i) ((w_1 b(Δτ_1)) + (w_2 b(Δτ_2))), Δτ_r = r_r (α[i,l] + α[up_r,l]) / 2 as the sweep forms it
// (k_sweep_level), b the third coefficient of linear_weights: the coefficient of S[i] in the last visit of site i by every
// angle.  upd(a,i) = 0 where the sweep of angle a never writes site i: the n1 sites of layer 1 of the angle's direction
// (their I is I_0) and the never-visited last site perm[n] (sweep positions < n1, and n - 1).  One thread per site, the
// angles in order, slot 1 then slot 2, the wavelengths inside: the tables [A][n] are read coalesced over the sites, once
// per angle; the α[up_r] rows are the only gathers.  No atomics: the same inputs give the same bits.  Runs once per
// session.  alpha and diag are (n, ld) rows; the padding columns are neither read nor written.
__global__ void __launch_bounds__(256)
k_lambda_diagonal(int64_t n, int nlam, int64_t ld, int A, DiagAngles ang, int32_t n1_up, int32_t n1_down,
                  const int32_t *__restrict__ rank_up, const int32_t *__restrict__ rank_down,
                  const int32_t *__restrict__ up1, const int32_t *__restrict__ up2, const double *__restrict__ w1,
                  const double *__restrict__ w2, const double *__restrict__ r1, const double *__restrict__ r2,
                  const double *__restrict__ alpha, double *diag)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t o = (size_t)i * (size_t)ld;
    for (int l = 0; l < nlam; l++) diag[o + l] = 0.0;
    const int32_t pos_up = rank_up[i], pos_down = rank_down[i];
    for (int a = 0; a < A; a++) {
        const int32_t pos = ang.down[a] ? pos_down : pos_up;
        if (pos < (ang.down[a] ? n1_down : n1_up) || (int64_t)pos == n - 1) continue;
        const size_t row = (size_t)a * (size_t)n + (size_t)i;
        const int32_t u1 = up1[row], u2 = up2[row];
        const double W1 = w1[row], W2 = w2[row], R1 = r1[row], R2 = r2[row];
        const bool in1 = u1 >= 0 && (int64_t)u1 < n, in2 = u2 >= 0 && (int64_t)u2 < n;     // (a visited site has both)
        for (int l = 0; l < nlam; l++) {
            const double a_c = alpha[o + l];
            double ca, cb, ce, t1 = 0.0, t2 = 0.0;
            if (in1) {
                linear_weights_ref_order(R1 * (a_c + alpha[(size_t)u1 * (size_t)ld + l]) / 2.0, ca, cb, ce);
                t1 = W1 * cb;
            }
            if (in2) {
                linear_weights_ref_order(R2 * (a_c + alpha[(size_t)u2 * (size_t)ld + l]) / 2.0, ca, cb, ce);
                t2 = W2 * cb;
            }
            diag[o + l] += ang.w[a] * (t1 + t2);
        }
    }
}

// caller holds p->mu and has chosen the device; weights per USER angle (θ = 90 angles have no table and add nothing)
int launch_lambda_diagonal(vrt_plan *p, int64_t nlam, int64_t ld, const double *d_alpha, const double *weights, double *d_diag,
                           hipStream_t st)
{
    vrt_grid *g = p->g;
    if (p->A > kMaxAngles) return fail(VRT_EINVAL, "too many active angles");
    if (nlam > INT32_MAX) return fail(VRT_EINVAL, "nlam too large");
    const DiagAngles ang = diag_angles(p, weights);
    const int64_t blocks = (g->n + 255) / 256;
    hipLaunchKernelGGL(k_lambda_diagonal, dim3((unsigned)std::max<int64_t>(blocks, 1)), dim3(256), 0, st, g->n, (int)nlam, ld,
                       p->A, ang, (int32_t)g->up.n1, (int32_t)g->down.n1, g->up.d_rank, g->down.d_rank, p->d_up1, p->d_up2,
                       p->d_w1, p->d_w2, p->d_r1, p->d_r2, d_alpha, d_diag);
    VRT_HIP_TRY(hipGetLastError());
    return VRT_OK;
}

// min over the entries of den = 1 - (1 - ε) Λ*: result[0] the minimum's IEEE bits (over the entries with den > 0; preset to
// all ones), result[1] set when an entry's den is not > 0.  Caller layout, (n, nlam) dense.
__global__ void __launch_bounds__(256)
k_ali_min_den(int64_t total, const double *__restrict__ eps, const double *__restrict__ diag,
              unsigned long long *__restrict__ result)
{
    __shared__ double wmin[4];
    __shared__ int wbad[4];
    double m = INFINITY;
    bool bad = false;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const double den = 1.0 - (1.0 - eps[t]) * diag[t];
        if (den > 0.0) m = fmin(m, den);
        else bad = true;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmin(m, __shfl_xor(m, off, 64));
    const unsigned long long any_bad = __ballot(bad);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { wmin[wave] = m; wbad[wave] = any_bad != 0ull; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double mm = fmin(fmin(wmin[0], wmin[1]), fmin(wmin[2], wmin[3]));
        atomicMin(&result[0], (unsigned long long)__double_as_longlong(mm));
        if (wbad[0] | wbad[1] | wbad[2] | wbad[3]) atomicMax(&result[1], 1ull);
    }
}

// min den of an operator about to be moved into a session: VRT_EINVAL if it is not > 0 somewhere; synchronises st
int check_min_den(int64_t total, const double *d_eps, const double *d_diag, unsigned long long *d_scalars, hipStream_t st)
{
    VRT_HIP_TRY(hipMemsetAsync(d_scalars, 0xFF, sizeof(unsigned long long), st));
    VRT_HIP_TRY(hipMemsetAsync(d_scalars + 1, 0, sizeof(unsigned long long), st));
    const int64_t blocks = std::min<int64_t>((total + 255) / 256, 256 * 16);
    hipLaunchKernelGGL(k_ali_min_den, dim3((unsigned)std::max<int64_t>(blocks, 1)), dim3(256), 0, st, total, d_eps, d_diag,
                       d_scalars);
    VRT_HIP_TRY(hipGetLastError());
    unsigned long long h[2] = {0, 0};
    VRT_HIP_TRY(hipMemcpyAsync(h, d_scalars, sizeof(h), hipMemcpyDeviceToHost, st));
    VRT_HIP_TRY(hipStreamSynchronize(st));
    if (h[1]) return fail(VRT_EINVAL, "the diagonal operator has 1 - (1 - eps) Lambda* <= 0 somewhere (eps = 0 in a cell "
                                      "whose Lambda* rounds to 1)");
    return VRT_OK;
}

// ---- host checks, before the device is touched ------------------------------------------------------------------------
int check_case(const vrt_continuum_case *cc, int64_t n)
{
    if (!cc) return fail(VRT_EINVAL, "the continuum case is NULL");
    if (cc->nlam < 1) return fail(VRT_EINVAL, "nlam must be >= 1");
    if (!cc->alpha || !cc->eps || !cc->B0) return fail(VRT_EINVAL, "NULL array in the continuum case");
    if (!std::isfinite(cc->eps_thick)) return fail(VRT_EINVAL, "eps_thick must be finite");
    if (n < 1) return fail(VRT_EINVAL, "the case needs at least one point");
    const int64_t total = n * cc->nlam;
    int64_t thick = 0;
    for (int64_t i = 0; i < total; i++) {
        const double a = cc->alpha[i], e = cc->eps[i];
        if (!std::isfinite(a) || !(a > 0.0)) return fail(VRT_EINVAL, "alpha must be finite and > 0 everywhere");
        if (!(e >= 0.0 && e <= 1.0)) return fail(VRT_EINVAL, "eps must lie in [0, 1] everywhere");
        if (!std::isfinite(cc->B0[i])) return fail(VRT_EINVAL, "B0 must be finite everywhere");
        thick += e > cc->eps_thick;
    }
    // (the reference's maximum over an empty set throws, lambda_continuum.jl:169)
    if (!thick) return fail(VRT_EINVAL, "no entry has eps > eps_thick: the criterion would be a maximum over nothing");
    return VRT_OK;
}

}  // namespace
}  // namespace vrt

using namespace vrt;

struct vrt_continuum {
    vrt_plan *p = nullptr;              // borrowed
    int device = 0;                     // of the plan's grid (destroying the session must not look into a plan that may be gone)
    int64_t n = 0, nlam = 0;
    double eps_thick = 0;
    std::vector<double> weights;
    // S and J (rows, or sweep order: vrt_source_store.h); beside them, in the store's order, B_0 and ε (rows, or their
    // up-order plane sets) and α as the sweeps take it (rows, or both orders one behind the other: alpha_mode)
    SourceStore sj;
    DevBuf<double> d_B0, d_eps, d_alpha;
    int alpha_mode = VRT_ALPHA_SITE_LAM;
    DevBuf<double> d_I0;                // B_0 of the bottom layer in perm_up order, (n1, nlam)
    DevBuf<unsigned long long> d_scalars;
    int64_t iterations = 0;
    NgState ng;                         // vrt_continuum_set_acceleration (off: nothing allocated, nothing run)
    // vrt_continuum_set_operator (0: nothing allocated, nothing run): Λ* in the caller's layout (n, nlam), and in the
    // store's order beside S (sweep order only: in rows d_diag itself is read)
    int op = 0;
    DevBuf<double> d_diag, d_L_up;
    const double *diag() const { return !op ? nullptr : d_L_up ? d_L_up.p : d_diag.p; }
};

struct vrt_regular_continuum {
    vrt_regular *r = nullptr;           // borrowed
    int device = 0, n_sweeps = 3;
    int64_t n = 0, nlam = 0;
    double eps_thick = 0;
    LineSolves ls;
    Stream st;
    RasterStore sj;                     // S and J, rows and planes, and what the solves start from (vrt_raster_store.h)
    DevBuf<double> d_B0, d_eps;         // per point, Julia order, (n, nlam)
    DevBuf<double> d_A_pl;              // α plane-major, wavelength slowest
    DevBuf<unsigned long long> d_scalars;
    int64_t iterations = 0;
    NgState ng;
    // vrt_regular_continuum_select_operator (0: nothing allocated, nothing run): Λ* in the caller's layout (n, nlam), formed
    // from the directions the session was created with (per user angle, host)
    int op = 0;
    DevBuf<double> d_diag;
    std::vector<double> k, weights;
    std::vector<int> dirs;
};

// Λ* of a raster from its plane-major α into d_diag, dense (n, nlam) in Julia point order
static int regular_diagonal(const vrt_regular *r, int64_t n_angles, const double *k, const int *dirs, const double *weights,
                            int64_t nlam, const double *d_alpha_pl, double *d_diag, hipStream_t st)
{
    DevBuf<double> diag_pl;
    int rc = diag_pl.alloc((size_t)(r->nz * r->nx * r->ny) * (size_t)nlam);
    if (rc) return rc;
    if ((rc = launch_regular_lambda_diagonal(r, n_angles, k, dirs, weights, nlam, d_alpha_pl, diag_pl, st))) return rc;
    if ((rc = launch_from_planes(r, nlam, diag_pl, d_diag, st))) return rc;
    VRT_HIP_TRY(hipStreamSynchronize(st));                   // (diag_pl goes here)
    return VRT_OK;
}

// the same from (n, ld) rows on the device, of which only the first nlam columns are read and written; synchronises st
static int regular_diagonal_rows(const vrt_regular *r, int64_t n_angles, const double *k, const int *dirs,
                                 const double *weights, int64_t nlam, int64_t ld, const double *d_alpha, double *d_diag,
                                 hipStream_t st)
{
    const int64_t n = r->nz * r->nx * r->ny;
    const size_t nS = (size_t)n * (size_t)nlam, row = sizeof(double) * (size_t)nlam, pitch = sizeof(double) * (size_t)ld;
    DevBuf<double> a_dense, a_pl, g_dense;
    int rc;
    if ((rc = a_pl.alloc(nS)) || (rc = g_dense.alloc(nS))) return rc;
    if (ld != nlam) {
        if ((rc = a_dense.alloc(nS))) return rc;
        VRT_HIP_TRY(hipMemcpy2DAsync(a_dense, row, d_alpha, pitch, row, (size_t)n, hipMemcpyDeviceToDevice, st));
        d_alpha = a_dense;
    }
    if ((rc = launch_to_planes(r, nlam, d_alpha, a_pl, st))) return rc;
    if ((rc = regular_diagonal(r, n_angles, k, dirs, weights, nlam, a_pl, g_dense, st))) return rc;
    VRT_HIP_TRY(hipMemcpy2DAsync(d_diag, pitch, g_dense, row, row, (size_t)n, hipMemcpyDeviceToDevice, st));
    VRT_HIP_TRY(hipStreamSynchronize(st));
    return VRT_OK;
}

// J_λ (lambda_continuum.jl:1-24) of every (angle, wavelength) solve into dJ_pl, chunk after chunk
static int continuum_J_pass(vrt_regular_continuum *s, hipStream_t st)
{
    vrt_regular *r = s->r;
    const LineSolves &ls = s->ls;
    const RasterStore &sj = s->sj;
    const int64_t vol = s->n, nlam = s->nlam, n_solve = ls.A * nlam;
    VRT_HIP_TRY(hipMemsetAsync(sj.J_planes(), 0, sizeof(double) * (size_t)(nlam * vol), st));
    int rc;
    for (int64_t g0 = 0; g0 < n_solve; g0 += ls.chunk) {
        const int64_t cnt = std::min(ls.chunk, n_solve - g0);
        if ((rc = regular_solve_planes(r, cnt, ls.hk.data() + 3 * g0, ls.d_ks + 3 * g0, ls.d_up + g0, sj.S_planes(), nlam, g0,
                                       s->d_A_pl, sj.I0_planes(), sj.zero_plane(), s->n_sweeps, st, /*alpha_per_lam=*/true)))
            return rc;
        if ((rc = launch_reduce_J_planes(r, ls, g0, cnt, sj.J_planes(), st))) return rc;
    }
    return VRT_OK;
}

extern "C" {

int vrt_continuum_case_check(const vrt_continuum_case *cc, int64_t n) { return check_case(cc, n); }

int vrt_continuum_update_dev(vrt_grid *g, int64_t nlam, int64_t ld, const double *dJ, const double *dB, const double *deps,
                             double eps_thick, const double *dS_old, double *dS_new, double *max_rel_change,
                             int64_t *n_thick, void *stream)
{
    if (!g || !dJ || !dB || !deps || !dS_old || !dS_new || !max_rel_change) return fail(VRT_EINVAL, "NULL argument");
    if (nlam < 1 || ld < nlam) return fail(VRT_EINVAL, "need nlam >= 1 and ld >= nlam");
    if (!std::isfinite(eps_thick)) return fail(VRT_EINVAL, "eps_thick must be finite");
    return guarded([&] {
        int rc = use_device(g->device);
        if (rc) return rc;
        std::lock_guard<std::mutex> lock(g->mu);
        if (!g->d_scalars && (rc = g->d_scalars.alloc(kUpdateWords))) return rc;
        hipStream_t st = (hipStream_t)stream;
        if ((rc = launch_continuum_update(g->n, nlam, ld, dJ, dB, deps, nullptr, eps_thick, dS_old, dS_new, g->d_scalars, st)))
            return rc;
        return read_criterion(g->d_scalars, 3, st, max_rel_change, n_thick);
    });
}

int vrt_continuum_ali_update_dev(vrt_grid *g, int64_t nlam, int64_t ld, const double *dJ, const double *dB, const double *deps,
                                 const double *d_diag, double eps_thick, const double *dS_old, double *dS_new,
                                 double *max_rel_change, int64_t *n_thick, void *stream)
{
    if (!g || !dJ || !dB || !deps || !d_diag || !dS_old || !dS_new || !max_rel_change) return fail(VRT_EINVAL, "NULL argument");
    if (nlam < 1 || ld < nlam) return fail(VRT_EINVAL, "need nlam >= 1 and ld >= nlam");
    if (!std::isfinite(eps_thick)) return fail(VRT_EINVAL, "eps_thick must be finite");
    return guarded([&] {
        int rc = use_device(g->device);
        if (rc) return rc;
        std::lock_guard<std::mutex> lock(g->mu);
        if (!g->d_scalars && (rc = g->d_scalars.alloc(kUpdateWords))) return rc;
        hipStream_t st = (hipStream_t)stream;
        if ((rc = launch_continuum_update(g->n, nlam, ld, dJ, dB, deps, d_diag, eps_thick, dS_old, dS_new, g->d_scalars, st)))
            return rc;
        return read_criterion(g->d_scalars, 3, st, max_rel_change, n_thick);
    });
}

int vrt_plan_lambda_diagonal_dev(vrt_plan *p, int64_t nlam, int64_t ld, const double *d_alpha, const double *weights_host,
                                 double *d_diag, void *stream)
{
    if (!p || !d_alpha || !weights_host || !d_diag) return fail(VRT_EINVAL, "NULL argument");
    if (nlam < 1 || ld < nlam) return fail(VRT_EINVAL, "need nlam >= 1 and ld >= nlam");
    return guarded([&] {
        std::lock_guard<std::mutex> lock(p->mu);
        int rc = use_device(p->g->device);
        if (rc) return rc;
        return launch_lambda_diagonal(p, nlam, ld, d_alpha, weights_host, d_diag, (hipStream_t)stream);
    });
}

int vrt_plan_lambda_diagonal(vrt_plan *p, int64_t nlam, int64_t ld, const double *alpha, const double *weights, double *diag)
{
    if (!p || !alpha || !weights || !diag) return fail(VRT_EINVAL, "NULL argument");
    if (nlam < 1 || ld < nlam) return fail(VRT_EINVAL, "need nlam >= 1 and ld >= nlam");
    return guarded([&] {
        std::lock_guard<std::mutex> lock(p->mu);
        vrt_grid *g = p->g;
        for (int64_t i = 0; i < g->n; i++)
            for (int64_t l = 0; l < nlam; l++) {
                const double a = alpha[i * ld + l];
                if (!std::isfinite(a) || !(a > 0.0)) return fail(VRT_EINVAL, "alpha must be finite and > 0 everywhere");
            }
        int rc = use_device(g->device);
        if (rc) return rc;
        hipStream_t st = g->stream;
        const size_t count = (size_t)g->n * (size_t)ld;
        DevBuf<double> d_alpha, d_diag;
        if ((rc = upload(d_alpha, alpha, count, st))) return rc;
        if ((rc = d_diag.alloc(count))) return rc;
        // (the padding columns of diag go back as they came)
        VRT_HIP_TRY(hipMemcpyAsync(d_diag, diag, sizeof(double) * count, hipMemcpyHostToDevice, st));
        if ((rc = launch_lambda_diagonal(p, nlam, ld, d_alpha, weights, d_diag, st))) return rc;
        VRT_HIP_TRY(hipMemcpyAsync(diag, d_diag, sizeof(double) * count, hipMemcpyDeviceToHost, st));
        VRT_HIP_TRY(hipStreamSynchronize(st));
        return VRT_OK;
    });
}

int vrt_continuum_create(vrt_plan *p, const vrt_continuum_case *cc, const double *weights, vrt_continuum **out)
{
    if (!out) return fail(VRT_EINVAL, "out is NULL");
    *out = nullptr;
    if (!p || !cc || !weights) return fail(VRT_EINVAL, "NULL argument");
    if (cc->nlam < 1) return fail(VRT_EINVAL, "nlam must be >= 1");
    if (!cc->alpha || !cc->eps || !cc->B0) return fail(VRT_EINVAL, "NULL array in the continuum case");
    if (!std::isfinite(cc->eps_thick)) return fail(VRT_EINVAL, "eps_thick must be finite");
    return guarded([&] {
        std::lock_guard<std::mutex> lock(p->mu);
        vrt_grid *g = p->g;
        int rc = check_case(cc, g->n);
        if (rc) return rc;
        if ((rc = use_device(g->device))) return rc;
        std::unique_ptr<vrt_continuum> s(new vrt_continuum());
        s->p = p;
        s->device = g->device;
        s->n = g->n;
        s->nlam = cc->nlam;
        s->eps_thick = cc->eps_thick;
        s->weights.assign(weights, weights + p->n_angles_user);
        const int64_t nlam = cc->nlam;
        const size_t nS = (size_t)g->n * (size_t)nlam;
        hipStream_t st = g->stream;
        const SourceStore::Form form = SourceStore::plan_keeps_planes(p) ? SourceStore::kPlanes : SourceStore::kRows;
#define VRT_S(expr) do { if ((rc = (expr))) return rc; } while (0)
        VRT_S(upload(s->d_B0, cc->B0, nS, st));
        VRT_S(s->d_I0.alloc((size_t)g->up.n1 * (size_t)nlam));
        // I_0 = B_λ(T) of the bottom layer perm_up[1 : layers_up[2] - 1] (:45-47), fixed over the iterations
        VRT_S(launch_gather_rows(g->up.n1, nlam, nlam, g->up.d_order, s->d_B0, s->d_I0, st));
        VRT_S(s->d_scalars.alloc(kUpdateWords));
        VRT_S(s->sj.create(p, nlam, form, s->d_B0, st));     // S_new = B_0, S_old = zero(S_new), :136-139
        VRT_S(s->sj.to_up_order(s->d_B0, st));
        VRT_S(upload(s->d_eps, cc->eps, nS, st));
        VRT_S(s->sj.to_up_order(s->d_eps, st));
        VRT_S(upload(s->d_alpha, cc->alpha, nS, st));
        VRT_S(s->sj.to_sweep_alpha(s->d_alpha, &s->alpha_mode, st));
#undef VRT_S
        VRT_HIP_TRY(hipStreamSynchronize(st));               // the host arrays may go after return
        *out = s.release();
        return VRT_OK;
    });
}

int vrt_continuum_iterate(vrt_continuum *s, double *max_rel_change)
{
    if (!s || !max_rel_change) return fail(VRT_EINVAL, "NULL argument");
    return guarded([&] {
        vrt_plan *p = s->p;
        std::lock_guard<std::mutex> lock(p->mu);
        vrt_grid *g = p->g;
        int rc = use_device(g->device);
        if (rc) return rc;
        hipStream_t st = g->stream;
        const int64_t n = s->n, nlam = s->nlam;
        SourceStore &sj = s->sj;
        // J_λ (:27-56) from S, in the store's form
        if ((rc = execute_locked(p, sj.exec_args(s->d_alpha, s->alpha_mode, s->d_I0, s->weights.data(), st)))) return rc;
        // S_new and the criterion (:148, :188)
        if (sj.form() == SourceStore::kPlanes) {
            // the old S is read from the plane the new one is written to
            if ((rc = launch_continuum_update_native(g, nlam, sj.J_plane(0), sj.J_plane(1), s->d_B0, s->d_eps, s->diag(),
                                                     s->eps_thick, sj.S_plane(0), sj.S_plane(1), s->d_scalars, st)))
                return rc;
        } else {
            // S_old = copy(S_new), :146: the current S is read where it is and the new one written to the other buffer; the
            // two change roles only once both launches are queued (a failure leaves the session's S what it was)
            if ((rc = launch_continuum_update(n, nlam, nlam, sj.J_rows(), s->d_B0, s->d_eps, s->diag(), s->eps_thick, sj.S_new(),
                                              sj.S_old(), s->d_scalars, st)))
                return rc;
            sj.swap_rows();
        }
        if ((rc = read_criterion(s->d_scalars, 3, st, max_rel_change))) return rc;
        if ((rc = patch_chain_check(p))) return rc;          // a chained sweep that gave up: THIS iteration's results are invalid
        s->iterations++;
        // history copy or Ng step on the S of the plain update (native: the up-order copy; an accepted x_acc becomes that copy
        // and the down-order copy is rewritten from it, value for value)
        return ng_after_update(s->ng, s->iterations, sj, st);
    });
}

int vrt_continuum_get(vrt_continuum *s, double *J, double *S)
{
    if (!s) return fail(VRT_EINVAL, "NULL session");
    return guarded([&] {
        vrt_plan *p = s->p;
        std::lock_guard<std::mutex> lock(p->mu);
        int rc = use_device(p->g->device);
        if (rc) return rc;
        return s->sj.download(J, S, s->nlam, 0, p->g->stream);
    });
}

int vrt_continuum_set_source(vrt_continuum *s, const double *S)
{
    if (!s || !S) return fail(VRT_EINVAL, "NULL argument");
    int rc = check_source(S, s->n * s->nlam);
    if (rc) return rc;
    return guarded([&] {
        vrt_plan *p = s->p;
        std::lock_guard<std::mutex> lock(p->mu);
        if ((rc = use_device(p->g->device))) return rc;
        hipStream_t st = p->g->stream;
        SourceStore::Staged staged;                          // beside the session: it is untouched until the copies are complete
        if ((rc = s->sj.stage(S, s->nlam, 0, staged, st))) return rc;
        VRT_HIP_TRY(hipStreamSynchronize(st));
        s->sj.adopt(staged);
        s->ng.have = 0;                                      // iterates of another S are no history of this one
        s->ng.last_applied = 0;
        return VRT_OK;
    });
}

int vrt_continuum_set_acceleration(vrt_continuum *s, int order, int start, int period)
{
    if (!s) return fail(VRT_EINVAL, "NULL session");
    int rc = ng_check_settings(order, start, period);
    if (rc) return rc;
    return guarded([&] {
        vrt_plan *p = s->p;
        std::lock_guard<std::mutex> lock(p->mu);
        if ((rc = use_device(p->g->device))) return rc;
        return ng_configure(s->ng, order, start, period, s->sj.ng_count());
    });
}

int vrt_continuum_last_acceleration(const vrt_continuum *s, int *applied, double sums[5], double coeffs[2])
{
    if (!s || !applied) return fail(VRT_EINVAL, "NULL argument");
    return ng_report(s->ng, applied, sums, coeffs);
}

int vrt_continuum_set_operator(vrt_continuum *s, int op)
{
    if (!s) return fail(VRT_EINVAL, "NULL session");
    if (op != 0 && op != 1) return fail(VRT_EINVAL, "operator must be 0 (plain) or 1 (diagonal)");
    return guarded([&] {
        vrt_plan *p = s->p;
        std::lock_guard<std::mutex> lock(p->mu);
        int rc = use_device(p->g->device);
        if (rc) return rc;
        if (op == s->op) return (int)VRT_OK;
        hipStream_t st = p->g->stream;
        if (op == 0) {
            VRT_HIP_TRY(hipStreamSynchronize(st));
            s->d_diag = DevBuf<double>();
            s->d_L_up = DevBuf<double>();
        } else {
            // Λ* from the session's α and weights, once; everything is built beside the session and moved in at the end
            const int64_t n = s->n, nlam = s->nlam;
            const size_t nS = (size_t)n * (size_t)nlam;
            DevBuf<double> diag, L_up, tmpA, tmpE;
            const double *alpha, *eps;                       // α and ε back in the caller's layout, value for value
            if ((rc = diag.alloc(nS))) return rc;
            if ((rc = s->sj.rows_of(s->d_alpha, tmpA, &alpha, st)) || (rc = s->sj.rows_of(s->d_eps, tmpE, &eps, st))) return rc;
            if ((rc = launch_lambda_diagonal(p, nlam, nlam, alpha, s->weights.data(), diag, st))) return rc;
            // min den = min (1 - (1 - ε) Λ*) must be > 0 (it is not only for ε = 0 with Λ* rounding to 1)
            if ((rc = check_min_den((int64_t)nS, eps, diag, s->d_scalars, st))) return rc;
            if ((rc = s->sj.up_order_of(diag, L_up, st))) return rc;
            if (L_up) VRT_HIP_TRY(hipStreamSynchronize(st));
            s->d_diag = std::move(diag);
            s->d_L_up = std::move(L_up);
        }
        s->op = op;
        s->ng.have = 0;                                      // iterates of another fixed-point map are no history of this one
        return (int)VRT_OK;
    });
}

int vrt_continuum_get_operator(vrt_continuum *s, int *op, double *diag)
{
    if (!s || !op) return fail(VRT_EINVAL, "NULL argument");
    return guarded([&] {
        vrt_plan *p = s->p;
        std::lock_guard<std::mutex> lock(p->mu);
        *op = s->op;
        if (!diag || !s->op) return (int)VRT_OK;
        int rc = use_device(p->g->device);
        if (rc) return rc;
        hipStream_t st = p->g->stream;
        VRT_HIP_TRY(hipMemcpyAsync(diag, s->d_diag, sizeof(double) * (size_t)s->n * (size_t)s->nlam, hipMemcpyDeviceToHost, st));
        VRT_HIP_TRY(hipStreamSynchronize(st));
        return (int)VRT_OK;
    });
}

void vrt_continuum_destroy(vrt_continuum *s)
{
    DeviceScope scope;
    if (!s) return;
    (void)hipSetDevice(s->device);
    delete s;
}

// ---- the regular grid ------------------------------------------------------------------------------------------------------
int vrt_regular_continuum_create(vrt_regular *r, int64_t n_angles, const double *k, const int *dirs, const double *weights,
                                 const vrt_continuum_case *cc, int n_sweeps, vrt_regular_continuum **out)
{
    if (!out) return fail(VRT_EINVAL, "out is NULL");
    *out = nullptr;
    if (!r || !k || !dirs || !weights || !cc) return fail(VRT_EINVAL, "NULL argument");
    if (cc->nlam < 1) return fail(VRT_EINVAL, "nlam must be >= 1");
    if (!cc->alpha || !cc->eps || !cc->B0) return fail(VRT_EINVAL, "NULL array in the continuum case");
    if (!std::isfinite(cc->eps_thick)) return fail(VRT_EINVAL, "eps_thick must be finite");
    if (n_sweeps < 1) return fail(VRT_EINVAL, "n_sweeps must be >= 1");
    int rc = check_angles(n_angles, k, dirs);
    if (rc) return rc;
    return guarded([&] {
        const int64_t vol = r->nz * r->nx * r->ny, nlam = cc->nlam;
        if ((rc = check_case(cc, vol))) return rc;
        if ((rc = use_device(r->device))) return rc;
        std::unique_ptr<vrt_regular_continuum> s(new vrt_regular_continuum());
        s->r = r;
        s->device = r->device;
        s->n_sweeps = n_sweeps;
        s->n = vol;
        s->nlam = nlam;
        s->eps_thick = cc->eps_thick;
        if ((rc = line_solves_init(s->ls, r, n_angles, k, dirs, weights, nlam))) return rc;
        s->k.assign(k, k + 3 * n_angles);
        s->dirs.assign(dirs, dirs + n_angles);
        s->weights.assign(weights, weights + n_angles);
        if ((rc = s->st.create())) return rc;
        hipStream_t st = s->st;
        const size_t nS = (size_t)vol * (size_t)nlam;
#define VRT_S(expr) do { if ((rc = (expr))) return rc; } while (0)
        DevBuf<double> tmp;
        VRT_S(upload(s->d_B0, cc->B0, nS, st));
        VRT_S(upload(s->d_eps, cc->eps, nS, st));
        VRT_S(s->sj.create(r, nlam, s->d_B0, st));           // S_new = B_0, :83-84; I_0 = B_λ(T[1, :, :]), :16
        VRT_S(upload(tmp, cc->alpha, nS, st));
        VRT_S(s->d_A_pl.alloc(nS));
        VRT_S(s->d_scalars.alloc(kUpdateWords));
        VRT_S(launch_to_planes(r, nlam, tmp, s->d_A_pl, st));             // α_cont, fixed over the iterations (:76)
#undef VRT_S
        VRT_HIP_TRY(hipStreamSynchronize(st));
        *out = s.release();
        return VRT_OK;
    });
}

int vrt_regular_continuum_iterate(vrt_regular_continuum *s, double *max_rel_change)
{
    if (!s || !max_rel_change) return fail(VRT_EINVAL, "NULL argument");
    return guarded([&] {
        int rc = use_device(s->device);
        if (rc) return rc;
        hipStream_t st = s->st;
        // J_λ (:1-24) from S_old = the last S_new (:93-94); S_new = (1 - ε) J + ε B_0 (:95) and the masked criterion (:169);
        // S_new also plane-major for the next solves
        RasterStore &sj = s->sj;
        if ((rc = continuum_J_pass(s, st))) return rc;
        if ((rc = sj.J_home(st))) return rc;
        if ((rc = launch_continuum_update(s->n, s->nlam, s->nlam, sj.J_rows(), s->d_B0, s->d_eps, s->op ? s->d_diag.p : nullptr,
                                          s->eps_thick, sj.S_rows(), sj.S_next(), s->d_scalars, st)))
            return rc;
        if ((rc = sj.S_written(st))) return rc;
        if ((rc = read_criterion(s->d_scalars, 3, st, max_rel_change))) return rc;
        s->r->timed = false;                                 // (the handle's events saw only the last chunk)
        s->iterations++;
        return ng_after_update(s->ng, s->iterations, sj, st);
    });
}

int vrt_regular_continuum_get(vrt_regular_continuum *s, double *J, double *S)
{
    if (!s) return fail(VRT_EINVAL, "NULL session");
    return guarded([&] {
        int rc = use_device(s->device);
        if (rc) return rc;
        return s->sj.download(J, S, s->st);
    });
}

int vrt_regular_continuum_set_source(vrt_regular_continuum *s, const double *S)
{
    if (!s || !S) return fail(VRT_EINVAL, "NULL argument");
    int rc = check_source(S, s->n * s->nlam);
    if (rc) return rc;
    return guarded([&] {
        if ((rc = use_device(s->device))) return rc;
        hipStream_t st = s->st;
        RasterStore::Staged staged;                          // beside the session: it is untouched until the copies are complete
        if ((rc = s->sj.stage(S, staged, st))) return rc;
        VRT_HIP_TRY(hipStreamSynchronize(st));
        s->sj.adopt(staged);
        s->ng.have = 0;
        s->ng.last_applied = 0;
        return VRT_OK;
    });
}

int vrt_regular_continuum_set_acceleration(vrt_regular_continuum *s, int order, int start, int period)
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

int vrt_regular_continuum_last_acceleration(const vrt_regular_continuum *s, int *applied, double sums[5], double coeffs[2])
{
    if (!s || !applied) return fail(VRT_EINVAL, "NULL argument");
    return ng_report(s->ng, applied, sums, coeffs);
}

int vrt_regular_continuum_select_operator(vrt_regular_continuum *s, int op)
{
    if (!s) return fail(VRT_EINVAL, "NULL session");
    if (op != 0 && op != 1) return fail(VRT_EINVAL, "operator must be 0 (plain) or 1 (diagonal)");
    return guarded([&] {
        int rc = use_device(s->device);
        if (rc) return rc;
        if (op == s->op) return (int)VRT_OK;
        hipStream_t st = s->st;
        if (op == 0) {
            VRT_HIP_TRY(hipStreamSynchronize(st));
            s->d_diag = DevBuf<double>();
        } else {
            // Λ* from the session's α and directions, once; built beside the session and moved in at the end
            const size_t nS = (size_t)s->n * (size_t)s->nlam;
            DevBuf<double> diag;
            if ((rc = diag.alloc(nS))) return rc;
            if ((rc = regular_diagonal(s->r, (int64_t)s->dirs.size(), s->k.data(), s->dirs.data(), s->weights.data(), s->nlam,
                                       s->d_A_pl, diag, st)))
                return rc;
            if ((rc = check_min_den((int64_t)nS, s->d_eps, diag, s->d_scalars, st))) return rc;
            s->d_diag = std::move(diag);
        }
        s->op = op;
        s->ng.have = 0;                                      // iterates of another fixed-point map are no history of this one
        return (int)VRT_OK;
    });
}

int vrt_regular_continuum_get_operator(vrt_regular_continuum *s, int *op, double *diag)
{
    if (!s || !op) return fail(VRT_EINVAL, "NULL argument");
    return guarded([&] {
        *op = s->op;
        if (!diag || !s->op) return (int)VRT_OK;
        int rc = use_device(s->device);
        if (rc) return rc;
        hipStream_t st = s->st;
        VRT_HIP_TRY(hipMemcpyAsync(diag, s->d_diag, sizeof(double) * (size_t)s->n * (size_t)s->nlam, hipMemcpyDeviceToHost, st));
        VRT_HIP_TRY(hipStreamSynchronize(st));
        return (int)VRT_OK;
    });
}

int vrt_regular_lambda_diagonal_dev(vrt_regular *r, int64_t n_angles, const double *k, const int *dirs, const double *weights,
                                    int64_t nlam, int64_t ld, const double *d_alpha, double *d_diag)
{
    if (!r || !k || !dirs || !weights || !d_alpha || !d_diag) return fail(VRT_EINVAL, "NULL argument");
    if (nlam < 1 || ld < nlam) return fail(VRT_EINVAL, "need nlam >= 1 and ld >= nlam");
    int rc = check_angles(n_angles, k, dirs);
    if (rc) return rc;
    return guarded([&] {
        if ((rc = use_device(r->device))) return rc;
        return regular_diagonal_rows(r, n_angles, k, dirs, weights, nlam, ld, d_alpha, d_diag, nullptr);
    });
}

int vrt_regular_lambda_diagonal(vrt_regular *r, int64_t n_angles, const double *k, const int *dirs, const double *weights,
                                int64_t nlam, int64_t ld, const double *alpha, double *diag)
{
    if (!r || !k || !dirs || !weights || !alpha || !diag) return fail(VRT_EINVAL, "NULL argument");
    if (nlam < 1 || ld < nlam) return fail(VRT_EINVAL, "need nlam >= 1 and ld >= nlam");
    int rc = check_angles(n_angles, k, dirs);
    if (rc) return rc;
    return guarded([&] {
        const int64_t n = r->nz * r->nx * r->ny;
        for (int64_t i = 0; i < n; i++)
            for (int64_t l = 0; l < nlam; l++) {
                const double a = alpha[i * ld + l];
                if (!std::isfinite(a) || !(a > 0.0)) return fail(VRT_EINVAL, "alpha must be finite and > 0 everywhere");
            }
        if ((rc = use_device(r->device))) return rc;
        const size_t count = (size_t)n * (size_t)ld;
        DevBuf<double> d_alpha, d_diag;
        if ((rc = upload(d_alpha, alpha, count, nullptr))) return rc;
        if ((rc = d_diag.alloc(count))) return rc;
        // (the padding columns of diag go back as they came)
        VRT_HIP_TRY(hipMemcpyAsync(d_diag, diag, sizeof(double) * count, hipMemcpyHostToDevice, nullptr));
        if ((rc = regular_diagonal_rows(r, n_angles, k, dirs, weights, nlam, ld, d_alpha, d_diag, nullptr))) return rc;
        VRT_HIP_TRY(hipMemcpy(diag, d_diag, sizeof(double) * count, hipMemcpyDeviceToHost));
        return VRT_OK;
    });
}

void vrt_regular_continuum_destroy(vrt_regular_continuum *s)
{
    DeviceScope scope;
    if (!s) return;
    (void)hipSetDevice(s->device);
    (void)hipStreamSynchronize(s->st);
    regular_release_workspace(s->r);                         // the chunk workspace goes with the session
    delete s;
}

}  // extern "C"
