// The two steps either side of the formal solve in a Λ-iteration, on the device (SURVEY.md 8f rows 2
// and 4), so that a whole iteration J -> S_new, R, populations -> α -> J ... stays in HBM:
//
//   k_line_opacity        per-angle α_tot = αline_λ + α_cont from per-site line parameters
//                         (src/lambda_iteration.jl:72-80, :89, :93-96; src/line.jl:121-137, :198-208,
//                         :219-225), written DIRECTLY in the sweep's native storage-pair layout
//                         (VRT_ALPHA_ANGLE_NATIVE): the (nλ, n, n_angles) array and its layout change
//                         never exist
//   k_rates_populations   radiative rates R (calculate_R, src/rates.jl:154-201 with Rij / Rji
//                         :226-364, σij :374-416, Gij :459-476) and the statistical-equilibrium
//                         populations (get_revised_populations, src/populations.jl:191-221) from J in
//                         place: per site a map over the wavelengths, nothing but R (9 n) and the
//                         populations (3 n) leaves the kernel
//
// The Voigt profile is Transparency.jl's `voigt_profile` (absent from the reference checkout,
// version unpinned): its documented algorithm, Humlíček's w4 (JQSRT 27, 437, 1982), is restated
// here as in oracle/vrt_oracle_physics.c (per-site divisors inverted once in the opacity kernel); parity for these two kernels is
// tolerance-based (1e-12 against that restatement; w4 itself is a 1e-4 approximation of the
// Faddeeva function).  All quantities are plain numbers in one unit system chosen by the caller;
// physical constants and unit factors come in as arguments.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>

#include "vrt_device.h"
#include "vrt_internal.h"
#include "vrt_line_case.h"
#include "vrt_voigt.h"

namespace vrt {

constexpr double kPi = 3.14159265358979323846;

// ---- opacity prologue -------------------------------------------------------------------------------
// one thread per storage position of an angle's direction (blockIdx.y = active angle: ONE launch for all of them); it
// walks the wavelength pairs, so the site's line parameters are read once and every pair plane is written coalesced
// (16 B/lane).  T2 = double2, or float2 for the fp32 VALUE path (the arithmetic stays fp64, the stored pair is rounded).
// The kernel is bound by the COUNT of its fp64 instructions (measured: time is linear in it, ~linear in nothing else --
// eight instead of four waves per SIMD change nothing), so what does not depend on the wavelength is
// folded per site: gamma / (4 pi c dlambda_D), strength / (sqrt(pi) dlambda_D), and the profile enters alpha_tot by one
// fused multiply-add (last-bit differences from the oracle's expression order; contract of this row: 1e-12).
struct OpacityAngles {
    double k[kMaxAngles][3];
    unsigned char down[kMaxAngles];
};
template <typename T2>
__global__ void __launch_bounds__(256)
k_line_opacity(int64_t n, int nlam, int npair, int lgB, const int32_t *__restrict__ store_up, const int32_t *__restrict__ store_down,
               OpacityAngles ang, const double *__restrict__ lambda, double lambda0, double c0, const double *__restrict__ velocity,
               const double *__restrict__ doppler, const double *__restrict__ gamma,
               const double *__restrict__ strength, const double *__restrict__ alpha_cont,
               T2 *__restrict__ out0 /* pair planes of the plan's native layout (vrt_device.h: pair_index), angle after angle */,
               size_t plane_pairs)
{
    exp2_table_fill();
    __syncthreads();
    const int64_t pos = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= n) return;
    const int ia = blockIdx.y;
    const int32_t site = (ang.down[ia] ? store_down : store_up)[pos];
    T2 *__restrict__ out = out0 + (size_t)ia * plane_pairs;
    // v_los = dot(velocity, -k)   (line.jl:126, :205)
    const double v_los = velocity[3 * (size_t)site] * (-ang.k[ia][0]) + velocity[3 * (size_t)site + 1] * (-ang.k[ia][1]) +
                         velocity[3 * (size_t)site + 2] * (-ang.k[ia][2]);
    const double dD = doppler[site], ac = alpha_cont[site];
    const double r_dD = 1.0 / dD;
    const double ga = gamma[site] / (4.0 * kPi * c0 * dD);                 // a = gamma lambda^2 / (4 pi c dlambda_D), broadening.jl:87-89
    const double sp = strength[site] / (sqrt(kPi) * dD);                   // alpha_line = strength H / (sqrt(pi) dlambda_D), line.jl:133, :219-225
    const double shift = lambda0 * v_los / c0;
    for (int q = 0; q < npair; q++) {
        double v2[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int l = 2 * q + h;
            if (l < nlam) {
                const double lam = lambda[l];
                const double a = ga * (lam * lam);
                const double v = (lam - lambda0 + shift) * r_dD;                       // line.jl:132
                v2[h] = fma(sp, humlicek_w4_re(v, a), ac);                             // lambda_iteration.jl:93-96
            } else
                v2[h] = ac;                                                            // padding wavelength: finite
        }
        T2 o;
        o.x = (decltype(o.x))v2[0];
        o.y = (decltype(o.y))v2[1];
        out[pair_index(q, pos, n, lgB, npair)] = o;
    }
}

int launch_line_opacity(vrt_plan *p, int64_t nlam, const double *d_lambda, double lambda0, double c0,
                        const double *d_velocity, const double *d_doppler, const double *d_gamma,
                        const double *d_strength, const double *d_alpha_cont, void *d_out, hipStream_t st, bool f32_out)
{
    vrt_grid *g = p->g;
    const int64_t n = g->n;
    const int npair = (int)((nlam + 1) / 2);
    const size_t plane_pairs = (size_t)npair * (size_t)n;
    if (p->A <= 0) return VRT_OK;
    OpacityAngles ang;
    std::memset(&ang, 0, sizeof(ang));
    for (int a = 0; a < p->A; a++) {
        for (int j = 0; j < 3; j++) ang.k[a][j] = p->k[3 * (size_t)a + (size_t)j];
        ang.down[a] = p->dir_of_active[(size_t)a] > 0 ? 0 : 1;
    }
    const dim3 grid((unsigned)((n + 255) / 256), (unsigned)p->A);
    if (f32_out)
        hipLaunchKernelGGL(k_line_opacity<float2>, grid, dim3(256), 0, st, n, (int)nlam, npair, native_lg(p, f32_out), g->up.d_store,
                           g->down.d_store, ang, d_lambda, lambda0, c0, d_velocity, d_doppler, d_gamma, d_strength, d_alpha_cont,
                           reinterpret_cast<float2 *>(d_out), plane_pairs);
    else
        hipLaunchKernelGGL(k_line_opacity<double2>, grid, dim3(256), 0, st, n, (int)nlam, npair, native_lg(p, f32_out), g->up.d_store,
                           g->down.d_store, ang, d_lambda, lambda0, c0, d_velocity, d_doppler, d_gamma, d_strength, d_alpha_cont,
                           reinterpret_cast<double2 *>(d_out), plane_pairs);
    VRT_HIP_TRY(hipGetLastError());
    return VRT_OK;
}

// ---- population-dependent line terms -----------------------------------------------------------------
// γ of the CURRENT populations and the λ-independent factor of αline_λ, per site:
//   γ = γ_static + γ_unsold (n_1 + n_2)     γ_constant, src/broadening.jl:63-82, called with
//                                            populations[:,1] .+ populations[:,2] each iteration (lambda_iteration.jl:72-75);
//                                            γ_static = natural width + the two Stark terms (electron density and
//                                            temperature only), γ_unsold = the van der Waals width per unit neutral density
//   strength = strength_const (n_1 B_ij - n_2 B_ji)      αline_λ, src/line.jl:219-225
// populations (n, 3) column-major as Julia's
__global__ void __launch_bounds__(256)
k_line_terms(int64_t n, const double *__restrict__ gamma_static, const double *__restrict__ gamma_unsold,
             const double *__restrict__ pops, double strength_const, double Bij, double Bji,
             double *__restrict__ gamma, double *__restrict__ strength)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double n1 = pops[i], n2 = pops[i + n];
    if (gamma) gamma[i] = gamma_static[i] + gamma_unsold[i] * (n1 + n2);
    if (strength) strength[i] = strength_const * (n1 * Bij - n2 * Bji);
}

int launch_line_terms(int64_t n, const double *d_gamma_static, const double *d_gamma_unsold, const double *d_pops,
                      double strength_const, double Bij, double Bji, double *d_gamma, double *d_strength, hipStream_t st)
{
    hipLaunchKernelGGL(k_line_terms, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, d_gamma_static,
                       d_gamma_unsold, d_pops, strength_const, Bij, Bji, d_gamma, d_strength);
    VRT_HIP_TRY(hipGetLastError());
    return VRT_OK;
}

// ---- rates + populations epilogue ------------------------------------------------------------------
struct RatesArgs {
    int64_t n, nlam, ld;
    int64_t blocks[6];                  // [lo, hi) of the bb, bf-level-1, bf-level-2 wavelength blocks
    const double *lambda, *planck2;     // [nlam] device
    const double *sigma_bf1, *sigma_bf2;   // device, one entry per wavelength of the block
    const double *J;                    // (nlam, n), leading dimension ld
    // ... or per sweep direction in sweep order (vrt_plan_execute_native_dev): J = J_up + J_down; threads walk the up order
    const double *J_up = nullptr, *J_down = nullptr;
    const int32_t *store_up = nullptr, *rank_down = nullptr;
    double lambda0, c0, sigma_bb_const, hc_over_kB, pref_ij, pref_ji;
    const double *doppler, *gamma, *temperature, *lte, *C, *atom_density;
    double *R, *populations;
    // ... or the same two plane sets stored as float (vrt_plan_execute_native_dev_f32), pairs in blocks of 2^lgB
    const float *Jf_up = nullptr, *Jf_down = nullptr;
    int lgB = 0, npair = 0;
};

__device__ __forceinline__ void solve2(const double A[4], const double b[2], double x[2])
{
    double a00 = A[0], a10 = A[1], a01 = A[2], a11 = A[3], b0 = b[0], b1 = b[1];
    if (fabs(a10) > fabs(a00)) {                    // partial pivoting
        double t;
        t = a00; a00 = a10; a10 = t;
        t = a01; a01 = a11; a11 = t;
        t = b0; b0 = b1; b1 = t;
    }
    const double m = a10 / a00;
    const double u11 = a11 - m * a01;
    const double y1 = b1 - m * b0;
    x[1] = y1 / u11;
    x[0] = (b0 - a01 * x[1]) / a00;
}

// The rate kernels run 91 Boltzmann factors and 51 Voigt profiles per site and are bound by that arithmetic: the per-site
// divisors (Δλ_D, T) are inverted once, 1/λ comes from the hardware estimate + two Newton steps, exp(-hc/λkT) from the
// table-driven exp_neg_tab -- last-bit differences from the oracle's divisions and libm (contract of this row: 1e-12).
__device__ __forceinline__ double rcp_newton(double d)
{
    double r = __builtin_amdgcn_rcp(d);
    r = fma(fma(-d, r, 1.0), r, r);
    return fma(fma(-d, r, 1.0), r, r);
}
// libm's exp(-x) is exactly 0 from x = 745.1332191019412 (exp(-x) <= 2^-1075) on, and the smallest subnormal 2^-1074 just
// below it: past the threshold the factor is 0 like the oracle's, below it x is clamped to exp_neg_tab's domain (x <= 745).
__device__ __forceinline__ double boltzmann(double hc_over_kT, double lam)      // exp(-hc / (λ k T)), rates.jl:473
{
    const double x = hc_over_kT * rcp_newton(lam);
    return x >= 745.1332191019412 ? 0.0 : exp_neg_tab(fmin(x, 745.0));
}

// R of site i out, its statistical equilibrium solved (n_levels = 2, populations.jl:191-221)
__device__ __forceinline__ void populations_from_rates(const RatesArgs &ra, int64_t i, const double R[9])
{
    const int64_t n = ra.n;
    double P[9];
#pragma unroll
    for (int q = 0; q < 9; q++) {
        ra.R[9 * (size_t)i + q] = R[q];
        P[q] = R[q] + ra.C[9 * (size_t)i + q];                                           // populations.jl:195
    }
    // statistical equilibrium, n_levels = 2 (populations.jl:205-219)
#define PP(r, c) P[((r) - 1) + 3 * ((c) - 1)]
    const double N = ra.atom_density[i];
    double A[4], b[2], x[2];
    A[0] = PP(1, 2) + PP(2, 1) + PP(2, 3);
    A[2] = PP(1, 2) - PP(3, 2);
    A[3] = PP(1, 3) + PP(3, 1) + PP(3, 2);
    A[1] = PP(1, 3) - PP(2, 3);
    b[0] = N * PP(1, 2);
    b[1] = N * PP(1, 3);
#undef PP
    solve2(A, b, x);
    ra.populations[i + n] = x[0];
    ra.populations[i + 2 * n] = x[1];
    ra.populations[i] = N - (x[0] + x[1]);
}

// NATIVE: J comes per sweep direction in sweep order; a thread takes the site at up position blockIdx * 256 + tid, so that
// the J_up loads of a wave are contiguous (and the J_down loads piecewise contiguous: layers are the units of both orders) --
// the per-site inputs become gathers instead, 25 values against the 2 x nlam of J.  The arithmetic of a site is the same.
// T = float: the plane sets hold floats in the plan's pair blocks; J = (float)(J_up + J_down), the J that
// vrt_plan_j_from_native_dev_f32 delivers, widened -- everything after that is the same arithmetic.
template <bool NATIVE, typename T = double>
__global__ void __launch_bounds__(256)
k_rates_populations(RatesArgs ra)
{
    exp2_table_fill();
    __syncthreads();
    const int tid = threadIdx.x;
    const int64_t n = ra.n, site0 = (int64_t)blockIdx.x * 256;
    const bool valid = site0 + tid < n;
    const int64_t slot = valid ? site0 + tid : n - 1;               // (a thread past the end works on the last site and stores nothing)
    const int64_t i = NATIVE ? (int64_t)ra.store_up[slot] : slot;
    const int64_t pdn = NATIVE ? (int64_t)ra.rank_down[i] : 0;
    int64_t pair_have = -1;
    double2 pair_J = make_double2(0.0, 0.0);
    auto J_native = [&](int64_t l) -> double {
        // J = J_up + J_down as k_combine_J forms it; the two wavelengths of a pair come with one 16-byte load per direction
        const int64_t q = l >> 1;
        if (q != pair_have) {
            double2 v = make_double2(0.0, 0.0);
            if constexpr (sizeof(T) == 8) {
            const size_t o = (size_t)q * (size_t)n;
            if (ra.J_up) v = reinterpret_cast<const double2 *>(ra.J_up)[o + (size_t)slot];
            if (ra.J_down) {
                const double2 u = reinterpret_cast<const double2 *>(ra.J_down)[o + (size_t)pdn];
                v.x = v.x + u.x; v.y = v.y + u.y;
            }
            } else {
                if (ra.Jf_up) v = to_d2(reinterpret_cast<const float2 *>(ra.Jf_up)[pair_index((int)q, slot, n, ra.lgB, ra.npair)]);
                if (ra.Jf_down) {
                    const double2 u = to_d2(reinterpret_cast<const float2 *>(ra.Jf_down)[pair_index((int)q, pdn, n, ra.lgB, ra.npair)]);
                    v.x = v.x + u.x; v.y = v.y + u.y;
                }
                v = to_d2(from_d2<float>(v));
            }
            pair_J = v;
            pair_have = q;
        }
        return (l & 1) ? pair_J.y : pair_J.x;
    };
    // J is (n, ld) with the wavelength fastest: a thread walking its own row makes every load of the wave touch 64
    // different lines.  The block's 256 rows are staged through LDS 16 wavelengths at a time instead (a site's 128
    // bytes by 16 neighbouring lanes), and a thread picks its row's values up from there (row stride 17: no conflicts)
    __shared__ double Jt[256 * 17];
    auto stage = [&](int64_t l0c, int64_t hi) {
        __syncthreads();                                            // the previous chunk has been consumed
        for (int idx = tid; idx < 256 * 16; idx += 256) {
            const int sr = idx >> 4, c = idx & 15;
            const int64_t site = site0 + sr, l = l0c + c;
            Jt[sr * 17 + c] = (site < n && l < hi) ? ra.J[(size_t)site * (size_t)ra.ld + (size_t)l] : 0.0;
        }
        __syncthreads();
    };
    const double hT = ra.hc_over_kB / ra.temperature[i];
    double R[9];
#pragma unroll
    for (int q = 0; q < 9; q++) R[q] = 0.0;
    // ionisation / recombination: levels 1, 2 <-> continuum (rates.jl:170-178)
    for (int level = 1; level <= 2; level++) {
        const int64_t lo = ra.blocks[2 * level], hi = ra.blocks[2 * level + 1];
        const double *__restrict__ sig = level == 1 ? ra.sigma_bf1 : ra.sigma_bf2;
        const double n_ratio = ra.lte[i + n * (level - 1)] / ra.lte[i + n * 2];
        double rij = 0.0, rji = 0.0, s_prev = 0.0, G_prev = 0.0, J_prev = 0.0;
        for (int64_t l = lo; l < hi; l++) {
            if (!NATIVE && ((l - lo) & 15) == 0) stage(l, hi);
            const double lam = ra.lambda[l], s = sig[l - lo], Jl = NATIVE ? J_native(l) : Jt[tid * 17 + (int)((l - lo) & 15)];
            const double G = n_ratio * boltzmann(hT, lam);                               // Gij, rates.jl:473
            if (l > lo) {
                const double lp = ra.lambda[l - 1], dl = lam - lp;
                rij += ra.pref_ij * ((lp * s_prev * J_prev + lam * s * Jl) * dl);      // :262-263
                rji += ra.pref_ji * ((s_prev * G_prev * lp * (ra.planck2[l - 1] + J_prev) +
                                      s * G * lam * (ra.planck2[l] + Jl)) * dl);        // :357-358
            }
            s_prev = s; G_prev = G; J_prev = Jl;
        }
        R[(level - 1) + 3 * 2] = rij;
        R[2 + 3 * (level - 1)] = rji;
    }
    // bound-bound 1 <-> 2 (rates.jl:183-191): σij carries the static Voigt profile of the site
    {
        const int64_t lo = ra.blocks[0], hi = ra.blocks[1];
        const double n_ratio = ra.lte[i] / ra.lte[i + n];
        const double dD = ra.doppler[i], gm = ra.gamma[i];
        const double r_dD = 1.0 / dD, r_a = 1.0 / (4.0 * kPi * ra.c0 * dD), r_prof = 1.0 / (sqrt(kPi) * dD);
        double rij = 0.0, rji = 0.0, s_prev = 0.0, G_prev = 0.0, J_prev = 0.0;
        for (int64_t l = lo; l < hi; l++) {
            if (!NATIVE && ((l - lo) & 15) == 0) stage(l, hi);
            const double lam = ra.lambda[l], Jl = NATIVE ? J_native(l) : Jt[tid * 17 + (int)((l - lo) & 15)];
            const double a = gm * (lam * lam) * r_a;
            const double v = (lam - ra.lambda0) * r_dD;                                  // rates.jl:408
            const double s = ra.sigma_bb_const * (humlicek_w4_re(v, a) * r_prof);
            const double G = n_ratio * boltzmann(hT, lam);
            if (l > lo) {
                const double lp = ra.lambda[l - 1], dl = lam - lp;
                rij += ra.pref_ij * ((lp * s_prev * J_prev + lam * s * Jl) * dl);      // :236-237
                rji += ra.pref_ji * ((s_prev * G_prev * lp * (ra.planck2[l - 1] + J_prev) +
                                      s * G * lam * (ra.planck2[l] + Jl)) * dl);        // :312-313
            }
            s_prev = s; G_prev = G; J_prev = Jl;
        }
        R[0 + 3 * 1] = rij;
        R[1 + 3 * 0] = rji;
    }
    if (valid) populations_from_rates(ra, i, R);
}

// ---- the same split over wavelength blocks (several devices: vrt_multi_lambda_*, vrt_multi.cpp) -------------------------
// A device that owns the wavelengths [l0, l1) forms ITS share of the six λ-integrals of a site: the trapezoid sums of
// k_rates_populations regrouped per wavelength, Σ_l W_l f_l with W_l = (λ_l - λ_l-1) [l > lo] + (λ_l+1 - λ_l) [l < hi - 1]
// inside each block [lo, hi) -- the same terms, summed in another order (1e-15 relative per term).  The shares are
// summed across the devices (ONE all-reduce of 6 n doubles: no J travels), then every device solves
// the statistical equilibrium of every site itself (k_populations_from_shares).
// shares[q][i], q = (bf1 ij, bf1 ji, bf2 ij, bf2 ji, bb ij, bb ji); J: this device's columns, (l1 - l0) per site
// NATIVE: this device's columns of J as sweep-order plane sets (local wavelength l - l0), threads on up positions
// T = float: those plane sets hold floats in the plan's pair blocks, npair = ceil((l1 - l0) / 2) pairs of them;
// J = (float)(J_up + J_down) widened, as k_rates_populations<true, float> forms it -- everything after that is the same
// arithmetic.  The padding wavelength of an odd l1 - l0 rides along in the last pair's load and is never handed out.
template <bool NATIVE, typename T = double>
__global__ void __launch_bounds__(256)
k_rates_partial(RatesArgs ra, int64_t l0, int64_t l1, double *__restrict__ shares)
{
    exp2_table_fill();
    __syncthreads();
    const int64_t slot = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n = ra.n;
    if (slot >= n) return;
    const int64_t i = NATIVE ? (int64_t)ra.store_up[slot] : slot;
    const int64_t pdn = NATIVE ? (int64_t)ra.rank_down[i] : 0;
    const double *__restrict__ Ji = NATIVE ? nullptr : ra.J + (size_t)i * (size_t)ra.ld - l0;      // indexed by the GLOBAL wavelength
    int64_t pair_have = -1;
    double2 pair_J = make_double2(0.0, 0.0);
    auto J_at = [&](int64_t l) -> double {
        if constexpr (!NATIVE) return Ji[l];
        const int64_t ll = l - l0, q = ll >> 1;
        if (q != pair_have) {                                   // J = J_up + J_down as k_combine_J forms it
            double2 v = make_double2(0.0, 0.0);
            if constexpr (sizeof(T) == 8) {
            const size_t o = (size_t)q * (size_t)n;
            if (ra.J_up) v = reinterpret_cast<const double2 *>(ra.J_up)[o + (size_t)slot];
            if (ra.J_down) {
                const double2 u = reinterpret_cast<const double2 *>(ra.J_down)[o + (size_t)pdn];
                v.x = v.x + u.x; v.y = v.y + u.y;
            }
            } else {
                if (ra.Jf_up) v = to_d2(reinterpret_cast<const float2 *>(ra.Jf_up)[pair_index((int)q, slot, n, ra.lgB, ra.npair)]);
                if (ra.Jf_down) {
                    const double2 u = to_d2(reinterpret_cast<const float2 *>(ra.Jf_down)[pair_index((int)q, pdn, n, ra.lgB, ra.npair)]);
                    v.x = v.x + u.x; v.y = v.y + u.y;
                }
                v = to_d2(from_d2<float>(v));
            }
            pair_J = v;
            pair_have = q;
        }
        return (ll & 1) ? pair_J.y : pair_J.x;
    };
    const double hT = ra.hc_over_kB / ra.temperature[i];
    for (int tr = 0; tr < 3; tr++) {                                              // bf level 1, bf level 2, bb
        const int64_t lo = ra.blocks[tr < 2 ? 2 * (tr + 1) : 0], hi = ra.blocks[tr < 2 ? 2 * (tr + 1) + 1 : 1];
        const double n_ratio = tr < 2 ? ra.lte[i + n * tr] / ra.lte[i + n * 2] : ra.lte[i] / ra.lte[i + n];
        const double *__restrict__ sig = tr == 0 ? ra.sigma_bf1 : ra.sigma_bf2;
        const double dD = ra.doppler[i], gm = ra.gamma[i];
        const double r_dD = 1.0 / dD, r_a = 1.0 / (4.0 * kPi * ra.c0 * dD), r_prof = 1.0 / (sqrt(kPi) * dD);
        double rij = 0.0, rji = 0.0;
        for (int64_t l = lo > l0 ? lo : l0; l < (hi < l1 ? hi : l1); l++) {
            const double lam = ra.lambda[l], Jl = J_at(l);
            double s;
            if (tr < 2) s = sig[l - lo];
            else {
                const double a = gm * (lam * lam) * r_a;
                const double v = (lam - ra.lambda0) * r_dD;                              // rates.jl:408
                s = ra.sigma_bb_const * (humlicek_w4_re(v, a) * r_prof);
            }
            const double G = n_ratio * boltzmann(hT, lam);                               // Gij, rates.jl:473
            double W = 0.0;
            if (l > lo) W += lam - ra.lambda[l - 1];
            if (l < hi - 1) W += ra.lambda[l + 1] - lam;
            rij += (lam * s * Jl) * W;                                                   // rates.jl:236-237, :262-263
            rji += (s * G * lam * (ra.planck2[l] + Jl)) * W;                             // :312-313, :357-358
        }
        shares[(size_t)(2 * tr) * (size_t)n + (size_t)i] = ra.pref_ij * rij;
        shares[(size_t)(2 * tr + 1) * (size_t)n + (size_t)i] = ra.pref_ji * rji;
    }
}

__global__ void __launch_bounds__(256)
k_populations_from_shares(RatesArgs ra, const double *__restrict__ shares)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n = ra.n;
    if (i >= n) return;
    double R[9];
#pragma unroll
    for (int q = 0; q < 9; q++) R[q] = 0.0;
    for (int level = 1; level <= 2; level++) {
        R[(level - 1) + 3 * 2] = shares[(size_t)(2 * (level - 1)) * (size_t)n + (size_t)i];
        R[2 + 3 * (level - 1)] = shares[(size_t)(2 * (level - 1) + 1) * (size_t)n + (size_t)i];
    }
    R[0 + 3 * 1] = shares[(size_t)4 * (size_t)n + (size_t)i];
    R[1 + 3 * 0] = shares[(size_t)5 * (size_t)n + (size_t)i];
    populations_from_rates(ra, i, R);
}

// the kernels' arguments from the launches' named ones (vrt_line_case.h); R and the populations are the launch's to add.
// nplane: the wavelengths the plane sets of J hold (all of the case, or a device's block)
static RatesArgs rates_args(const RatesIn &in, const RatesJ &J, int64_t nplane)
{
    RatesArgs ra{};
    ra.n = in.n; ra.nlam = in.nlam; ra.ld = J.ld;
    for (int q = 0; q < 6; q++) ra.blocks[q] = in.k.blocks[q];
    ra.lambda = in.small.lambda; ra.planck2 = in.small.planck2;
    ra.sigma_bf1 = in.small.sigma_bf1; ra.sigma_bf2 = in.small.sigma_bf2;
    ra.lambda0 = in.k.lambda0; ra.c0 = in.k.c0; ra.sigma_bb_const = in.k.sigma_bb_const; ra.hc_over_kB = in.k.hc_over_kB;
    ra.pref_ij = in.k.pref_ij; ra.pref_ji = in.k.pref_ji;
    ra.doppler = in.doppler; ra.gamma = in.gamma; ra.temperature = in.temperature; ra.lte = in.lte;
    ra.C = in.C; ra.atom_density = in.atom_density;
    ra.J = J.rows;
    ra.J_up = J.up; ra.J_down = J.down;
    ra.Jf_up = J.up_f; ra.Jf_down = J.down_f;
    if (J.plan) {
        ra.lgB = native_lg(J.plan, true); ra.npair = (int)((nplane + 1) / 2);
    }
    if (const vrt_grid *g = J.plan ? J.plan->g : J.grid) {          // the orders the plane sets are stored in
        ra.store_up = g->up.d_store; ra.rank_down = g->down.d_srank;
    }
    return ra;
}

// this device's share of the rate integrals: wavelengths [l0, l1) of the FULL wavelength arrays of `in`; J holds those
// columns only (J.ld values per site, or sweep-order planes of l1 - l0 wavelengths: doubles, or floats in the pair
// blocks of J.plan's float layout)
int launch_rates_partial(const RatesIn &in, const RatesJ &J, int64_t l0, int64_t l1, double *d_shares, hipStream_t st)
{
    const RatesArgs ra = rates_args(in, J, l1 - l0);
    const dim3 grid((unsigned)((in.n + 255) / 256));
    if (J.up || J.down)
        hipLaunchKernelGGL(k_rates_partial<true>, grid, dim3(256), 0, st, ra, l0, l1, d_shares);
    else if (J.up_f || J.down_f)
        hipLaunchKernelGGL((k_rates_partial<true, float>), grid, dim3(256), 0, st, ra, l0, l1, d_shares);
    else
        hipLaunchKernelGGL(k_rates_partial<false>, grid, dim3(256), 0, st, ra, l0, l1, d_shares);
    VRT_HIP_TRY(hipGetLastError());
    return VRT_OK;
}

// R (9 n) and the populations (3 n) from the summed shares
int launch_populations_from_shares(int64_t n, const double *d_shares, const double *d_C, const double *d_atom_density,
                                   double *d_R, double *d_populations, hipStream_t st)
{
    RatesArgs ra{};
    ra.n = n;
    ra.C = d_C; ra.atom_density = d_atom_density; ra.R = d_R; ra.populations = d_populations;
    hipLaunchKernelGGL(k_populations_from_shares, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ra, d_shares);
    VRT_HIP_TRY(hipGetLastError());
    return VRT_OK;
}

// J in rows (a grid's sites, or n points without a grid: the regular-grid Λ-iteration), in a grid's sweep-order planes,
// or in a plan's float plane sets: J = (float)(J_up + J_down), widened
int launch_rates_populations(const RatesIn &in, const RatesJ &J, double *d_R, double *d_populations, hipStream_t st)
{
    RatesArgs ra = rates_args(in, J, in.nlam);
    ra.R = d_R; ra.populations = d_populations;
    const dim3 grid((unsigned)((in.n + 255) / 256));
    if (J.up || J.down)
        hipLaunchKernelGGL(k_rates_populations<true>, grid, dim3(256), 0, st, ra);
    else if (!J.up_f && !J.down_f)
        hipLaunchKernelGGL(k_rates_populations<false>, grid, dim3(256), 0, st, ra);
    else
        hipLaunchKernelGGL((k_rates_populations<true, float>), grid, dim3(256), 0, st, ra);
    VRT_HIP_TRY(hipGetLastError());
    return VRT_OK;
}

// ---- raster opacity and source function for an emergent spectrum (plotter, src/plot_utils.jl:297-355) -------------------
// One thread per point of the GHOSTED output (nz, nx + 2, ny + 2): a ghost point evaluates the interior point it wraps to
// (periodic_borders, src/atmosphere.jl:191-214) with the same instructions, so it holds that value bit for bit and the
// regular solver reads the arrays as they are.  The point's fields are read once and the launch's wavelengths walked;
// per (point, wavelength) one Voigt profile -- humlicek_w4_re, as k_line_opacity -- and one Planck function:
//   alpha_l = strength_const (n1 Bij - n2 Bji) H(a, v) / (sqrt(pi) dlambda_D)   line.jl:121-137, :219-225
//   S_l = src_const / (g_ratio n1 / n2 - 1)      source_line (line.jl:385-393)     S_c = planck2 / (exp(hc/kB / (lambda T)) - 1)
//   S = (alpha_l S_l + alpha_c S_c) / (alpha_l + alpha_c),  alpha_tot = alpha_l + alpha_c
// The per-point divisors are folded as in k_line_opacity (last-bit differences from the oracle; contract 1e-12).
constexpr int kSynthLam = 32;                        // wavelengths of one launch, passed by value
struct SynthLam { double lam[kSynthLam], planck2[kSynthLam]; };
struct SynthArgs {
    int64_t nz, nx, ny;                              // interior raster
    double k[3], lambda0, c0, hc_over_kB, strength_const, Bij, Bji, src_const, g_ratio;
    const double *velocity, *doppler, *gamma_static, *gamma_unsold, *temperature, *alpha_cont, *pops;
    double *S, *alpha;                               // (nlam, ny + 2, nx + 2, nz) numpy order
};

__global__ void __launch_bounds__(256)
k_synth_opacity(SynthArgs sa, SynthLam sl, int64_t l0, int nl)
{
    exp2_table_fill();
    __syncthreads();
    const int64_t nz = sa.nz, nx = sa.nx, ny = sa.ny, nxg = nx + 2, nyg = ny + 2, volg = nz * nxg * nyg;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= volg) return;
    const int64_t iz = t % nz, gx = (t / nz) % nxg, gy = t / (nz * nxg);
    const int64_t ix = gx == 0 ? nx - 1 : gx == nxg - 1 ? 0 : gx - 1;      // ghost column 1 = arr[:, end, :] (:200)
    const int64_t iy = gy == 0 ? ny - 1 : gy == nyg - 1 ? 0 : gy - 1;
    const int64_t vol = nz * nx * ny, i = iz + nz * (ix + nx * iy);
    const double n1 = sa.pops[i], n2 = sa.pops[i + vol];
    // v_los = dot(velocity, -k)   (line.jl:126, :205)
    const double v_los = sa.velocity[i] * (-sa.k[0]) + sa.velocity[i + vol] * (-sa.k[1]) + sa.velocity[i + 2 * vol] * (-sa.k[2]);
    const double dD = sa.doppler[i], ac = sa.alpha_cont[i], T = sa.temperature[i];
    const double gamma = sa.gamma_static[i] + sa.gamma_unsold[i] * (n1 + n2);      // γ_constant, broadening.jl:63-82
    const double strength = sa.strength_const * (n1 * sa.Bij - n2 * sa.Bji);
    const double S_l = sa.src_const / (sa.g_ratio * n1 / n2 - 1.0);
    const double r_dD = 1.0 / dD;
    const double ga = gamma / (4.0 * kPi * sa.c0 * dD);
    const double sp = strength / (sqrt(kPi) * dD);
    const double shift = sa.lambda0 * v_los / sa.c0;
    for (int l = 0; l < nl; l++) {
        const double lam = sl.lam[l];
        const double a = ga * (lam * lam);
        const double v = (lam - sa.lambda0 + shift) * r_dD;
        const double al = sp * humlicek_w4_re(v, a);
        const double S_c = sl.planck2[l] / (exp(sa.hc_over_kB / (lam * T)) - 1.0);
        const int64_t o = (l0 + l) * volg + t;
        sa.alpha[o] = al + ac;
        sa.S[o] = (al * S_l + ac * S_c) / (al + ac);
    }
}

}  // namespace vrt

using namespace vrt;

static int synth_opacity_checks(int64_t nz, int64_t nx, int64_t ny, const double *k, int64_t nlam, const double *lambda,
                                const double *planck2, const void *velocity, const void *doppler, const void *gamma_static,
                                const void *gamma_unsold, const void *temperature, const void *alpha_cont,
                                const void *populations, const void *S, const void *alpha)
{
    if (!k || !lambda || !planck2 || !velocity || !doppler || !gamma_static || !gamma_unsold || !temperature ||
        !alpha_cont || !populations || !S || !alpha)
        return fail(VRT_EINVAL, "NULL argument");
    if (nz < 1 || nx < 1 || ny < 1) return fail(VRT_EINVAL, "raster sizes must be >= 1");
    if (nlam < 1) return fail(VRT_EINVAL, "nlam must be >= 1");
    if (S == alpha) return fail(VRT_EINVAL, "S and alpha must be distinct arrays");
    const double nrm = std::sqrt(k[0] * k[0] + k[1] * k[1] + k[2] * k[2]);
    if (!(std::fabs(nrm - 1.0) < 1e-6)) return fail(VRT_EINVAL, "k is not a unit vector");
    return VRT_OK;
}

static int synth_opacity_launch(int64_t nz, int64_t nx, int64_t ny, const double *k, int64_t nlam, const double *lambda,
                                const double *planck2, double lambda0, double c0, double hc_over_kB, double strength_const,
                                double Bij, double Bji, double src_const, double g_ratio, const double *d_velocity,
                                const double *d_doppler, const double *d_gamma_static, const double *d_gamma_unsold,
                                const double *d_temperature, const double *d_alpha_cont, const double *d_populations,
                                double *d_S, double *d_alpha, hipStream_t st)
{
    SynthArgs sa;
    sa.nz = nz; sa.nx = nx; sa.ny = ny;
    for (int j = 0; j < 3; j++) sa.k[j] = k[j];
    sa.lambda0 = lambda0; sa.c0 = c0; sa.hc_over_kB = hc_over_kB; sa.strength_const = strength_const;
    sa.Bij = Bij; sa.Bji = Bji; sa.src_const = src_const; sa.g_ratio = g_ratio;
    sa.velocity = d_velocity; sa.doppler = d_doppler; sa.gamma_static = d_gamma_static; sa.gamma_unsold = d_gamma_unsold;
    sa.temperature = d_temperature; sa.alpha_cont = d_alpha_cont; sa.pops = d_populations;
    sa.S = d_S; sa.alpha = d_alpha;
    const int64_t volg = nz * (nx + 2) * (ny + 2);
    for (int64_t l0 = 0; l0 < nlam; l0 += kSynthLam) {
        const int nl = (int)std::min<int64_t>(kSynthLam, nlam - l0);
        SynthLam sl;
        std::memset(&sl, 0, sizeof(sl));
        for (int l = 0; l < nl; l++) {
            sl.lam[l] = lambda[l0 + l];
            sl.planck2[l] = planck2[l0 + l];
        }
        hipLaunchKernelGGL(k_synth_opacity, dim3((unsigned)((volg + 255) / 256)), dim3(256), 0, st, sa, sl, l0, nl);
    }
    VRT_HIP_TRY(hipGetLastError());
    return VRT_OK;
}

extern "C" int vrt_synth_opacity_dev(int64_t nz, int64_t nx, int64_t ny, const double *k, int64_t nlam,
                                     const double *lambda, const double *planck2, double lambda0, double c0,
                                     double hc_over_kB, double strength_const, double Bij, double Bji, double src_const,
                                     double g_ratio, const double *d_velocity, const double *d_doppler,
                                     const double *d_gamma_static, const double *d_gamma_unsold,
                                     const double *d_temperature, const double *d_alpha_cont,
                                     const double *d_populations, double *d_S, double *d_alpha, void *stream)
{
    return guarded([&] {
        int rc = synth_opacity_checks(nz, nx, ny, k, nlam, lambda, planck2, d_velocity, d_doppler, d_gamma_static,
                                      d_gamma_unsold, d_temperature, d_alpha_cont, d_populations, d_S, d_alpha);
        if (rc || (rc = use_current_device())) return rc;
        return synth_opacity_launch(nz, nx, ny, k, nlam, lambda, planck2, lambda0, c0, hc_over_kB, strength_const, Bij, Bji,
                                    src_const, g_ratio, d_velocity, d_doppler, d_gamma_static, d_gamma_unsold, d_temperature,
                                    d_alpha_cont, d_populations, d_S, d_alpha, (hipStream_t)stream);
    });
}

extern "C" int vrt_synth_opacity(int device, int64_t nz, int64_t nx, int64_t ny, const double *k, int64_t nlam,
                                 const double *lambda, const double *planck2, double lambda0, double c0,
                                 double hc_over_kB, double strength_const, double Bij, double Bji, double src_const,
                                 double g_ratio, const double *velocity, const double *doppler, const double *gamma_static,
                                 const double *gamma_unsold, const double *temperature, const double *alpha_cont,
                                 const double *populations, double *S, double *alpha)
{
    return guarded([&] {
        int rc = synth_opacity_checks(nz, nx, ny, k, nlam, lambda, planck2, velocity, doppler, gamma_static, gamma_unsold,
                                      temperature, alpha_cont, populations, S, alpha);
        if (rc || (rc = use_device(device))) return rc;
        const size_t vol = (size_t)(nz * nx * ny), out = (size_t)(nz * (nx + 2) * (ny + 2)) * (size_t)nlam;
        // one device block: velocity (3) | doppler | gamma_static | gamma_unsold | temperature | alpha_cont | populations (2)
        // | S | alpha
        DevBuf<double> d;
        if ((rc = d.alloc(10 * vol + 2 * out))) return rc;
        const double *src[7] = {velocity, doppler, gamma_static, gamma_unsold, temperature, alpha_cont, populations};
        const size_t len[7] = {3 * vol, vol, vol, vol, vol, vol, 2 * vol};
        double *dp[7] = {};
        size_t off = 0;
        hipError_t e = hipSuccess;
        for (int f = 0; f < 7 && e == hipSuccess; f++) {
            dp[f] = d + off;
            e = hipMemcpy(dp[f], src[f], sizeof(double) * len[f], hipMemcpyHostToDevice);
            off += len[f];
        }
        double *dS = d + off, *dA = dS + out;
        if (e != hipSuccess) return fail(VRT_ENODEVICE, std::string("vrt_synth_opacity: ") + hipGetErrorString(e));
        if ((rc = synth_opacity_launch(nz, nx, ny, k, nlam, lambda, planck2, lambda0, c0, hc_over_kB, strength_const, Bij,
                                       Bji, src_const, g_ratio, dp[0], dp[1], dp[2], dp[3], dp[4], dp[5], dp[6], dS, dA,
                                       nullptr)))
            return rc;
        if ((e = hipDeviceSynchronize()) != hipSuccess ||
            (e = hipMemcpy(S, dS, sizeof(double) * out, hipMemcpyDeviceToHost)) != hipSuccess ||
            (e = hipMemcpy(alpha, dA, sizeof(double) * out, hipMemcpyDeviceToHost)) != hipSuccess)
            return fail(VRT_ENODEVICE, std::string("vrt_synth_opacity: ") + hipGetErrorString(e));
        return VRT_OK;
    });
}
