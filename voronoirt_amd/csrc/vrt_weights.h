// linear_weights (functions.jl:484-500) on the device: every copy of the three-branch formula, the two hand-written
// exponentials they use and the wave-uniform branch dispatch of the patch kernels.  The branch constants 5e-4 and 50
// appear in code in this file only (tests/test_host.py scans for a further copy); tests/probes/weights_probe.hip
// calls every function here directly and tests/test_weights_domain.py judges each against a 40-digit reference.
#pragma once

#include <hip/hip_runtime.h>

namespace vrt {

// ---- the reference's order of operations: libm exp, plain divisions (level path, regular-grid solver) ----

__device__ __forceinline__ void linear_weights_ref_order(double dtau, double &a, double &b, double &e)
{
    if (dtau < 5e-4) {                                   // functions.jl:484-500
        e = 1.0 - dtau + 0.5 * (dtau * dtau);
        a = dtau * (0.5 - dtau / 3.0);
        b = dtau * (0.5 - dtau / 6.0);
    } else if (dtau > 50.0) {
        e = 0.0;
        a = 1.0 / dtau;
        b = 1.0 - a;
    } else {
        e = exp(-dtau);
        a = (1.0 - e) / dtau - e;
        b = 1.0 - a - e;
    }
}

// ---- step / tile paths ----
// linear_weights (functions.jl:484-500) with the arithmetic trimmed for the ALU-bound phase 1:
// one Newton-refined reciprocal shared by the thick and the exponential branch, the Taylor
// branch's /3 and /6 as multiplications, and exp(-x) for the only range it is needed in
// (5e-4 <= x <= 50: no overflow, underflow, NaN or subnormal handling).  Each piece is accurate
// to ~1 ulp; results differ from the oracle's libm at the 1e-16 level (contract: 1e-10).
__device__ __forceinline__ double exp_neg(double x)       // exp(-x), 5e-4 <= x <= 50
{
    const double t = -x;
    const double kf = rint(t * 1.4426950408889634074);    // k = round(t / ln 2), |k| <= 73
    double r = fma(-kf, 6.93147180369123816490e-01, t);   // Cody-Waite: ln2 = hi + lo
    r = fma(-kf, 1.90821492927058770002e-10, r);           // |r| <= 0.3466
    double p = 1.0 / 6227020800.0;                         // Taylor to r^13/13!: remainder < 4e-18
    p = fma(p, r, 1.0 / 479001600.0);
    p = fma(p, r, 1.0 / 39916800.0);
    p = fma(p, r, 1.0 / 3628800.0);
    p = fma(p, r, 1.0 / 362880.0);
    p = fma(p, r, 1.0 / 40320.0);
    p = fma(p, r, 1.0 / 5040.0);
    p = fma(p, r, 1.0 / 720.0);
    p = fma(p, r, 1.0 / 120.0);
    p = fma(p, r, 1.0 / 24.0);
    p = fma(p, r, 1.0 / 6.0);
    p = fma(p, r, 0.5);
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    return ldexp(p, (int)kf);
}

// exp(-x) for 0 <= x <= 745 (the patch kernels call it for 5e-4 <= x <= 50, the rate kernels up to 745), table-driven: -x = N ln2/32 + r with |r| <= ln2/64, exp(-x) = 2^(N >> 5) T[N & 31] p(r),
// T[j] = 2^(j/32) from a 32-entry LDS table (one 8-byte read per evaluation, conflict-free: the 32 entries cover the
// 64 banks once) and p the degree-5 Taylor polynomial (remainder r^6/720 < 2.3e-15).  Against the degree-10 polynomial
// on |r| <= ln2/2 it replaces: four fused multiply-adds fewer per evaluation, and five of its eleven non-inline fp64
// constants -- ten scalar registers of a kernel that is short of exactly those.  Relative error ~3e-15 (contract 1e-10).
static __device__ const double kExp2_32[32] = {
    1.0, 1.0218971486541166, 1.0442737824274138, 1.0671404006768237, 1.0905077326652577, 1.1143867425958924,
    1.1387886347566916, 1.1637248587775775, 1.189207115002721, 1.215247359980469, 1.241857812073484, 1.2690509571917332,
    1.2968395546510096, 1.3252366431597413, 1.3542555469368927, 1.383909881963832, 1.4142135623730951, 1.4451808069770467,
    1.4768261459394993, 1.5091644275934228, 1.5422108254079407, 1.5759808451078865, 1.6104903319492543, 1.645755478153965,
    1.681792830507429, 1.718619298122478, 1.7562521603732995, 1.7947090750031072, 1.8340080864093424, 1.8741676341103,
    1.9152065613971474, 1.9571441241754002};
__device__ __forceinline__ double *exp2_table()
{
    __shared__ double t[32];
    return t;
}
// every kernel that evaluates it: fill the table, then a barrier before the first evaluation
__device__ __forceinline__ void exp2_table_fill()
{
    if (threadIdx.x < 32) exp2_table()[threadIdx.x] = kExp2_32[threadIdx.x];
}
// the two halves of the fill for a kernel with other loads to wait for at its start: the table's load beside them, the
// write behind them (every thread writes: no branch for the load to sink into)
__device__ __forceinline__ double exp2_table_load() { return kExp2_32[threadIdx.x & 31u]; }
__device__ __forceinline__ void exp2_table_store(double v) { exp2_table()[threadIdx.x & 31u] = v; }
// Past x = 708.4 the result is subnormal: the final ldexp rounds it to the subnormal grid (steps of 2^-1074).
__device__ __forceinline__ double exp_neg_tab(double x)          // exp(-x), 0 <= x <= 745
{
    const double t = -x;
    const double nf = rint(t * 46.16624130844683);            // N = round(t 32 / ln 2), |N| <= 34394
    double r = fma(-nf, 0.021660849335603416, t);             // Cody-Waite: ln2/32 = hi (29 bits) + lo
    r = fma(-nf, 5.689487495325457e-11, r);                   // |r| <= 0.01084
    const int N = (int)nf;
    double p = 1.0 / 120.0;
    p = fma(p, r, 1.0 / 24.0);
    p = fma(p, r, 1.0 / 6.0);
    p = fma(p, r, 0.5);
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    return ldexp(p * exp2_table()[N & 31], N >> 5);
}

__device__ __forceinline__ void lin_weights(double dtau, double &a, double &b, double &e)
{
    // reciprocal of dtau (only consumed when dtau >= 5e-4): hardware estimate + 2 Newton steps.  The residual 1 - dtau rc
    // is far below 1 for finite dtau, so fmin(residual, 1) leaves it alone; for dtau = +Inf (rc = 0) the residual is
    // -Inf 0 + 1 = NaN, fmin returns its other operand and rc stays 0: a = 1/Inf = 0, b = 1 like the reference.
    double rc = __builtin_amdgcn_rcp(dtau);
    rc = fma(fmin(fma(-dtau, rc, 1.0), 1.0), rc, rc);
    rc = fma(fmin(fma(-dtau, rc, 1.0), 1.0), rc, rc);
    const double ee = exp_neg(fmin(fmax(dtau, 5e-4), 50.0));
    if (!(dtau >= 5e-4)) {                                 // Taylor branch; a NaN goes here too and comes out as NaN in a, b AND e
        e = 1.0 - dtau + 0.5 * (dtau * dtau);
        a = dtau * (0.5 - dtau * (1.0 / 3.0));
        b = dtau * (0.5 - dtau * (1.0 / 6.0));
    } else if (dtau > 50.0) {
        e = 0.0;
        a = rc;
        b = 1.0 - a;
    } else {
        e = ee;
        a = (1.0 - e) * rc - e;
        b = 1.0 - a - e;
    }
}

// ---- patch kernels ----
// exp(-x) for 5e-4 <= x <= 50: the table-driven exp_neg_tab above (every patch kernel fills the table)
__device__ __forceinline__ double exp_neg10(double x) { return exp_neg_tab(x); }

// The kernel is bound by its fp64 arithmetic (two exponentials and a dozen weights per site, angle and
// wavelength; MI355X issues a wave's fp64 instruction in 4 cycles), so the weights are written with explicit
// fused multiply-adds -- a third fewer instructions than the reference's expression order, results within a few
// ulp of it (the parity contract is 1e-10; the build-wide -ffp-contract=off stays for the neighbour search).
//
// linear_weights (functions.jl:484-500) without control flow inside a lane; `MODE` is wave-uniform:
//   0  no lane has 5e-4 <= Δτ <= 50: thin or thick only, no exponential (optically thin upper layers and
//      thick bottom layers are most of a stratified atmosphere; a wave's lanes are neighbouring sites of a layer)
//   1  no lane is thin: no Taylor branch
//   2  general
// The thick branch (Δτ > 50: e = 0, a = 1/Δτ, b = 1 - a) needs no select for a and b: the exponential itself is set to 0
// there, and with e = 0 the general formulas ARE fma(1, rc, -0) = rc and (1 - rc) - 0 -- bit for bit what MODE 0 returns,
// for every Δτ up to +Inf.  (Leaving e = exp(-50) = 1.9e-22 in them rounds to the same values only while 1.9e-22 is below
// half an ulp of 1/Δτ, Δτ < 5.8e5: beyond that a lane's result depended on its wave mates through MODE.)
// A NaN counts as thin, here and in the ballots below, so that it comes out as NaN in a, b and e (MODE 1 never sees one).
template <int MODE>
__device__ __forceinline__ void lin_weights_fma(double dtau, double &a, double &b, double &e)
{
    double rc = __builtin_amdgcn_rcp(dtau);                 // only consumed when dtau >= 5e-4
    // v_rcp_f64 is good to ~2^-23: one Newton step -> 1e-14.  fmin(residual, 1) changes nothing for finite dtau; for
    // dtau = +Inf (rc = 0, residual NaN) it keeps rc = 0: a = 0, b = 1 like the reference's 1/Inf
    rc = fma(fmin(fma(-dtau, rc, 1.0), 1.0), rc, rc);
    double e_thin = 0.0, a_thin = 0.0, b_thin = 0.0;
    if (MODE != 1) {
        e_thin = fma(dtau, fma(0.5, dtau, -1.0), 1.0);
        a_thin = dtau * fma(dtau, -1.0 / 3.0, 0.5);
        b_thin = dtau * fma(dtau, -1.0 / 6.0, 0.5);
    }
    const bool thin = !(dtau >= 5e-4);
    if (MODE == 0) {
        e = thin ? e_thin : 0.0;
        a = thin ? a_thin : rc;
        b = thin ? b_thin : 1.0 - rc;
        return;
    }
    const double e_mid = dtau > 50.0 ? 0.0 : exp_neg10(fmin(dtau, 50.0));
    const double a_mid = fma(1.0 - e_mid, rc, -e_mid), b_mid = (1.0 - a_mid) - e_mid;
    if (MODE == 1) {
        e = e_mid; a = a_mid; b = b_mid;
    } else {
        e = thin ? e_thin : e_mid;
        a = thin ? a_thin : a_mid;
        b = thin ? b_thin : b_mid;
    }
}

// one wavelength of an entry: both upwinds' shares of a visit, t_r = ((e_r I_ur + a_r S_ur) + b_r S_c) w_r with
// I_ur gathered as 0 unless upwind r lies in an earlier layer; g_r = e_r wg_r, wg_r = w_r if upwind r lies in the
// site's own layer, else 0.  c = t_1 + t_2.  dt_r = r_r (α_c + α_ur) / 2 (trapezoidal, functions.jl:393).
template <int MODE>
__device__ __forceinline__ void entry_terms(double dt1, double dt2, double w1, double w2, double wg1, double wg2,
                                            double S_c, double S_1, double S_2, double I_1, double I_2, double &c,
                                            double &g1, double &g2)
{
    double ca1, cb1, ce1, ca2, cb2, ce2;
    lin_weights_fma<MODE>(dt1, ca1, cb1, ce1);
    lin_weights_fma<MODE>(dt2, ca2, cb2, ce2);
    const double t1 = fma(cb1, S_c, fma(ce1, I_1, ca1 * S_1)) * w1;
    const double t2 = fma(cb2, S_c, fma(ce2, I_2, ca2 * S_2)) * w2;
    c = t1 + t2;
    g1 = ce1 * wg1;
    g2 = ce2 * wg2;
}

// the same with the wave-uniform choice of MODE from the two optical depths of every lane
__device__ __forceinline__ void entry_lambda(double rh1, double rh2, double w1, double w2, double wg1, double wg2,
                                             double a_c, double a_1, double a_2, double S_c, double S_1, double S_2,
                                             double I_1, double I_2, double &c, double &g1, double &g2)
{
    const double d1 = rh1 * (a_c + a_1), d2 = rh2 * (a_c + a_2);
    const bool mid = ((d1 >= 5e-4) & (d1 <= 50.0)) | ((d2 >= 5e-4) & (d2 <= 50.0));
    const bool thin = !(d1 >= 5e-4) | !(d2 >= 5e-4);
    if (__ballot(mid) == 0ull) entry_terms<0>(d1, d2, w1, w2, wg1, wg2, S_c, S_1, S_2, I_1, I_2, c, g1, g2);
    else if (__ballot(thin) == 0ull) entry_terms<1>(d1, d2, w1, w2, wg1, wg2, S_c, S_1, S_2, I_1, I_2, c, g1, g2);
    else entry_terms<2>(d1, d2, w1, w2, wg1, wg2, S_c, S_1, S_2, I_1, I_2, c, g1, g2);
}

// The same, one upwind at a time: `next` (the optical depth the following evaluation starts from) is tied to this
// one's results by a compiler fence, so that the four evaluations of an entry's pair follow each other instead of
// being interleaved (the compiler's own order needs 72 registers, this one 64).  The
// weights w_r are read from the thread's LDS slots where they are used (pw1, pw2), not held.
template <int MODE>
__device__ __forceinline__ void entry_terms_seq(double dt1, double dt2, const double *pw1, const double *pw2, bool in1,
                                                bool in2, double S_c, double S_1, double S_2, double I_1, double I_2,
                                                double &c, double &g1, double &g2, double &next)
{
    double ca, cb, ce;
    lin_weights_fma<MODE>(dt1, ca, cb, ce);
    const double w1 = *pw1;
    double t1 = fma(cb, S_c, fma(ce, I_1, ca * S_1)) * w1;
    g1 = in1 ? ce * w1 : 0.0;
    asm volatile("" : "+v"(t1), "+v"(g1), "+v"(dt2));
    lin_weights_fma<MODE>(dt2, ca, cb, ce);
    const double w2 = *pw2;
    const double t2 = fma(cb, S_c, fma(ce, I_2, ca * S_2)) * w2;
    c = t1 + t2;
    g2 = in2 ? ce * w2 : 0.0;
    asm volatile("" : "+v"(c), "+v"(g2), "+v"(next));
}
__device__ __forceinline__ void entry_lambda_seq(double d1, double d2, const double *pw1, const double *pw2, bool in1,
                                                 bool in2, double S_c, double S_1, double S_2, double I_1, double I_2,
                                                 double &c, double &g1, double &g2, double &next)
{
    const bool mid = ((d1 >= 5e-4) & (d1 <= 50.0)) | ((d2 >= 5e-4) & (d2 <= 50.0));
    const bool thin = !(d1 >= 5e-4) | !(d2 >= 5e-4);
    if (__ballot(mid) == 0ull) entry_terms_seq<0>(d1, d2, pw1, pw2, in1, in2, S_c, S_1, S_2, I_1, I_2, c, g1, g2, next);
    else if (__ballot(thin) == 0ull) entry_terms_seq<1>(d1, d2, pw1, pw2, in1, in2, S_c, S_1, S_2, I_1, I_2, c, g1, g2, next);
    else entry_terms_seq<2>(d1, d2, pw1, pw2, in1, in2, S_c, S_1, S_2, I_1, I_2, c, g1, g2, next);
}

// The same visit with the upwind intensities applied LAST (the data-as-flag chained launch, where a workgroup waits for
// exactly those): everything that does not need I_1, I_2 -- the four weights, a_r S_ur, the couplings -- is formed while the
// gathers are in flight or repeated, and what is left behind the wait is three dependent operations per upwind.  The
// same operations on the same values in the same association as entry_terms_seq: bit-identical.
struct LateTerms { double ce1, p1, cb1, ce2, p2, cb2; };
template <int MODE>
__device__ __forceinline__ void late_coeffs(double dt1, double dt2, double S_1, double S_2, LateTerms &L, double &next)
{
    double ca, cb, ce;
    lin_weights_fma<MODE>(dt1, ca, cb, ce);
    L.ce1 = ce; L.p1 = ca * S_1; L.cb1 = cb;
    asm volatile("" : "+v"(L.ce1), "+v"(L.p1), "+v"(L.cb1), "+v"(dt2));
    lin_weights_fma<MODE>(dt2, ca, cb, ce);
    L.ce2 = ce; L.p2 = ca * S_2; L.cb2 = cb;
    asm volatile("" : "+v"(L.ce2), "+v"(L.p2), "+v"(L.cb2), "+v"(next));
}
__device__ __forceinline__ void late_lambda(double d1, double d2, double S_1, double S_2, LateTerms &L, double &next)
{
    const bool mid = ((d1 >= 5e-4) & (d1 <= 50.0)) | ((d2 >= 5e-4) & (d2 <= 50.0));
    const bool thin = !(d1 >= 5e-4) | !(d2 >= 5e-4);
    if (__ballot(mid) == 0ull) late_coeffs<0>(d1, d2, S_1, S_2, L, next);
    else if (__ballot(thin) == 0ull) late_coeffs<1>(d1, d2, S_1, S_2, L, next);
    else late_coeffs<2>(d1, d2, S_1, S_2, L, next);
}
__device__ __forceinline__ void late_apply(const LateTerms &L, const double *pw1, const double *pw2, bool in1, bool in2,
                                           double S_c, double I_1, double I_2, double &c, double &g1, double &g2)
{
    const double w1 = *pw1, w2 = *pw2;
    const double t1 = fma(L.cb1, S_c, fma(L.ce1, I_1, L.p1)) * w1;
    const double t2 = fma(L.cb2, S_c, fma(L.ce2, I_2, L.p2)) * w2;
    c = t1 + t2;
    g1 = in1 ? L.ce1 * w1 : 0.0;
    g2 = in2 ? L.ce2 * w2 : 0.0;
}

}  // namespace vrt
