// Re w4(x + i y), Humlíček's Voigt function, and its complex helpers: ONE device definition for every kernel that
// evaluates a line profile (vrt_physics.hip: the Voronoi opacity, rates and synthesis kernels; vrt_regular_lambda.hip:
// the raster opacity of the regular-grid Λ-iteration), so that the paths agree point for point.  Kernels that call it
// fill the exp2 table first (exp2_table_fill, vrt_weights.h).
#pragma once

#include <hip/hip_runtime.h>

#include "vrt_device.h"

namespace vrt {

// d = a b + c as ONE three-address instruction.  hipcc turns a Horner step whose addend is a constant kept in a vector
// register into a copy of the constant plus a two-address v_fmac (the opacity kernel: 67 of its 583 vector instructions were
// such copies, and its time is its vector-instruction count); the three-address form needs no copy.
__device__ __forceinline__ double fma3(double a, double b, double c)
{
#ifdef VRT_NO_FMA3
    return fma(a, b, c);
#else
    double d;
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
#endif
}

struct cplx { double re, im; };
__device__ __forceinline__ cplx c_mul(cplx a, cplx b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ __forceinline__ cplx c_add(cplx a, cplx b) { return {a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ cplx c_sub(cplx a, cplx b) { return {a.re - b.re, a.im - b.im}; }
__device__ __forceinline__ cplx c_real(double x) { return {x, 0.0}; }
__device__ __forceinline__ cplx c_scale(cplx a, double s) { return {a.re * s, a.im * s}; }

// Re w4(x + i y), y >= 0: Humlíček's four regions.  The opacity kernel is bound by this arithmetic (51 evaluations
// per site and angle, ~290 fp64 instruction slots each as the oracle writes it), so the Horner steps use fused
// multiply-adds (c + t p in 4 instructions instead of 7) and the one real part that is needed is formed with a
// Newton-refined reciprocal instead of two divisions: last-bit differences from the oracle (contract 1e-12).
__device__ __forceinline__ cplx c_fma(cplx t, cplx p, double c)           // c + t p
{
    return {fma(t.re, p.re, fma(-t.im, p.im, c)), fma(t.re, p.im, t.im * p.re)};
}
__device__ __forceinline__ cplx c_fms(cplx t, cplx p, double c)           // c - t p
{
    return {fma(-t.re, p.re, fma(t.im, p.im, c)), -fma(t.re, p.im, t.im * p.re)};
}
__device__ __forceinline__ double c_div_re(cplx a, cplx b)                // Re(a / b)
{
    const double d = fma(b.re, b.re, b.im * b.im);
    double r = __builtin_amdgcn_rcp(d);
    r = fma(fma(-d, r, 1.0), r, r);
    r = fma(fma(-d, r, 1.0), r, r);                        // (v_rcp_f64 is good to ~2^-23: the second step is needed below 1e-13)
    return fma(a.re, b.re, a.im * b.im) * r;
}
// cos z for the |z| <= ~12 that region 4 of w4 can produce (z = -2 x y, |x| + y < 5.5): when every lane of the wave has
// |z| <= pi/4 -- the narrow damping wings of a stellar atmosphere: always -- its Taylor polynomial to z^14 (remainder
// 1e-15); otherwise Cody-Waite reduction by pi/2 (fdlibm's two-part split: exact for |k| <= 2^20) and the sine /
// cosine polynomials of the reduced argument.  (libm's cos drags its large-argument reduction into the kernel:
// 102 -> VGPRs and a third of this region's instructions.)
__device__ __forceinline__ double cos_poly(double z2)
{
    double p = -1.0 / 87178291200.0;
    p = fma3(p, z2, 1.0 / 479001600.0);
    p = fma3(p, z2, -1.0 / 3628800.0);
    p = fma3(p, z2, 1.0 / 40320.0);
    p = fma3(p, z2, -1.0 / 720.0);
    p = fma3(p, z2, 1.0 / 24.0);
    p = fma(p, z2, -0.5);
    return fma(p, z2, 1.0);
}
__device__ __forceinline__ double cos_small(double z)
{
    if (__ballot(fabs(z) > 0.78539816339744831) == 0ull) return cos_poly(z * z);
    const double kf = rint(z * 0.63661977236758134308);
    double r = fma(-kf, 1.57079632673412561417e+00, z);
    r = fma(-kf, 6.07710050650619224932e-11, r);
    const double r2 = r * r;
    double sp = -1.0 / 1307674368000.0;
    sp = fma(sp, r2, 1.0 / 6227020800.0);
    sp = fma(sp, r2, -1.0 / 39916800.0);
    sp = fma(sp, r2, 1.0 / 362880.0);
    sp = fma(sp, r2, -1.0 / 5040.0);
    sp = fma(sp, r2, 1.0 / 120.0);
    sp = fma(sp, r2, -1.0 / 6.0);
    const double sn = fma(sp * r2, r, r), cs = cos_poly(r2);
    const int q = (int)kf & 3;
    const double v = (q & 1) ? sn : cs;
    return (q == 1 || q == 2) ? -v : v;
}

// A polynomial with REAL coefficients at a complex point z costs two fused multiply-adds per coefficient, not the four of
// a complex Horner step (Knuth, TAOCP 4.6.4 (3): with r = 2 Re z, s = |z|^2 the pair a_j = b_(j-1) + r a_(j-1),
// b_j = c_j - s a_(j-1) ends in P(z) = z a + b).  Regions 3 and 4 of w4 are quotients of such polynomials -- in t and in
// m = -t^2 -- and carry ~70 % of the kernel's instructions; against the oracle's complex Horner form the result differs by
// <= 7e-14 relative over the regions' whole domain (contract 1e-12; w4's own accuracy is 1e-4).
__device__ __forceinline__ void zp_step(double &a, double &b, double r, double ms, double c)
{
    const double a0 = a;
    a = fma(r, a0, b);
    b = fma3(ms, a0, c);
}
__device__ __forceinline__ cplx zp_value(cplx z, double a, double b) { return {fma(z.re, a, b), z.im * a}; }

static __device__ double humlicek_w4_re(double x, double y)
{
    const cplx t = {y, -x};
    const double s = fabs(x) + y;
    if (s >= 15.0) return c_div_re(c_scale(t, 0.5641896), c_fma(t, t, 0.5));
    if (s >= 5.5) {
        const cplx u = c_mul(t, t);
        return c_div_re(c_mul(t, c_add(c_real(1.410474), c_scale(u, 0.5641896))), c_fma(u, c_add(c_real(3.0), u), 0.75));
    }
    const double t2 = fma(x, x, y * y);                    // |t|^2
    if (y >= 0.195 * fabs(x) - 0.176) {
        const double r = y + y, ms = -t2;
        double na = 0.5642236, nb = 3.778987;
        zp_step(na, nb, r, ms, 11.96482);
        zp_step(na, nb, r, ms, 20.20933);
        zp_step(na, nb, r, ms, 16.4955);
        double da = 1.0, db = 6.699398;
        zp_step(da, db, r, ms, 21.69274);
        zp_step(da, db, r, ms, 39.27121);
        zp_step(da, db, r, ms, 38.82363);
        zp_step(da, db, r, ms, 16.4955);
        return c_div_re(zp_value(t, na, nb), zp_value(t, da, db));
    }
    // region 4 in m = -t^2 = (x^2 - y^2, 2 x y): every coefficient positive
    const cplx m = {fma(x, x, -(y * y)), 2.0 * (x * y)};
    const double r = m.re + m.re, ms = -(t2 * t2);         // |m|^2 = |t|^4
    double na = 0.56419, nb = 1.320522;
    zp_step(na, nb, r, ms, 35.76683);
    zp_step(na, nb, r, ms, 219.0313);
    zp_step(na, nb, r, ms, 1540.787);
    zp_step(na, nb, r, ms, 3321.9905);
    zp_step(na, nb, r, ms, 36183.31);
    double da = 1.0, db = 1.841439;
    zp_step(da, db, r, ms, 61.57037);
    zp_step(da, db, r, ms, 364.2191);
    zp_step(da, db, r, ms, 2186.181);
    zp_step(da, db, r, ms, 9022.228);
    zp_step(da, db, r, ms, 24322.84);
    zp_step(da, db, r, ms, 32066.6);
    // exp(u.re) cos(u.im), u = t^2 = -m: here y < 0.195 |x| - 0.176, so u.re < 0 (table-driven exp_neg_tab,
    // vrt_device.h) and |u.im| is small for the narrow damping wings of a stellar atmosphere: when every lane of the
    // wave has |u.im| <= pi/4 the cosine is its Taylor polynomial to z^14 (remainder 1e-15), no range reduction.
    const double ex = exp_neg_tab(m.re);
    return ex * cos_small(m.im) - c_div_re(c_mul(t, zp_value(m, na, nb)), zp_value(m, da, db));
}

}  // namespace vrt
