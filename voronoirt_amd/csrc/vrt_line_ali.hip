// The diagonal approximate operator Λ* of the LINE Λ-iteration on a Voronoi plan (vrt_lambda_use_operator,
// vrt_line_lambda_diagonal_dev).  The definition, the angle order and the treatment of layer 1 and of the never-visited
// last site are those of k_lambda_diagonal (vrt_continuum.hip); what differs is where α comes from.  In the line loop
// α_tot differs per angle (the Doppler shift of v_los = dot(velocity, -k)) and changes every iterate (γ and the line
// strength follow the populations), and it exists only in the plan's native per-angle layout (VRT_ALPHA_ANGLE_NATIVE:
// wavelength pairs in pair blocks, at the storage position of the angle's direction).  So Λ* is formed from that buffer,
// every iterate, after the opacity kernel and on its stream; nothing of it is kept from one iterate to the next.
//
//   Λ*[i,l] = Σ_a w_a upd(a,i) ((W_1 b(Δτ_1)) + (W_2 b(Δτ_2))),  Δτ_r = R_r (α_a[i,l] + α_a[up_r(a,i),l]) / 2
//
// The update that uses it is the ALI instantiation of k_lambda_update / k_lambda_update_native (vrt_kernels.hip).
#include <algorithm>
#include <cstdint>

#include "vrt_device.h"

namespace vrt {
namespace {

constexpr int kDiagPairs = 4;           // wavelength pairs per thread: 12 independent 16-byte loads per angle

// One thread per (site, group of kDiagPairs wavelength pairs; blockIdx.y = the group): the thread walks the angles in
// order, slot 1 then slot 2, and keeps its eight sums in registers -- `diag = 0; diag += w_a (t_1 + t_2)` per
// contributing angle, the operations of k_lambda_diagonal in its order, so one angle alone gives that kernel's bits.  No
// atomics: the same inputs give the same bits.
//   PLANES: thread index = UP storage position; Λ* leaves as an up-order plane set ([pair][pos][2], one 16-byte store
//           per pair, the padding wavelength of an odd nlam zero) -- what k_lambda_update_native<true> reads
//   rows:   thread index = site; Λ* leaves as (n, ld) rows, the padding columns untouched
// Every α access is one 16-byte pair: the centre at the site's storage position of the angle's direction (contiguous
// over the lanes for the up angles of PLANES, piecewise contiguous otherwise: a layer is a layer in every order), the two
// upwinds at srank[up_r] -- the only gathers besides the tables' rows.  The [A][n] upwind tables are in site order and
// read once per (angle, thread); the groups of a site re-read them (40 bytes per angle against 3 x 64 of α).
template <bool PLANES>
__global__ void __launch_bounds__(256)
k_line_lambda_diagonal(int64_t n, int nlam, int npair, int lgB, int64_t ld, int A, DiagAngles ang, int32_t n1_up, int32_t n1_down,
                       const int32_t *__restrict__ store_up, const int32_t *__restrict__ srank_up,
                       const int32_t *__restrict__ srank_down, const int32_t *__restrict__ up1,
                       const int32_t *__restrict__ up2, const double *__restrict__ w1, const double *__restrict__ w2,
                       const double *__restrict__ r1, const double *__restrict__ r2, const double2 *__restrict__ alpha,
                       double *__restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int q0 = (int)blockIdx.y * kDiagPairs;
    const int32_t site = PLANES ? store_up[t] : (int32_t)t;
    const int32_t pos_up = PLANES ? (int32_t)t : srank_up[site], pos_down = srank_down[site];
    // the group's pairs in the native layout: offset of the pair inside its block's plane, log2 of the block's width
    size_t base[kDiagPairs];
    int lw[kDiagPairs];
#pragma unroll
    for (int u = 0; u < kDiagPairs; u++) {
        const int q = q0 + u < npair ? q0 + u : npair - 1;          // (past the end: the last pair again, unused)
        int k0;
        pair_block_at(q, npair, lgB, k0, lw[u]);
        base[u] = (size_t)k0 * (size_t)n + (size_t)(q - k0);
    }
    double2 acc[kDiagPairs];
#pragma unroll
    for (int u = 0; u < kDiagPairs; u++) acc[u] = make_double2(0.0, 0.0);
    const size_t plane = (size_t)npair * (size_t)n;                  // pairs of one angle's block
    for (int a = 0; a < A; a++) {
        const bool down = ang.down[a] != 0;
        // upd(a, i): layer 1 of the direction keeps I_0, perm[n] is never visited -- storage positions [0, n1) and n - 1,
        // the same sites as the sweep positions k_lambda_diagonal tests (layers are contiguous in both orders)
        const int32_t pos = down ? pos_down : pos_up;
        if (pos < (down ? n1_down : n1_up) || (int64_t)pos == n - 1) continue;
        const size_t row = (size_t)a * (size_t)n + (size_t)site;
        const int32_t u1 = up1[row], u2 = up2[row];
        const double W1 = w1[row], W2 = w2[row], R1 = r1[row], R2 = r2[row];
        const bool in1 = u1 >= 0 && (int64_t)u1 < n, in2 = u2 >= 0 && (int64_t)u2 < n;     // (a visited site has both)
        const int32_t *__restrict__ srank = down ? srank_down : srank_up;
        const size_t p1 = in1 ? (size_t)srank[u1] : (size_t)pos, p2 = in2 ? (size_t)srank[u2] : (size_t)pos;
        const double2 *__restrict__ al = alpha + (size_t)a * plane;
        double2 ac[kDiagPairs], a1[kDiagPairs], a2[kDiagPairs];
#pragma unroll
        for (int u = 0; u < kDiagPairs; u++) {
            ac[u] = al[base[u] + ((size_t)pos << lw[u])];
            a1[u] = al[base[u] + (p1 << lw[u])];
            a2[u] = al[base[u] + (p2 << lw[u])];
        }
        const double w = ang.w[a];
#pragma unroll
        for (int u = 0; u < kDiagPairs; u++) {
            double ca, cb, ce, t1x = 0.0, t2x = 0.0, t1y = 0.0, t2y = 0.0;
            if (in1) {
                linear_weights_ref_order(R1 * (ac[u].x + a1[u].x) / 2.0, ca, cb, ce);
                t1x = W1 * cb;
                linear_weights_ref_order(R1 * (ac[u].y + a1[u].y) / 2.0, ca, cb, ce);
                t1y = W1 * cb;
            }
            if (in2) {
                linear_weights_ref_order(R2 * (ac[u].x + a2[u].x) / 2.0, ca, cb, ce);
                t2x = W2 * cb;
                linear_weights_ref_order(R2 * (ac[u].y + a2[u].y) / 2.0, ca, cb, ce);
                t2y = W2 * cb;
            }
            acc[u].x += w * (t1x + t2x);
            acc[u].y += w * (t1y + t2y);
        }
    }
#pragma unroll
    for (int u = 0; u < kDiagPairs; u++) {
        const int q = q0 + u;
        if (q >= npair) break;
        const bool second = 2 * q + 1 < nlam;                        // (an odd count: the half pair's second wavelength is padding)
        if (PLANES) {
            reinterpret_cast<double2 *>(out)[(size_t)q * (size_t)n + (size_t)t] = make_double2(acc[u].x, second ? acc[u].y : 0.0);
        } else {
            double *row = out + (size_t)site * (size_t)ld + 2 * (size_t)q;
            row[0] = acc[u].x;
            if (second) row[1] = acc[u].y;
        }
    }
}

}  // namespace

int launch_line_lambda_diagonal(vrt_plan *p, int64_t nlam, const double *d_alpha_native, const double *weights, int64_t ld,
                                double *d_rows, double *d_up_planes, hipStream_t st)
{
    vrt_grid *g = p->g;
    if (p->A > kMaxAngles) return fail(VRT_EINVAL, "too many active angles");
    if (p->A != (int)p->n_angles_user) return fail(VRT_EINVAL, "per-angle alpha needs every angle active (no θ = 90 direction)");
    if (nlam > INT32_MAX - 1) return fail(VRT_EINVAL, "nlam too large");
    if (((uintptr_t)d_alpha_native | (uintptr_t)d_up_planes) & 15)
        return fail(VRT_EINVAL, "the native alpha and a sweep-order plane set must be 16-byte aligned");
    const int npair = (int)((nlam + 1) / 2);
    const int groups = (npair + kDiagPairs - 1) / kDiagPairs;
    if (groups > 65535) return fail(VRT_EINVAL, "nlam too large");
    const DiagAngles ang = diag_angles(p, weights);
    const dim3 grid((unsigned)std::max<int64_t>((g->n + 255) / 256, 1), (unsigned)groups);
#define VRT_LINE_DIAG(PLANES, out)                                                                                          \
    hipLaunchKernelGGL(k_line_lambda_diagonal<PLANES>, grid, dim3(256), 0, st, g->n, (int)nlam, npair, native_lg(p, false), ld, \
                       p->A, ang, (int32_t)g->up.n1, (int32_t)g->down.n1, g->up.d_store, g->up.d_srank, g->down.d_srank,    \
                       p->d_up1, p->d_up2, p->d_w1, p->d_w2, p->d_r1, p->d_r2,                                              \
                       reinterpret_cast<const double2 *>(d_alpha_native), out)
    if (d_up_planes) VRT_LINE_DIAG(true, d_up_planes);
    else VRT_LINE_DIAG(false, d_rows);
#undef VRT_LINE_DIAG
    VRT_HIP_TRY(hipGetLastError());
    return VRT_OK;
}

}  // namespace vrt

using namespace vrt;

extern "C" int vrt_line_lambda_diagonal_dev(vrt_plan *p, int64_t nlam, const double *d_alpha_native, const double *weights_host,
                                            int64_t ld, double *d_diag, void *stream)
{
    if (!p || !d_alpha_native || !weights_host || !d_diag) return fail(VRT_EINVAL, "NULL argument");
    if (nlam < 1 || ld < nlam) return fail(VRT_EINVAL, "need nlam >= 1 and ld >= nlam");
    return guarded([&] {
        std::lock_guard<std::mutex> lock(p->mu);
        int rc = use_device(p->g->device);
        if (rc) return rc;
        return launch_line_lambda_diagonal(p, nlam, d_alpha_native, weights_host, ld, d_diag, nullptr, (hipStream_t)stream);
    });
}
