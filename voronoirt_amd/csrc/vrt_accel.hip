// Ng acceleration of the Λ-iteration (Ng 1974, J. Chem. Phys. 61, 2680; Olson, Auer & Buchler 1986, JQSRT 35, 431), second
// order: from the last four iterates x0 (newest) .. x3 of the source function, extrapolate along the two slowest error modes.
// Per element, in exactly this order of operations (the build is -ffp-contract=off):
//   w  = 1 / x0
//   q1 = (x0 - 2 x1) + x2          q2 = ((x0 - x1) - x2) + x3          q3 = x0 - x1
//   A1 = Σ (w q1) q1   B1 = Σ (w q1) q2   C1 = Σ (w q1) q3   B2 = Σ (w q2) q2   C2 = Σ (w q2) q3
// On the host, in double:
//   det = A1 B2 - B1 B1    a = (C1 B2 - C2 B1) / det    b = (C2 A1 - C1 B1) / det    c = (1 - a) - b
//   x_acc = (c x0 + a x1) + b x2
// Two streaming kernels (k_ng_sums: 4 loads, no store; k_ng_apply: 3 loads, 1 store) and a one-workgroup reduction of the
// per-workgroup partial sums.  No floating-point atomics: for a given element count the launch shape, the assignment of
// elements to accumulators and the order of every addition are fixed, so the five sums are the same bits run after run.
//
// The sums, the coefficients and the apply are separate steps (ng_sums, ng_coefficients, ng_apply; public as vrt_ng_sums_dev,
// vrt_ng_coefficients, vrt_ng_apply_dev): vrt_ng_accelerate_dev and ng_after_iterate run the three on one array; a caller
// that holds S in several arrays runs the first and the last per array and adds the partial sums in one fixed order
// (vrt_multi_lambda_iterate does, one array per member, over the phases of vrt_internal.h).
//
// Element ranges (NgRange): `dense` contiguous doubles (an even count, read as double2), then `tail` doubles `tstride` apart.
// A caller-layout array is (count & ~1, count & 1, 1); a sweep-order plane set with an odd wavelength count is every full
// pair plane dense, then the first halves of the last plane's pairs (stride 2) -- the padding wavelength is never touched.
#include <cfloat>
#include <cmath>
#include <cstring>

#include "vrt_internal.h"

namespace vrt {
namespace {

constexpr int kNgThreads = 256;
constexpr int kNgMaxGroups = 2048;          // 8 workgroups per CU of an MI355X; the partial-sum slots of the workspace
constexpr int kNgUnroll = 4;                // double2 per lane and array in flight, one accumulator set each
constexpr size_t kNgWorkspace = 5 * (size_t)kNgMaxGroups + 8;       // partials | 5 sums | verdict word (in a double's slot)

// workgroups for `pairs` double2 and `tail` single elements: a function of the counts alone (run-to-run determinism)
inline int ng_groups(int64_t pairs, int64_t tail)
{
    const int64_t per = (int64_t)kNgThreads * kNgUnroll;
    const int64_t g = std::max((pairs + per - 1) / per, (tail + per - 1) / per);
    return (int)std::max<int64_t>(1, std::min<int64_t>(g, kNgMaxGroups));
}

template <bool VEC>
__device__ inline double2 ng_load2(const double *__restrict__ x, int64_t j)
{
    if (VEC) return reinterpret_cast<const double2 *>(x)[j];          // global_load_dwordx4
    return make_double2(x[2 * j], x[2 * j + 1]);
}

struct NgAcc {
    double A1 = 0.0, B1 = 0.0, C1 = 0.0, B2 = 0.0, C2 = 0.0;
};

// the five terms of one element; the two elements of a double2 are added first, then into the accumulator
__device__ inline void ng_terms(double x0, double x1, double x2, double x3, double t[5])
{
    const double w = 1.0 / x0;
    const double q1 = (x0 - 2.0 * x1) + x2;
    const double q2 = ((x0 - x1) - x2) + x3;
    const double q3 = x0 - x1;
    const double wq1 = w * q1, wq2 = w * q2;
    t[0] = wq1 * q1; t[1] = wq1 * q2; t[2] = wq1 * q3; t[3] = wq2 * q2; t[4] = wq2 * q3;
}

__device__ inline void ng_add2(NgAcc &s, const double2 &x0, const double2 &x1, const double2 &x2, const double2 &x3)
{
    double tx[5], ty[5];
    ng_terms(x0.x, x1.x, x2.x, x3.x, tx);
    ng_terms(x0.y, x1.y, x2.y, x3.y, ty);
    s.A1 += tx[0] + ty[0]; s.B1 += tx[1] + ty[1]; s.C1 += tx[2] + ty[2]; s.B2 += tx[3] + ty[3]; s.C2 += tx[4] + ty[4];
}

// LONGEST CHAIN OF ADDITIONS (the L of the tests' bound 2^-40 Σ|t| = L 2^-53 Σ|t|, L <= 8192).  At the largest array a
// session can hold (4 M sites x 100 wavelengths = 2 x 10^8 double2) and 2048 x 256 lanes each accumulator takes every
// 2048 * 256 * 4-th double2: ceil(2e8 / 2 097 152) = 96 additions of a pair sum that is 1 addition itself; then 2 to fold
// the four accumulators, 6 in the wave, 2 across the four waves, 7 + 6 + 2 in the final reduction of 2048 partials: L = 122.
// The tail of an odd wavelength count adds at most ceil(4e6 / 524 288) = 8 to one accumulator.
template <bool VEC>
__global__ void __launch_bounds__(kNgThreads)
k_ng_sums(int64_t pairs, int64_t tail, int64_t tstride, const double *__restrict__ x0, const double *__restrict__ x1,
          const double *__restrict__ x2, const double *__restrict__ x3, double *__restrict__ partial /* [5][gridDim.x] */)
{
    __shared__ double wsum[5][kNgThreads / 64];
    NgAcc acc[kNgUnroll];
    const int64_t lanes = (int64_t)gridDim.x * kNgThreads;
    const int64_t lane = (int64_t)blockIdx.x * kNgThreads + threadIdx.x;
    // every trip loads kNgUnroll independent double2 of each array (16 x 16 bytes in flight per lane) before it computes
    for (int64_t j0 = lane; j0 < pairs; j0 += lanes * kNgUnroll) {
        double2 v0[kNgUnroll], v1[kNgUnroll], v2[kNgUnroll], v3[kNgUnroll];
#pragma unroll
        for (int u = 0; u < kNgUnroll; u++) {
            const int64_t j = j0 + (int64_t)u * lanes;
            if (j < pairs) {
                v0[u] = ng_load2<VEC>(x0, j); v1[u] = ng_load2<VEC>(x1, j);
                v2[u] = ng_load2<VEC>(x2, j); v3[u] = ng_load2<VEC>(x3, j);
            }
        }
#pragma unroll
        for (int u = 0; u < kNgUnroll; u++)
            if (j0 + (int64_t)u * lanes < pairs) ng_add2(acc[u], v0[u], v1[u], v2[u], v3[u]);
    }
    const double *t0 = x0 + 2 * pairs, *t1 = x1 + 2 * pairs, *t2 = x2 + 2 * pairs, *t3 = x3 + 2 * pairs;
    for (int64_t i = lane; i < tail; i += lanes) {
        const int64_t o = i * tstride;
        double t[5];
        ng_terms(t0[o], t1[o], t2[o], t3[o], t);
        acc[0].A1 += t[0]; acc[0].B1 += t[1]; acc[0].C1 += t[2]; acc[0].B2 += t[3]; acc[0].C2 += t[4];
    }
    double s[5];
    s[0] = (acc[0].A1 + acc[1].A1) + (acc[2].A1 + acc[3].A1);
    s[1] = (acc[0].B1 + acc[1].B1) + (acc[2].B1 + acc[3].B1);
    s[2] = (acc[0].C1 + acc[1].C1) + (acc[2].C1 + acc[3].C1);
    s[3] = (acc[0].B2 + acc[1].B2) + (acc[2].B2 + acc[3].B2);
    s[4] = (acc[0].C2 + acc[1].C2) + (acc[2].C2 + acc[3].C2);
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 5; k++) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s[k] += __shfl_down(s[k], off, 64);
        if ((threadIdx.x & 63) == 0) wsum[k][wave] = s[k];
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        const int k = threadIdx.x;
        partial[(size_t)k * gridDim.x + blockIdx.x] = (wsum[k][0] + wsum[k][1]) + (wsum[k][2] + wsum[k][3]);
    }
}

// one workgroup: lane t adds the partials t, t + 256, ... in that order, then the wave and the four waves as above
__global__ void __launch_bounds__(kNgThreads)
k_ng_final(int groups, const double *__restrict__ partial, double *__restrict__ sums)
{
    __shared__ double wsum[5][kNgThreads / 64];
    const int wave = threadIdx.x >> 6;
    for (int k = 0; k < 5; k++) {
        double s = 0.0;
        for (int g = threadIdx.x; g < groups; g += kNgThreads) s += partial[(size_t)k * groups + g];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
        if ((threadIdx.x & 63) == 0) wsum[k][wave] = s;
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        const int k = threadIdx.x;
        sums[k] = (wsum[k][0] + wsum[k][1]) + (wsum[k][2] + wsum[k][3]);
    }
}

__device__ inline double ng_value(double a, double b, double c, double x0, double x1, double x2, bool &bad)
{
    const double v = (c * x0 + a * x1) + b * x2;
    if (!(v > 0.0) || !(v <= DBL_MAX)) bad = true;           // NaN, <= 0 or Inf: a source function stays finite and positive
    return v;
}

template <bool VEC>
__global__ void __launch_bounds__(kNgThreads)
k_ng_apply(int64_t pairs, int64_t tail, int64_t tstride, double a, double b, double c, const double *__restrict__ x0,
           const double *__restrict__ x1, const double *__restrict__ x2, double *__restrict__ out,
           unsigned *__restrict__ verdict)
{
    bool bad = false;
    const int64_t lanes = (int64_t)gridDim.x * kNgThreads;
    const int64_t lane = (int64_t)blockIdx.x * kNgThreads + threadIdx.x;
    for (int64_t j0 = lane; j0 < pairs; j0 += lanes * kNgUnroll) {
        double2 v0[kNgUnroll], v1[kNgUnroll], v2[kNgUnroll];
#pragma unroll
        for (int u = 0; u < kNgUnroll; u++) {
            const int64_t j = j0 + (int64_t)u * lanes;
            if (j < pairs) { v0[u] = ng_load2<VEC>(x0, j); v1[u] = ng_load2<VEC>(x1, j); v2[u] = ng_load2<VEC>(x2, j); }
        }
#pragma unroll
        for (int u = 0; u < kNgUnroll; u++) {
            const int64_t j = j0 + (int64_t)u * lanes;
            if (j >= pairs) break;
            double2 r;
            r.x = ng_value(a, b, c, v0[u].x, v1[u].x, v2[u].x, bad);
            r.y = ng_value(a, b, c, v0[u].y, v1[u].y, v2[u].y, bad);
            if (VEC) reinterpret_cast<double2 *>(out)[j] = r;
            else { out[2 * j] = r.x; out[2 * j + 1] = r.y; }
        }
    }
    const int64_t base = 2 * pairs;
    for (int64_t i = lane; i < tail; i += lanes) {
        const int64_t o = base + i * tstride;
        out[o] = ng_value(a, b, c, x0[o], x1[o], x2[o], bad);
    }
    if (__syncthreads_or(bad) && threadIdx.x == 0) *verdict = 1u;       // (every writer stores the same word)
}

// the down-order copy of a sweep-order plane set from its up-order copy: the same values, so the two stay permutations
// of each other bit for bit (the layout of k_lambda_update_native)
__global__ void __launch_bounds__(256)
k_ng_mirror(int64_t n, int npair, const int32_t *__restrict__ store_up, const int32_t *__restrict__ rank_down,
            const double2 *__restrict__ Su, double2 *__restrict__ Sd)
{
    for (int64_t pos = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; pos < n; pos += (int64_t)gridDim.x * blockDim.x) {
        const size_t pd = (size_t)rank_down[store_up[pos]];
        for (int q = 0; q < npair; q++) Sd[(size_t)q * (size_t)n + pd] = Su[(size_t)q * (size_t)n + (size_t)pos];
    }
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

bool ng_coefficients(const double sums[5], double coeffs[2])
{
    const double A1 = sums[0], B1 = sums[1], C1 = sums[2], B2 = sums[3], C2 = sums[4];
    const double det = A1 * B2 - B1 * B1;
    coeffs[0] = (C1 * B2 - C2 * B1) / det;
    coeffs[1] = (C2 * A1 - C1 * B1) / det;
    for (int k = 0; k < 5; k++)
        if (!std::isfinite(sums[k])) return false;
    return std::isfinite(det) && det != 0.0;
}

int ng_sums(const NgRange &rg, const double *x0, const double *x1, const double *x2, const double *x3, double *d_ws,
            double sums[5], hipStream_t st)
{
    const int64_t pairs = rg.dense / 2;
    const int groups = ng_groups(pairs, rg.tail);
    const bool vec = aligned16(x0) && aligned16(x1) && aligned16(x2) && aligned16(x3);
    double *d_sums = d_ws + 5 * (size_t)kNgMaxGroups;
    if (vec)
        hipLaunchKernelGGL(k_ng_sums<true>, dim3((unsigned)groups), dim3(kNgThreads), 0, st, pairs, rg.tail, rg.tstride, x0, x1, x2,
                           x3, d_ws);
    else
        hipLaunchKernelGGL(k_ng_sums<false>, dim3((unsigned)groups), dim3(kNgThreads), 0, st, pairs, rg.tail, rg.tstride, x0, x1, x2,
                           x3, d_ws);
    VRT_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_ng_final, dim3(1), dim3(kNgThreads), 0, st, groups, (const double *)d_ws, d_sums);
    VRT_HIP_TRY(hipGetLastError());
    VRT_HIP_TRY(hipMemcpyAsync(sums, d_sums, 5 * sizeof(double), hipMemcpyDeviceToHost, st));
    VRT_HIP_TRY(hipStreamSynchronize(st));
    return VRT_OK;
}

int ng_apply(const NgRange &rg, double a, double b, const double *x0, const double *x1, const double *x2, double *out,
             double *d_ws, bool *ok, hipStream_t st)
{
    const int64_t pairs = rg.dense / 2;
    const int groups = ng_groups(pairs, rg.tail);
    const bool vec = aligned16(x0) && aligned16(x1) && aligned16(x2) && aligned16(out);
    unsigned *d_verdict = reinterpret_cast<unsigned *>(d_ws + 5 * (size_t)kNgMaxGroups + 5);
    const double c = (1.0 - a) - b;
    VRT_HIP_TRY(hipMemsetAsync(d_verdict, 0, sizeof(unsigned), st));
    if (vec)
        hipLaunchKernelGGL(k_ng_apply<true>, dim3((unsigned)groups), dim3(kNgThreads), 0, st, pairs, rg.tail, rg.tstride, a, b, c,
                           x0, x1, x2, out, d_verdict);
    else
        hipLaunchKernelGGL(k_ng_apply<false>, dim3((unsigned)groups), dim3(kNgThreads), 0, st, pairs, rg.tail, rg.tstride, a, b, c,
                           x0, x1, x2, out, d_verdict);
    VRT_HIP_TRY(hipGetLastError());
    unsigned bad = 1;
    VRT_HIP_TRY(hipMemcpyAsync(&bad, d_verdict, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    VRT_HIP_TRY(hipStreamSynchronize(st));
    *ok = bad == 0;
    return VRT_OK;
}

int launch_ng_mirror(vrt_grid *g, int64_t nlam, const double *dS_up, double *dS_down, hipStream_t st)
{
    const int npair = (int)((nlam + 1) / 2);
    const int64_t blocks = std::min<int64_t>((g->n + 255) / 256, 256 * 16);
    hipLaunchKernelGGL(k_ng_mirror, dim3((unsigned)std::max<int64_t>(blocks, 1)), dim3(256), 0, st, g->n, npair, g->up.d_store,
                       g->down.d_srank, reinterpret_cast<const double2 *>(dS_up), reinterpret_cast<double2 *>(dS_down));
    VRT_HIP_TRY(hipGetLastError());
    return VRT_OK;
}

// ---- the sessions' side: schedule, history, the step ----------------------------------------------------------------
int ng_check_settings(int order, int start, int period)
{
    if (order != 0 && order != 2) return fail(VRT_EINVAL, "acceleration order must be 0 (off) or 2");
    if (order == 2 && (start < 4 || period < 4)) return fail(VRT_EINVAL, "acceleration needs start >= 4 and period >= 4");
    return VRT_OK;
}

void ng_release(NgState &ng)
{
    for (DevBuf<double> &h : ng.hist) h.reset();
    ng.d_ws.reset();
    ng.have = 0;
}

int ng_configure(NgState &ng, int order, int start, int period, size_t alloc_count)
{
    ng.last_applied = 0;
    ng.have = 0;
    if (order == 0) {
        ng.order = ng.start = ng.period = 0;
        ng_release(ng);
        return VRT_OK;
    }
    int rc;
    for (DevBuf<double> &h : ng.hist)
        if (!h && (rc = h.alloc(alloc_count))) { ng_release(ng); ng.order = 0; return rc; }
    if (!ng.d_ws && (rc = ng.d_ws.alloc(kNgWorkspace))) { ng_release(ng); ng.order = 0; return rc; }
    ng.order = order; ng.start = start; ng.period = period;
    return VRT_OK;
}

// After the plain update of iterate number `iterate` (1-based), for a session that holds S in ONE array: the phases of
// vrt_internal.h in turn.  A recording iterate keeps S as x_d; a due one with the three before it kept takes the step, x_acc
// written over x3's buffer, which then BECOMES the session's S (a rejected step leaves S untouched).
int ng_after_iterate(NgState &ng, int64_t iterate, DevBuf<double> &S, size_t alloc_count, const NgRange &rg, hipStream_t st)
{
    ng.last_applied = 0;
    const int due = ng_due(ng, iterate);
    if (due == kNgNothing) return VRT_OK;
    if (due != kNgStep) return ng_record(ng, due, S, alloc_count, st);
    if (!ng_take_history(ng)) return VRT_OK;    // switched on too late for this one: nothing due
    int rc;
    if ((rc = ng_sums(rg, S, ng.hist[0], ng.hist[1], ng.hist[2], ng.d_ws, ng.last_sums, st))) return rc;
    ng.last_applied = -1;
    const bool valid = ng_coefficients(ng.last_sums, ng.last_coeffs);
    NgPiece piece{&ng, &S, false};
    if (valid && (rc = ng_apply(rg, ng.last_coeffs[0], ng.last_coeffs[1], S, ng.hist[0], ng.hist[1], ng.hist[2], ng.d_ws, &piece.good, st)))
        return rc;
    if (ng_commit(&piece, 1, valid)) ng.last_applied = 1;
    return VRT_OK;
}

int ng_report(const NgState &ng, int *applied, double sums[5], double coeffs[2])
{
    *applied = ng.last_applied;
    if (ng.last_applied) {
        if (sums) std::memcpy(sums, ng.last_sums, sizeof(ng.last_sums));
        if (coeffs) std::memcpy(coeffs, ng.last_coeffs, sizeof(ng.last_coeffs));
    }
    return VRT_OK;
}

}  // namespace vrt

using namespace vrt;

// (a caller-layout array of `count` doubles: ng_S_range(count, 1, false))
extern "C" int vrt_ng_sums_dev(int64_t count, const double *d_x0, const double *d_x1, const double *d_x2, const double *d_x3,
                               double sums[5], void *stream)
{
    if (!d_x0 || !d_x1 || !d_x2 || !d_x3 || !sums) return fail(VRT_EINVAL, "NULL argument");
    if (count < 1) return fail(VRT_EINVAL, "count must be >= 1");
    return guarded([&] {
        int rc = use_current_device();
        if (rc) return rc;
        DevBuf<double> ws;
        if ((rc = ws.alloc(kNgWorkspace))) return rc;
        return ng_sums(ng_S_range(count, 1, false), d_x0, d_x1, d_x2, d_x3, ws, sums, (hipStream_t)stream);
    });
}

extern "C" int vrt_ng_coefficients(const double sums[5], double coeffs[2])
{
    if (!sums || !coeffs) return fail(VRT_EINVAL, "NULL argument");
    double ab[2];
    if (!ng_coefficients(sums, ab)) return 0;
    coeffs[0] = ab[0]; coeffs[1] = ab[1];
    return 1;
}

extern "C" int vrt_ng_apply_dev(int64_t count, double a, double b, const double *d_x0, const double *d_x1, const double *d_x2,
                                double *d_out, int *good, void *stream)
{
    if (!d_x0 || !d_x1 || !d_x2 || !d_out || !good) return fail(VRT_EINVAL, "NULL argument");
    if (count < 1) return fail(VRT_EINVAL, "count must be >= 1");
    return guarded([&] {
        int rc = use_current_device();
        if (rc) return rc;
        DevBuf<double> ws;
        if ((rc = ws.alloc(kNgWorkspace))) return rc;
        bool ok = false;
        *good = 0;
        if ((rc = ng_apply(ng_S_range(count, 1, false), a, b, d_x0, d_x1, d_x2, d_out, ws, &ok, (hipStream_t)stream))) return rc;
        *good = ok ? 1 : 0;
        return VRT_OK;
    });
}

// the three pieces above in one call, on one workspace
extern "C" int vrt_ng_accelerate_dev(int64_t count, const double *d_x0, const double *d_x1, const double *d_x2,
                                     const double *d_x3, double *d_out, double sums[5], double coeffs[2], int *applied,
                                     void *stream)
{
    if (!d_x0 || !d_x1 || !d_x2 || !d_x3 || !d_out || !sums || !coeffs || !applied) return fail(VRT_EINVAL, "NULL argument");
    if (count < 1) return fail(VRT_EINVAL, "count must be >= 1");
    return guarded([&] {
        int rc = use_current_device();
        if (rc) return rc;
        hipStream_t st = (hipStream_t)stream;
        DevBuf<double> ws;
        if ((rc = ws.alloc(kNgWorkspace))) return rc;
        const NgRange rg = ng_S_range(count, 1, false);
        *applied = 0;
        if ((rc = ng_sums(rg, d_x0, d_x1, d_x2, d_x3, ws, sums, st))) return rc;
        if (!ng_coefficients(sums, coeffs)) return VRT_OK;
        bool ok = false;
        if ((rc = ng_apply(rg, coeffs[0], coeffs[1], d_x0, d_x1, d_x2, d_out, ws, &ok, st))) return rc;
        *applied = ok ? 1 : 0;
        return VRT_OK;
    });
}
