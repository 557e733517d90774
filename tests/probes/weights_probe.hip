// Test infrastructure only (tests/test_weights_domain.py): calls every function of voronoirt_amd/csrc/vrt_weights.h
// directly, one element per thread, so that a test can judge each copy of linear_weights, each exponential and the
// wave-uniform branch dispatch per value.  Built by voronoirt_amd/build.py:build_probe() into
// voronoirt_amd/libvrt_weights_probe.so with the product's own flags; the product library neither links nor names it.
// All pointers are device pointers; every call runs on the null stream and returns after the kernel has finished
// (0, or the hipError_t).  Element i is thread i % 256 of block i / 256: lane i % 64 of wave i / 64.
#include <hip/hip_runtime.h>

#include "vrt_weights.h"

using namespace vrt;

namespace {

constexpr int kBlock = 256;

__global__ void __launch_bounds__(kBlock) k_probe_exp(int which, long long n, const double *x, double *out)
{
    exp2_table_fill();                                   // as every kernel that evaluates exp_neg_tab does
    __syncthreads();
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    out[i] = which == 0 ? exp_neg(x[i]) : exp_neg_tab(x[i]);
}

__global__ void __launch_bounds__(kBlock) k_probe_weights(int which, long long n, const double *dtau, double *a, double *b, double *e)
{
    exp2_table_fill();
    __syncthreads();
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const double d = dtau[i];
    double ca, cb, ce;
    switch (which) {                                     // uniform over the launch
    case 0: linear_weights_ref_order(d, ca, cb, ce); break;
    case 1: lin_weights(d, ca, cb, ce); break;
    case 2: lin_weights_fma<0>(d, ca, cb, ce); break;
    case 3: lin_weights_fma<1>(d, ca, cb, ce); break;
    default: lin_weights_fma<2>(d, ca, cb, ce); break;
    }
    a[i] = ca; b[i] = cb; e[i] = ce;
}

// in[11][n] = d1, d2, w1, w2, in1, in2 (0.0 / 1.0), S_c, S_1, S_2, I_1, I_2; out[3][n] = c, g1, g2.  The dispatchers ballot over the
// wave, so a wave's lanes all take part: threads past n leave only after the barrier and belong to no wave that holds an element
// when n is a multiple of 64 (the caller pads).
__global__ void __launch_bounds__(kBlock) k_probe_entry(int which, long long n, const double *in, double *out)
{
    __shared__ double s_w1[kBlock], s_w2[kBlock];        // the kernels read the weights from per-thread LDS slots
    exp2_table_fill();
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    const int tid = threadIdx.x;
    if (i < n) { s_w1[tid] = in[2 * n + i]; s_w2[tid] = in[3 * n + i]; }
    __syncthreads();
    if (i >= n) return;
    const double d1 = in[0 * n + i], d2 = in[1 * n + i];
    const bool in1 = in[4 * n + i] != 0.0, in2 = in[5 * n + i] != 0.0;
    const double S_c = in[6 * n + i], S_1 = in[7 * n + i], S_2 = in[8 * n + i], I_1 = in[9 * n + i], I_2 = in[10 * n + i];
    double c, g1, g2, sink = 0.0;
    if (which == 0) {
        // entry_lambda forms Δτ = rh (α_c + α_u) itself: rh = Δτ, α_c = 1, α_u = 0 hands it Δτ unchanged
        const double w1 = s_w1[tid], w2 = s_w2[tid];
        entry_lambda(d1, d2, w1, w2, in1 ? w1 : 0.0, in2 ? w2 : 0.0, 1.0, 0.0, 0.0, S_c, S_1, S_2, I_1, I_2, c, g1, g2);
    } else if (which == 1) {
        entry_lambda_seq(d1, d2, s_w1 + tid, s_w2 + tid, in1, in2, S_c, S_1, S_2, I_1, I_2, c, g1, g2, sink);
    } else {
        LateTerms L;
        late_lambda(d1, d2, S_1, S_2, L, sink);
        late_apply(L, s_w1 + tid, s_w2 + tid, in1, in2, S_c, I_1, I_2, c, g1, g2);
    }
    out[i] = c; out[n + i] = g1; out[2 * n + i] = g2;
}

int finish()
{
    hipError_t err = hipGetLastError();
    if (err == hipSuccess) err = hipDeviceSynchronize();
    return (int)err;
}

unsigned blocks(long long n) { return (unsigned)((n + kBlock - 1) / kBlock); }

}  // namespace

extern "C" {

// which: 0 exp_neg (5e-4 <= x <= 50), 1 exp_neg_tab (0 <= x <= 745)
int probe_exp(int which, long long n, const double *x, double *out)
{
    if (n <= 0 || which < 0 || which > 1) return -1;
    hipLaunchKernelGGL(k_probe_exp, dim3(blocks(n)), dim3(kBlock), 0, 0, which, n, x, out);
    return finish();
}

// which: 0 linear_weights_ref_order, 1 lin_weights, 2 / 3 / 4 lin_weights_fma<0> / <1> / <2>
int probe_weights(int which, long long n, const double *dtau, double *a, double *b, double *e)
{
    if (n <= 0 || which < 0 || which > 4) return -1;
    hipLaunchKernelGGL(k_probe_weights, dim3(blocks(n)), dim3(kBlock), 0, 0, which, n, dtau, a, b, e);
    return finish();
}

// which: 0 entry_lambda, 1 entry_lambda_seq, 2 late_lambda + late_apply; in[11][n], out[3][n] (see k_probe_entry);
// n a multiple of 64
int probe_entry(int which, long long n, const double *in, double *out)
{
    if (n <= 0 || n % 64 != 0 || which < 0 || which > 2) return -1;
    hipLaunchKernelGGL(k_probe_entry, dim3(blocks(n)), dim3(kBlock), 0, 0, which, n, in, out);
    return finish();
}

}  // extern "C"
