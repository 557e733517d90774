// Internal: the regular-grid solver handle and the entry of its solve kernels (vrt_regular.hip), shared with the
// line Λ-iteration on the raster (vrt_regular_lambda.hip).  The S and J of a raster session stand behind RasterStore
// (vrt_raster_store.h), which includes this header for the layout launches below.
#pragma once

#include <vector>

#include "vrt_internal.h"

// ---- device-resident form: a handle owns the grid axes and the (grow-only) workspaces -----------
struct vrt_regular {
    int device = 0;
    int64_t nz = 0, nx = 0, ny = 0;
    vrt::DevBuf<double> d_g;               // z | x | y
    std::vector<double> h_g;               // the same on the host (launch geometry)
    vrt::DevWork<double> d_S, d_A, d_I, d_coef, d_xy;                      // capacities in doubles
    vrt::DevBuf<double> d_k;
    vrt::DevBuf<int> d_up;
    int64_t cap_k = 0;                     // of d_k and d_up, in solves
    vrt::Event ev[3];
    bool timed = false;
    int last_form = -1, last_threads = 0;  // what regular_launch chose last (vrt_regular_last_launch_form); -1: nothing yet
    int force_threads = 0;                 // VRT_REG_THREADS, read once at creation (tests: forces the launch shape)
    int xy_split = 1;                      // VRT_REG_XY (creation): 0 = all-xy batches through k_regular_solve too;
                                           //   2 = split, upwind plane read from memory instead of LDS (tests)
    vrt::DevWork<double> d_I0;             // vrt_regular_emergent_dev: the bottom planes of S of one chunk
    int64_t emergent_bytes = (int64_t)8 << 30;  // VRT_REG_EMERGENT_BYTES (creation): workspace cap of an emergent chunk
    int64_t lambda_bytes = (int64_t)64 << 30;   // VRT_REG_LAMBDA_BYTES (creation): workspace cap of a line-J chunk
                                                //   (smaller chunks run fewer solves at once: DESIGN §7f)
};

namespace vrt {

// |k| = 1 and k_z != 0 for every one of n_solve directions (host)
int regular_check_k(int64_t n_solve, const double *k);

// frees the solve workspaces (alpha, I, coefficients) a line pass grew; the next call that needs them allocates again
void regular_release_workspace(vrt_regular *r);

// n_solve solves whose inputs are already plane-major on the device (no transposes) into r->d_I ([solve][iz][iy][ix]):
// solve s is direction dk[s] (hk: the same directions on the host, which choose the launch), dup[s] (1 up, 0 down),
// wavelength l = (s + lam_offset) % lam_period of dS ([l][iz][iy][ix]) and, if up, of dI0 ([l][iy][ix]); a down solve
// starts from the plane dI0_zero.  dalpha holds one plane-major array per solve, or (alpha_per_lam: the continuum, whose
// alpha is the same for every angle) one per wavelength, read like dS.  Asynchronous on st.
int regular_solve_planes(vrt_regular *r, int64_t n_solve, const double *hk, const double *dk, const int *dup, const double *dS,
                         int64_t lam_period, int64_t lam_offset, const double *dalpha, const double *dI0,
                         const double *dI0_zero, int n_sweeps, hipStream_t st, bool alpha_per_lam = false);

// ---- pieces of the Λ-iteration on the raster (vrt_regular_lambda.hip) shared with the continuum session (vrt_continuum.hip)
// (n, nlam) wavelength-fastest in Julia point order <-> plane-major [l][iz][iy][ix]; B_0's bottom planes [l][iy][ix]
int launch_to_planes(const vrt_regular *r, int64_t nlam, const double *in, double *out, hipStream_t st);
int launch_from_planes(const vrt_regular *r, int64_t nlam, const double *in, double *out, hipStream_t st);
int launch_bottom_planes(const vrt_regular *r, int64_t nlam, const double *B0, double *out, hipStream_t st);
// the checks of a direction set, before the device is touched
int check_angles(int64_t n_angles, const double *k, const int *dirs);
// The (angle, wavelength) solves of a direction set: solve g = a nlam + l over the active angles
struct LineSolves {
    int64_t A = 0, nlam = 0, chunk = 1;
    std::vector<double> hk;             // 3 per solve, host (the launch choice of regular_solve_planes)
    DevBuf<double> d_ka, d_w, d_ks;     // 3 per active angle, 1 per active angle, 3 per solve
    DevBuf<int> d_up;                   // per solve: 1 up, 0 down
};
int line_solves_init(LineSolves &ls, const vrt_regular *r, int64_t n_angles, const double *k, const int *dirs,
                     const double *weights, int64_t nlam);
// J[l][p] += w_a I[g - g0][p] over the chunk's solves [g0, g0 + cnt) held in r->d_I, in quadrature order
int launch_reduce_J_planes(const vrt_regular *r, const LineSolves &ls, int64_t g0, int64_t cnt, double *dJ_pl, hipStream_t st);
// Λ* of accelerated Λ-iteration (k_regular_lambda_diagonal, vrt_regular.hip) from a plane-major α into a plane-major
// d_diag_pl, both [l][iz][iy][ix]; k, dirs, weights per USER angle on the host (dirs = 0 is skipped; more than kMaxAngles
// active ones: VRT_EINVAL)
int launch_regular_lambda_diagonal(const vrt_regular *r, int64_t n_angles, const double *k, const int *dirs,
                                   const double *weights, int64_t nlam, const double *d_alpha_pl, double *d_diag_pl,
                                   hipStream_t st);
// Λ* of the line Λ-iteration (k_regular_line_lambda_diagonal): d_diag_pl[l][p] += w_a c_a(p; α_a[l]) over the chunk's solves
// [g0, g0 + cnt), whose α stands in d_alpha_chunk as [g - g0][iz][iy][ix]; in quadrature order, bit-identical for any
// chunking.  The caller zeroes d_diag_pl before the first chunk.
int launch_regular_line_lambda_diagonal(const vrt_regular *r, const LineSolves &ls, int64_t g0, int64_t cnt,
                                        const double *d_alpha_chunk, double *d_diag_pl, hipStream_t st);

}  // namespace vrt
