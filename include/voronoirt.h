/*
 * voronoirt.h -- C ABI of libvrt_hip.so, the MI355X (gfx950) formal solver that drops in behind
 * VoronoiRT's Julia driver surface.
 *
 * The reference (meudnaes/VoronoiRT) has no FFI of its own: the boundary is the pair of Julia
 * methods `Delaunay_upII` / `Delaunay_downII` (src/irregular_ray_tracing.jl:15-82, :96-163),
 * their caller `J_λ_voronoi` (src/lambda_iteration.jl:60-113, src/lambda_continuum.jl:27-56) and
 * the grid constructor `read_cell` (src/voronoi_utils.jl:36-85).  A maintainer redefines those
 * methods to `ccall` the entry points below (INTEGRATION.md shows the Julia shim).
 *
 * Conventions (identical to the reference's Julia arrays, so Julia buffers pass unconverted):
 *   - all arrays column-major as Julia stores them, ids 1-based, int64 (`Int`), float64
 *   - positions  (3, n): pos[3*i + c], c = 0:z 1:x 2:y                 voronoi_utils.jl:8
 *   - neighbours (n, D1): nbr[i + n*j], column 0 = count, columns 1.. = ids; ids <= 0 are walls
 *     (-5 = z_min / bottom, -6 = z_max / top)                          voronoi_utils.jl:9,60-61,97,141
 *   - S, alpha, J (nlam, n): x[l + ld*i], wavelength fastest, ld >= nlam   lambda_iteration.jl:60-70
 *   - bounds[6] = z_min, z_max, x_min, x_max, y_min, y_max              io.jl:122-124
 * Every function returns 0 on success and a negative VRT_E* code on failure; it never throws
 * or aborts across the boundary.  vrt_last_error() returns a thread-local message.
 * Host entry points take host pointers and copy through PCIe; *_dev entry points take device
 * pointers (hipMalloc'ed or torch tensors) and a hipStream_t passed as void*.
 * There is NO CPU fallback: without a usable HIP device every compute call fails with
 * VRT_ENODEVICE.
 */
#ifndef VORONOIRT_H
#define VORONOIRT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VRT_OK 0
#define VRT_EINVAL (-1)     /* bad argument (null pointer, size mismatch, |k| != 1, ...)      */
#define VRT_EGRID (-2)      /* malformed grid: id out of range, unreachable site, D >= cap ... */
#define VRT_ENODEVICE (-3)  /* no HIP device / HIP runtime error                               */
#define VRT_ENOMEM (-4)     /* out of host or device memory, from every entry point            */
#define VRT_EIO (-5)        /* neighbour file unreadable / unparsable                          */

typedef struct vrt_grid vrt_grid;   /* replaces struct VoronoiSites, voronoi_utils.jl:7-28 */
typedef struct vrt_plan vrt_plan;   /* per-(grid, angle set) upwind tables + sweep schedule  */

/* alpha layouts accepted by the batched entry points */
#define VRT_ALPHA_SITE 0        /* alpha[n]                 same for every wavelength and angle  */
#define VRT_ALPHA_SITE_LAM 1    /* alpha[n][ld]             same for every angle (continuum)      */
#define VRT_ALPHA_ANGLE_SITE_LAM 2 /* alpha[n_angles][n][ld] per angle (line: lambda_iteration.jl:89-96) */
/* per angle, already in the library's NATIVE layout (device entry points only): for every angle a
 * block of vrt_plan_native_alpha_count / n_angles doubles holding wavelength PAIRS (an odd nlam is
 * padded with one finite wavelength), B = vrt_plan_native_pair_block(p) pairs of a site side by
 * side: the pairs form blocks of B, then (B not dividing the pair count) one block per set bit of
 * the remainder, widest first; pair q of a block [q0, q0 + w) at storage position pos is pair
 * element q0 * n + pos * w + (q - q0), each element two values (wavelengths 2q, 2q + 1); pos = the
 * site's position in the storage order of the angle's direction (vrt_grid_get_storage_order).
 * B = 1: element (l, pos) at ((l/2) * n + pos) * 2 + l%2.  Written by vrt_plan_alpha_to_native_dev
 * or vrt_line_opacity_dev -- callers need not know the layout; it saves the 2 x 8 B per (site,
 * angle, wavelength) of the layout change on every execute. */
#define VRT_ALPHA_ANGLE_NATIVE 3
/* alpha per (site, wavelength), the same for every angle (VRT_ALPHA_SITE_LAM: the continuum of
 * src/lambda_continuum.jl:27-56, where it does not change from one Λ-iteration to the next), handed over in SWEEP ORDER:
 * two plane sets of vrt_plan_native_plane_count(p, nlam) doubles one behind the other -- the up directions' order, then
 * the down directions' -- as vrt_plan_to_native_dev(p, nlam, ld, alpha, buf, buf + count, ...) writes them, once.
 * Accepted by vrt_plan_execute_native_dev[_f32] only (floats and vrt_plan_to_native_dev_f32 with the float entry): no layout
 * change of any kind is then left inside a step. */
#define VRT_ALPHA_SITE_LAM_NATIVE 4

const char *vrt_last_error(void);
int vrt_version(void);
/* number of visible HIP devices (0 if none); never fails */
int vrt_device_count(void);

/* ---- grid: replaces read_cell, src/voronoi_utils.jl:36-85 ---------------------------------
 * Builds BFS layers from the bottom (-5) and top (-6) walls (:93-174), the stable sort
 * permutations (:72,77), the reduced layer offsets with the reference's r[end] = n quirk
 * (:253-269), CSR-packs the neighbour lists, uploads, and computes the Delaunay lines (:186-245)
 * on the device.  `device` is the HIP device ordinal; device < 0 builds a HOST-ONLY handle (layers,
 * permutations, schedule introspection) on which every compute entry point fails with
 * VRT_ENODEVICE. */
int vrt_grid_create(int64_t n, const double *pos_zxy, const int64_t *nbr, int64_t D1,
                    const double bounds[6], int device, vrt_grid **out);
/* same, parsing the voro++ "%i %n" neighbour file (rt_preprocessing/output_sites.cc:49) the way
 * read_cell does (voronoi_utils.jl:42-70; max_guess = 70) */
int vrt_grid_create_from_file(const char *neighbours_file, int64_t n, const double *pos_zxy,
                              const double bounds[6], int device, vrt_grid **out);
void vrt_grid_destroy(vrt_grid *g);

/* ---- in-process tessellation: replaces the fork/exec of the voro++ wrapper
 * rt_preprocessing/output_sites.cc:35-49 (`voro`, src/functions.jl:13-23), the text round trip
 * (src/io.jl:8-40) and its parse (src/voronoi_utils.jl:42-63).  Voronoi cells of the sites in the
 * box, periodic in x and y, walls at z_min (-5) and z_max (-6); host code, multi-threaded, no GPU.
 *   nbr (n, D1) column-major out: exactly the matrix read_cell builds (column 0 = count, then the
 *   neighbour ids, 1-based); D1 = max_guess + 1 = 71 mirrors voronoi_utils.jl:42; *max_count
 *   receives maximum(nbr[:,1]).
 * The neighbour SET of every cell is the tessellation's; their ORDER inside a row (walls first,
 * then by increasing distance) is not voro++'s, which cannot be known without voro++ -- and the
 * reference's upwind rule depends on it (voronoi_utils.jl:378-386). */
int vrt_tessellate(int64_t n, const double *pos_zxy, const double bounds[6], int64_t D1, int64_t *nbr,
                   int64_t *max_count);
/* writes such a matrix as the voro++ "%i %n" text file read_cell parses (one line per cell) */
int vrt_write_neighbours_file(const char *path, int64_t n, const int64_t *nbr, int64_t D1);

/* ---- the same tessellation on the device (csrc/vrt_tessellate.hip): bounds check, search grid, one cell per wave and
 * the rows are built on `device`; vrt_tessellate's matrix for sites in general position, element for element.
 * THE ROW, exactly (both the host and the device entries): the walls first, -5 before -6; then the neighbours in
 * ascending (s, d2, j) of the periodic image of site j that made the surviving face -- s the Chebyshev distance, in
 * cells of the search grid, between the image's grid cell and the site's (the shell vrt_tessellate found it in),
 * d2 = dx*dx + dy*dy + dz*dz of (x_j + shift_x - x_i, y_j + shift_y - y_i, z_j - z_i), j the site id.  Left out: the
 * faces of the periodic start box, the site's own images, faces of area <= 1e-14 Lx Ly, and a second image of a
 * neighbour already listed.  Column 0 holds the count, the entries beyond it are zero.
 *   A cell that does not fit the kernel's fixed capacities (64 planes, 128 vertices at a time), or whose vertex list
 *   stops being a closed surface (exactly degenerate input: lattices), is recomputed by vrt_tessellate's host code, that
 *   site only; *host_sites (may be NULL) receives how many were.  On exactly degenerate input the listed slivers depend on
 *   rounding and may differ between the entries.
 *   n >= 1 (a single site has the row 2, -5, -6); a site outside the closed box is VRT_EINVAL naming the lowest such
 *   site, a row of more than D1 - 1 entries VRT_EGRID, both with vrt_tessellate's messages.  Every argument is checked
 *   before the device is touched.  Both entries are synchronous.
 * vrt_tessellate_gpu: host arrays; a refused or failed call leaves nbr as it was.
 * vrt_tessellate_dev: d_pos_zxy (n, 3) and d_nbr (n, D1) are device pointers on `device` (vrt_sample_sites_dev's output
 *   goes in directly); the kernels run on `stream`, which is synchronised; the positions are downloaded only if a site
 *   has to be recomputed on the host.  After a failed call d_nbr is undefined. */
int vrt_tessellate_gpu(int device, int64_t n, const double *pos_zxy, const double bounds[6], int64_t D1,
                       int64_t *nbr, int64_t *max_count, int64_t *host_sites);
int vrt_tessellate_dev(int device, int64_t n, const double *d_pos_zxy, const double bounds[6], int64_t D1,
                       int64_t *d_nbr, int64_t *max_count, int64_t *host_sites, void *stream);
/* event times of this process's last device tessellation (tools/tessellate_probe.py): sites, then milliseconds of the
 * grid build (bounds check included), the cell kernel, and the row assembly with any host recomputation; any of the four
 * may be NULL, all four is VRT_EINVAL */
int vrt_tessellate_last_phases(int64_t *n, double *grid_ms, double *cells_ms, double *rows_ms);
/* planes a cell holds at once in this build of the device tessellation (64; the tests' variant library lowers it) */
int64_t vrt_tessellate_capacity(void);
/* vrt_tessellate's cells for the m listed sites only (1-based ids, any order, no repeats): their rows of nbr (n, D1) are
 * written, the others left as they are; *max_count: the largest count among the listed.  Host code; what the device
 * entries recompute a site with. */
int vrt_tessellate_sites(int64_t n, const double *pos_zxy, const double bounds[6], int64_t D1, int64_t m,
                         const int64_t *sites, int64_t *nbr, int64_t *max_count);

/* introspection (parity tests; all values exactly as the reference's Julia fields, 1-based) */
int64_t vrt_grid_n(const vrt_grid *g);
int64_t vrt_grid_max_neighbours(const vrt_grid *g);             /* D = size(neighbours,2)-1   */
int64_t vrt_grid_num_layer_offsets(const vrt_grid *g, int dir); /* length(layers_up/down)     */
int vrt_grid_get_layers(const vrt_grid *g, int dir, int64_t *out); /* dir > 0 up, < 0 down   */
int vrt_grid_get_perm(const vrt_grid *g, int dir, int64_t *out);   /* n entries               */
/* Delaunay_lines as (3, D, n) column-major; wall slots are filled with 0 */
int vrt_grid_get_delaunay_lines(const vrt_grid *g, double *out);

/* ---- direction helper: k = [cos θ, cos ϕ sin θ, sin ϕ sin θ], lambda_iteration.jl:87 ------ */
void vrt_direction(double theta_deg, double phi_deg, double k[3]);

/* ---- plan: per-angle upwind tables (smallest_angle, voronoi_utils.jl:360-396, + weights and
 * path lengths, irregular_ray_tracing.jl:50-51,66) and the exact Gauss-Seidel dependency
 * schedule of irregular_ray_tracing.jl:37-80 / :118-161.  k is (3, n_angles) column-major; a
 * direction with k[0] < 0 is an "up" ray (θ > 90), k[0] > 0 "down"; k[0] == 0 (θ = 90) is
 * skipped exactly as the reference's callers do (lambda_iteration.jl:98,104). */
int vrt_plan_create(vrt_grid *g, int64_t n_angles, const double *k, int n_sweeps, vrt_plan **out);
/* same with an explicit sweep direction per angle (dirs[i] > 0 up / perm_up, < 0 down / perm_down,
 * 0 = skip), as Delaunay_upII / Delaunay_downII use whatever k they are handed; dirs == NULL
 * infers the direction from the sign of k[0] */
int vrt_plan_create_ex(vrt_grid *g, int64_t n_angles, const double *k, const int *dirs,
                       int n_sweeps, vrt_plan **out);
void vrt_plan_destroy(vrt_plan *p);
int64_t vrt_plan_num_levels(const vrt_plan *p);
int64_t vrt_plan_num_nodes(const vrt_plan *p);   /* live (site, sweep) updates per wavelength */
/* upwind table of one angle: up (2, n) 1-based ids, dots/w/r (2, n); any pointer may be NULL */
int vrt_plan_get_upwind(const vrt_plan *p, int64_t angle, int64_t *up, double *dots, double *w,
                        double *r);

/* ---- formal solve, all angles x all wavelengths: replaces the loop body of J_λ_voronoi ------
 *   S      (nlam, n) with leading dimension ld
 *   alpha  see VRT_ALPHA_*
 *   I0_up  (nlam, n1_up)   boundary intensity for up rays, ordered like perm_up[1:n1_up]
 *          (lambda_iteration.jl:99-101); NULL = zeros.  I0_down likewise (:105-106).
 *   RESERVED VALUE: where a step of one or two wavelength pairs runs as ONE chained launch (option VRT_CHAIN_DATAFLAG,
 *          default auto), an intensity is its own "written" flag, and "not yet written" is the quiet NaN whose 32-bit
 *          halves are both 0x7FF87FF8 (as a float: 0x7FF87FF8).  An ordinary NaN (0x7FF8000000000000, 0x7FC00000)
 *          propagates like anywhere else; an I0 or S that makes an intensity carry exactly the reserved pattern
 *          stalls its readers until the bounded wait expires (VRT_CHAIN_SPIN, ~2 s) and the call fails with
 *          VRT_ENODEVICE instead of returning it.  VRT_CHAIN_DATAFLAG=0 removes the reservation.
 *   weights[n_angles]      quadrature weights
 *   J      (nlam, n) out:  J = Σ_angles w · I  (lambda_iteration.jl:102,107), may be NULL
 *   I_out  (nlam, n, n_angles) out: per-angle intensities, may be NULL
 */
int vrt_plan_execute(vrt_plan *p, int64_t nlam, int64_t ld, const double *S, const double *alpha,
                     int alpha_mode, const double *I0_up, const double *I0_down,
                     const double *weights, double *J, double *I_out);
/* device-pointer variant; I0 leading dimension is nlam; I_out leading dimension is ld */
int vrt_plan_execute_dev(vrt_plan *p, int64_t nlam, int64_t ld, const double *dS,
                         const double *dalpha, int alpha_mode, const double *dI0_up,
                         const double *dI0_down, const double *weights_host, double *dJ,
                         double *dI_out, void *stream);
/* ---- native layout of per-angle alpha (VRT_ALPHA_ANGLE_NATIVE) ------------------------------
 * storage order of a direction: out[pos] = 1-based site id at storage position pos (layers
 * contiguous like perm_up / perm_down; inside a layer strips of lattice columns, rows of y inside a strip, a row by x --
 * neighbouring positions are neighbouring sites of a row; VRT_STORE_ORDER=morton at grid creation: a Morton curve over (x, y)). */
int vrt_grid_get_storage_order(const vrt_grid *g, int dir, int64_t *out);
/* number of doubles of the native per-angle alpha buffer for nlam wavelengths */
int64_t vrt_plan_native_alpha_count(const vrt_plan *p, int64_t nlam);
/* pairs per block B of the plan's native layout (1, 2, 4, 8 or 16; option VRT_PAIR_BLOCK at creation) */
int vrt_plan_native_pair_block(const vrt_plan *p);
/* the same for the FLOAT native buffer (vrt_plan_alpha_to_native_dev_f32, vrt_line_opacity_dev_f32): at least 2,
 * two neighbouring pairs being one 16-byte access of the fp32 kernel (option VRT_PATCH_QUAD, default on) */
int vrt_plan_native_pair_block_f32(const vrt_plan *p);
/* converts the caller's (nlam, n, n_angles) alpha (VRT_ALPHA_ANGLE_SITE_LAM) once, e.g. per
 * Λ-iteration when alpha changes, so that every execute of that iteration reads it in place */
int vrt_plan_alpha_to_native_dev(vrt_plan *p, int64_t nlam, int64_t ld, const double *dalpha,
                                 double *dalpha_native, void *stream);
/* the same for the fp32 VALUE path: float in, vrt_plan_native_alpha_count(p, nlam) FLOATS out, for
 * vrt_plan_execute_dev_f32 with VRT_ALPHA_ANGLE_NATIVE */
int vrt_plan_alpha_to_native_dev_f32(vrt_plan *p, int64_t nlam, int64_t ld, const float *dalpha,
                                     float *dalpha_native, void *stream);

/* ---- S and J in SWEEP ORDER (device entry points): what a device-resident Λ-iteration keeps between its steps ----
 * The sweep reads S and reduces J per sweep direction in that direction's storage order; a caller that produces S and
 * consumes J on the device (S_new = (1 - ε) J + ε B, the rate integrals: src/lambda_iteration.jl:261-263,
 * src/rates.jl:154-201) can keep both in that form and save the two layout changes of every execute (1 M sites x 51
 * wavelengths: 0.75 of 8.3 ms).  Per direction (up: θ > 90, down: θ < 90) ONE plane set of
 * vrt_plan_native_plane_count(p, nlam) doubles: element (l, pos) at ((l/2) * n + pos) * 2 + l%2, pos = the site's
 * position in vrt_grid_get_storage_order of the direction; an odd nlam is padded with one wavelength (S: any finite
 * value, J: unspecified).  Needs a plan on a layer path with VRT_PAIR_BLOCK=1 (the default for doubles). */
int64_t vrt_plan_native_plane_count(const vrt_plan *p, int64_t nlam);
/* caller's (nlam, n) array with leading dimension ld -> the plane sets of both directions (either may be NULL) */
int vrt_plan_to_native_dev(vrt_plan *p, int64_t nlam, int64_t ld, const double *d_in, double *d_up, double *d_down,
                           void *stream);
/* the plane set of ONE direction (dir > 0: up) -> the caller's (nlam, n) array */
int vrt_plan_from_native_dev(vrt_plan *p, int dir, int64_t nlam, int64_t ld, const double *d_native, double *d_out,
                             void *stream);
/* J[site][l] = J_up + J_down (a direction without angles: NULL), the sum vrt_plan_execute_dev forms itself */
int vrt_plan_j_from_native_dev(vrt_plan *p, int64_t nlam, int64_t ld, const double *dJ_up, const double *dJ_down,
                               double *dJ, void *stream);
/* vrt_plan_execute_dev with S read from and J reduced into sweep-order plane sets, in place.  alpha_mode:
 * VRT_ALPHA_SITE, VRT_ALPHA_ANGLE_NATIVE or VRT_ALPHA_SITE_LAM_NATIVE.  dJ_up / dJ_down: both or neither; the plane set of a direction without
 * angles comes back zeroed.  The results are those of vrt_plan_execute_dev bit for bit (J = J_up + J_down). */
int vrt_plan_execute_native_dev(vrt_plan *p, int64_t nlam, const double *dS_up, const double *dS_down,
                                const double *dalpha, int alpha_mode, const double *dI0_up, const double *dI0_down,
                                const double *weights_host, double *dJ_up, double *dJ_down, void *stream);
/* The same four with FLOAT storage (vrt_plan_execute_dev_f32's values; arithmetic in double): the plane sets hold
 * vrt_plan_native_plane_count(p, nlam) floats per direction, wavelength pairs in blocks of
 * vrt_plan_native_pair_block_f32(p) as in the float native alpha; the patch path only.  J_up + J_down (vrt_plan_j_from_native_dev_f32)
 * equals the J of vrt_plan_execute_dev_f32 bit for bit. */
int vrt_plan_to_native_dev_f32(vrt_plan *p, int64_t nlam, int64_t ld, const float *d_in, float *d_up, float *d_down,
                               void *stream);
int vrt_plan_from_native_dev_f32(vrt_plan *p, int dir, int64_t nlam, int64_t ld, const float *d_native, float *d_out,
                                 void *stream);
int vrt_plan_j_from_native_dev_f32(vrt_plan *p, int64_t nlam, int64_t ld, const float *dJ_up, const float *dJ_down,
                                   float *dJ, void *stream);
int vrt_plan_execute_native_dev_f32(vrt_plan *p, int64_t nlam, const float *dS_up, const float *dS_down,
                                    const float *dalpha, int alpha_mode, const float *dI0_up, const float *dI0_down,
                                    const double *weights_host, float *dJ_up, float *dJ_down, void *stream);

/* The two steps either side of the sweep in a device-resident Λ-iteration, on the same sweep-order plane sets (what
 * vrt_lambda_iterate runs internally): vrt_lambda_update_dev -- S_new = (1 - ε) J + ε B and the criterion's maximum
 * (src/lambda_iteration.jl:261-263, :325-349) -- with J = J_up + J_down, B in the UP order (vrt_plan_to_native_dev, once),
 * the OLD S read from dS_up and overwritten there, its down-order copy written to dS_down; and vrt_rates_populations_dev
 * (src/rates.jl:154-201, src/populations.jl:191-221) reading J from the two plane sets.  Arguments otherwise as their
 * caller-layout counterparts; results bit for bit theirs. */
int vrt_lambda_update_native_dev(vrt_grid *g, int64_t nlam, const double *dJ_up, const double *dJ_down,
                                 const double *dB_up, const double *deps, double *dS_up, double *dS_down,
                                 double *max_rel_change, void *stream);
int vrt_rates_populations_native_dev(vrt_grid *g, int64_t nlam, const double *lambda, const int64_t blocks[6],
                                     const double *dJ_up, const double *dJ_down, const double *planck2,
                                     double lambda0, double c0, const double *d_doppler_width, const double *d_gamma,
                                     double sigma_bb_const, const double *sigma_bf1, const double *sigma_bf2,
                                     const double *d_temperature, const double *d_lte_populations, double hc_over_kB,
                                     double pref_ij, double pref_ji, const double *d_C, const double *d_atom_density,
                                     double *d_R, double *d_populations, void *stream);
/* The same two on FLOAT sweep-order plane sets (vrt_plan_to_native_dev_f32, vrt_plan_execute_native_dev_f32).  They take the
 * PLAN: the float layout depends on vrt_plan_native_pair_block_f32(p); VRT_EINVAL before anything is launched on a plan
 * that is not on the patch path.  Arithmetic in double; the update rounds in exactly these places:
 *   J     = (float)((double)J_up + (double)J_down)      the J vrt_plan_j_from_native_dev_f32 delivers: the J a caller
 *                                                        downloads is the J that S was formed from
 *   S_new = (float)((1 - ε) (double)J + ε (double)B)
 *   d     = |1 - (double)S_old / (double)S_new|          over the nlam physical wavelengths only
 * The pad wavelength of an odd nlam is written as 0 and takes no part in the maximum.  B in the up order, the old S read
 * from dS_up and overwritten there, the down-order copy written to dS_down, either J pointer NULL for a direction without
 * angles, NaN -> NaN, as vrt_lambda_update_native_dev.  The rates read the same rounded float J, widened, and from there
 * run the arithmetic of vrt_rates_populations_native_dev; R and the populations stay double. */
int vrt_lambda_update_native_dev_f32(vrt_plan *p, int64_t nlam, const float *dJ_up, const float *dJ_down,
                                     const float *dB_up, const double *deps, float *dS_up, float *dS_down,
                                     double *max_rel_change, void *stream);
int vrt_rates_populations_native_dev_f32(vrt_plan *p, int64_t nlam, const double *lambda, const int64_t blocks[6],
                                         const float *dJ_up, const float *dJ_down, const double *planck2,
                                         double lambda0, double c0, const double *d_doppler_width, const double *d_gamma,
                                         double sigma_bb_const, const double *sigma_bf1, const double *sigma_bf2,
                                         const double *d_temperature, const double *d_lte_populations, double hc_over_kB,
                                         double pref_ij, double pref_ji, const double *d_C, const double *d_atom_density,
                                         double *d_R, double *d_populations, void *stream);
/* The rates step split over wavelength ranges (what a member of vrt_multi_lambda runs; a one-process-per-GPU caller builds
 * the same loop from these).  vrt_rate_shares_native_dev[_f32]: the share of the wavelengths [l0, l1) of the case's nlam in
 * the six λ-integrals of a site, the trapezoid sums regrouped per wavelength -- Σ_l W_l f_l with
 * W_l = (λ_l - λ_l-1) [l > lo] + (λ_l+1 - λ_l) [l < hi - 1] inside each block [lo, hi), the prefactor applied last -- so that
 * the shares of a partition of [0, nlam), added, are the integrals of vrt_rates_populations_native_dev to the rounding of
 * that regrouping (1e-12).  lambda, blocks, planck2, sigma_bf1 / sigma_bf2 describe ALL nlam wavelengths; the J plane sets
 * hold the l1 - l0 wavelengths of the range only, wavelength l at local index l - l0: doubles in the grid's two orders
 * (vrt_plan_native_plane_count(p, l1 - l0) each), or floats in the plan's float layout of l1 - l0 wavelengths, J formed as
 * (float)(J_up + J_down) and widened, as vrt_rates_populations_native_dev_f32 forms it.  The padding wavelength of an odd
 * l1 - l0 is never used, whatever it holds.  Either J pointer may be NULL for a direction without angles.
 * d_shares [6][n]: (bf1 ij, bf1 ji, bf2 ij, bf2 ji, bb ij, bb ji) of site i at [q n + i].  0 <= l0 <= l1 <= nlam; l0 == l1
 * gives six zero planes (both J pointers may then be NULL); a transition without a wavelength in [l0, l1) gets exactly 0.
 * vrt_populations_from_shares_dev: R (3, 3, n) and the populations (n, 3) from the SUMMED shares, on the current device
 * (src/populations.jl:191-221). */
int vrt_rate_shares_native_dev(vrt_grid *g, int64_t nlam, int64_t l0, int64_t l1, const double *lambda,
                               const int64_t blocks[6], const double *dJ_up, const double *dJ_down, const double *planck2,
                               double lambda0, double c0, const double *d_doppler_width, const double *d_gamma,
                               double sigma_bb_const, const double *sigma_bf1, const double *sigma_bf2,
                               const double *d_temperature, const double *d_lte_populations, double hc_over_kB,
                               double pref_ij, double pref_ji, double *d_shares, void *stream);
int vrt_rate_shares_native_dev_f32(vrt_plan *p, int64_t nlam, int64_t l0, int64_t l1, const double *lambda,
                                   const int64_t blocks[6], const float *dJ_up, const float *dJ_down, const double *planck2,
                                   double lambda0, double c0, const double *d_doppler_width, const double *d_gamma,
                                   double sigma_bb_const, const double *sigma_bf1, const double *sigma_bf2,
                                   const double *d_temperature, const double *d_lte_populations, double hc_over_kB,
                                   double pref_ij, double pref_ji, double *d_shares, void *stream);
int vrt_populations_from_shares_dev(int64_t n, const double *d_shares, const double *d_C, const double *d_atom_density,
                                    double *d_R, double *d_populations, void *stream);

/* fp32 VALUE path (BASELINE config C5): S, alpha, I_0, J and the per-angle intensities are stored
 * as float, halving the bytes of this bandwidth-bound path; the geometry tables and all
 * arithmetic stay fp64.  Results agree with the fp64 solve to fp32 storage rounding (~1e-6
 * relative).  Runs on the layer-step kernels (coefficients handed over and level tiles held as
 * float) when no layer exceeds 18 432 sites, on the level kernels otherwise. */
int vrt_plan_execute_dev_f32(vrt_plan *p, int64_t nlam, int64_t ld, const float *dS,
                             const float *dalpha, int alpha_mode, const float *dI0_up,
                             const float *dI0_down, const double *weights_host, float *dJ,
                             float *dI_out, void *stream);
/* time (ms, HIP events on the launch stream) the sweep kernels of the last execute took, and the
 * number of sweep-kernel launches it made (waits for the sweep; VRT_ENODEVICE if its chained patch launch gave up
 * waiting for a dependency -- a bounded spin expired: the results of that execute are invalid; also reported by the
 * next execute of the plan) */
int vrt_plan_last_sweep_timing(const vrt_plan *p, double *ms, int64_t *launches);
/* how the patch path cut this plan (introspection for the tests only: nothing in a solve needs it): out[0] = patches of all angles and layers, out[1] = the fewest patches
 * any (angle, layer >= 2) has, out[2] = slots of the work lists of the per-layer launches and out[3] = how many of them are
 * padding (both 0 until a per-layer execute has built the lists) */
int vrt_plan_patch_layout(const vrt_plan *p, int64_t *out);
/* which block of a per-layer patch launch does what (introspection for the tests only; host only): the grid of a launch
 * with `nrow` rows of the work list, `nsplit` workgroups per item and sibling (an item has `steps` >= nsplit pair steps),
 * 1 << lg_siblings siblings and `nred` reduction blocks, in dispatch order `order` (option VRT_PATCH_ORDER: 0 interleaved,
 * 1 share-major).  dims[4] = gridDim.x, gridDim.y, the order taken (0 where share-major order would pass 65 535 grid rows,
 * or with one split) and the rows that hold patch blocks; blocks (or NULL) = six numbers per block in the grid's linear
 * order (x first): role (0 patch, 1 reduction), XCD lane, work-list row, split, sibling, share in pair steps -- a
 * reduction block: 1, its index among the reduction blocks, zeros. */
int vrt_patch_dispatch_map(int order, int nrow, int nsplit, int lg_siblings, int64_t nred, int steps, int64_t *dims, int32_t *blocks);
/* which pair elements the blocks of a launch's patch grid reduce when the J reduction rides in them (option
 * VRT_PATCH_REDUCE_RIDE; introspection for the tests only; host only): the patch grid of vrt_patch_dispatch_map(order, nrow,
 * nsplit, lg_siblings, 0 reduction blocks), storage position ranges [lo[r], hi[r]) (r = 0, 1; an empty range: none) of a grid
 * of n sites, npair wavelength pairs in pair blocks of 1 << lg_block, NT threads per block.  dims[4] = blocks of the patch
 * grid, chunks (NT elements) of range 0, of range 1, and 1 where the launch rides -- 0: four chunks per block do not cover
 * the ranges, the launch keeps its reduction rows, nothing else is written.  elems (or NULL) = for the blocks
 * [first_block, first_block + nblocks) of the grid's linear order 4 x NT numbers each ([round][thread]): the index of the
 * pair element in the plane set [npair][n], | 1 << 62 for range 1; -1: nothing. */
int vrt_patch_ride_map(int order, int nrow, int nsplit, int lg_siblings, int npair, int lg_block, int NT, int64_t n, const int32_t *lo,
                       const int32_t *hi, int64_t first_block, int64_t nblocks, int64_t *dims, int64_t *elems);
/* the riding form in the last sweep of a plan (introspection for the tests only): out[0] = per-layer launches whose
 * reduction rode in their patch blocks, out[1] = the most chunks a block of such a launch took (0: none rode) */
int vrt_plan_patch_ride_stats(const vrt_plan *p, int64_t *out);
/* timeline of the last sweep's per-layer patch launches (diagnostics build of the library with option VRT_PATCH_TIMELINE=1
 * only; VRT_EINVAL otherwise): waits for the device, then launches[12 per launch] = layer, stream group, gridDim.x,
 * gridDim.y, work-list rows, splits, log2 siblings, order, patch rows, reduction blocks, first block, pair steps of an
 * item; stamps[3 per block, linear grid order] = start, end (wall clock ticks), share in pair steps (| 1 << 32: a
 * reduction block; a patch block that reduced a riding slice: bits 33-46 its elements, bits 48-63 the ticks from its start
 * to its J store); counts[3] = launches, blocks, wall clock rate in kHz */
int vrt_plan_patch_timeline(vrt_plan *p, int64_t cap_launches, int64_t cap_blocks, int64_t *launches, uint64_t *stamps, int64_t *counts);
/* VRT_OK, or the give-up of a chained patch launch that has finished since the last check (VRT_ENODEVICE: the results of
 * that execute are invalid).  The entry points that synchronise themselves (vrt_plan_execute, vrt_plan_execute_line,
 * vrt_lambda_iterate, vrt_multi_*) report it from the call it spoiled; a caller of the ASYNCHRONOUS entry points
 * (vrt_plan_execute_dev, _native_dev, _f32) calls this -- or vrt_plan_last_sweep_timing -- after it has synchronised
 * its stream.  No synchronisation here. */
int vrt_plan_check(vrt_plan *p);
/* which device path the last execute took: 1 = "levels" (one launch per dependency level),
 * 2 = "tiles" (one persistent launch), 3 = "steps" (two launches per BFS layer), 4 = "patches" (layers cut
 * into patches, the default: ONE chained launch for every layer, or one fused launch per BFS layer); 0 = none yet.  The paths give the
 * same results; option VRT_PATH selects one (performance experiments, the parity tests' cross-checks). */
int vrt_plan_last_path(const vrt_plan *p);
/* Tuning options (performance experiments and the tests' cross-checks; results never depend on them).
 * Every option has a default; an environment variable of the option's name presets it and is read ONCE,
 * when a plan is created -- an execute reads no environment.  vrt_plan_set_option changes an option of a
 * live plan; vrt_grid_set_option sets it for the plans vrt_delaunay_up / _down cache inside the grid.
 *   VRT_PATH = auto | levels | tiles | steps | patches
 *   VRT_PATCH_Q, VRT_PATCH_TARGET              wavelength pairs at a time / workgroups per launch of the patch kernel
 *   VRT_PATCH_ORDER = 0 | 1                    dispatch order of the workgroups of a per-layer patch launch: an item's
 *                                              workgroups side by side, or share-major -- every item's longest share of
 *                                              wavelength-pair steps first (default 1)
 *   VRT_PATCH_REDUCE_RIDE = 0 | 1              the J reduction of a per-layer launch in reduction blocks of their own behind
 *                                              its patch blocks (default 0), or inside the patch blocks' start-up (1)
 *   VRT_PATCH_K, VRT_PATCH_NT, VRT_PATCH_OWN  entries per thread, threads, owned sites per patch (creation only)
 *   VRT_PATCH_LEAN = 0 | 1                     the 64-register patch kernel, four workgroups per CU (default 1)
 *   VRT_PATCH_CHAIN = 0 | 1 | 2                every layer inside ONE launch, ordered by the data's own dependencies: never
 *                                              (one launch per layer and direction), wherever the kernel exists, auto
 *                                              (default: where a layer alone cannot fill the chip)
 *   VRT_CHAIN_PAIRS, VRT_CHAIN_SPIN            wavelength-pair blocks per item of the chained launch at most (default 9); polls
 *                                              (x 1024) after which a waiting workgroup gives up (default 2048)
 *   VRT_CHAIN_DATAFLAG = 0 | 1 | 2             chained launch, fp64: the stored intensities are their own flags (the planes are
 *                                              filled with a NaN pattern before the launch; a gather that still holds it
 *                                              is repeated) instead of progress words: never, always, auto (default: for
 *                                              one or two wavelength pairs, where the fill is cheaper than the words)
 *   VRT_PATCH_QUAD = 0 | 1                     fp32 storage: four wavelengths per lane (creation only; default 1)
 *   VRT_PAIR_BLOCK = 1 | 2 | 4 | 8 | 16        wavelength pairs of a site side by side in the patch path's planes and
 *                                              in the plan's native alpha (creation only; default 1)
 *   VRT_STEP_K, VRT_STEP_SINGLE, VRT_STEP_PAIRS, VRT_STEP_XCD, VRT_STEP_STREAMS, VRT_STEP_LEVEL_MAP,
 *   VRT_STEP_GROUP_DIR, VRT_TILE_WIDE, VRT_TILE_PRE                variants of the older paths
 * VRT_EINVAL for an unknown name, a value out of range, or a creation-only option on a live plan. */
int vrt_plan_set_option(vrt_plan *p, const char *name, const char *value);
int vrt_grid_set_option(vrt_grid *g, const char *name, const char *value);

/* ---- schedule introspection (host only, works on a device < 0 grid handle) -----------------
 * The dependency schedule of one direction given an upwind table `up` (2, n), 1-based ids as
 * returned by vrt_plan_get_upwind (0 = none).  Nodes are the surviving (site, sweep) visits of
 * irregular_ray_tracing.jl:37-80 sorted by level; zflags bit 0/1 = the read of I[upwind 1/2]
 * sees the initial zero.  level_off has num_levels + 1 entries. */
typedef struct vrt_schedule vrt_schedule;
int vrt_schedule_build(const vrt_grid *g, int dir, const int64_t *up, int n_sweeps, vrt_schedule **out);
int64_t vrt_schedule_num_nodes(const vrt_schedule *s);
int64_t vrt_schedule_num_levels(const vrt_schedule *s);
int vrt_schedule_get(const vrt_schedule *s, int64_t *site, int32_t *zflags, int64_t *level_off);
void vrt_schedule_destroy(vrt_schedule *s);
/* The layer-local form of the same schedule used by the LDS layer-tile kernel: vis[n] packs up to
 * four 8-bit in-layer visit levels per site (0 = none), nlev[num_layer_offsets] the level count
 * of each layer (index = 1-based layer).  VRT_EINVAL if it does not fit that encoding. */
int vrt_layer_schedule(const vrt_grid *g, int dir, const int64_t *up, int n_sweeps, uint32_t *vis,
                       int32_t *nlev, int64_t *n_visits);
/* Thread assignment of the layer-step level kernel for such a `vis` (introspection, host only):
 * store[n] = 1-based site id at each storage position (layers contiguous, the storage order inside);
 * self[n] = 0-based storage position held by each sorted index: inside every layer the
 * positions are sorted (stably) by visit pattern -- first, then second, ... visit level. */
int vrt_layer_sorted_slots(const vrt_grid *g, int dir, const uint32_t *vis, int64_t *store, int64_t *self);

/* Patch schedule of the fused layer kernel ("patches" path; introspection, host only): every BFS layer
 * is cut into ranges of about `own_target` consecutive storage positions, and each range carries
 * the in-layer dependency cone of its sites (own sites + a halo of neighbouring sites' visits it
 * recomputes), at most `entry_cap` entries.  Step 1: counts[0..5] = patches, entries, visits
 * executed over all patches, live visits of the unsplit schedule, largest entry count of a patch,
 * layer offsets (= vrt_grid_num_layer_offsets + 1).  Step 2 (vrt_patch_schedule_get): layer_patch_off
 * [counts[5]], patch_own_lo / patch_own_cnt / patch_nlev [patches], patch_ent_off [patches + 1],
 * entry_pos (0-based storage position) / entry_vis / entry_loc [entries]; any pointer may be NULL. */
typedef struct vrt_patch_schedule vrt_patch_schedule;
int vrt_patch_schedule_build(const vrt_grid *g, int dir, const int64_t *up, int n_sweeps, int own_target,
                             int entry_cap, vrt_patch_schedule **out, int64_t counts[6]);
int vrt_patch_schedule_get(const vrt_patch_schedule *s, int32_t *layer_patch_off, int32_t *patch_own_lo,
                           int32_t *patch_own_cnt, int32_t *patch_nlev, int64_t *patch_ent_off,
                           int32_t *entry_pos, uint32_t *entry_vis, uint32_t *entry_loc);
/* Dependencies BETWEEN patches (what the chained launch of the patch path waits on, vrt_patch.hip: k_patch_chain):
 * patch q gathers, as upwind intensities of EARLIER layers (irregular_ray_tracing.jl:75), values that the
 * patches dep_list[dep_off[q] .. dep_off[q+1]) store (sorted patch indices of this schedule; the boundary layer
 * and the never-visited last site have no owner).  dep_off [patches + 1] first, then dep_list [dep_off[patches]];
 * either pointer may be NULL. */
int vrt_patch_schedule_get_deps(const vrt_patch_schedule *s, int64_t *dep_off, int32_t *dep_list);
/* The angle's layer schedule as the patch builder derives it on the way (plan creation uses this one): same contents as
 * vrt_layer_schedule's outputs (vis[n], nlev[vrt_grid_num_layer_offsets], *n_visits); any pointer may be NULL. */
int vrt_patch_schedule_get_layers(const vrt_patch_schedule *s, uint32_t *vis, int32_t *nlev, int64_t *n_visits);
void vrt_patch_schedule_destroy(vrt_patch_schedule *s);

/* ---- single solves: drop-in bodies for Delaunay_upII / Delaunay_downII --------------------
 * (src/irregular_ray_tracing.jl:15-20,96-101).  nI0 must equal layers[2]-1 of the direction.
 * The plan for k is cached inside the grid. */
int vrt_delaunay_up(vrt_grid *g, const double k[3], const double *S, const double *I0,
                    int64_t nI0, const double *alpha, int n_sweeps, double *I_out);
int vrt_delaunay_down(vrt_grid *g, const double k[3], const double *S, const double *I0,
                      int64_t nI0, const double *alpha, int n_sweeps, double *I_out);

/* ---- resampling between the sites and regular rasters --------------------------------------------
 * The two ends of every reference run: initialise (src/voronoi_utils.jl:687-707, trilinear src/functions.jl:207-248) puts a
 * raster's fields on the sites; Voronoi_to_Raster (:407-617) and Voronoi_to_Raster_inv_dist (:773-816, inv_dist_itp
 * :848-860) bring site fields back to a raster, as the searchlight images do (compare_searchlight.jl:116-141).
 *   distance  d = sqrt((dz*dz + dx*dx) + dy*dy) in (z, x, y); VRT_METRIC_PERIODIC_XY takes dx = qx - px, then
 *             dx -= Lx if dx > Lx/2, dx += Lx if dx < -Lx/2 (the same for y), and first wraps a query x outside
 *             [x_min, x_max] to x - Lx*floor((x - x_min)/Lx) (y likewise), so ghost-cell axes (periodic_borders) work
 *   nearest   the smallest (d, id): on a tie the lowest site id
 *   k = 2     the two smallest (d, id) in that order
 *   inv_dist  f = (v1/d1 + v2/d2)/(1/d1 + 1/d2) in inv_dist_itp's order (inv = 1/d; avg += inv; f += v*inv; f/avg);
 *             d1 == 0 gives v1 (the reference's Inf/Inf = NaN there)
 *   trilinear the reference's: interval = searchsortedfirst(axis, v) - 1 clamped to [0, n-2] (a site at exactly z[1]
 *             is no BoundsError), x then y then z with its expressions
 * PRECONDITION of the nearest search: the neighbour rows are the Voronoi neighbours of the sites in the x/y-periodic box
 * (vrt_tessellate, voro++, read_cell of a voro++ file; a row missing a neighbour that lists it is completed).  It walks to
 * ever closer neighbours from a seed site, so on other
 * graphs (e.g. jittered lattices with fixed lists) it ends at a local minimum; a walk that exceeds its step or tie-set cap
 * fails the call with VRT_EGRID.  Queries: z in [z_min, z_max]; x, y in the box under VRT_METRIC_EUCLIDEAN.
 * Every argument is checked before the device is touched (a host-only grid: VRT_EINVAL or VRT_ENODEVICE).  The calls
 * synchronise (a failed walk is reported as a status).  Option VRT_NEAREST_CELLS = auto | cells per axis
 * (vrt_grid_set_option): the cell list that seeds the walks; results never depend on it. */
#define VRT_METRIC_EUCLIDEAN   0  /* plain distance in (z, x, y): the reference's KDTree (voronoi_utils.jl:437-442) */
#define VRT_METRIC_PERIODIC_XY 1  /* minimum image in x and y: the geometry of the tessellation itself            */
#define VRT_RASTER_NEAREST     1  /* Voronoi_to_Raster: value of the nearest site                                  */
#define VRT_RASTER_INV_DIST2   2  /* Voronoi_to_Raster_inv_dist: the two nearest sites, weights 1/d (p = 1, n_k = 2)  */
/* k = 1 or 2 nearest sites of nq points q (3, nq); idx (k, nq) 1-based, dist (k, nq) may be NULL.  Host pointers. */
int vrt_grid_nearest(vrt_grid *g, int64_t nq, const double *q_zxy, int metric, int k, int64_t *idx, double *dist);
/* sites -> raster.  Fields (nf, n) with leading dimension ld (the layout of S in vrt_plan_execute_dev); raster
 * (nz, nx, ny, nf), element [iz + nz*(ix + nx*(iy + ny*f))]: per field the array layout vrt_regular_execute_dev reads
 * (S_stride = nz*nx*ny).  Axes (ascending, >= 1 point each) on the host; fields and raster on the device. */
int vrt_grid_to_raster_dev(vrt_grid *g, int64_t nz, int64_t nx, int64_t ny, const double *z, const double *x,
                           const double *y, int metric, int mode, int64_t nf, int64_t ld, const double *d_fields,
                           double *d_raster, void *stream);
/* raster -> sites, trilinear; axes >= 2 points, every site inside their ranges; fields (nf, n) written with ld */
int vrt_raster_to_grid_dev(vrt_grid *g, int64_t nz, int64_t nx, int64_t ny, const double *z, const double *x,
                           const double *y, int64_t nf, const double *d_raster, int64_t ld, double *d_fields,
                           void *stream);
/* the same from host arrays, staged through the device */
int vrt_grid_to_raster(vrt_grid *g, int64_t nz, int64_t nx, int64_t ny, const double *z, const double *x,
                       const double *y, int metric, int mode, int64_t nf, int64_t ld, const double *fields,
                       double *raster);
int vrt_raster_to_grid(vrt_grid *g, int64_t nz, int64_t nx, int64_t ny, const double *z, const double *x,
                       const double *y, int64_t nf, const double *raster, int64_t ld, double *fields);
/* the last nearest search of the grid (vrt_grid_nearest or vrt_grid_to_raster*): HIP-event times of the walk and of the
 * gather (0 for vrt_grid_nearest), queries, walk steps summed over the queries, queries that took the Euclidean
 * cell-list search; any pointer may be NULL */
int vrt_grid_raster_stats(const vrt_grid *g, double *nearest_ms, double *gather_ms, int64_t *queries,
                          int64_t *walk_steps, int64_t *fallbacks);

/* ---- sites sampled from a raster density (rejection_sampling, src/functions.jl:79-120) --------------------------------
 * The first step of every reference run (compare_line.jl:51-125): sample_from_invNH_invT & co. (src/sample_grids.jl)
 * form a quantity on the raster and draw the sites from it by rejection.
 *   box       z_0 = z[0], dz = z[nz-1] - z[0]; the same for x and y.  q_min = min q, q_max = max q, dq = q_max - q_min
 *   proposal  j = 0, 1, 2, ...: u_c = U(seed, c, j) for c = 0..3, U = synth.counter_uniform: splitmix64 of
 *             (j ^ splitmix64(seed * 0x100000001B3 + c)), >> 11, times 2^-53
 *             zr = u_0*dz + z_0, xr = u_1*dx + x_0, yr = u_2*dy + y_0 (multiply, then add)
 *   accept    trilinear(q; zr, xr, yr) > u_3*dq + q_min: the reference's test, so the sites are distributed
 *             proportionally to q - q_min (not to q).  trilinear as vrt_raster_to_grid's (clamped interval, x, y, z)
 *   result    pos_zxy (n_sites, 3) rows (z, x, y): the first n_sites accepted proposals in increasing j;
 *             *proposals_used (may be NULL) = 1 + the j of the last of them.  The result is a function of (axes,
 *             quantity, n_sites, seed) alone: not of batch, launch shape or device.  (The reference draws from Julia's
 *             global RNG; its stream is not reproduced.)
 * Axes: >= 2 points, finite, strictly ascending, on the host.  quantity: (ny, nx, nz), element iz + nz*(ix + nx*iy) --
 * the raster layout of vrt_raster_to_grid; every value finite and q_max > q_min (otherwise the reference never ends).
 * batch: proposals per device batch, 0 = chosen from the acceptance seen so far (clamped to 2^24).  max_proposals: the
 * cap, 0 = 1000*n_sites + 2^20; a cap reached before n_sites are accepted is VRT_EINVAL, vrt_last_error giving the
 * accepted and proposed counts and *proposals_used the proposals made (the _dev form has then written the accepted
 * rows, the host form nothing).  Every argument check -- for the host form also the quantity's -- runs before the
 * device is touched; the _dev form takes q_min, q_max and the finiteness from a device reduction.  Synchronous (one
 * int64 read per batch). */
int vrt_sample_sites(int device, int64_t nz, int64_t nx, int64_t ny, const double *z, const double *x, const double *y,
                     const double *quantity, int64_t n_sites, uint64_t seed, int64_t batch, int64_t max_proposals,
                     double *pos_zxy, int64_t *proposals_used);
int vrt_sample_sites_dev(int device, int64_t nz, int64_t nx, int64_t ny, const double *z, const double *x,
                         const double *y, const double *d_quantity, int64_t n_sites, uint64_t seed, int64_t batch,
                         int64_t max_proposals, double *d_pos_zxy, int64_t *proposals_used, void *stream);

/* ---- Λ-iteration epilogue on the device (the physics-free part) -----------
 * S_new[l,i] = (1 - eps[i]) J[l,i] + eps[i] B[l,i]           (src/lambda_iteration.jl:261-263)
 * *max_rel_change = max |1 - S_old/S_new|, NaN if any term is NaN  (criterion, :325-349)
 * All arrays are device pointers, (nlam, n) with leading dimension ld, eps[n]; S_new may alias
 * neither S_old nor J.  Synchronises `stream` (the scalar comes back to the host), so a whole
 * Λ-iteration J -> S_new -> J ... stays device-resident. */
int vrt_lambda_update_dev(vrt_grid *g, int64_t nlam, int64_t ld, const double *dJ, const double *dB,
                          const double *deps, const double *dS_old, double *dS_new,
                          double *max_rel_change, void *stream);

/* ---- fused per-angle opacity prologue -------------------------------------
 * alpha_tot = alphaline_lambda + alpha_cont for EVERY angle of the plan from per-site line parameters,
 * written directly in the native layout of VRT_ALPHA_ANGLE_NATIVE -- replaces the per-angle part of
 * J_λ_voronoi between the angle loop header and the formal solve: damping_λ
 * (src/lambda_iteration.jl:72-80, src/broadening.jl:87-89), compute_voigt_profile with the
 * line-of-sight velocity of -k (src/line.jl:121-137, :198-208), αline_λ (src/line.jl:219-225) and
 * α_tot = αline + α_cont (src/lambda_iteration.jl:93-96):
 *   v_los = dot(velocity, -k);  a = γ λ²/(4π c0 ΔλD);  v = (λ - λ0 + λ0 v_los/c0)/ΔλD
 *   alpha = line_strength * H(a, v)/(sqrt(π) ΔλD) + alpha_cont
 * H = Re w4(v + i a), Humlíček's w4 as Transparency.jl's voigt_profile (absent from the reference
 * checkout; tolerance-based parity).  Plain numbers in one unit system of the caller's choice:
 *   lambda[nlam] (host), lambda0, c0;  device: velocity (3, n) rows z,x,y; doppler_width ΔλD[n];
 *   gamma[n]; line_strength[n] = h c0/(4π λ0) (n_i B_ij - n_j B_ji); alpha_cont[n];
 *   alpha_native: vrt_plan_native_alpha_count(p, nlam) doubles, out. */
int vrt_line_opacity_dev(vrt_plan *p, int64_t nlam, const double *lambda, double lambda0, double c0,
                         const double *d_velocity, const double *d_doppler_width, const double *d_gamma,
                         const double *d_line_strength, const double *d_alpha_cont, double *d_alpha_native,
                         void *stream);
/* the same with the result STORED as float (fp32 value path; per-site inputs and arithmetic stay fp64):
 * vrt_plan_native_alpha_count(p, nlam) floats for vrt_plan_execute_dev_f32 with VRT_ALPHA_ANGLE_NATIVE */
int vrt_line_opacity_dev_f32(vrt_plan *p, int64_t nlam, const double *lambda, double lambda0, double c0,
                             const double *d_velocity, const double *d_doppler_width, const double *d_gamma,
                             const double *d_line_strength, const double *d_alpha_cont, float *d_alpha_native,
                             void *stream);

/* ---- the same from HOST arrays: the whole body of J_λ_voronoi, line case, in one call --------------------
 * src/lambda_iteration.jl:72-111 for a host without device arrays of its own (the reference's Julia driver):
 * uploads the seven per-site line vectors, λ and S (about (nλ + 7) n doubles -- NOT α_tot (nλ, n, n_angles),
 * which is nλ n_angles n), makes α_tot of every angle on the device in the native layout, solves every
 * angle x wavelength and returns J.  Arguments as vrt_line_opacity_dev / vrt_plan_execute, all host pointers;
 * gamma[n] is γ_constant of the current populations (or vrt_lambda_* below keeps the whole loop on the device). */
int vrt_plan_execute_line(vrt_plan *p, int64_t nlam, int64_t ld, const double *lambda, double lambda0, double c0,
                          const double *velocity, const double *doppler_width, const double *gamma,
                          const double *line_strength, const double *alpha_cont, const double *S, const double *I0_up,
                          const double *I0_down, const double *weights, double *J);

/* ---- population-dependent line terms on the device ------------------------------------------------------
 *   gamma[i]         = gamma_static[i] + gamma_unsold[i] (n_1 + n_2)     γ_constant, src/broadening.jl:63-82, which
 *                      J_λ_voronoi evaluates with populations[:,1] .+ populations[:,2] in EVERY iteration
 *                      (lambda_iteration.jl:72-75).  gamma_static = natural width + linear + quadratic Stark
 *                      (electron density and temperature only: fixed), gamma_unsold = γ_unsold per unit
 *                      neutral-hydrogen density (van der Waals; linear in the density) -- both come from the
 *                      caller, whose Transparency.jl holds the constants
 *   line_strength[i] = strength_const (n_1 B_ij - n_2 B_ji)              αline_λ, src/line.jl:219-225
 * populations (n, 3) as Julia's; gamma or line_strength may be NULL.  Device pointers. */
int vrt_line_terms_dev(vrt_grid *g, const double *d_gamma_static, const double *d_gamma_unsold,
                       const double *d_populations, double strength_const, double Bij, double Bji, double *d_gamma,
                       double *d_line_strength, void *stream);

/* ---- Λ_voronoi's loop with library-owned device state (src/lambda_iteration.jl:205-300) -----------------
 * For a single-process host with HOST arrays: create uploads the per-site inputs Λ_voronoi derives before its
 * loop, starts in LTE with S = B_0 (:232-240); every vrt_lambda_iterate is one pass of the loop body --
 *   γ, line strength of the current populations -> α_tot of every angle (:72-96) -> J_λ (:84-111) ->
 *   S_new = (1 - ε) J + ε B_0 and max |1 - S_old/S_new| (:261-263, :325-349) -> R, populations (:269, :274)
 * -- and returns that maximum (NaN like Julia's); vrt_lambda_get downloads what the caller wants to keep
 * (the reference checkpoints populations and S_new each iteration, :280-281).  All arrays host, (…) = Julia
 * dims; plain numbers in one unit system, unit factors folded into the constants as in
 * vrt_rates_populations_dev.  weights[n_angles] of the plan's quadrature. */
typedef struct vrt_lambda vrt_lambda;
typedef struct vrt_line_case {
    int64_t nlam;
    const double *lambda;            /* [nlam]: bound-bound block first, then the two bound-free blocks */
    int64_t blocks[6];               /* their [lo, hi) offsets, 0-based (line.λidx) */
    double lambda0, c0;
    const double *velocity;          /* (3, n) rows z, x, y */
    const double *doppler_width;     /* [n] ΔλD */
    const double *gamma_static;      /* [n] see vrt_line_terms_dev */
    const double *gamma_unsold;      /* [n] */
    const double *alpha_cont;        /* [n] */
    const double *eps;               /* [n] destruction probability ε */
    const double *temperature;       /* [n] */
    const double *atom_density;      /* [n] */
    const double *B0;                /* (nlam, n) Planck function */
    const double *lte_populations;   /* (n, 3) */
    const double *C;                 /* (3, 3, n) collisional rates */
    const double *planck2;           /* [nlam] 2 h c0² / λ⁵ in J's unit */
    const double *sigma_bf1, *sigma_bf2;   /* σic per wavelength of the two bound-free blocks */
    double strength_const, Bij, Bji;       /* αline_λ = strength_const (n_1 B_ij - n_2 B_ji) φ */
    double sigma_bb_const, hc_over_kB, pref_ij, pref_ji;
} vrt_line_case;
int vrt_lambda_create(vrt_plan *p, const vrt_line_case *lc, const double *weights, vrt_lambda **out);
int vrt_lambda_iterate(vrt_lambda *s, double *max_rel_change);
/* J, S (nlam, n), populations (n, 3), R (3, 3, n), gamma [n] of the last iteration; any pointer may be NULL */
int vrt_lambda_get(vrt_lambda *s, double *J, double *S, double *populations, double *R, double *gamma);
void vrt_lambda_destroy(vrt_lambda *s);
/* The same session with FLOAT storage (the fp32 value path: arithmetic in double).  S and J in both sweep orders, B in
 * the up order, I_0 and the native α are held as float; the double B_0 of the case is staged, converted and freed, so
 * that after create the session holds no double array of size nλ·n or nλ·n·angles.  An iterate runs the line terms, the
 * float opacity prologue, vrt_plan_execute_native_dev_f32, vrt_lambda_update_native_dev_f32 and
 * vrt_rates_populations_native_dev_f32 (their roundings: above); only the criterion's scalar comes back.
 * VRT_EINVAL on a plan that is not on the patch path or with VRT_LAMBDA_NATIVE=0: there is no fp64 fallback.
 * vrt_lambda_get returns J and S as doubles holding exactly the float values (J the combined rounded sum);
 * vrt_lambda_set_state validates as for a double session, then rounds S to float (an S that came from vrt_lambda_get of
 * such a session is float-representable: it continues bit for bit); vrt_lambda_set_acceleration returns VRT_EINVAL and
 * changes nothing -- the Ng kernels are written for the [pair][pos][2] double layout, float variants are a later step.
 * vrt_lambda_storage: the bytes per stored value of a session, 8 or 4 (VRT_EINVAL for NULL). */
int vrt_lambda_create_f32(vrt_plan *p, const vrt_line_case *lc, const double *weights, vrt_lambda **out);
int vrt_lambda_storage(const vrt_lambda *s);

/* ---- several GPUs of a node from ONE host process -------------------------------------
 * The object owns a grid + plan per device and -- when the devices are distinct -- an in-process RCCL
 * communicator (ncclCommInitAll; librccl is dlopen'ed on first use).  vrt_multi_execute is vrt_plan_execute for
 * the node: the angle x wavelength loop of J_λ_voronoi (src/lambda_iteration.jl:84-111) sharded
 *   by wavelength blocks when nlam >= devices (51 over 8 -> 7,7,7,6,6,6,6,6; every device owns whole rows of J,
 *   which go home by strided copies: no exchange), or
 *   by angles otherwise (ups and downs dealt separately), the partial J's summed by ONE RCCL all-reduce.
 * Arguments as vrt_grid_create + vrt_plan_create_ex / vrt_plan_execute (host pointers; alpha_mode 0..2).
 * The same device listed twice is a rehearsal on a one-GPU box: no RCCL, the partial sums are added by a
 * kernel.  vrt_multi_set_shard: "auto" | "lambda" | "angle"; vrt_multi_last_shard: 1 lambda, 2 angle. */
typedef struct vrt_multi vrt_multi;
int vrt_multi_create(int n_devices, const int *devices, int64_t n, const double *pos_zxy, const int64_t *nbr, int64_t D1,
                     const double bounds[6], int64_t n_angles, const double *k, const int *dirs, int n_sweeps,
                     vrt_multi **out);
int vrt_multi_execute(vrt_multi *m, int64_t nlam, int64_t ld, const double *S, const double *alpha, int alpha_mode,
                      const double *I0_up, const double *I0_down, const double *weights, double *J);
int vrt_multi_set_shard(vrt_multi *m, const char *mode);
int vrt_multi_last_shard(const vrt_multi *m);
int vrt_multi_uses_rccl(const vrt_multi *m);
void vrt_multi_destroy(vrt_multi *m);
/* vrt_plan_execute_line for the node (the body of J_λ_voronoi, line method, src/lambda_iteration.jl:72-111, from host
 * arrays): the wavelengths go to the devices in contiguous blocks, every device makes the per-angle α_tot of ITS
 * wavelengths itself (it never exists on the host and never crosses PCIe) and owns whole rows J[l, :]: no exchange.
 * Arguments as vrt_plan_execute_line. */
int vrt_multi_execute_line(vrt_multi *m, int64_t nlam, int64_t ld, const double *lambda, double lambda0, double c0,
                           const double *velocity, const double *doppler_width, const double *gamma,
                           const double *line_strength, const double *alpha_cont, const double *S, const double *I0_up,
                           const double *I0_down, const double *weights, double *J);
/* The Λ-iteration session of vrt_lambda_* across the devices of a vrt_multi (BASELINE configs[3];
 * src/lambda_iteration.jl:205-300).  Every device owns a contiguous block of the wavelengths and a copy of the per-site
 * state; per iteration it runs, for its wavelengths, the line terms, α_tot of every angle, the sweep, S_new with its
 * share of the convergence maximum, and its share of the six λ-integrals of the radiative rates (src/rates.jl:154-201,
 * regrouped per wavelength: Σ_l W_l f_l).  The shares are summed by ONE RCCL all-reduce of 6 n doubles -- J never
 * travels -- and every device solves the statistical equilibrium of every site itself
 * (src/populations.jl:191-221).  Results equal the one-device session's to the rounding of that regrouping (1e-12).
 * vrt_multi_lambda_get assembles J and S_new (n, nlam) from the devices' blocks; populations (n, 3), R (3, 3, n) and γ [n]
 * come from the first device.  LIFETIME: a session uses its vrt_multi in every call but vrt_multi_lambda_destroy --
 * destroy the session FIRST; vrt_multi_lambda_iterate / _get on a session whose vrt_multi is gone are undefined. */
typedef struct vrt_multi_lambda vrt_multi_lambda;
int vrt_multi_lambda_create(vrt_multi *m, const vrt_line_case *lc, const double *weights, vrt_multi_lambda **out);
int vrt_multi_lambda_iterate(vrt_multi_lambda *s, double *max_rel_change);
int vrt_multi_lambda_get(vrt_multi_lambda *s, double *J, double *S, double *populations, double *R, double *gamma);
void vrt_multi_lambda_destroy(vrt_multi_lambda *s);
/* The same session with FLOAT storage, as vrt_lambda_create_f32 is to vrt_lambda_create.  Every device keeps S and J of
 * ITS wavelength block in both sweep orders, B_0 of the block in the up order (rounded once), I_0 and the native α as
 * float; the staged double B_0 is freed, so that after create no device holds a double array of size nλ_block·n or
 * nλ_block·n·angles.  An iterate of a device: the line terms, the float opacity prologue at its wavelength offset,
 * vrt_plan_execute_native_dev_f32, vrt_lambda_update_native_dev_f32 and vrt_rate_shares_native_dev_f32 on its block; the
 * all-reduce of 6 n doubles and the statistical equilibrium are those of the double session.  Every wavelength is solved by
 * exactly one device and a solve does not see the other wavelengths of its block: J and S of an iterate equal the
 * one-device float session's on the same populations bit for bit; the populations differ from its by the 1e-12 regrouping.
 * VRT_EINVAL when ANY device's plan is not on the patch path or with VRT_LAMBDA_NATIVE=0: there is no fp64 fallback.
 * vrt_multi_lambda_get returns J and S as doubles holding exactly the float values; vrt_multi_lambda_set_state validates
 * as for a double session, then rounds S to float; vrt_multi_lambda_set_acceleration (voronoirt_multi_accel.h) returns
 * VRT_EINVAL on a float session and changes nothing.  vrt_multi_lambda_storage: 8 or 4 (VRT_EINVAL for NULL). */
int vrt_multi_lambda_create_f32(vrt_multi *m, const vrt_line_case *lc, const double *weights, vrt_multi_lambda **out);
int vrt_multi_lambda_storage(const vrt_multi_lambda *s);

/* ---- rates + populations of the Λ-iteration epilogue on the device --------
 * calculate_R (src/rates.jl:154-201: Rij / Rji λ-trapezoids :226-364, σij with the site's static
 * Voigt profile :374-416, Gij :459-476) and get_revised_populations (src/populations.jl:191-221,
 * the per-site 2 x 2 solve) for the reference's 2-level + continuum atom, from J in place:
 *   R_ij = Σ_l pref_ij ((λ_l σ_l J_l + λ_l+1 σ_l+1 J_l+1)(λ_l+1 - λ_l))
 *   R_ji = Σ_l pref_ji ((σ_l G_l λ_l (P_l + J_l) + σ_l+1 G_l+1 λ_l+1 (P_l+1 + J_l+1))(λ_l+1 - λ_l))
 *   G_l = LTE[i]/LTE[j] exp(-hc_over_kB/(λ_l T)),  P_l = planck2[l] = 2 h c0²/λ_l⁵ in J's unit
 * pref_ij / pref_ji = 2π/(h c0) times the unit factors the reference gets from Unitful (and its
 * explicit /1000 in Rij, rates.jl:237,263).  blocks = [lo, hi) (0-based) of the bound-bound, level-1
 * bound-free and level-2 bound-free wavelength blocks (line.λidx).  Host: lambda[nlam],
 * planck2[nlam], sigma_bf1 / sigma_bf2 (σic per wavelength of the block).  Device: J (nlam, n) with
 * leading dimension ld, doppler_width[n], gamma[n], temperature[n], lte_populations (n, 3),
 * C (3, 3, n) collisional rates, atom_density[n]; out: R (3, 3, n), populations (n, 3). */
int vrt_rates_populations_dev(vrt_grid *g, int64_t nlam, int64_t ld, const double *lambda,
                              const int64_t blocks[6], const double *dJ, const double *planck2,
                              double lambda0, double c0, const double *d_doppler_width, const double *d_gamma,
                              double sigma_bb_const, const double *sigma_bf1, const double *sigma_bf2,
                              const double *d_temperature, const double *d_lte_populations, double hc_over_kB,
                              double pref_ij, double pref_ji, const double *d_C, const double *d_atom_density,
                              double *d_R, double *d_populations, void *stream);

/* ---- regular-grid short characteristics ---------------------------------
 * Drop-in bodies for short_characteristics_up / short_characteristics_down
 * (src/characteristics.jl:19-95, :110-180), batched over independent solves the way
 * J_λ_regular loops over angles and wavelengths (src/lambda_iteration.jl:1-58).
 *   z[nz], x[nx], y[ny]   grid axes (x, y carry the reference's one-cell periodic ghost border)
 *   k (3, n_solve), up[n_solve] (1: rays travel up, boundary at z[1]; 0: down, boundary at z[end])
 *   S, alpha (nz, nx, ny[, n_solve]) Julia order a[iz + nz*(ix + nx*iy)]; stride 0 = shared by all
 *   solves, nz*nx*ny = one array per solve
 *   I0 (nx, ny, n_solve), I_out (nz, nx, ny, n_solve)
 * Host pointers; the arrays are staged through the device. */
int vrt_short_characteristics(int64_t nz, int64_t nx, int64_t ny, const double *z, const double *x,
                              const double *y, int64_t n_solve, const double *k, const int *up,
                              const double *S, int64_t S_stride, const double *alpha,
                              int64_t alpha_stride, const double *I0, int n_sweeps, int device,
                              double *I_out);

/* Device-resident form: a handle owns the grid axes and the workspaces; dS, dalpha, dI0, dI_out are
 * device pointers in the layouts above, k and up stay on the host; asynchronous on `stream`.
 * field_period > 0: solve s reads the S / alpha array number s % field_period (solves ordered
 * direction-major with the wavelength fastest share one array per wavelength); 0: array s.
 * vrt_regular_last_solve_ms: HIP-event time of the last execute's solve kernel(s) (synchronise first).
 * A handle serves one caller at a time (its workspaces are reused by every execute).
 * A batch in which every ray cuts the horizontal plane first on every plane (steep rays: xy_up_ray / xy_down_ray
 * only, src/characteristics.jl:72, :191-372) runs as a chip-wide coefficient kernel + one light march per solve,
 * with 3 doubles per point, plane and solve of extra workspace (chunks of at most 2 GiB); results are bit-identical
 * to the single kernel's.  Environment, read at vrt_regular_create (diagnostics and tests): VRT_REG_XY = 0 keeps the
 * single kernel for such batches, 2 reads the upwind plane back from memory instead of LDS; VRT_REG_THREADS forces
 * the workgroup size. */
typedef struct vrt_regular vrt_regular;
int vrt_regular_create(int64_t nz, int64_t nx, int64_t ny, const double *z, const double *x,
                       const double *y, int device, vrt_regular **out);
void vrt_regular_destroy(vrt_regular *r);
int vrt_regular_execute_dev(vrt_regular *r, int64_t n_solve, const double *k, const int *up,
                            const double *dS, int64_t S_stride, const double *dalpha,
                            int64_t alpha_stride, int64_t field_period, const double *dI0,
                            int n_sweeps, double *dI_out, void *stream);
int vrt_regular_last_solve_ms(const vrt_regular *r, double *ms);

/* What the last batch of solves on r was launched as (read-only host bookkeeping; any entry that solves on r sets it,
 * the Λ-iteration sessions included; before the first solve: VRT_EINVAL).  *form = one of the kernels below; for the
 * two k_regular_solve forms OR-ed with the row flags: set where the rows of a yz plane (ny - 2 points) / of an xz plane
 * (nx - 2 points) fit one point per thread and take the pipelined row march, clear where they take the strided row
 * loop.  *threads = the workgroup size of that kernel. */
enum {
    VRT_REG_FORM_SOLVE256 = 0,          /* k_regular_solve<256>: one workgroup walks all planes of a solve */
    VRT_REG_FORM_SOLVE1024 = 1,         /* k_regular_solve<1024> */
    VRT_REG_FORM_XY_MARCH_LDS1 = 2,     /* all-xy batch: k_reg_xy_coefs + k_reg_xy_march_lds<1> (points per thread) */
    VRT_REG_FORM_XY_MARCH_LDS2 = 3,     /* ... <2> */
    VRT_REG_FORM_XY_MARCH_LDS4 = 4,     /* ... <4> */
    VRT_REG_FORM_XY_MARCH_LDS0 = 5,     /* ... <0>: any number of points per thread, coefficients loaded where used */
    VRT_REG_FORM_XY_MARCH_MEM = 6,      /* k_reg_xy_coefs + k_reg_xy_march_mem: upwind plane read back from memory */
    VRT_REG_FORM_KERNEL_MASK = 0xff,
    VRT_REG_FORM_YZ_ROW_MARCH = 0x100,
    VRT_REG_FORM_XZ_ROW_MARCH = 0x200
};
int vrt_regular_last_launch_form(const vrt_regular *r, int *form, int *threads);

/* ---- the line Λ-iteration on the regular grid (J_λ_regular, Λ_regular: src/lambda_iteration.jl:1-58, :116-205) ----
 * The regular half of the reference's comparison, the twin of vrt_plan_execute_line / vrt_lambda_* on a vrt_regular r.
 * Points are all nz nx ny points of r, the periodic ghost border included, in Julia order i = iz + nz (ix + nx iy); the
 * arrays are laid out as vrt_line_case's with n = nz nx ny: S, J, B_0 (nlam, n), populations (n, 3), R (3, 3, n).
 * Directions: k (3, n_angles) unit vectors (z, x, y), dirs[a] = 1 for an up solve (θ > 90), -1 for a down solve
 * (θ < 90), 0 for an angle that adds nothing (θ = 90; its k is not checked), weights[n_angles].
 *
 * vrt_regular_execute_line: J = Σ_a w_a I_a of every (angle, wavelength) solve from host arrays: per angle α_tot =
 *   line_strength H(a, v) / (√π ΔλD) + alpha_cont with v_los = dot(velocity, -k), as vrt_line_opacity_dev, made on
 *   the device; the up solves start from I0_up (nx, ny, nlam), element [ix + nx (iy + ny l)]: one bottom plane per
 *   wavelength, the layout of vrt_short_characteristics' I0 (NULL: zeros); the down solves start from zeros.
 * vrt_regular_lambda_create / _iterate / _get / _destroy: Λ_regular's loop with the contract of vrt_lambda_*: create
 *   uploads the line case and starts in LTE with S = B_0; one iterate is γ and the line strength of the current
 *   populations -> α_tot of every angle -> J (I_0 of the up solves: B_0's bottom plane) -> S_new = (1 - ε) J + ε B_0
 *   and max |1 - S_old/S_new| (NaN propagates) -> R -> populations; get returns what is asked for (any pointer may be
 *   NULL; before the first iterate J, R and gamma are zeros).  The session borrows r, which must outlive it; r serves
 *   one caller at a time.
 * The solves go through in chunks whose workspace (α_tot, I, coefficients) stays under a byte cap (64 GiB;
 * VRT_REG_LAMBDA_BYTES, read at vrt_regular_create); J is bit-identical for any chunking.  The workspace lives on r
 * until vrt_regular_execute_line returns or the session is destroyed.
 * vrt_regular_last_solve_ms times vrt_regular_execute_dev and vrt_regular_emergent_dev only: after these entries it
 * answers VRT_EINVAL until the next of those.  Every argument is checked before the device is touched (NULL,
 * n_angles < 1, dirs outside {-1, 0, 1}, |k| != 1 or k_z = 0 where dirs != 0, nlam < 1 (the session: < 2, and its
 * wavelength blocks), n_sweeps < 1: VRT_EINVAL). */
typedef struct vrt_regular_lambda vrt_regular_lambda;
int vrt_regular_execute_line(vrt_regular *r, int64_t n_angles, const double *k, const int *dirs, const double *weights,
                             int64_t nlam, const double *lambda, double lambda0, double c0, const double *velocity,
                             const double *doppler_width, const double *gamma, const double *line_strength,
                             const double *alpha_cont, const double *S, const double *I0_up, int n_sweeps, double *J);
int vrt_regular_lambda_create(vrt_regular *r, int64_t n_angles, const double *k, const int *dirs, const double *weights,
                              const vrt_line_case *lc, int n_sweeps, vrt_regular_lambda **out);
int vrt_regular_lambda_iterate(vrt_regular_lambda *s, double *max_rel_change);
int vrt_regular_lambda_get(vrt_regular_lambda *s, double *J, double *S, double *populations, double *R, double *gamma);
void vrt_regular_lambda_destroy(vrt_regular_lambda *s);

/* ---- Ng acceleration of the Λ-iteration (Ng 1974, J. Chem. Phys. 61, 2680; Olson, Auer & Buchler 1986, JQSRT 35, 431) ----
 * Plain Λ-iteration converges like 1 - ε.  The second-order Ng step extrapolates from the last four iterates x0 (newest)
 * .. x3 of S along the two slowest error modes; it needs no approximate operator and changes no sweep kernel.  Per element
 *   w = 1/x0,  q1 = (x0 - 2 x1) + x2,  q2 = ((x0 - x1) - x2) + x3,  q3 = x0 - x1
 *   A1 = Σ (w q1) q1,  B1 = Σ (w q1) q2,  C1 = Σ (w q1) q3,  B2 = Σ (w q2) q2,  C2 = Σ (w q2) q3
 *   det = A1 B2 - B1 B1,  a = (C1 B2 - C2 B1)/det,  b = (C2 A1 - C1 B1)/det,  c = (1 - a) - b      (host, double)
 *   x_acc = (c x0 + a x1) + b x2
 * in exactly this order of operations.  The sums are formed without floating-point atomics in a fixed order: the same
 * count gives the same bits run after run.  A step is REJECTED, all or nothing, when a sum or det is not finite, det == 0,
 * or any x_acc is not finite or not > 0 (a source function stays positive: the criterion divides by it).
 *
 * vrt_ng_accelerate_dev, standalone: device pointers on the current HIP device; synchronises `stream`; d_out aliases no
 * input.  sums[5] = A1 B1 C1 B2 C2, coeffs[2] = a b, *applied = 1, or 0 when rejected (d_out then unspecified). */
int vrt_ng_accelerate_dev(int64_t count, const double *d_x0, const double *d_x1, const double *d_x2,
                          const double *d_x3, double *d_out, double sums[5], double coeffs[2], int *applied,
                          void *stream);
/* The pieces of that call, for a caller that holds S in several arrays (blocks of one device, one block per device or
 * per process): vrt_ng_sums_dev on every piece, the five sums added piece by piece in one fixed order, vrt_ng_coefficients
 * once, vrt_ng_apply_dev on every piece, and the step taken only if every piece reports good.
 * vrt_ng_sums_dev: the five sums over `count` elements -- for the same arrays the same bits as vrt_ng_accelerate_dev's.
 * vrt_ng_coefficients (host only): det, a, b as above into coeffs[2]; returns 1, or 0 with coeffs untouched when a sum or
 *   det is not finite or det == 0 (VRT_EINVAL for a NULL argument).
 * vrt_ng_apply_dev: d_out = x_acc for the given a, b; *good = 1, or 0 when any x_acc is not finite or not > 0 (d_out then
 *   unspecified).  d_out aliases no input.  Both *_dev calls work on the current HIP device and synchronise `stream`. */
int vrt_ng_sums_dev(int64_t count, const double *d_x0, const double *d_x1, const double *d_x2, const double *d_x3,
                    double sums[5], void *stream);
int vrt_ng_coefficients(const double sums[5], double coeffs[2]);
int vrt_ng_apply_dev(int64_t count, double a, double b, const double *d_x0, const double *d_x1, const double *d_x2,
                     double *d_out, int *good, void *stream);
/* The single-device sessions: order 0 = off (default), 2 = the step above.  The first step is due after iterate number
 * `start` (>= 4), the next ones after every `period` further iterates (>= 4, so that an extrapolated S never enters a
 * history).  Anything else: VRT_EINVAL; with order 0, start and period are ignored.  Callable between any two iterates (a
 * due iterate whose three predecessors were not all recorded takes no step); order 0 frees the history.
 * vrt_*_iterate returns what it returns without acceleration -- max |1 - S_old/S_new| of the PLAIN update, formed before
 * any extrapolation; after an accepted step the S the session holds (what the next iterate solves with, what *_get
 * returns) is x_acc.  Populations, R, γ and J are not extrapolated: the next iterate recomputes them from its J.  Only
 * S of the three iterates before a due one is copied (three extra S arrays while acceleration is on; none when off, and
 * a session that never asks for acceleration runs exactly what it ran before).  The Voronoi session forms the sums over
 * the n nlam physical entries of its up-order copy of S and applies the same a, b to both sweep-order copies.
 * vrt_multi_lambda_* has NO acceleration entry in this file: its S is split over the devices, and the two entries that take
 * the step over the members' blocks (vrt_multi_lambda_set_acceleration, vrt_multi_lambda_last_acceleration) stand with their
 * contract in voronoirt_multi_accel.h, which this header includes at its end; the companion library
 * libvrt_hip_multi_accel.so exports them (libvrt_hip.so exports what THIS file declares).  A caller that holds S in
 * pieces of its own has the three pieces of the step above (vrt_ng_sums_dev, vrt_ng_coefficients, vrt_ng_apply_dev). */
int vrt_lambda_set_acceleration(vrt_lambda *s, int order, int start, int period);
int vrt_regular_lambda_set_acceleration(vrt_regular_lambda *s, int order, int start, int period);
/* what the LAST iterate did: *applied = 1 taken, 0 none due, -1 due but rejected; sums / coeffs (either may be NULL)
 * valid unless 0 */
int vrt_lambda_last_acceleration(const vrt_lambda *s, int *applied, double sums[5], double coeffs[2]);
int vrt_regular_lambda_last_acceleration(const vrt_regular_lambda *s, int *applied, double sums[5],
                                         double coeffs[2]);

/* ---- resuming a line session from saved S and populations (src/recover_simulation.jl: recover_voronoi, recover_regular) ----
 * The reference writes populations and S_new after every pass (src/lambda_iteration.jl:280-281) and reads the two back to
 * carry on.  They are the complete state of a line session: every iterate begins by recomputing γ and the line strength
 * from the current populations and reads S from where the last update wrote it; everything else is a constant of the case.
 * vrt_*_lambda_set_state replaces that state by host arrays with the dims the matching *_get writes: S (nlam, n),
 * populations (n, 3); for the regular session n = nz nx ny, ghost border included.  Either pointer may be NULL: that part
 * of the state stays as it is; both NULL is VRT_EINVAL.  S must be finite and > 0 everywhere (the rule of
 * vrt_continuum_set_source), the populations finite and >= 0: both are checked on the host before the device is touched
 * (VRT_EINVAL).  On any failure, an allocation failure included, the session is untouched -- its next iterate is the one it
 * would have run anyway: the new state is built in device copies beside the session and moved in once they are complete.
 * The call returns after its copies have completed (the host arrays may go).
 * Afterwards the session continues exactly as one that had reached this state by iterating: with acceleration off, a fresh
 * session given the *_get output of another session after k iterates returns, from its first iterate on, the scalar, J, S,
 * populations, R and γ of the other's iterates k+1, k+2, ... bit for bit.  J, R and γ as *_get returns them are NOT
 * changed by this call: they stay those of the last iterate THIS session ran (zeros before its first).  A recorded Ng
 * history is dropped as vrt_continuum_set_source drops it (a step that falls due before three further iterates are
 * recorded is not taken; *_last_acceleration reports 0 until the next iterate); the acceleration settings and the
 * iterate counter stay.  The state *_get returns right after an accepted Ng step is the extrapolated S in both sweep-order
 * copies, and resumes like any other.  vrt_lambda_set_state takes the plan's lock as vrt_lambda_iterate does;
 * vrt_multi_lambda_set_state gives every device the columns of its wavelength block of S and a full copy of the
 * populations.  A session that never calls these entries allocates and runs nothing extra. */
int vrt_lambda_set_state(vrt_lambda *s, const double *S, const double *populations);
int vrt_regular_lambda_set_state(vrt_regular_lambda *s, const double *S, const double *populations);
int vrt_multi_lambda_set_state(vrt_multi_lambda *s, const double *S, const double *populations);

/* ---- the continuum scattering Λ-iteration on both grids (src/lambda_continuum.jl) --------------------------------------
 * Λ_voronoi (:109-160) and Λ_regular (:58-107), the loop of the reference's production run (src/compare_continuum.jl), with
 * library-owned device state: coherent scattering at nlam independent wavelengths (the reference: one, 500 nm), α_cont
 * fixed over the iterations.  One iterate is one pass of the loop body (:145-150; :92-97 on the regular grid):
 *   J = Σ_a w_a I_a(S_old)   J_λ_voronoi :27-56 / J_λ_regular :1-24.  I_0 of the up solves is B_0 -- not S -- of the bottom
 *                            layer perm_up[1 : layers_up[2] - 1] per wavelength (:45-47), on the regular grid B_0's bottom
 *                            plane (:16); the down solves start from zeros (:51, :19); θ = 90 adds nothing
 *   S_new = (1 - ε) J + ε B_0   at EVERY entry (:148, :95), ε per (point, wavelength); operations and their order as
 *                            vrt_lambda_update_dev
 *   *max_rel_change = max |1 - S_old/S_new| over the THICK entries, ε > eps_thick (strict; thick = ε_λ .> 1e-4, :133, :80;
 *                            criterion :162-198).  A NaN at a thick entry makes it NaN; a NaN at a thin entry is not seen
 *                            (Julia indexes before it takes the maximum, :169, :188).  The first iterate compares with S = B_0.
 * vrt_continuum_case: host arrays (nlam, n) Julia dims as vrt_line_case's B0, element [l + nlam * site]; n = the grid's
 *   sites, or all nz nx ny points of a vrt_regular (ghost border included, Julia order i = iz + nz (ix + nx iy)).
 *   vrt_continuum_case_check answers what create would say about the arrays, for n points, without any handle or device:
 *   VRT_EINVAL for NULL pointers, nlam < 1, eps_thick not finite, α not finite or <= 0, ε outside [0, 1] or not finite,
 *   B0 not finite, and for a case without a single thick entry (the reference's maximum over an empty set throws).
 * vrt_continuum_create (p: a plan of the quadrature, weights[n_angles]) / vrt_regular_continuum_create (directions as
 *   vrt_regular_lambda_create, whose direction checks apply; n_sweeps >= 1): upload the case, S = B_0.  Every argument is
 *   checked before the device is touched.  The Voronoi session keeps S, J, B_0, ε and α in SWEEP ORDER
 *   (vrt_plan_to_native_dev once at create, then vrt_plan_execute_native_dev with VRT_ALPHA_SITE_LAM_NATIVE and a masked
 *   update on the plane sets per iterate: no layout change inside the loop); with VRT_LAMBDA_NATIVE=0, or on a plan
 *   without a sweep-order form, it keeps the caller's layout (vrt_plan_execute_dev + vrt_continuum_update_dev's kernel).
 *   Both give the same S, J and scalar bit for bit.  The regular session runs the chunked solves of vrt_regular_lambda_*
 *   (VRT_REG_LAMBDA_BYTES) with ONE α array per wavelength shared by all angles; J is bit-identical for any chunking.
 *   The sessions borrow p / r, which must outlive them.
 * _get: J and S (nlam, n) of the last iterate, either may be NULL; before the first iterate J is zeros and S is B_0.
 * _set_source: replaces S by a host array (nlam, n) -- a warm start, or the resume of a run of which only S was kept
 *   (the recover_* use of src/recover_simulation.jl).  An S that is not finite or not > 0 somewhere: VRT_EINVAL, the
 *   session untouched.  Drops any recorded Ng history; afterwards the session continues exactly as one that had reached
 *   that S by iterating.
 * _set_acceleration / _last_acceleration: the contract of vrt_lambda_set_acceleration above (order 0 or 2, start and
 *   period >= 4, a step all or nothing with the positivity verdict, the returned scalar that of the plain update); the
 *   sums run over all n nlam physical entries, thin ones included.  A session that never asks allocates and runs nothing
 *   extra.
 * vrt_continuum_update_dev: the masked update alone for a caller with its own device arrays on g's device: J, B, eps,
 *   S_old, S_new (nlam, n) with leading dimension ld (eps per entry, unlike vrt_lambda_update_dev's eps[n]); S_new may
 *   alias neither S_old nor J.  *n_thick (may be NULL) = the number of entries with eps > eps_thick; none: the scalar is
 *   0.  Synchronises `stream`.
 * There is NO multi-device continuum session: vrt_multi_lambda_* splits wavelength blocks over the devices, and the one
 * wavelength of a continuum run cannot be split that way.
 *
 * Accelerated Λ-iteration (ALI) with a diagonal approximate operator (Olson, Auer & Buchler 1986), on both grids.
 * Plain Λ-iteration converges like 1 - ε because in thick cells most of J at a site is the site's own S coming straight
 * back; the local operator Λ* is that part, and the update solves for it instead of lagging behind it.  Ng acceleration
 * (above) needs no approximate operator; this is the scheme that has one, and the two compose.
 * vrt_plan_lambda_diagonal_dev: Λ* of a plan and an α in the VRT_ALPHA_SITE_LAM layout (n, ld), into d_diag (n, ld):
 *     Λ*[i,l] = Σ_a weights[a] · upd(a,i) · ( (w_1 b(Δτ_1)) + (w_2 b(Δτ_2)) )
 *     Δτ_r    = r_r (α[i,l] + α[up_r,l]) / 2            (trapezoidal, as the sweep)
 *     b       = third coefficient of linear_weights: Δτ < 5e-4: Δτ (1/2 - Δτ/6); Δτ > 50: 1 - 1/Δτ; else 1 - a - e
 *   the coefficient of S[i] in the last Gauss-Seidel visit I[i] = Σ_r w_r (e_r I[up_r] + a_r S[up_r] + b_r S[i]), summed
 *   over the plan's angles in quadrature order (θ = 90 angles are skipped); up_r, w_r, r_r are the entries
 *   vrt_plan_get_upwind returns for that angle.  upd(a,i) is 1 where the sweep of angle a updates site i and 0 at the
 *   sites of layer 1 of the angle's direction (their I is I_0, independent of S) and at the never-visited site perm[n] of
 *   that direction.  A slot 2 that duplicates slot 1 has w_2 = 0 and adds nothing.  Angles in order, slot 1 then slot 2,
 *   no floating-point atomics: the same inputs give the same bits.  0 <= Λ* <= the true diagonal Λ_ii (every coefficient
 *   of Λ is >= 0).  weights_host[n_angles] on the host; asynchronous on `stream`; the padding columns of d_diag are not
 *   written.  vrt_plan_lambda_diagonal: the same from host arrays, which also checks that α is finite and > 0.
 *   Both check NULL pointers, nlam >= 1 and ld >= nlam before the device is touched.
 * vrt_continuum_ali_update_dev: the contract of vrt_continuum_update_dev with d_diag (nlam, n; leading dimension ld) = Λ*;
 *   per entry, with t = 1 - ε:
 *     num = t (J - Λ* S_old) + ε B0,    den = 1 - t Λ*,    S_new = num / den
 *   which is S_old + (S_fs - S_old) / den with S_fs the plain update, written so that num >= 0.  The criterion is
 *   unchanged in kind: max |1 - S_old/S_new| over the entries with ε > eps_thick, the same NaN rule and thick count.
 * vrt_continuum_set_operator: op 0 = plain Λ-iteration (the default), 1 = the diagonal operator, anything else VRT_EINVAL;
 *   callable between any two iterates.  Turning it on computes Λ* from the session's α and weights, once (and, in the
 *   sweep-order session, its up-order plane set), then reduces min den on the device: if that is not > 0 -- only for
 *   ε = 0 where Λ* rounds to 1 -- VRT_EINVAL, the session untouched.  Turning it off frees Λ*.  A change of the operator
 *   drops any recorded Ng history, as _set_source does; _set_source keeps the operator.  With Ng on, the step runs on the
 *   S the ALI update produced, and the returned scalar is that of the ALI update, formed before any extrapolation.  Both
 *   layouts give the same S, J and scalar bit for bit.  A session that never calls it allocates and runs nothing extra.
 * vrt_continuum_get_operator: *op, and -- when on and diag is not NULL -- Λ* (nlam, n) Julia dims.
 * The raster: vrt_regular_lambda_diagonal_dev / vrt_regular_lambda_diagonal / vrt_regular_continuum_select_operator /
 * _get_operator are the same four entries on a vrt_regular (directions, dirs and weights per angle as
 * vrt_regular_continuum_create, whose direction checks apply; alpha and diag (nlam, n) Julia dims over all nz nx ny
 * points, leading dimension ld).  There
 *     Λ*[p,l] = Σ_a weights[a] · c_a(p,l),    c_a = the coefficient of S[p] in I_a[p] after ONE sweep of the raster solve
 *   summed over the angles in quadrature order (dirs = 0 skipped), from the reference's arithmetic (bilinear, linear_weights)
 *   with Δτ = r (α_c + α_u) / 2, the cut argmin(r_z, r_x, r_y) and the interpolation indices exactly as
 *   vrt_regular_execute_dev forms them for the point's plane:
 *     xy plane:                  c = b(Δτ)          (S_u and I_u come from the upwind plane)
 *     yz plane, xz plane (up):   c = b(Δτ) + e(Δτ) · v · a(Δτ_q) · u      the second term is the point's S coming back through
 *                                the row marched just before it, q: u the weight of the point in q's interpolated S_u, v that
 *                                of q in the point's I_u (the carried row); 0 in the first row of the march
 *     xz plane (down):           c = e(Δτ) · v · a(Δτ_q) · u              xz_down_ray reads its centre S and α from the plane
 *                                above, so the point's own S has no b term there
 *   c_a = 0 on the boundary plane of the angle's direction (iz = 0 up, iz = nz - 1 down: I is I_0) and at every ghost point
 *   (ix = 0, nx - 1 or iy = 0, ny - 1: I there is a copy of an interior point's I), so Λ* is exactly 0 on the ghost border.
 *   This is the diagonal of the one-sweep Λ: it does not depend on n_sweeps, and 0 <= Λ* <= the diagonal for any number of
 *   sweeps.  More than 64 active angles: VRT_EINVAL.  The same inputs give the same bits.  The _dev form runs on the null
 *   stream and returns when Λ* is written; padding columns are neither read nor written.  The host form also checks that α
 *   is finite and > 0.  Both check NULL pointers, nlam >= 1, ld >= nlam and the directions before the device is touched.
 *   vrt_regular_continuum_select_operator / _get_operator: the contract of the Voronoi entries (Λ* from the session's α, min
 *   den checked before anything is moved in, a change drops the Ng history, _set_source keeps the operator, a session that
 *   never calls it allocates and runs nothing extra); the update is vrt_continuum_ali_update_dev's kernel.
 *   The setter is named _select_operator here, not _set_operator.
 * Out of scope: the regular-grid continuum session with the exact diagonal of its n_sweeps-sweep operator (its Λ* is the
 * one-sweep diagonal, a lower bound of it), the line sessions other than the Voronoi one on one device with double
 * storage (that one has its own operator entries, below: vrt_lambda_use_operator), and any multi-device form. */
typedef struct vrt_continuum vrt_continuum;
typedef struct vrt_regular_continuum vrt_regular_continuum;
typedef struct vrt_continuum_case {
    int64_t nlam;          /* >= 1; the reference uses 1 (500 nm).  Wavelengths are independent (coherent scattering) */
    const double *alpha;   /* (nlam, n) α_cont = α_s + α_a (:128), fixed over the iterations; finite, > 0 */
    const double *eps;     /* (nlam, n) ε = α_a / α_cont (:131) */
    const double *B0;      /* (nlam, n) Planck function (:136); S starts as B0 */
    double eps_thick;      /* the criterion sees only entries with eps > eps_thick (strict; the reference: 1e-4) */
} vrt_continuum_case;
int vrt_continuum_case_check(const vrt_continuum_case *cc, int64_t n);
int vrt_continuum_create(vrt_plan *p, const vrt_continuum_case *cc, const double *weights, vrt_continuum **out);
int vrt_continuum_iterate(vrt_continuum *s, double *max_rel_change);
int vrt_continuum_get(vrt_continuum *s, double *J, double *S);
int vrt_continuum_set_source(vrt_continuum *s, const double *S);
int vrt_continuum_set_acceleration(vrt_continuum *s, int order, int start, int period);
int vrt_continuum_last_acceleration(const vrt_continuum *s, int *applied, double sums[5], double coeffs[2]);
void vrt_continuum_destroy(vrt_continuum *s);
int vrt_regular_continuum_create(vrt_regular *r, int64_t n_angles, const double *k, const int *dirs,
                                 const double *weights, const vrt_continuum_case *cc, int n_sweeps,
                                 vrt_regular_continuum **out);
int vrt_regular_continuum_iterate(vrt_regular_continuum *s, double *max_rel_change);
int vrt_regular_continuum_get(vrt_regular_continuum *s, double *J, double *S);
/* The new S and its plane-major copy are staged beside the session and swapped in once both are complete: a failure
 * leaves the session as it was, at the price of two transient n·nλ arrays during the call. */
int vrt_regular_continuum_set_source(vrt_regular_continuum *s, const double *S);
int vrt_regular_continuum_set_acceleration(vrt_regular_continuum *s, int order, int start, int period);
int vrt_regular_continuum_last_acceleration(const vrt_regular_continuum *s, int *applied, double sums[5],
                                            double coeffs[2]);
void vrt_regular_continuum_destroy(vrt_regular_continuum *s);
int vrt_continuum_update_dev(vrt_grid *g, int64_t nlam, int64_t ld, const double *dJ, const double *dB,
                             const double *deps, double eps_thick, const double *dS_old, double *dS_new,
                             double *max_rel_change, int64_t *n_thick, void *stream);
int vrt_plan_lambda_diagonal_dev(vrt_plan *p, int64_t nlam, int64_t ld, const double *d_alpha,
                                 const double *weights_host, double *d_diag, void *stream);
int vrt_plan_lambda_diagonal(vrt_plan *p, int64_t nlam, int64_t ld, const double *alpha, const double *weights,
                             double *diag);
int vrt_continuum_ali_update_dev(vrt_grid *g, int64_t nlam, int64_t ld, const double *dJ, const double *dB,
                                 const double *deps, const double *d_diag, double eps_thick, const double *dS_old,
                                 double *dS_new, double *max_rel_change, int64_t *n_thick, void *stream);
int vrt_continuum_set_operator(vrt_continuum *s, int op);
int vrt_continuum_get_operator(vrt_continuum *s, int *op, double *diag /* (nlam, n) Julia dims, may be NULL */);
int vrt_regular_lambda_diagonal_dev(vrt_regular *r, int64_t n_angles, const double *k, const int *dirs,
                                    const double *weights, int64_t nlam, int64_t ld, const double *d_alpha,
                                    double *d_diag);
int vrt_regular_lambda_diagonal(vrt_regular *r, int64_t n_angles, const double *k, const int *dirs,
                                const double *weights, int64_t nlam, int64_t ld, const double *alpha, double *diag);
int vrt_regular_continuum_select_operator(vrt_regular_continuum *s, int op);
int vrt_regular_continuum_get_operator(vrt_regular_continuum *s, int *op,
                                       double *diag /* (nlam, n) Julia dims, may be NULL */);

/* ---- accelerated Λ-iteration of the LINE session on a Voronoi plan ---------------------------------------------------
 * The reference multiplies every collisional rate by BOOST = 2.0e9 "instead of developing operator splitting"
 * (src/rates.jl:1-3): with physical rates ε is 1e-4 ... 1e-6 at line centre and the plain loop does not converge in any
 * affordable number of iterates.  Here the line session takes the same diagonal operator as the continuum session.
 * In the line loop α_tot differs per angle (v_los = dot(velocity, -k)) and follows the populations, so Λ* is formed every
 * iterate from the α the sweep of that iterate reads:
 *     Λ*[i,l] = Σ_a w_a upd(a,i) (W_1(a,i) b(Δτ_1) + W_2(a,i) b(Δτ_2)),   Δτ_r = R_r(a,i) (α_a[i,l] + α_a[up_r(a,i),l]) / 2
 * upd, the tables, b, the angle order and the operation order are those of vrt_plan_lambda_diagonal_dev above; α_a is
 * angle a's block of the native per-angle buffer (VRT_ALPHA_ANGLE_NATIVE: vrt_line_opacity_dev,
 * vrt_plan_alpha_to_native_dev).  With one angle's weight alone the result is vrt_plan_lambda_diagonal_dev's bit for bit.
 * vrt_line_lambda_diagonal_dev: Λ* into d_diag, (nlam, n) with leading dimension ld, padding columns neither read nor
 *   written; any pair block of the plan, an odd nlam included; weights_host[n_angles]; asynchronous on `stream`; no
 *   floating-point atomics: the same inputs give the same bits.  VRT_EINVAL for NULL pointers, nlam < 1, ld < nlam
 *   (before the device is touched) and for a plan with an inactive (θ = 90) angle, as vrt_lambda_create.
 * vrt_lambda_ali_update_dev / vrt_lambda_ali_update_native_dev: the contracts of vrt_lambda_update_dev and
 *   vrt_lambda_update_native_dev with Λ* beside the other arrays (rows; the UP-order plane set of vrt_plan_to_native_dev).
 *   Per entry, with t = 1 - ε[site]:
 *     num = t (J - Λ* S_old) + ε B,    den = 1 - t Λ*,    S_new = num / den
 *   An entry whose den is not > 0 -- only ε = 0 in a cell whose Λ* rounds to 1 -- takes the plain update
 *   (1 - ε) J + ε B and is counted in *fallback_entries: any per-entry choice of a local operator leaves the fixed point
 *   where it is, and S is updated in place, so the update never refuses half way.  The criterion is unchanged:
 *   max |1 - S_old/S_new|, NaN -> NaN.
 * vrt_lambda_use_operator: op 0 = plain Λ-iteration (the default), 1 = the diagonal operator; callable between any two
 *   iterates.  On: one array of the size of S beside the session; every vrt_lambda_iterate then forms Λ* after the
 *   opacity, on the session's stream, and runs the ALI update; the fallback count comes home with the criterion's words.
 *   Rates and populations come from the iterate's J as before, Ng acceleration sees the ALI S as it sees the plain one.
 *   Λ* is a pure function of the populations and is kept over no iterate: vrt_lambda_set_state resumes an ALI run bit for
 *   bit with nothing more to save (select the operator in the new session).  Off: the array is freed.  A session that never
 *   calls it runs the launches it ran before.  VRT_EINVAL, nothing changed: NULL, op outside {0, 1}, a float-storage
 *   session (vrt_lambda_storage == 4).  (The setter is named _use_operator: the names _set_operator and _select_operator
 *   stay free on the line and multi-device sessions, as the host tests of the continuum operators require.)
 * vrt_lambda_get_operator: *op and -- may be NULL -- the fallback count of the last iterate.
 * Out of scope: the float-storage, the multi-device and the regular-grid line sessions. */
int vrt_line_lambda_diagonal_dev(vrt_plan *p, int64_t nlam, const double *d_alpha_native, const double *weights_host,
                                 int64_t ld, double *d_diag, void *stream);
int vrt_lambda_ali_update_dev(vrt_grid *g, int64_t nlam, int64_t ld, const double *dJ, const double *dB,
                              const double *deps, const double *d_diag, const double *dS_old, double *dS_new,
                              double *max_rel_change, int64_t *fallback_entries, void *stream);
int vrt_lambda_ali_update_native_dev(vrt_grid *g, int64_t nlam, const double *dJ_up, const double *dJ_down,
                                     const double *dB_up, const double *deps, const double *d_diag_up, double *dS_up,
                                     double *dS_down, double *max_rel_change, int64_t *fallback_entries, void *stream);
int vrt_lambda_use_operator(vrt_lambda *s, int op);
int vrt_lambda_get_operator(const vrt_lambda *s, int *op, int64_t *fallback_entries_last_iterate);

/* ---- accelerated Λ-iteration of the LINE session on a regular grid ----------------------------------------------------
 * The regular-grid line session (vrt_regular_lambda_*, the raster half of the reference's compare_line.jl) has these
 * entries of its own: the same diagonal operator, so that both halves of the comparison can run the same method.  Its Λ*
 * is the raster's one-sweep diagonal (vrt_regular_lambda_diagonal_dev above) with an α of its own per angle, formed every
 * iterate from the α_tot the solves of that iterate read:
 *     Λ*[p,l] = Σ_a weights[a] · c_a(p; α_a[l])
 * over the ACTIVE angles in quadrature order (dirs = 0 skipped and never read); c_a is exactly the per-angle coefficient of
 * vrt_regular_lambda_diagonal_dev (one function on the device serves both) taken with angle a's α planes of wavelength l.
 * Exactly 0 on the ghost border and on the angle's boundary plane.  With one α for every angle the result is
 * vrt_regular_lambda_diagonal's bit for bit, and with one angle active it is that entry's with that angle alone.  Any
 * number of active angles.  No atomics: the same inputs give the same bits.
 * vrt_regular_line_lambda_diagonal_dev: d_alpha_pl plane-major per ACTIVE angle in order, [a][l][iz][iy][ix]; d_diag_pl
 *   [l][iz][iy][ix], every element written; asynchronous work on `stream`, which is synchronised before return.
 * vrt_regular_line_lambda_diagonal: the same from host arrays.  alpha (nlam, n, n_angles) Julia dims -- C order
 *   (n_angles, n, ld) -- in Julia point order for every USER angle, the blocks of inactive angles are never read; diag
 *   (nlam, n) with leading dimension ld, padding columns neither read nor written.  Also checks that the α that is read is
 *   finite and > 0.
 *   Both check NULL pointers, nlam >= 1 (the host form: ld >= nlam) and the directions, as vrt_regular_lambda_diagonal[_dev]
 *   does, before the device is touched.
 * vrt_regular_lambda_use_operator: op 0 = plain Λ-iteration (the default), 1 = the diagonal operator; callable between any
 *   two iterates.  On: two arrays of the size of S beside the session (Λ* plane-major as the solves' chunks leave it, and as
 *   rows for the update).  Every vrt_regular_lambda_iterate then zeroes the planes, forms Λ* chunk by chunk right after the
 *   chunk's opacity while that α stands in the workspace (bit-identical for any VRT_REG_LAMBDA_BYTES), and runs the update of
 *   vrt_lambda_ali_update_dev -- the fallback rule and count included, which come home with the criterion's words.  Rates
 *   and populations come from the iterate's J as before; Ng acceleration sees the ALI S; a change of the operator drops any
 *   recorded Ng history.  Nothing of Λ* survives an iterate: vrt_regular_lambda_set_state resumes an ALI run bit for bit
 *   (select the operator in the new session).  Off: both arrays are freed and the session runs as one that never called
 *   this.  VRT_EINVAL, nothing changed: NULL, op outside {0, 1}.  (Named _use_operator as on the Voronoi line session.)
 * vrt_regular_lambda_get_operator: *op and -- may be NULL -- the fallback count of the last iterate.
 * Still without an operator: the float-storage and the multi-device line sessions. */
int vrt_regular_line_lambda_diagonal_dev(vrt_regular *r, int64_t n_angles, const double *k, const int *dirs,
                                         const double *weights, int64_t nlam, const double *d_alpha_pl,
                                         double *d_diag_pl, void *stream);
int vrt_regular_line_lambda_diagonal(vrt_regular *r, int64_t n_angles, const double *k, const int *dirs,
                                     const double *weights, int64_t nlam, int64_t ld, const double *alpha, double *diag);
int vrt_regular_lambda_use_operator(vrt_regular_lambda *s, int op);
int vrt_regular_lambda_get_operator(const vrt_regular_lambda *s, int *op, int64_t *fallback_entries_last_iterate);

/* ---- emergent spectra: opacity / source function, top-plane intensity, tau = 1 heights ------------------------------
 * The last step of a reference study (write_top_intensity, write_tau_unity and plotter, src/plot_utils.jl:61-140,
 * :297-355, :434-576) on a regular raster.  Plain numbers in one unit system, constants folded in by the caller.
 * Raster fields without ghost cells are (nz, nx, ny) Julia order, element [iz + nz*(ix + nx*iy)], one field after the
 * other (the layout vrt_grid_to_raster_dev writes); the ghosted arrays carry the one-cell periodic border of
 * periodic_borders (src/atmosphere.jl:191-214): (nz, nx + 2, ny + 2) per wavelength, wavelength slowest.
 *
 * vrt_synth_opacity_dev: for one direction k and nlam wavelengths, per raster point
 *   gamma = gamma_static + gamma_unsold (n1 + n2),  a, v as vrt_line_opacity_dev with v_los = dot(velocity, -k),
 *   alpha_l = strength_const (n1 Bij - n2 Bji) H(a, v) / (sqrt(pi) dlambda_D),  S_l = src_const / (g_ratio n1/n2 - 1),
 *   S_c = planck2[l] / (exp(hc_over_kB / (lambda[l] T)) - 1),
 *   S = (alpha_l S_l + alpha_c S_c) / (alpha_l + alpha_c),  alpha_tot = alpha_l + alpha_c
 * written to d_S and d_alpha, ghosted; the ghost points hold their wrapped interior values bit for bit.
 * nz, nx, ny are the interior sizes; velocity is 3 fields (z, x, y), populations >= 2 fields (n1, n2).  lambda and
 * planck2 [nlam] on the host (chunk wavelengths by passing slices).  Runs on the calling thread's current HIP device,
 * asynchronous on `stream`.
 *
 * vrt_regular_emergent_dev: r is a vrt_regular on the GHOSTED axes; dS, dalpha (nlam ghosted arrays).  Per wavelength
 * an up solve along k with I_0 = the bottom plane of that wavelength's S; only the top plane's interior is written,
 * dI_top (nlam, ny - 2, nx - 2) numpy order [l][iy][ix] (r's sizes).  Wavelengths go through in chunks whose workspace
 * stays under a byte cap (8 GiB; VRT_REG_EMERGENT_BYTES, read at vrt_regular_create); bit-identical to the top interior
 * plane of vrt_regular_execute_dev on the same inputs, whatever the chunking.  Asynchronous on `stream`.
 *
 * vrt_tau_unity_dev: d_alpha ghosted as above on the INTERIOR axes z[nz] (strictly ascending), x[nx], y[ny] (uniform,
 * periodic with period nx dx, ny dy).  Per wavelength and column the tau of the path from the top plane along the
 * up solve's characteristic traced back downward (plane iz at x + s k_x, y + s k_y, s = (z_top - z[iz]) / |k_z|,
 * alpha interpolated bilinearly, trapezoid as cumtrapz); d_height (nlam, ny, nx) = the z of the first argmin
 * |tau - 1|.  At k = (+-1, 0, 0) this is write_tau_unity(DATA) exactly; the inclined reference's defects are not
 * reproduced.  Non-finite alpha follows Julia's argmin: the first plane from the top whose tau is NaN
 * is the minimum, and a lateral fraction of exactly 0 takes the grid value without reading the other node, so that at
 * k = (+-1, 0, 0) a column depends on its own values alone.  Runs on the current HIP device and synchronises `stream`.
 *
 * Every argument is checked before the device is touched (k_z = 0 where a march needs it, |k| != 1, nlam < 1, axes,
 * NULL pointers: VRT_EINVAL).  The host-pointer forms stage the arrays through `device` and return when done. */
int vrt_synth_opacity_dev(int64_t nz, int64_t nx, int64_t ny, const double *k, int64_t nlam, const double *lambda,
                          const double *planck2, double lambda0, double c0, double hc_over_kB, double strength_const,
                          double Bij, double Bji, double src_const, double g_ratio, const double *d_velocity,
                          const double *d_doppler, const double *d_gamma_static, const double *d_gamma_unsold,
                          const double *d_temperature, const double *d_alpha_cont, const double *d_populations,
                          double *d_S, double *d_alpha, void *stream);
int vrt_synth_opacity(int device, int64_t nz, int64_t nx, int64_t ny, const double *k, int64_t nlam,
                      const double *lambda, const double *planck2, double lambda0, double c0, double hc_over_kB,
                      double strength_const, double Bij, double Bji, double src_const, double g_ratio,
                      const double *velocity, const double *doppler, const double *gamma_static,
                      const double *gamma_unsold, const double *temperature, const double *alpha_cont,
                      const double *populations, double *S, double *alpha);
int vrt_regular_emergent_dev(vrt_regular *r, const double *k, int64_t nlam, const double *dS, const double *dalpha,
                             int n_sweeps, double *dI_top, void *stream);
/* nz, nx, ny, z, x, y: the ghosted axes, as vrt_regular_create */
int vrt_top_intensity(int64_t nz, int64_t nx, int64_t ny, const double *z, const double *x, const double *y,
                      const double *k, int64_t nlam, const double *S, const double *alpha, int n_sweeps, int device,
                      double *I_top);
int vrt_tau_unity_dev(int64_t nz, int64_t nx, int64_t ny, const double *z, const double *x, const double *y,
                      const double *k, int64_t nlam, const double *d_alpha, double *d_height, void *stream);
int vrt_tau_unity(int64_t nz, int64_t nx, int64_t ny, const double *z, const double *x, const double *y,
                  const double *k, int64_t nlam, const double *alpha, int device, double *height);

#ifdef __cplusplus
}
#endif
#include "voronoirt_multi_accel.h"
#endif /* VORONOIRT_H */
