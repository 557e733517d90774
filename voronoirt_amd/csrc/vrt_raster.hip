// Resampling between the Voronoi sites and regular rasters: the step at each end of every reference
// run.  Voronoi_to_Raster / Voronoi_to_Raster_inv_dist (src/voronoi_utils.jl:407-617, :773-816, inv_dist_itp :848-860)
// answer a KD-tree query per raster point; initialise (:687-707) interpolates a raster onto the sites with trilinear
// (src/functions.jl:207-248).
// The sites themselves are drawn here too: rejection_sampling (src/functions.jl:79-120) from a raster density, with
// k_trilinear's interpolation (vrt_sample_sites[_dev], below).
//
// Nearest search without a tree: a greedy walk over the grid's own neighbour rows (DESIGN.md "Raster resampling").
// Under the x/y minimum-image metric a walk that moves to a strictly closer Voronoi neighbour ends at the nearest site;
// the sites within a relative 1e-12 of that distance (ties, and near-ties that rounding makes unequal) are collected by
// a bounded search over neighbour rows and the smallest (distance, id) among them wins -- np.argmin over a brute-force
// row.  The second nearest is one of those ties or the end of a second walk that leaves the first out.  The plain Euclidean metric of the
// reference's KDTree reuses that answer when its displacements needed no wrap (no site is closer in Euclidean terms
// than in minimum-image terms) and otherwise searches rings of a uniform cell list exactly.  The cell list (built once
// per grid on the host, deterministic) also gives the walk its starting site: it decides speed only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "vrt_internal.h"

namespace vrt {

namespace {

constexpr int kNearThreads = 256;
constexpr int kTieCap = 32;             // sites of one tie set (8 at a corner of a cubic lattice)
constexpr int kWalkCap = 4096;          // walk steps (each strictly decreases the distance)
constexpr double kTieTol = 1e-12;       // relative: a near-tie is searched like a tie
constexpr int kChunk = 16;              // fields per LDS transpose chunk
constexpr int kGatherThreads = 256;     // four waves, 64 raster points (or sites) each

struct NearArgs {
    const double *pos;
    const int32_t *adj_ptr, *adj;    // symmetric site adjacency, 0-based (walls dropped)
    const int32_t *cell_start, *cell_sites, *seed;
    int ncz, ncx, ncy;               // cells per axis, their origin and edges
    double loz, lox, loy, hz, hx, hy, hmin;
    double Lx, Ly, x_min, x_max, y_min, y_max;
    int periodic, k;
    int64_t nq;
    const double *q;                 // (3, nq) z, x, y -- or NULL: the raster points of the axes below
    const double *az, *ax, *ay;
    int64_t nz, nx, ny;
    int32_t *idx1, *idx2;            // 0-based
    double *d1, *d2;
    unsigned long long *stats;       // [0] walk failure, [1] walk steps, [2] Euclidean fallbacks
};

__device__ __forceinline__ double sq3(double dz, double dx, double dy) { return sqrt((dz * dz + dx * dx) + dy * dy); }

__device__ __forceinline__ double dist_mi(double qz, double qx, double qy, const double *__restrict__ p, double Lx,
                                          double Ly)
{
    const double dz = qz - p[0];
    double dx = qx - p[1], dy = qy - p[2];
    if (dx > 0.5 * Lx) dx -= Lx; else if (dx < -0.5 * Lx) dx += Lx;
    if (dy > 0.5 * Ly) dy -= Ly; else if (dy < -0.5 * Ly) dy += Ly;
    return sq3(dz, dx, dy);
}

__device__ __forceinline__ double dist_eu(double qz, double qx, double qy, const double *__restrict__ p)
{
    return sq3(qz - p[0], qx - p[1], qy - p[2]);
}

__device__ __forceinline__ bool key_less(double da, int a, double db, int b) { return da < db || (da == db && a < b); }

// the two smallest (distance, id) so far; selects, not branches (branches here made the compiler keep the four on the stack)
__device__ __forceinline__ void keep2(double d, int j, double &d1, int &i1, double &d2, int &i2)
{
    const bool l1 = key_less(d, j, d1, i1), l2 = key_less(d, j, d2, i2);
    d2 = l1 ? d1 : (l2 ? d : d2);
    i2 = l1 ? i1 : (l2 ? j : i2);
    d1 = l1 ? d : d1;
    i1 = l1 ? j : i1;
}

__device__ __forceinline__ int cell_of(double v, double lo, double h, int nc)
{
    int c = (int)floor((v - lo) / h);
    return c < 0 ? 0 : (c >= nc ? nc - 1 : c);
}

// x, y of a periodic query wrapped into the box (a point on the box already is left as it is)
__device__ __forceinline__ double wrap(double v, double lo, double hi, double L)
{
    return (v < lo || v > hi) ? v - L * floor((v - lo) / L) : v;
}

struct Walk {
    int i1, i2;                      // the two smallest (distance, id) found; i2 = -1 if none
    double e1, e2;
};

// Walks from `cur` to ever closer neighbours (minimum image), never visiting `skip`; then, if a neighbour is within the
// tie tolerance, collects that tie set (at most kTieCap sites, slot s at set[s * kNearThreads]) and returns its two
// smallest (distance, id).  Without a tie: the end site and its closest neighbour.
__device__ __forceinline__ Walk descend(const NearArgs &a, double qz, double qx, double qy, int cur, int skip,
                                        int32_t *set, unsigned &steps, bool &fail)
{
    double dc = dist_mi(qz, qx, qy, a.pos + 3 * (int64_t)cur, a.Lx, a.Ly);
    double dn;
    int jn;
    bool tie = false;
    for (;;) {
        dn = INFINITY; jn = -1;
        for (int e = a.adj_ptr[cur]; e < a.adj_ptr[cur + 1]; e++) {
            const int j = a.adj[e];
            if (j == skip) continue;
            const double d = dist_mi(qz, qx, qy, a.pos + 3 * (int64_t)j, a.Lx, a.Ly);
            if (key_less(d, j, dn, jn)) { dn = d; jn = j; }
        }
        if (dn < dc) {
            cur = jn; dc = dn;
            if (++steps > (unsigned)kWalkCap) { fail = true; break; }
            continue;
        }
        tie = dn <= dc * (1.0 + kTieTol);
        break;
    }
    Walk w{cur, jn, dc, dn};
    if (tie && !fail) {
        // a tie set is connected through faces
        const double thr = dc * (1.0 + kTieTol);
        set[0] = cur;
        int cnt = 1;
        w.e2 = INFINITY; w.i2 = -1;
        for (int head = 0; head < cnt && !fail; head++) {
            const int s = set[head * kNearThreads];
            for (int e = a.adj_ptr[s]; e < a.adj_ptr[s + 1]; e++) {
                const int j = a.adj[e];
                if (j == skip) continue;
                const double d = dist_mi(qz, qx, qy, a.pos + 3 * (int64_t)j, a.Lx, a.Ly);
                if (!(d <= thr)) continue;
                bool seen = false;
                for (int u = 0; u < cnt; u++) seen |= set[u * kNearThreads] == j;
                if (seen) continue;
                if (cnt == kTieCap) { fail = true; break; }
                set[cnt++ * kNearThreads] = j;
                keep2(d, j, w.e1, w.i1, w.e2, w.i2);
            }
        }
    }
    return w;
}

__global__ void __launch_bounds__(kNearThreads) k_nearest(NearArgs a)
{
    __shared__ int32_t s_tie[kTieCap * kNearThreads];
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned steps = 0, fallback = 0;      // (a wave's sum fits: 64 x the step cap)
    if (t < a.nq) {
        double qz, qx, qy;
        if (a.q) {
            qz = a.q[3 * t]; qx = a.q[3 * t + 1]; qy = a.q[3 * t + 2];
        } else {
            const int64_t iz = t % a.nz, r = t / a.nz;
            qz = a.az[iz]; qx = a.ax[r % a.nx]; qy = a.ay[r / a.nx];
        }
        if (a.periodic) {
            qx = wrap(qx, a.x_min, a.x_max, a.Lx);
            qy = wrap(qy, a.y_min, a.y_max, a.Ly);
        }
        const int c = (cell_of(qz, a.loz, a.hz, a.ncz) * a.ncx + cell_of(qx, a.lox, a.hx, a.ncx)) * a.ncy +
                      cell_of(qy, a.loy, a.hy, a.ncy);
        bool fail = false;
        Walk w = descend(a, qz, qx, qy, a.seed[c], -1, s_tie + threadIdx.x, steps, fail);
        if (a.k == 2 && !fail && !(w.e2 <= w.e1 * (1.0 + kTieTol))) {
            // no tie with the first: the second is the nearest of the other sites.  Near a z wall the face it shares
            // with the first can lie outside the box (not listed), so walk again with the first left out, from the
            // first's closest neighbour: every neighbour of the first is then no closer, and the cells of the others
            // only grew, so the walk argument holds for them
            if (w.i2 < 0) {
                fail = true;               // a site without site neighbours
            } else {
                const Walk v = descend(a, qz, qx, qy, w.i2, w.i1, s_tie + threadIdx.x, steps, fail);
                w.i2 = v.i1;
                w.e2 = v.e1;
            }
        }
        int i1 = w.i1, i2 = w.i2;
        double e1 = w.e1, e2 = w.e2;
        if (!a.periodic && !fail) {
            // Euclidean: d >= the minimum-image d for every site, so a minimum-image answer whose own distances are
            // unchanged is the Euclidean answer; otherwise search the cell list in rings
            const bool same = dist_eu(qz, qx, qy, a.pos + 3 * (int64_t)i1) == e1 &&
                              (a.k < 2 || dist_eu(qz, qx, qy, a.pos + 3 * (int64_t)i2) == e2);
            if (!same) {
                fallback = 1;
                e1 = e2 = INFINITY; i1 = i2 = -1;
                const int cz = cell_of(qz, a.loz, a.hz, a.ncz), cx = cell_of(qx, a.lox, a.hx, a.ncx),
                          cy = cell_of(qy, a.loy, a.hy, a.ncy);
                const int rmax = max(a.ncz, max(a.ncx, a.ncy));
                for (int r = 0; r <= rmax; r++) {
                    // sites outside the cells of rings <= r - 1 are at least (r - 1) * hmin away
                    if (r > 0 && (double)(r - 1) * a.hmin * (1.0 - 1e-9) > (a.k < 2 ? e1 : e2)) break;
                    for (int iz = max(cz - r, 0); iz <= min(cz + r, a.ncz - 1); iz++)
                        for (int ix = max(cx - r, 0); ix <= min(cx + r, a.ncx - 1); ix++)
                            for (int iy = max(cy - r, 0); iy <= min(cy + r, a.ncy - 1); iy++) {
                                if (max(abs(iz - cz), max(abs(ix - cx), abs(iy - cy))) != r) continue;
                                const int cc = (iz * a.ncx + ix) * a.ncy + iy;
                                for (int u = a.cell_start[cc]; u < a.cell_start[cc + 1]; u++) {
                                    const int j = a.cell_sites[u];
                                    keep2(dist_eu(qz, qx, qy, a.pos + 3 * (int64_t)j), j, e1, i1, e2, i2);
                                }
                            }
                }
            }
        }
        if (i2 < 0) i2 = i1;          // (k = 1, or a failed walk: never read as an answer)
        if (fail) atomicOr(a.stats, 1ull);
        a.idx1[t] = i1;
        if (a.d1) a.d1[t] = e1;
        if (a.k == 2) {
            a.idx2[t] = i2;
            if (a.d2) a.d2[t] = e2;
        }
    }
    // statistics: one atomic per wave
    for (int o = 32; o > 0; o >>= 1) {
        steps += __shfl_xor(steps, o);
        fallback += __shfl_xor(fallback, o);
    }
    if ((threadIdx.x & 63) == 0 && (steps || fallback)) {
        atomicAdd(a.stats + 1, (unsigned long long)steps);
        atomicAdd(a.stats + 2, (unsigned long long)fallback);
    }
}

// raster[p + P*f] = fields[f + ld*owner(p)] (mode 1) or inv_dist_itp of the two nearest (mode 2).  A wave owns 64
// consecutive raster points: it reads rows with lanes across fields (16 fields x 4 points per instruction), transposes
// through LDS and writes every field plane as 512 contiguous bytes.
__global__ void __launch_bounds__(kGatherThreads)
k_gather(int64_t P, int64_t nf, int64_t ld, int mode, const int32_t *__restrict__ idx1, const int32_t *__restrict__ idx2,
         const double *__restrict__ d1, const double *__restrict__ d2, const double *__restrict__ fields,
         double *__restrict__ raster)
{
    __shared__ double tile[kGatherThreads / 64][64 * (kChunk + 1)];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t p0 = ((int64_t)blockIdx.x * (kGatherThreads / 64) + wave) * 64;
    double *tw = tile[wave];
    const int fl = lane % kChunk, sub = lane / kChunk;
    for (int64_t f0 = 0; f0 < nf; f0 += kChunk) {
        const int64_t f = f0 + fl;
        for (int it = 0; it < 64 / (64 / kChunk); it++) {
            const int j = it * (64 / kChunk) + sub;
            const int64_t p = p0 + j;
            double v = 0.0;
            if (p < P && f < nf) {
                const int a = idx1[p];
                const double v1 = fields[f + ld * (int64_t)a];
                if (mode == VRT_RASTER_NEAREST) {
                    v = v1;
                } else {
                    const double e1 = d1[p];
                    if (e1 == 0.0) {
                        v = v1;           // the reference gives Inf/Inf = NaN here
                    } else {
                        const double v2 = fields[f + ld * (int64_t)idx2[p]];
                        const double inv1 = 1.0 / e1, inv2 = 1.0 / d2[p];
                        double avg = 0.0, s = 0.0;    // inv_dist_itp, voronoi_utils.jl:848-860, p = 1
                        avg += inv1;
                        s += v1 * inv1;
                        avg += inv2;
                        s += v2 * inv2;
                        v = s / avg;
                    }
                }
            }
            tw[j * (kChunk + 1) + fl] = v;
        }
        __syncthreads();
        const int64_t p = p0 + lane;
        for (int c = 0; c < kChunk && f0 + c < nf; c++)
            if (p < P) raster[p + P * (f0 + c)] = tw[lane * (kChunk + 1) + c];
        __syncthreads();
    }
}

// fields[f + ld*i] = trilinear(site i) of raster plane f (src/functions.jl:207-248).  One thread per site finds its
// cell and weights; the values go through LDS so that each site's row is written contiguously.
__device__ __forceinline__ int interval(const double *__restrict__ ax, int n, double v)
{
    int lo = 0, hi = n;                       // first index with ax[i] >= v (searchsortedfirst - 1, 0-based)
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ax[mid] < v) lo = mid + 1; else hi = mid;
    }
    const int i = lo - 1;
    return i < 0 ? 0 : (i > n - 2 ? n - 2 : i);
}

// k_trilinear's expressions on one cell (the sampler's; k_trilinear keeps its own copy, whose code this helper would
// reschedule): r = the cell's (iz, ix, iy) corner, sx / sy the x / y strides of the raster
__device__ __forceinline__ double trilinear_cell(const double *__restrict__ r, int64_t sx, int64_t sy, double x_d,
                                                 double y_d, double z_d)
{
    const double c000 = r[0], c010 = r[sy], c100 = r[sx], c110 = r[sx + sy];
    const double c001 = r[1], c011 = r[1 + sy], c101 = r[1 + sx], c111 = r[1 + sx + sy];
    const double c00 = c000 * (1 - x_d) + c100 * x_d;
    const double c01 = c001 * (1 - x_d) + c101 * x_d;
    const double c10 = c010 * (1 - x_d) + c110 * x_d;
    const double c11 = c011 * (1 - x_d) + c111 * x_d;
    const double c0 = c00 * (1 - y_d) + c10 * y_d;
    const double c1 = c01 * (1 - y_d) + c11 * y_d;
    return c0 * (1 - z_d) + c1 * z_d;
}

__global__ void __launch_bounds__(kGatherThreads)
k_trilinear(int64_t n, const double *__restrict__ pos, int nz, int nx, int ny, const double *__restrict__ axes, int use_lds,
            int64_t nf, const double *__restrict__ raster, int64_t ld, double *__restrict__ fields)
{
    extern __shared__ double s_axes[];
    __shared__ double tile[kGatherThreads / 64][64 * (kChunk + 1)];
    const int naxes = nz + nx + ny;
    if (use_lds) {
        for (int u = threadIdx.x; u < naxes; u += blockDim.x) s_axes[u] = axes[u];
        __syncthreads();
    }
    const double *az = use_lds ? s_axes : axes;
    const double *ax = az + nz, *ay = ax + nx;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t i0 = ((int64_t)blockIdx.x * (kGatherThreads / 64) + wave) * 64;
    const int64_t i = i0 + lane;
    const int64_t P = (int64_t)nz * nx * ny;
    int64_t b000 = 0;
    int64_t sx = nz, sy = (int64_t)nz * nx;
    double x_d = 0.0, y_d = 0.0, z_d = 0.0;
    if (i < n) {
        const double zk = pos[3 * i], xk = pos[3 * i + 1], yk = pos[3 * i + 2];
        const int iz = interval(az, nz, zk), ix = interval(ax, nx, xk), iy = interval(ay, ny, yk);
        x_d = (xk - ax[ix]) / (ax[ix + 1] - ax[ix]);
        y_d = (yk - ay[iy]) / (ay[iy + 1] - ay[iy]);
        z_d = (zk - az[iz]) / (az[iz + 1] - az[iz]);
        b000 = iz + (int64_t)nz * (ix + (int64_t)nx * iy);
    }
    double *tw = tile[wave];
    const int fl = lane % kChunk, sub = lane / kChunk;
    for (int64_t f0 = 0; f0 < nf; f0 += kChunk) {
        for (int c = 0; c < kChunk; c++) {
            double v = 0.0;
            if (i < n && f0 + c < nf) {
                const double *r = raster + P * (f0 + c) + b000;
                const double c000 = r[0], c010 = r[sy], c100 = r[sx], c110 = r[sx + sy];
                const double c001 = r[1], c011 = r[1 + sy], c101 = r[1 + sx], c111 = r[1 + sx + sy];
                const double c00 = c000 * (1 - x_d) + c100 * x_d;
                const double c01 = c001 * (1 - x_d) + c101 * x_d;
                const double c10 = c010 * (1 - x_d) + c110 * x_d;
                const double c11 = c011 * (1 - x_d) + c111 * x_d;
                const double c0 = c00 * (1 - y_d) + c10 * y_d;
                const double c1 = c01 * (1 - y_d) + c11 * y_d;
                v = c0 * (1 - z_d) + c1 * z_d;
            }
            tw[lane * (kChunk + 1) + c] = v;
        }
        __syncthreads();
        for (int it = 0; it < 64 / (64 / kChunk); it++) {
            const int j = it * (64 / kChunk) + sub;
            if (i0 + j < n && f0 + fl < nf) fields[f0 + fl + ld * (i0 + j)] = tw[j * (kChunk + 1) + fl];
        }
        __syncthreads();
    }
}

// ---- rejection sampling of sites from a raster density (src/functions.jl:79-120; DESIGN.md "Site sampling") --------
// Proposal j draws u_c = counter_uniform(seed, c, j), c = 0..3 (synth.counter_uniform), and is accepted iff
// trilinear(q; u_0*dz + z_0, u_1*dx + x_0, u_2*dy + y_0) > u_3*dq + q_min.  A batch [j0, j0 + count) runs as three
// launches: flags (one ballot mask and its popcount per 64 proposals), one workgroup scanning the counts, and the
// write of every accepted proposal at (accepted before the batch) + rank.  No launch depends on workgroup order.
constexpr int kSampleThreads = 256;
constexpr int kSampleGrid = 4096;                   // workgroups of a flags / write launch (grid-stride beyond)
constexpr int kScanThreads = 1024;
constexpr int kScanPer = 4;                         // counts per scan thread and tile
constexpr int kSampleLdsAxes = 4096;                // axes (doubles) staged in LDS up to 32 KiB
constexpr int kMinMaxThreads = 256;
constexpr int kMinMaxGrid = 1024;

struct SampleArgs {
    const double *axes;               // z (nz), x (nx), y (ny)
    const double *q;                  // (ny, nx, nz): element iz + nz*(ix + nx*iy)
    int nz, nx, ny, use_lds;
    uint64_t key[4];                  // splitmix64(seed * 0x100000001B3 + c)
    double z0, dz, x0, dx, y0, dy, qmin, dq;
};

__host__ __device__ __forceinline__ uint64_t splitmix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

__device__ __forceinline__ double uniform01(uint64_t key, uint64_t j)
{
    return (double)(splitmix64(j ^ key) >> 11) * (1.0 / 9007199254740992.0);
}

__global__ void __launch_bounds__(kSampleThreads)
k_sample_flags(SampleArgs a, uint64_t j0, int64_t count, unsigned long long *__restrict__ masks,
               int32_t *__restrict__ counts)
{
    extern __shared__ double s_axes[];
    if (a.use_lds) {
        for (int u = threadIdx.x; u < a.nz + a.nx + a.ny; u += blockDim.x) s_axes[u] = a.axes[u];
        __syncthreads();
    }
    const double *az = a.use_lds ? s_axes : a.axes;
    const double *ax = az + a.nz, *ay = ax + a.nx;
    const int64_t sx = a.nz, sy = (int64_t)a.nz * a.nx;
    // (the loop bound is the same for every thread of the workgroup: the ballot below runs in full waves)
    for (int64_t base = (int64_t)blockIdx.x * kSampleThreads; base < count; base += (int64_t)gridDim.x * kSampleThreads) {
        const int64_t t = base + threadIdx.x;
        bool acc = false;
        if (t < count) {
            const uint64_t j = j0 + (uint64_t)t;
            const double zr = uniform01(a.key[0], j) * a.dz + a.z0;
            const double xr = uniform01(a.key[1], j) * a.dx + a.x0;
            const double yr = uniform01(a.key[2], j) * a.dy + a.y0;
            const double u3 = uniform01(a.key[3], j);
            const int iz = interval(az, a.nz, zr), ix = interval(ax, a.nx, xr), iy = interval(ay, a.ny, yr);
            const double x_d = (xr - ax[ix]) / (ax[ix + 1] - ax[ix]);
            const double y_d = (yr - ay[iy]) / (ay[iy + 1] - ay[iy]);
            const double z_d = (zr - az[iz]) / (az[iz + 1] - az[iz]);
            const double v = trilinear_cell(a.q + (iz + (int64_t)a.nz * (ix + (int64_t)a.nx * iy)), sx, sy, x_d, y_d, z_d);
            acc = v > u3 * a.dq + a.qmin;
        }
        const unsigned long long m = __ballot(acc);
        const int64_t w = t >> 6;
        if ((threadIdx.x & 63) == 0 && w * 64 < count) {
            masks[w] = m;
            counts[w] = __popcll(m);
        }
    }
}

// exclusive scan of the W per-wave counts in place (tiles of kScanThreads * kScanPer); state[1] = accepted before the
// batch, state[0] += the batch's accepted
__global__ void __launch_bounds__(kScanThreads) k_sample_scan(int64_t W, int32_t *__restrict__ counts,
                                                               int64_t *__restrict__ state)
{
    __shared__ int32_t s_wave[kScanThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int32_t carry = 0;                                // a batch holds at most kSampleBatchMax proposals
    for (int64_t t0 = 0; t0 < W; t0 += kScanThreads * kScanPer) {
        const int64_t i0 = t0 + (int64_t)threadIdx.x * kScanPer;
        int32_t v[kScanPer], s = 0;
#pragma unroll
        for (int k = 0; k < kScanPer; k++) {
            v[k] = i0 + k < W ? counts[i0 + k] : 0;
            s += v[k];
        }
        int32_t inc = s;                              // inclusive scan over the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int32_t y = __shfl_up(inc, o);
            if (lane >= o) inc += y;
        }
        if (lane == 63) s_wave[wave] = inc;
        __syncthreads();
        int32_t before = 0, tile = 0;
#pragma unroll
        for (int u = 0; u < kScanThreads / 64; u++) {
            const int32_t c = s_wave[u];
            before += u < wave ? c : 0;
            tile += c;
        }
        int32_t run = carry + before + (inc - s);
#pragma unroll
        for (int k = 0; k < kScanPer; k++) {
            if (i0 + k < W) counts[i0 + k] = run;
            run += v[k];
        }
        carry += tile;
        __syncthreads();                              // s_wave is rewritten by the next tile
    }
    if (threadIdx.x == 0) {
        const int64_t total = state[0];
        state[1] = total;
        state[0] = total + carry;
    }
}

// every accepted proposal of the batch whose index (state[1] + offset of its wave + rank in the mask) is < n writes
// its position, recomputed from j; the n-th accepted one records its j in state[2]
__global__ void __launch_bounds__(kSampleThreads)
k_sample_write(SampleArgs a, uint64_t j0, int64_t count, const unsigned long long *__restrict__ masks,
               const int32_t *__restrict__ offsets, int64_t *__restrict__ state, int64_t n, double *__restrict__ pos)
{
    const int64_t first = state[1];
    if (first >= n) return;
    const int lane = threadIdx.x & 63;
    for (int64_t t = (int64_t)blockIdx.x * kSampleThreads + threadIdx.x; t < count;
         t += (int64_t)gridDim.x * kSampleThreads) {
        const int64_t w = t >> 6;
        const unsigned long long m = masks[w];
        if (!((m >> lane) & 1ull)) continue;
        const int64_t idx = first + offsets[w] + __popcll(m & ((1ull << lane) - 1ull));
        if (idx >= n) continue;
        const uint64_t j = j0 + (uint64_t)t;
        pos[3 * idx] = uniform01(a.key[0], j) * a.dz + a.z0;
        pos[3 * idx + 1] = uniform01(a.key[1], j) * a.dx + a.x0;
        pos[3 * idx + 2] = uniform01(a.key[2], j) * a.dy + a.y0;
        if (idx == n - 1) state[2] = (int64_t)j;
    }
}

// per workgroup: min and max of the finite values of q and the number of values that are not finite (exact: the min
// and max of a set are members of it)
__global__ void __launch_bounds__(kMinMaxThreads) k_minmax(int64_t P, const double *__restrict__ q,
                                                           double *__restrict__ part)
{
    __shared__ double s[3][kMinMaxThreads / 64];
    double mn = INFINITY, mx = -INFINITY, bad = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kMinMaxThreads + threadIdx.x; i < P; i += (int64_t)gridDim.x * kMinMaxThreads) {
        const double v = q[i];
        if (isfinite(v)) {
            mn = fmin(mn, v);
            mx = fmax(mx, v);
        } else {
            bad += 1.0;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        mn = fmin(mn, __shfl_xor(mn, o));
        mx = fmax(mx, __shfl_xor(mx, o));
        bad += __shfl_xor(bad, o);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { s[0][wave] = mn; s[1][wave] = mx; s[2][wave] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int u = 1; u < kMinMaxThreads / 64; u++) {
            mn = fmin(mn, s[0][u]);
            mx = fmax(mx, s[1][u]);
            bad += s[2][u];
        }
        part[3 * blockIdx.x] = mn;
        part[3 * blockIdx.x + 1] = mx;
        part[3 * blockIdx.x + 2] = bad;
    }
}

}  // namespace

// ---- locator: uniform cell list + per-cell seeds, built on the host -------------------------------------------------
struct RasterLocator {
    int64_t requested = -1;                  // g->nearest_cells it was built for
    int nc[3] = {1, 1, 1};
    double lo[3] = {0, 0, 0}, h[3] = {1, 1, 1};
    DevBuf<int32_t> d_cell_start, d_cell_sites, d_seed;
    DevBuf<int32_t> d_adj_ptr, d_adj;        // symmetric closure of the neighbour rows, 0-based
    DevBuf<unsigned long long> d_stats;
    DevWork<char> d_work;                    // idx1, idx2, d1, d2 of the raster points / queries (grow-only)
    DevWork<double> d_axes;
    Event ev[3];
    double last_ms[2] = {0, 0};
    unsigned long long last_stats[3] = {0, 0, 0};
    int64_t last_nq = 0;
};

void raster_locator_delete(RasterLocator *L) { delete L; }

namespace {

int build_locator(vrt_grid *g)
{
    if (g->locator && g->locator->requested == g->nearest_cells) return VRT_OK;
    g->locator.reset();
    std::unique_ptr<RasterLocator, RasterLocatorDelete> L(new RasterLocator());     // (the grid gets it when it is complete)
    L->requested = g->nearest_cells;
    const int64_t n = g->n;
    // the cells cover the box and every site (a site is inside its cell, which the ring search's bound relies on)
    double hi[3];
    for (int c = 0; c < 3; c++) { L->lo[c] = g->bounds[2 * c]; hi[c] = g->bounds[2 * c + 1]; }
    for (int64_t i = 0; i < n; i++)
        for (int c = 0; c < 3; c++) {
            L->lo[c] = std::min(L->lo[c], g->pos[3 * (size_t)i + c]);
            hi[c] = std::max(hi[c], g->pos[3 * (size_t)i + c]);
        }
    double ext[3];
    for (int c = 0; c < 3; c++) ext[c] = hi[c] > L->lo[c] ? hi[c] - L->lo[c] : 1.0;
    if (g->nearest_cells > 0) {
        for (int c = 0; c < 3; c++) L->nc[c] = (int)g->nearest_cells;
    } else {
        // about two sites per cell, cubic cells
        const double edge = std::cbrt(ext[0] * ext[1] * ext[2] * 2.0 / (double)n);
        for (int c = 0; c < 3; c++) L->nc[c] = (int)std::max(1.0, std::min(256.0, std::floor(ext[c] / edge)));
    }
    for (int c = 0; c < 3; c++) L->h[c] = ext[c] / L->nc[c];
    const int64_t ncell = (int64_t)L->nc[0] * L->nc[1] * L->nc[2];
    auto cell = [&](int64_t i) {
        int ci[3];
        for (int c = 0; c < 3; c++) {
            int v = (int)std::floor((g->pos[3 * (size_t)i + c] - L->lo[c]) / L->h[c]);
            ci[c] = v < 0 ? 0 : (v >= L->nc[c] ? L->nc[c] - 1 : v);
        }
        return ((int64_t)ci[0] * L->nc[1] + ci[1]) * L->nc[2] + ci[2];
    };
    std::vector<int32_t> start((size_t)ncell + 1, 0), sites((size_t)n), seed((size_t)ncell, -1);
    std::vector<int64_t> of((size_t)n);
    for (int64_t i = 0; i < n; i++) { of[(size_t)i] = cell(i); start[(size_t)of[(size_t)i] + 1]++; }
    for (int64_t c = 0; c < ncell; c++) start[(size_t)c + 1] += start[(size_t)c];
    {
        std::vector<int32_t> cur(start.begin(), start.end() - 1);
        for (int64_t i = 0; i < n; i++) sites[(size_t)cur[(size_t)of[(size_t)i]]++] = (int32_t)i;   // ascending ids
    }
    // seeds: the lowest id of a cell; an empty cell takes the seed of the nearest non-empty cell (multi-source BFS)
    std::vector<int64_t> queue;
    queue.reserve((size_t)ncell);
    for (int64_t c = 0; c < ncell; c++)
        if (start[(size_t)c + 1] > start[(size_t)c]) { seed[(size_t)c] = sites[(size_t)start[(size_t)c]]; queue.push_back(c); }
    for (size_t head = 0; head < queue.size(); head++) {
        const int64_t c = queue[head];
        const int cz = (int)(c / ((int64_t)L->nc[1] * L->nc[2])), cx = (int)((c / L->nc[2]) % L->nc[1]),
                  cy = (int)(c % L->nc[2]);
        const int nb[6][3] = {{cz - 1, cx, cy}, {cz + 1, cx, cy}, {cz, cx - 1, cy}, {cz, cx + 1, cy}, {cz, cx, cy - 1}, {cz, cx, cy + 1}};
        for (const auto &v : nb) {
            if (v[0] < 0 || v[0] >= L->nc[0] || v[1] < 0 || v[1] >= L->nc[1] || v[2] < 0 || v[2] >= L->nc[2]) continue;
            const int64_t d = ((int64_t)v[0] * L->nc[1] + v[1]) * L->nc[2] + v[2];
            if (seed[(size_t)d] < 0) { seed[(size_t)d] = seed[(size_t)c]; queue.push_back(d); }
        }
    }
    // the walk follows the symmetric closure of the rows: lists read from a file need not be symmetric (the golden
    // grid's are not), and a site missing from a row can leave the walk at a local minimum
    std::vector<int32_t> adj_ptr((size_t)n + 1, 0), adj;
    {
        std::vector<int32_t> deg((size_t)n, 0);
        for (int64_t i = 0; i < n; i++)
            for (int32_t e = g->rowptr[(size_t)i]; e < g->rowptr[(size_t)i + 1]; e++)
                if (g->col[(size_t)e] > 0) { deg[(size_t)i]++; deg[(size_t)g->col[(size_t)e] - 1]++; }
        for (int64_t i = 0; i < n; i++) adj_ptr[(size_t)i + 1] = adj_ptr[(size_t)i] + deg[(size_t)i];
        adj.resize((size_t)adj_ptr[(size_t)n]);
        std::vector<int32_t> cur(adj_ptr.begin(), adj_ptr.end() - 1);
        for (int64_t i = 0; i < n; i++)
            for (int32_t e = g->rowptr[(size_t)i]; e < g->rowptr[(size_t)i + 1]; e++) {
                const int32_t j = g->col[(size_t)e] - 1;
                if (j < 0) continue;
                adj[(size_t)cur[(size_t)i]++] = j;
                adj[(size_t)cur[(size_t)j]++] = (int32_t)i;
            }
        int32_t w = 0;                       // sort and de-duplicate every row, compacting in place
        for (int64_t i = 0; i < n; i++) {
            const int32_t b = adj_ptr[(size_t)i], e = adj_ptr[(size_t)i + 1];
            std::sort(adj.begin() + b, adj.begin() + e);
            adj_ptr[(size_t)i] = w;
            for (int32_t u = b; u < e; u++)
                if (u == b || adj[(size_t)u] != adj[(size_t)u - 1]) adj[(size_t)w++] = adj[(size_t)u];
        }
        adj_ptr[(size_t)n] = w;
        adj.resize((size_t)w);
    }
    int rc;
    if ((rc = L->d_adj_ptr.alloc((size_t)n + 1))) return rc;
    if ((rc = L->d_adj.alloc(adj.size()))) return rc;
    VRT_HIP_TRY(hipMemcpy(L->d_adj_ptr, adj_ptr.data(), sizeof(int32_t) * adj_ptr.size(), hipMemcpyHostToDevice));
    if (!adj.empty()) VRT_HIP_TRY(hipMemcpy(L->d_adj, adj.data(), sizeof(int32_t) * adj.size(), hipMemcpyHostToDevice));
    if ((rc = L->d_cell_start.alloc((size_t)ncell + 1))) return rc;
    if ((rc = L->d_cell_sites.alloc((size_t)n))) return rc;
    if ((rc = L->d_seed.alloc((size_t)ncell))) return rc;
    if ((rc = L->d_stats.alloc(3))) return rc;
    VRT_HIP_TRY(hipMemcpy(L->d_cell_start, start.data(), sizeof(int32_t) * start.size(), hipMemcpyHostToDevice));
    VRT_HIP_TRY(hipMemcpy(L->d_cell_sites, sites.data(), sizeof(int32_t) * sites.size(), hipMemcpyHostToDevice));
    VRT_HIP_TRY(hipMemcpy(L->d_seed, seed.data(), sizeof(int32_t) * seed.size(), hipMemcpyHostToDevice));
    for (Event &e : L->ev)
        if ((rc = e.create())) return rc;
    g->locator = std::move(L);
    return VRT_OK;
}

bool finite_ascending(const double *a, int64_t n)
{
    for (int64_t i = 0; i < n; i++)
        if (!std::isfinite(a[i]) || (i > 0 && !(a[i] > a[i - 1]))) return false;
    return true;
}

constexpr int64_t kMaxPoints = ((int64_t)1 << 31) - 1;

int check_raster_points(const vrt_grid *g, int64_t nz, int64_t nx, int64_t ny, const double *z, const double *x,
                        const double *y, int metric)
{
    if (!z || !x || !y) return fail(VRT_EINVAL, "NULL axis");
    if (nz < 1 || nx < 1 || ny < 1) return fail(VRT_EINVAL, "every raster axis needs at least one point");
    if (nz > kMaxPoints || nx > kMaxPoints || ny > kMaxPoints || nz * nx > kMaxPoints || nz * nx * ny > kMaxPoints)
        return fail(VRT_EINVAL, "raster has more than 2^31 - 1 points");
    if (!finite_ascending(z, nz) || !finite_ascending(x, nx) || !finite_ascending(y, ny))
        return fail(VRT_EINVAL, "raster axes must be finite and strictly ascending");
    const double *b = g->bounds;
    if (z[0] < b[0] || z[nz - 1] > b[1]) return fail(VRT_EINVAL, "raster z outside [z_min, z_max]");
    if (metric == VRT_METRIC_EUCLIDEAN && (x[0] < b[2] || x[nx - 1] > b[3] || y[0] < b[4] || y[ny - 1] > b[5]))
        return fail(VRT_EINVAL, "raster x or y outside the box (VRT_METRIC_EUCLIDEAN)");
    return VRT_OK;
}

int check_metric(const vrt_grid *g, int metric)
{
    if (metric != VRT_METRIC_EUCLIDEAN && metric != VRT_METRIC_PERIODIC_XY) return fail(VRT_EINVAL, "unknown metric");
    if (metric == VRT_METRIC_PERIODIC_XY && !(g->bounds[3] > g->bounds[2] && g->bounds[5] > g->bounds[4]))
        return fail(VRT_EINVAL, "VRT_METRIC_PERIODIC_XY needs x_max > x_min and y_max > y_min");
    return VRT_OK;
}

NearArgs near_args(vrt_grid *g, int metric, int k)
{
    const RasterLocator *L = g->locator.get();
    NearArgs a{};
    a.pos = g->d_pos; a.adj_ptr = L->d_adj_ptr; a.adj = L->d_adj;
    a.cell_start = L->d_cell_start; a.cell_sites = L->d_cell_sites; a.seed = L->d_seed;
    a.ncz = L->nc[0]; a.ncx = L->nc[1]; a.ncy = L->nc[2];
    a.loz = L->lo[0]; a.lox = L->lo[1]; a.loy = L->lo[2];
    a.hz = L->h[0]; a.hx = L->h[1]; a.hy = L->h[2];
    a.hmin = std::min(a.hz, std::min(a.hx, a.hy));
    a.x_min = g->bounds[2]; a.x_max = g->bounds[3]; a.y_min = g->bounds[4]; a.y_max = g->bounds[5];
    a.Lx = a.x_max - a.x_min; a.Ly = a.y_max - a.y_min;
    a.periodic = metric == VRT_METRIC_PERIODIC_XY;
    a.k = k;
    a.stats = L->d_stats;
    return a;
}

// runs the walk of a.nq queries (workspace pointers set by the caller); records the kernel's events
int launch_nearest(RasterLocator *L, NearArgs &a, hipStream_t st)
{
    VRT_HIP_TRY(hipMemsetAsync(L->d_stats, 0, 3 * sizeof(unsigned long long), st));
    VRT_HIP_TRY(hipEventRecord(L->ev[0], st));
    const int64_t blocks = (a.nq + kNearThreads - 1) / kNearThreads;
    hipLaunchKernelGGL(k_nearest, dim3((unsigned)blocks), dim3(kNearThreads), 0, st, a);
    VRT_HIP_TRY(hipGetLastError());
    VRT_HIP_TRY(hipEventRecord(L->ev[1], st));
    L->last_nq = a.nq;
    return VRT_OK;
}

// waits for the stream, reads the statistics and reports a walk that hit its caps
int finish(RasterLocator *L, hipStream_t st, bool gather)
{
    VRT_HIP_TRY(hipMemcpyAsync(L->last_stats, L->d_stats, sizeof(L->last_stats), hipMemcpyDeviceToHost, st));
    VRT_HIP_TRY(hipStreamSynchronize(st));
    float t = 0.f;
    VRT_HIP_TRY(hipEventElapsedTime(&t, L->ev[0], L->ev[1]));
    L->last_ms[0] = t;
    L->last_ms[1] = 0;
    if (gather) {
        VRT_HIP_TRY(hipEventElapsedTime(&t, L->ev[1], L->ev[2]));
        L->last_ms[1] = t;
    }
    if (L->last_stats[0])
        return fail(VRT_EGRID, "nearest-site walk exceeded its step or tie-set cap: the neighbour lists are not the "
                               "Voronoi neighbours of the sites");
    return VRT_OK;
}

int to_raster_impl(vrt_grid *g, int64_t nz, int64_t nx, int64_t ny, const double *z, const double *x, const double *y,
                   int metric, int mode, int64_t nf, int64_t ld, const double *d_fields, double *d_raster, hipStream_t st)
{
    int rc = build_locator(g);
    if (rc) return rc;
    RasterLocator *L = g->locator.get();
    const int64_t P = nz * nx * ny;
    const int k = mode == VRT_RASTER_INV_DIST2 ? 2 : 1;
    if ((rc = L->d_work.grow((size_t)P * (k == 2 ? 24 : 4)))) return rc;
    if ((rc = L->d_axes.grow((size_t)(nz + nx + ny)))) return rc;
    VRT_HIP_TRY(hipMemcpyAsync(L->d_axes, z, sizeof(double) * nz, hipMemcpyHostToDevice, st));
    VRT_HIP_TRY(hipMemcpyAsync(L->d_axes + nz, x, sizeof(double) * nx, hipMemcpyHostToDevice, st));
    VRT_HIP_TRY(hipMemcpyAsync(L->d_axes + nz + nx, y, sizeof(double) * ny, hipMemcpyHostToDevice, st));
    NearArgs a = near_args(g, metric, k);
    a.nq = P;
    a.az = L->d_axes; a.ax = L->d_axes + nz; a.ay = L->d_axes + nz + nx;
    a.nz = nz; a.nx = nx; a.ny = ny;
    char *w = (char *)L->d_work;
    if (k == 2) {
        a.d1 = (double *)w; a.d2 = a.d1 + P;
        a.idx1 = (int32_t *)(a.d2 + P); a.idx2 = a.idx1 + P;
    } else {
        a.idx1 = (int32_t *)w;
    }
    if ((rc = launch_nearest(L, a, st))) return rc;
    const int64_t blocks = (P + kGatherThreads - 1) / kGatherThreads;
    hipLaunchKernelGGL(k_gather, dim3((unsigned)blocks), dim3(kGatherThreads), 0, st, P, nf, ld, mode, a.idx1, a.idx2,
                       a.d1, a.d2, d_fields, d_raster);
    VRT_HIP_TRY(hipGetLastError());
    VRT_HIP_TRY(hipEventRecord(L->ev[2], st));
    return finish(L, st, true);
}

int to_raster_checks(vrt_grid *g, int64_t nz, int64_t nx, int64_t ny, const double *z, const double *x, const double *y,
                     int metric, int mode, int64_t nf, int64_t ld, const void *fields, const void *raster)
{
    if (!g || !fields || !raster) return fail(VRT_EINVAL, "NULL argument");
    int rc = check_metric(g, metric);
    if (rc) return rc;
    if (mode != VRT_RASTER_NEAREST && mode != VRT_RASTER_INV_DIST2) return fail(VRT_EINVAL, "unknown raster mode");
    if ((rc = check_raster_points(g, nz, nx, ny, z, x, y, metric))) return rc;
    if (nf < 1 || ld < nf) return fail(VRT_EINVAL, "need nf >= 1 and ld >= nf");
    const int64_t P = nz * nx * ny;
    if (nf > (INT64_MAX / 8) / P || ld > (INT64_MAX / 8) / g->n) return fail(VRT_EINVAL, "field array size overflows");
    return VRT_OK;
}

int to_grid_checks(vrt_grid *g, int64_t nz, int64_t nx, int64_t ny, const double *z, const double *x, const double *y,
                   int64_t nf, int64_t ld, const void *raster, const void *fields)
{
    if (!g || !z || !x || !y || !raster || !fields) return fail(VRT_EINVAL, "NULL argument");
    if (nz < 2 || nx < 2 || ny < 2) return fail(VRT_EINVAL, "trilinear needs at least two points on every axis");
    if (nz > kMaxPoints || nx > kMaxPoints || ny > kMaxPoints || nz * nx > kMaxPoints || nz * nx * ny > kMaxPoints)
        return fail(VRT_EINVAL, "raster has more than 2^31 - 1 points");
    if (!finite_ascending(z, nz) || !finite_ascending(x, nx) || !finite_ascending(y, ny))
        return fail(VRT_EINVAL, "raster axes must be finite and strictly ascending");
    if (nf < 1 || ld < nf) return fail(VRT_EINVAL, "need nf >= 1 and ld >= nf");
    const int64_t P = nz * nx * ny;
    if (nf > (INT64_MAX / 8) / P || ld > (INT64_MAX / 8) / g->n) return fail(VRT_EINVAL, "field array size overflows");
    for (int64_t i = 0; i < g->n; i++) {
        const double *p = &g->pos[3 * (size_t)i];
        if (!(p[0] >= z[0] && p[0] <= z[nz - 1] && p[1] >= x[0] && p[1] <= x[nx - 1] && p[2] >= y[0] && p[2] <= y[ny - 1]))
            return fail(VRT_EINVAL, "site " + std::to_string(i + 1) + " lies outside the raster's axis ranges");
    }
    return VRT_OK;
}

int to_grid_impl(vrt_grid *g, int64_t nz, int64_t nx, int64_t ny, const double *z, const double *x, const double *y,
                 int64_t nf, const double *d_raster, int64_t ld, double *d_fields, hipStream_t st)
{
    int rc = build_locator(g);      // (holds the axes' workspace)
    if (rc) return rc;
    RasterLocator *L = g->locator.get();
    const int64_t na = nz + nx + ny;
    rc = L->d_axes.grow((size_t)na);
    if (rc) return rc;
    VRT_HIP_TRY(hipMemcpyAsync(L->d_axes, z, sizeof(double) * nz, hipMemcpyHostToDevice, st));
    VRT_HIP_TRY(hipMemcpyAsync(L->d_axes + nz, x, sizeof(double) * nx, hipMemcpyHostToDevice, st));
    VRT_HIP_TRY(hipMemcpyAsync(L->d_axes + nz + nx, y, sizeof(double) * ny, hipMemcpyHostToDevice, st));
    const int use_lds = na <= 3072;         // 24 KiB beside the 35 KiB transpose tile
    const int64_t blocks = (g->n + kGatherThreads - 1) / kGatherThreads;
    hipLaunchKernelGGL(k_trilinear, dim3((unsigned)blocks), dim3(kGatherThreads), use_lds ? sizeof(double) * na : 0, st,
                       g->n, g->d_pos, (int)nz, (int)nx, (int)ny, L->d_axes, use_lds, nf, d_raster, ld, d_fields);
    VRT_HIP_TRY(hipGetLastError());
    VRT_HIP_TRY(hipStreamSynchronize(st));
    return VRT_OK;
}

// ---- rejection sampling: host side ----------------------------------------------------------------------------------
constexpr int64_t kSampleBatchMax = (int64_t)1 << 24;      // proposals per batch: 2 MiB of masks, 1 MiB of counts
constexpr int64_t kSampleBatchMin = (int64_t)1 << 16;

int sample_checks(int device, int64_t nz, int64_t nx, int64_t ny, const double *z, const double *x, const double *y,
                  const void *quantity, int64_t n_sites, int64_t batch, int64_t max_proposals, const void *pos)
{
    if (!z || !x || !y || !quantity || !pos) return fail(VRT_EINVAL, "NULL argument");
    if (device < 0) return fail(VRT_EINVAL, "device ordinal must be >= 0");
    if (nz < 2 || nx < 2 || ny < 2) return fail(VRT_EINVAL, "trilinear needs at least two points on every axis");
    if (nz > kMaxPoints || nx > kMaxPoints || ny > kMaxPoints || nz * nx > kMaxPoints || nz * nx * ny > kMaxPoints)
        return fail(VRT_EINVAL, "raster has more than 2^31 - 1 points");
    if (!finite_ascending(z, nz) || !finite_ascending(x, nx) || !finite_ascending(y, ny))
        return fail(VRT_EINVAL, "raster axes must be finite and strictly ascending");
    if (!(z[nz - 1] - z[0] < INFINITY && x[nx - 1] - x[0] < INFINITY && y[ny - 1] - y[0] < INFINITY))
        return fail(VRT_EINVAL, "raster axis extent overflows");
    if (n_sites < 1 || n_sites > kMaxPoints) return fail(VRT_EINVAL, "n_sites must be in [1, 2^31 - 1]");
    if (batch < 0) return fail(VRT_EINVAL, "batch must be >= 0 (0: the library chooses)");
    if (max_proposals < 0) return fail(VRT_EINVAL, "max_proposals must be >= 0 (0: the default cap)");
    return VRT_OK;
}

// q_min, q_max of the quantity: every value finite and q_max > q_min, else the reference's loop never ends
int check_range(int64_t nonfinite, double qmin, double qmax)
{
    if (nonfinite) return fail(VRT_EINVAL, "quantity has " + std::to_string(nonfinite) + " values that are not finite");
    if (!(qmax - qmin > 0.0) || !(qmax - qmin < INFINITY))
        return fail(VRT_EINVAL, "quantity is constant (q_max == q_min) or its range overflows: nothing can be accepted");
    return VRT_OK;
}

// next batch under batch = 0: the proposals that the acceptance seen so far needs for the remaining sites, plus a
// quarter, or four times the last batch while nothing has been accepted
int64_t next_batch(int64_t n, int64_t accepted, int64_t proposed, int64_t last)
{
    double want;
    if (proposed == 0) want = 2.0 * (double)n;
    else if (accepted == 0) want = 4.0 * (double)last;
    else want = 1.25 * (double)(n - accepted) * ((double)proposed / (double)accepted) + 4096.0;
    return (int64_t)std::min((double)kSampleBatchMax, std::max((double)kSampleBatchMin, want));
}

int sample_impl(int64_t nz, int64_t nx, int64_t ny, const double *z, const double *x, const double *y,
                const double *d_q, double qmin, double qmax, int64_t n, uint64_t seed, int64_t batch,
                int64_t max_proposals, double *d_pos, int64_t *proposals_used, hipStream_t st)
{
    SampleArgs a{};
    a.q = d_q;
    a.nz = (int)nz; a.nx = (int)nx; a.ny = (int)ny;
    for (int c = 0; c < 4; c++) a.key[c] = splitmix64(seed * 0x100000001B3ull + (uint64_t)c);
    a.z0 = z[0]; a.dz = z[nz - 1] - z[0];
    a.x0 = x[0]; a.dx = x[nx - 1] - x[0];
    a.y0 = y[0]; a.dy = y[ny - 1] - y[0];
    a.qmin = qmin; a.dq = qmax - qmin;
    const int64_t na = nz + nx + ny;
    a.use_lds = na <= kSampleLdsAxes;
    const int64_t cap = max_proposals > 0 ? max_proposals : 1000 * n + ((int64_t)1 << 20);
    const int64_t bmax = std::min(batch > 0 ? std::min(batch, kSampleBatchMax) : kSampleBatchMax, cap);
    DevBuf<double> axes;
    DevBuf<unsigned long long> masks;
    DevBuf<int32_t> counts;
    DevBuf<int64_t> state;            // accepted so far, accepted before the batch, j of the n-th accepted
    int rc;
    if ((rc = axes.alloc((size_t)na)) || (rc = masks.alloc((size_t)((bmax + 63) / 64))) ||
        (rc = counts.alloc((size_t)((bmax + 63) / 64))) || (rc = state.alloc(3)))
        return rc;
    a.axes = axes;
    VRT_HIP_TRY(hipMemcpyAsync(axes, z, sizeof(double) * nz, hipMemcpyHostToDevice, st));
    VRT_HIP_TRY(hipMemcpyAsync(axes + nz, x, sizeof(double) * nx, hipMemcpyHostToDevice, st));
    VRT_HIP_TRY(hipMemcpyAsync(axes + nz + nx, y, sizeof(double) * ny, hipMemcpyHostToDevice, st));
    VRT_HIP_TRY(hipMemsetAsync(state, 0, 3 * sizeof(int64_t), st));
    const size_t lds = a.use_lds ? sizeof(double) * (size_t)na : 0;
    int64_t proposed = 0, accepted = 0, count = 0;
    while (accepted < n && proposed < cap) {
        count = std::min(batch > 0 ? bmax : next_batch(n, accepted, proposed, count), cap - proposed);
        const unsigned blocks = (unsigned)std::min<int64_t>((count + kSampleThreads - 1) / kSampleThreads, kSampleGrid);
        hipLaunchKernelGGL(k_sample_flags, dim3(blocks), dim3(kSampleThreads), lds, st, a, (uint64_t)proposed, count,
                           masks, counts);
        VRT_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_sample_scan, dim3(1), dim3(kScanThreads), 0, st, (count + 63) / 64, counts, state);
        VRT_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_sample_write, dim3(blocks), dim3(kSampleThreads), 0, st, a, (uint64_t)proposed, count,
                           masks, counts, state, n, d_pos);
        VRT_HIP_TRY(hipGetLastError());
        VRT_HIP_TRY(hipMemcpyAsync(&accepted, state, sizeof(int64_t), hipMemcpyDeviceToHost, st));
        VRT_HIP_TRY(hipStreamSynchronize(st));
        proposed += count;
    }
    if (accepted < n) {
        if (proposals_used) *proposals_used = proposed;
        return fail(VRT_EINVAL, "rejection sampling: " + std::to_string(accepted) + " of " + std::to_string(n) +
                                    " sites accepted in " + std::to_string(proposed) +
                                    " proposals (max_proposals reached)");
    }
    int64_t last_j = 0;
    VRT_HIP_TRY(hipMemcpyAsync(&last_j, state + 2, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    VRT_HIP_TRY(hipStreamSynchronize(st));
    if (proposals_used) *proposals_used = last_j + 1;
    return VRT_OK;
}

}  // namespace
}  // namespace vrt

using namespace vrt;

extern "C" int vrt_grid_nearest(vrt_grid *g, int64_t nq, const double *q_zxy, int metric, int k, int64_t *idx,
                                double *dist)
{
    return guarded([&]() -> int {
        if (!g || !q_zxy || !idx) return fail(VRT_EINVAL, "NULL argument");
        int rc = check_metric(g, metric);
        if (rc) return rc;
        if (k != 1 && k != 2) return fail(VRT_EINVAL, "k must be 1 or 2");
        if (nq < 0 || nq > kMaxPoints) return fail(VRT_EINVAL, "nq must be in [0, 2^31 - 1]");
        const double *b = g->bounds;
        for (int64_t t = 0; t < nq; t++) {
            const double *q = q_zxy + 3 * t;
            if (!(q[0] >= b[0] && q[0] <= b[1])) return fail(VRT_EINVAL, "query z outside [z_min, z_max] (or NaN)");
            if (metric == VRT_METRIC_EUCLIDEAN ? !(q[1] >= b[2] && q[1] <= b[3] && q[2] >= b[4] && q[2] <= b[5])
                                               : !(std::isfinite(q[1]) && std::isfinite(q[2])))
                return fail(VRT_EINVAL, "query x or y outside the box (or not finite)");
        }
        if ((rc = use_device(g->device))) return rc;
        if (nq == 0) return VRT_OK;
        std::lock_guard<std::mutex> lock(g->mu);
        if ((rc = build_locator(g))) return rc;
        RasterLocator *L = g->locator.get();
        // workspace: queries (3 nq doubles), d1, d2, idx1, idx2
        if ((rc = L->d_work.grow((size_t)nq * (24 + 16 + 8)))) return rc;
        double *dq = (double *)L->d_work.get();
        NearArgs a = near_args(g, metric, k);
        a.nq = nq;
        a.q = dq;
        a.d1 = dq + 3 * nq; a.d2 = a.d1 + nq;
        a.idx1 = (int32_t *)(a.d2 + nq); a.idx2 = a.idx1 + nq;
        hipStream_t st = nullptr;
        VRT_HIP_TRY(hipMemcpyAsync(dq, q_zxy, sizeof(double) * 3 * nq, hipMemcpyHostToDevice, st));
        if ((rc = launch_nearest(L, a, st))) return rc;
        std::vector<int32_t> i1((size_t)nq), i2(k == 2 ? (size_t)nq : 0);
        std::vector<double> e1((size_t)nq), e2(k == 2 ? (size_t)nq : 0);
        VRT_HIP_TRY(hipMemcpyAsync(i1.data(), a.idx1, sizeof(int32_t) * nq, hipMemcpyDeviceToHost, st));
        VRT_HIP_TRY(hipMemcpyAsync(e1.data(), a.d1, sizeof(double) * nq, hipMemcpyDeviceToHost, st));
        if (k == 2) {
            VRT_HIP_TRY(hipMemcpyAsync(i2.data(), a.idx2, sizeof(int32_t) * nq, hipMemcpyDeviceToHost, st));
            VRT_HIP_TRY(hipMemcpyAsync(e2.data(), a.d2, sizeof(double) * nq, hipMemcpyDeviceToHost, st));
        }
        if ((rc = finish(L, st, false))) return rc;
        for (int64_t t = 0; t < nq; t++) {
            idx[k * t] = (int64_t)i1[(size_t)t] + 1;
            if (dist) dist[k * t] = e1[(size_t)t];
            if (k == 2) {
                idx[k * t + 1] = (int64_t)i2[(size_t)t] + 1;
                if (dist) dist[k * t + 1] = e2[(size_t)t];
            }
        }
        return VRT_OK;
    });
}

extern "C" int vrt_grid_to_raster_dev(vrt_grid *g, int64_t nz, int64_t nx, int64_t ny, const double *z, const double *x,
                                      const double *y, int metric, int mode, int64_t nf, int64_t ld, const double *d_fields,
                                      double *d_raster, void *stream)
{
    return guarded([&]() -> int {
        int rc = to_raster_checks(g, nz, nx, ny, z, x, y, metric, mode, nf, ld, d_fields, d_raster);
        if (rc) return rc;
        if ((rc = use_device(g->device))) return rc;
        std::lock_guard<std::mutex> lock(g->mu);
        return to_raster_impl(g, nz, nx, ny, z, x, y, metric, mode, nf, ld, d_fields, d_raster, (hipStream_t)stream);
    });
}

extern "C" int vrt_grid_to_raster(vrt_grid *g, int64_t nz, int64_t nx, int64_t ny, const double *z, const double *x,
                                  const double *y, int metric, int mode, int64_t nf, int64_t ld, const double *fields,
                                  double *raster)
{
    return guarded([&]() -> int {
        int rc = to_raster_checks(g, nz, nx, ny, z, x, y, metric, mode, nf, ld, fields, raster);
        if (rc) return rc;
        if ((rc = use_device(g->device))) return rc;
        std::lock_guard<std::mutex> lock(g->mu);
        const size_t nfield = (size_t)ld * (size_t)(g->n - 1) + (size_t)nf, nout = (size_t)(nz * nx * ny) * (size_t)nf;
        DevBuf<double> df, dr;
        if ((rc = df.alloc(nfield)) || (rc = dr.alloc(nout))) return rc;
        if (hipMemcpy(df, fields, sizeof(double) * nfield, hipMemcpyHostToDevice) != hipSuccess)
            rc = fail(VRT_ENODEVICE, "HIP error uploading the fields");
        if (!rc) rc = to_raster_impl(g, nz, nx, ny, z, x, y, metric, mode, nf, ld, df, dr, nullptr);
        if (!rc && hipMemcpy(raster, dr, sizeof(double) * nout, hipMemcpyDeviceToHost) != hipSuccess)
            rc = fail(VRT_ENODEVICE, "HIP error downloading the raster");
        return rc;
    });
}

extern "C" int vrt_raster_to_grid_dev(vrt_grid *g, int64_t nz, int64_t nx, int64_t ny, const double *z, const double *x,
                                      const double *y, int64_t nf, const double *d_raster, int64_t ld, double *d_fields,
                                      void *stream)
{
    return guarded([&]() -> int {
        int rc = to_grid_checks(g, nz, nx, ny, z, x, y, nf, ld, d_raster, d_fields);
        if (rc) return rc;
        if ((rc = use_device(g->device))) return rc;
        std::lock_guard<std::mutex> lock(g->mu);
        return to_grid_impl(g, nz, nx, ny, z, x, y, nf, d_raster, ld, d_fields, (hipStream_t)stream);
    });
}

extern "C" int vrt_raster_to_grid(vrt_grid *g, int64_t nz, int64_t nx, int64_t ny, const double *z, const double *x,
                                  const double *y, int64_t nf, const double *raster, int64_t ld, double *fields)
{
    return guarded([&]() -> int {
        int rc = to_grid_checks(g, nz, nx, ny, z, x, y, nf, ld, raster, fields);
        if (rc) return rc;
        if ((rc = use_device(g->device))) return rc;
        std::lock_guard<std::mutex> lock(g->mu);
        const size_t nin = (size_t)(nz * nx * ny) * (size_t)nf, nout = (size_t)ld * (size_t)(g->n - 1) + (size_t)nf;
        DevBuf<double> dr, df;
        if ((rc = dr.alloc(nin)) || (rc = df.alloc(nout))) return rc;
        // the caller's padding between rows (ld > nf) is kept as it is
        if (hipMemcpy(dr, raster, sizeof(double) * nin, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(df, fields, sizeof(double) * nout, hipMemcpyHostToDevice) != hipSuccess)
            rc = fail(VRT_ENODEVICE, "HIP error uploading the raster");
        if (!rc) rc = to_grid_impl(g, nz, nx, ny, z, x, y, nf, dr, ld, df, nullptr);
        if (!rc && hipMemcpy(fields, df, sizeof(double) * nout, hipMemcpyDeviceToHost) != hipSuccess)
            rc = fail(VRT_ENODEVICE, "HIP error downloading the fields");
        return rc;
    });
}

extern "C" int vrt_grid_raster_stats(const vrt_grid *g, double *nearest_ms, double *gather_ms, int64_t *queries,
                                     int64_t *walk_steps, int64_t *fallbacks)
{
    if (!g) return fail(VRT_EINVAL, "NULL grid");
    const RasterLocator *L = g->locator.get();
    if (nearest_ms) *nearest_ms = L ? L->last_ms[0] : 0.0;
    if (gather_ms) *gather_ms = L ? L->last_ms[1] : 0.0;
    if (queries) *queries = L ? L->last_nq : 0;
    if (walk_steps) *walk_steps = L ? (int64_t)L->last_stats[1] : 0;
    if (fallbacks) *fallbacks = L ? (int64_t)L->last_stats[2] : 0;
    return VRT_OK;
}

extern "C" int vrt_sample_sites(int device, int64_t nz, int64_t nx, int64_t ny, const double *z, const double *x,
                                const double *y, const double *quantity, int64_t n_sites, uint64_t seed, int64_t batch,
                                int64_t max_proposals, double *pos_zxy, int64_t *proposals_used)
{
    return guarded([&]() -> int {
        int rc = sample_checks(device, nz, nx, ny, z, x, y, quantity, n_sites, batch, max_proposals, pos_zxy);
        if (rc) return rc;
        const int64_t P = nz * nx * ny;
        double qmin = INFINITY, qmax = -INFINITY;
        int64_t nonfinite = 0;
        for (int64_t i = 0; i < P; i++) {
            const double v = quantity[i];
            if (!std::isfinite(v)) { nonfinite++; continue; }
            qmin = std::min(qmin, v);
            qmax = std::max(qmax, v);
        }
        if ((rc = check_range(nonfinite, qmin, qmax))) return rc;
        if ((rc = use_device(device))) return rc;
        DevBuf<double> dq, dp;
        if ((rc = dq.alloc((size_t)P)) || (rc = dp.alloc((size_t)n_sites * 3))) return rc;
        hipStream_t st = nullptr;
        if (hipMemcpy(dq, quantity, sizeof(double) * P, hipMemcpyHostToDevice) != hipSuccess)
            rc = fail(VRT_ENODEVICE, "HIP error uploading the quantity");
        int64_t used = 0;
        if (!rc) rc = sample_impl(nz, nx, ny, z, x, y, dq, qmin, qmax, n_sites, seed, batch, max_proposals, dp, &used, st);
        // on an error (a reached cap included) pos_zxy is left as it was
        if (!rc && hipMemcpy(pos_zxy, dp, sizeof(double) * 3 * n_sites, hipMemcpyDeviceToHost) != hipSuccess)
            rc = fail(VRT_ENODEVICE, "HIP error downloading the positions");
        if (proposals_used) *proposals_used = used;
        return rc;
    });
}

extern "C" int vrt_sample_sites_dev(int device, int64_t nz, int64_t nx, int64_t ny, const double *z, const double *x,
                                    const double *y, const double *d_quantity, int64_t n_sites, uint64_t seed,
                                    int64_t batch, int64_t max_proposals, double *d_pos_zxy, int64_t *proposals_used,
                                    void *stream)
{
    return guarded([&]() -> int {
        int rc = sample_checks(device, nz, nx, ny, z, x, y, d_quantity, n_sites, batch, max_proposals, d_pos_zxy);
        if (rc) return rc;
        if ((rc = use_device(device))) return rc;
        hipStream_t st = (hipStream_t)stream;
        const int64_t P = nz * nx * ny;
        const int blocks = (int)std::min<int64_t>((P + kMinMaxThreads - 1) / kMinMaxThreads, kMinMaxGrid);
        std::vector<double> part((size_t)blocks * 3);
        DevBuf<double> dpart;
        if ((rc = dpart.alloc(part.size()))) return rc;
        hipLaunchKernelGGL(k_minmax, dim3(blocks), dim3(kMinMaxThreads), 0, st, P, d_quantity, dpart);
        if (hipGetLastError() != hipSuccess ||
            hipMemcpyAsync(part.data(), dpart, sizeof(double) * part.size(), hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return fail(VRT_ENODEVICE, "HIP error in the quantity's min/max reduction");
        double qmin = INFINITY, qmax = -INFINITY, bad = 0.0;
        for (int b = 0; b < blocks; b++) {
            qmin = std::min(qmin, part[3 * (size_t)b]);
            qmax = std::max(qmax, part[3 * (size_t)b + 1]);
            bad += part[3 * (size_t)b + 2];
        }
        if ((rc = check_range((int64_t)bad, qmin, qmax))) return rc;
        int64_t used = 0;
        rc = sample_impl(nz, nx, ny, z, x, y, d_quantity, qmin, qmax, n_sites, seed, batch, max_proposals, d_pos_zxy,
                         &used, st);
        if (proposals_used) *proposals_used = used;
        return rc;
    });
}
