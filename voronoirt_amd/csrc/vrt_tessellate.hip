// Voronoi tessellation on the device: vrt_tessellate_gpu / vrt_tessellate_dev (include/voronoirt.h).
//
// The specification is tessellate_host (vrt_tessellate.cpp): the same start box, search grid, candidate images, `eps`,
// 4 r2max test, area threshold and duplicate rule.  A candidate farther than twice the farthest vertex cannot cut, and
// the final cell does not depend on the order of the cuts, so the kernel culls by grid cell and cuts the nearest pending
// candidate of a 64-candidate batch first; the row is then ordered by the host's key (shell, d2, j), which is a pure
// function of the surviving faces.
//
// One wave per site, sites in bucket order.  The cell lives in LDS as a list of planes (normal, offset, id, shell, d2)
// and a list of vertices held as plane triples with a cached position (three-plane intersection).  A cut marks the
// vertices outside the new plane, finds for every edge (plane pair) of an outside vertex the one other vertex on it,
// and where that one is inside makes the vertex (pair, new plane).  Nothing is oriented: the area of a face is the
// sum of |fan triangle . normal| over its edges.  A site whose cell does not fit the capacities, or whose vertex
// list stops being a closed surface (every edge shared by exactly two vertices), is flagged, its row is not written,
// and the host code recomputes it (tessellate_host_sites).
#include <climits>

#include "vrt_internal.h"

#ifndef VRT_TESS_FACES
#define VRT_TESS_FACES 64               // planes a cell holds at once (dead ones are squeezed out when it is full)
#endif

namespace vrt {
namespace {

constexpr int kWave = 64;
constexpr int kF = VRT_TESS_FACES;
constexpr int kV = 2 * kF;              // a simple polytope of F faces has 2F - 4 vertices
constexpr int kVR = (kV + kWave - 1) / kWave;   // vertex slots per lane
constexpr int kRec = kF + 1;            // ints per site record: count (or -1: flagged), entries
static_assert(kF >= 8 && kF <= kWave, "one lane per plane");

struct TessGeom {
    double z_min, z_max, x_min, x_max, y_min, y_max, Lx, Ly, Lz, cx, cy, cz, cmin, eps, amin, slack;
    int gx, gy, gz, smax;
    int64_t n;
};

enum { kBadSite = 0, kGridSite = 1, kFlagged = 2, kMaxCount = 3, kScalars = 4 };

__device__ inline int cell_of(double v, double lo, double c, int g)
{
    const double f = floor((v - lo) / c);
    const int i = f >= (double)g ? g : (f < 0.0 ? -1 : (int)f);      // (NaN: -1)
    return min(max(i, 0), g - 1);
}

// the lowest site outside the closed box (kBadSite); cell of every site and the cell counts
__global__ void __launch_bounds__(256) k_tess_bin(TessGeom G, const double *__restrict__ pos, int *__restrict__ cell_of_site,
                                                  int *__restrict__ count, int *__restrict__ scalars)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= G.n) return;
    const double z = pos[3 * i], x = pos[3 * i + 1], y = pos[3 * i + 2];
    if (!(z >= G.z_min && z <= G.z_max && x >= G.x_min && x <= G.x_max && y >= G.y_min && y <= G.y_max))
        atomicMin(&scalars[kBadSite], (int)i);
    const int c = (cell_of(x, G.x_min, G.cx, G.gx) * G.gy + cell_of(y, G.y_min, G.cy, G.gy)) * G.gz +
                  cell_of(z, G.z_min, G.cz, G.gz);
    cell_of_site[i] = c;
    atomicAdd(&count[c], 1);
}

// exclusive scan of the counts by one workgroup: start[0 .. ncell], cur = start
__global__ void __launch_bounds__(1024) k_tess_scan(int ncell, const int *__restrict__ count, int *__restrict__ start,
                                                    int *__restrict__ cur)
{
    __shared__ int part[1024];
    const int t = threadIdx.x, chunk = (ncell + 1023) / 1024;
    const int lo = min(t * chunk, ncell), hi = min(lo + chunk, ncell);
    int s = 0;
    for (int c = lo; c < hi; c++) s += count[c];
    part[t] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int v = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int base = part[t] - s;
    for (int c = lo; c < hi; c++) {
        start[c] = base;
        cur[c] = base;
        base += count[c];
    }
    if (t == 1023) start[ncell] = part[1023];
}

__global__ void __launch_bounds__(256) k_tess_fill(int64_t n, const int *__restrict__ cell_of_site, int *__restrict__ cur,
                                                   int *__restrict__ unsorted)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    unsorted[atomicAdd(&cur[cell_of_site[i]], 1)] = (int)i;
}

// every bucket in ascending site order, whatever order the atomics of k_tess_fill dealt
__global__ void __launch_bounds__(256) k_tess_rank(int64_t n, const int *__restrict__ cell_of_site, const int *__restrict__ start,
                                                   const int *__restrict__ unsorted, int *__restrict__ item)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = cell_of_site[i], e0 = start[c], e1 = start[c + 1];
    int r = 0;
    for (int e = e0; e < e1; e++) r += unsorted[e] < (int)i;
    item[e0 + r] = (int)i;
}

// ---- the cell of one site, held by one wave ---------------------------------------------------------------------------
struct CellLds {
    double nx[kF], ny[kF], nz[kF], d[kF], d2[kF];      // plane k keeps n . x <= d; d2: squared distance of its image
    int id[kF], shell[kF];                             // neighbour (1-based), wall (-5 / -6) or 0; shell of the image
    double px[kV], py[kV], pz[kV];                     // vertex positions
    unsigned tri[kV];                                  // its three planes, a | b << 8 | c << 16
    unsigned char out[kV];
    unsigned char map[kF];
    double key_d2[kF];                                 // row assembly
    int key_shell[kF], key_id[kF], key_ok[kF];
};

__device__ inline bool has(unsigned t, unsigned p) { return (t & 255u) == p || ((t >> 8) & 255u) == p || (t >> 16) == p; }

__device__ inline void vertex_of(const CellLds &C, unsigned a, unsigned b, unsigned c, double &x, double &y, double &z)
{
    const double ax = C.nx[a], ay = C.ny[a], az = C.nz[a], bx = C.nx[b], by = C.ny[b], bz = C.nz[b], cx = C.nx[c],
                 cy = C.ny[c], cz = C.nz[c];
    const double bcx = by * cz - bz * cy, bcy = bz * cx - bx * cz, bcz = bx * cy - by * cx;      // b x c
    const double cax = cy * az - cz * ay, cay = cz * ax - cx * az, caz = cx * ay - cy * ax;      // c x a
    const double abx = ay * bz - az * by, aby = az * bx - ax * bz, abz = ax * by - ay * bx;      // a x b
    const double det = ax * bcx + ay * bcy + az * bcz;
    const double da = C.d[a], db = C.d[b], dc = C.d[c];
    x = (da * bcx + db * cax + dc * abx) / det;
    y = (da * bcy + db * cay + dc * aby) / det;
    z = (da * bcz + db * caz + dc * abz) / det;
}

__device__ inline double wave_max(double v)
{
    for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    return v;
}

__device__ inline int popc_below(unsigned long long b, int lane) { return __popcll(b & ((1ull << lane) - 1ull)); }

// the largest squared vertex distance
__device__ inline double cell_r2(const CellLds &C, int T, int lane)
{
    double r = 0.0;
    for (int v = lane; v < T; v += kWave) r = fmax(r, C.px[v] * C.px[v] + C.py[v] * C.py[v] + C.pz[v] * C.pz[v]);
    return wave_max(r);
}

// Planes without a vertex leave the list.  Returns the new plane count.
__device__ int squeeze_planes(CellLds &C, int F, int T, int lane)
{
    bool used = false;
    if (lane < F)
        for (int v = 0; v < T && !used; v++) used = has(C.tri[v], (unsigned)lane);
    const unsigned long long b = __ballot(used);
    const int to = popc_below(b, lane);
    double r[5] = {0, 0, 0, 0, 0};
    int ri = 0, rs = 0;
    if (used) {
        r[0] = C.nx[lane]; r[1] = C.ny[lane]; r[2] = C.nz[lane]; r[3] = C.d[lane]; r[4] = C.d2[lane];
        ri = C.id[lane]; rs = C.shell[lane];
        C.map[lane] = (unsigned char)to;
    }
    __syncthreads();
    if (used) {
        C.nx[to] = r[0]; C.ny[to] = r[1]; C.nz[to] = r[2]; C.d[to] = r[3]; C.d2[to] = r[4];
        C.id[to] = ri; C.shell[to] = rs;
    }
    for (int v = lane; v < T; v += kWave) {
        const unsigned t = C.tri[v];
        C.tri[v] = (unsigned)C.map[t & 255u] | (unsigned)C.map[(t >> 8) & 255u] << 8 | (unsigned)C.map[t >> 16] << 16;
    }
    __syncthreads();
    return __popcll(b);
}

// Cuts the cell with n . x <= d (the caller has seen a vertex outside).  F, T, r2max are wave-uniform; returns false when
// the cell no longer fits or is no closed surface (the site is flagged).
__device__ bool cut_cell(CellLds &C, int &F, int &T, double &r2max, double nx, double ny, double nz, double d, double d2, int id,
                         int shell, double eps, int lane)
{
    if (F == kF) F = squeeze_planes(C, F, T, lane);
    if (F == kF) return false;
    const unsigned f = (unsigned)F;
    if (lane == 0) {
        C.nx[f] = nx; C.ny[f] = ny; C.nz[f] = nz; C.d[f] = d; C.d2[f] = d2;
        C.id[f] = id; C.shell[f] = shell;
    }
    bool o[kVR];
#pragma unroll
    for (int r = 0; r < kVR; r++) {
        const int v = lane + r * kWave;
        o[r] = v < T && (nx * C.px[v] + ny * C.py[v] + nz * C.pz[v]) - d > eps;
        if (v < kV) C.out[v] = o[r];
    }
    __syncthreads();
    // the vertices this lane keeps and makes, in registers
    unsigned keep_t[kVR], new_t[kVR][3];
    double keep_p[kVR][3], new_p[kVR][3][3];
    bool is_new[kVR][3], bad = false;
#pragma unroll
    for (int r = 0; r < kVR; r++) {
        const int v = lane + r * kWave;
        is_new[r][0] = is_new[r][1] = is_new[r][2] = false;
        if (v < T && !o[r]) {
            keep_t[r] = C.tri[v];
            keep_p[r][0] = C.px[v]; keep_p[r][1] = C.py[v]; keep_p[r][2] = C.pz[v];
        }
        if (!o[r]) continue;
        const unsigned t = C.tri[v], pl[3] = {t & 255u, (t >> 8) & 255u, t >> 16};
#pragma unroll
        for (int e = 0; e < 3; e++) {
            const unsigned p = pl[e], q = pl[(e + 1) % 3];
            int cnt = 0, w_in = 0;
            for (int w = 0; w < T; w++) {
                const unsigned tw = C.tri[w];
                if (w != v && has(tw, p) && has(tw, q)) {
                    cnt++;
                    w_in = !C.out[w];
                }
            }
            if (cnt != 1) bad = true;
            else if (w_in) {
                is_new[r][e] = true;
                new_t[r][e] = p | q << 8 | f << 16;
                vertex_of(C, p, q, f, new_p[r][e][0], new_p[r][e][1], new_p[r][e][2]);
            }
        }
    }
    // survivors to the front, the new vertices behind them, both in slot order
    int base = 0, keep_to[kVR], new_to[kVR][3];
#pragma unroll
    for (int r = 0; r < kVR; r++) {
        const int v = lane + r * kWave;
        const unsigned long long b = __ballot(v < T && !o[r]);
        keep_to[r] = base + popc_below(b, lane);
        base += __popcll(b);
    }
    const int kept = base;
#pragma unroll
    for (int r = 0; r < kVR; r++)
#pragma unroll
        for (int e = 0; e < 3; e++) {
            const unsigned long long b = __ballot(is_new[r][e]);
            new_to[r][e] = base + popc_below(b, lane);
            base += __popcll(b);
        }
    const bool broken = __ballot(bad) != 0ull || base - kept < 3 || base > kV;
    __syncthreads();                                    // every lane has read what it moves
    if (broken) return false;
#pragma unroll
    for (int r = 0; r < kVR; r++) {
        const int v = lane + r * kWave;
        if (v < T && !o[r]) {
            const int to = keep_to[r];
            C.tri[to] = keep_t[r];
            C.px[to] = keep_p[r][0]; C.py[to] = keep_p[r][1]; C.pz[to] = keep_p[r][2];
        }
#pragma unroll
        for (int e = 0; e < 3; e++)
            if (is_new[r][e]) {
                const int to = new_to[r][e];
                C.tri[to] = new_t[r][e];
                C.px[to] = new_p[r][e][0]; C.py[to] = new_p[r][e][1]; C.pz[to] = new_p[r][e][2];
            }
    }
    T = base;
    F = F + 1;
    __syncthreads();
    r2max = cell_r2(C, T, lane);
    return true;
}

// One candidate per lane of the items [e0, e1) with the image shift (sx, sy); the pending ones cut nearest first.
__device__ bool cut_range(CellLds &C, int &F, int &T, double &r2max, const TessGeom &G, const double *__restrict__ pos,
                          const int *__restrict__ item, int e0, int e1, double sx, double sy, int shell, int i, double xi,
                          double yi, double zi, int lane)
{
    for (int eb = e0; eb < e1; eb += kWave) {
        const int e = eb + lane;
        int j = -1;
        double dx = 0, dy = 0, dz = 0, d2 = 0;
        bool pending = false;
        if (e < e1) {
            j = item[e];
            dx = pos[3 * (int64_t)j + 1] + sx - xi;
            dy = pos[3 * (int64_t)j + 2] + sy - yi;
            dz = pos[3 * (int64_t)j] - zi;
            d2 = dx * dx + dy * dy + dz * dz;
            pending = !(j == i && sx == 0 && sy == 0);
        }
        for (int round = 0; round < kWave; round++) {
            pending = pending && !(d2 > 4.0 * r2max);
            if (pending) {                              // a candidate that cuts nothing now never will: the cell only shrinks
                const double h = 0.5 * d2;
                bool any_out = false;
                for (int v = 0; v < T && !any_out; v++) any_out = (dx * C.px[v] + dy * C.py[v] + dz * C.pz[v]) - h > G.eps;
                pending = any_out;
            }
            const unsigned long long b = __ballot(pending);
            if (!b) break;
            // the nearest pending candidate, ties to the lowest site
            double best = pending ? d2 : INFINITY;
            for (int off = 32; off >= 1; off >>= 1) best = fmin(best, __shfl_xor(best, off));
            int bj = pending && d2 == best ? j : INT_MAX;
            for (int off = 32; off >= 1; off >>= 1) bj = min(bj, __shfl_xor(bj, off));
            const unsigned long long sel = __ballot(pending && d2 == best && j == bj);
            const int L = __ffsll((long long)sel) - 1;
            const double cxn = __shfl(dx, L), cyn = __shfl(dy, L), czn = __shfl(dz, L), cd2 = __shfl(d2, L);
            if (!cut_cell(C, F, T, r2max, cxn, cyn, czn, 0.5 * cd2, cd2, bj + 1, shell, G.eps, lane)) return false;
            if (lane == L) pending = false;
        }
    }
    return true;
}

// does the entry of plane k stand before that of plane l in the row?
__device__ inline bool row_before(const CellLds &C, int k, int l)
{
    const int kid = C.key_id[k], lid = C.key_id[l];
    if (kid < 0 || lid < 0) return kid < 0 && (lid > 0 || kid > lid);          // walls first, -5 before -6
    const int ks = C.key_shell[k], ls = C.key_shell[l];
    const double kd = C.key_d2[k], ld = C.key_d2[l];
    return ks < ls || (ks == ls && (kd < ld || (kd == ld && (kid < lid || (kid == lid && k < l)))));
}

__global__ void __launch_bounds__(kWave) k_tess_cells(TessGeom G, const double *__restrict__ pos, const int *__restrict__ start,
                                                      const int *__restrict__ item, int *__restrict__ rec)
{
    __shared__ CellLds C;
    const int lane = threadIdx.x;
    const int i = item[blockIdx.x];
    const double zi = pos[3 * (int64_t)i], xi = pos[3 * (int64_t)i + 1], yi = pos[3 * (int64_t)i + 2];
    // the start box: walls in z, half a period in x and y
    const double hx = 0.5 * G.Lx, hy = 0.5 * G.Ly, zlo = G.z_min - zi, zhi = G.z_max - zi;
    if (lane < 6) {
        const double bx[6] = {0, 0, 0, 1, 0, -1}, by[6] = {0, 0, -1, 0, 1, 0}, bz[6] = {-1, 1, 0, 0, 0, 0};
        const double bd[6] = {-zlo, zhi, hy, hx, hy, hx};
        const int bid[6] = {-5, -6, 0, 0, 0, 0};
        C.nx[lane] = bx[lane]; C.ny[lane] = by[lane]; C.nz[lane] = bz[lane]; C.d[lane] = bd[lane];
        C.d2[lane] = 0.0; C.id[lane] = bid[lane]; C.shell[lane] = -1;
    }
    if (lane < 8) {
        const unsigned pz = lane & 4 ? 1u : 0u, px = lane & 1 ? 3u : 5u, py = lane & 2 ? 4u : 2u;
        C.tri[lane] = pz | px << 8 | py << 16;
        C.px[lane] = lane & 1 ? hx : -hx;
        C.py[lane] = lane & 2 ? hy : -hy;
        C.pz[lane] = lane & 4 ? zhi : zlo;
    }
    __syncthreads();
    int F = 6, T = 8;
    double r2max = cell_r2(C, T, lane);
    const int ix = cell_of(xi, G.x_min, G.cx, G.gx), iy = cell_of(yi, G.y_min, G.cy, G.gy), iz = cell_of(zi, G.z_min, G.cz, G.gz);
    bool ok = true;
    for (int s = 0; s <= G.smax && ok; s++) {
        if (s > 0) {
            const double reach = (s - 1) * G.cmin;
            if (reach * reach > 4.0 * r2max) break;
        }
        for (int dx = -s; dx <= s && ok; dx++) {
            int cxw = ix + dx;
            double sx = 0;
            while (cxw < 0) { cxw += G.gx; sx -= G.Lx; }
            while (cxw >= G.gx) { cxw -= G.gx; sx += G.Lx; }
            // distance from the site to the (unwrapped) column of grid cells, less a slack for the cells' rounded edges
            const double x_lo = G.x_min + (ix + dx) * G.cx - xi, x_hi = x_lo + G.cx;
            const double gapx = fmax(fmax(x_lo, -x_hi) - G.slack, 0.0);
            for (int dy = -s; dy <= s && ok; dy++) {
                const double y_lo = G.y_min + (iy + dy) * G.cy - yi, y_hi = y_lo + G.cy;
                const double gapy = fmax(fmax(y_lo, -y_hi) - G.slack, 0.0);
                const double room = 4.0 * r2max - (gapx * gapx + gapy * gapy);
                if (room < 0.0) continue;
                int cyw = iy + dy;
                double sy = 0;
                while (cyw < 0) { cyw += G.gy; sy -= G.Ly; }
                while (cyw >= G.gy) { cyw -= G.gy; sy += G.Ly; }
                // grid cells of this column that can hold a cutting site
                const double rz = sqrt(room) + G.slack;
                const double flo = floor((zi - rz - G.z_min) / G.cz) - 1.0, fhi = floor((zi + rz - G.z_min) / G.cz) + 1.0;
                const int near_lo = flo < 0.0 ? 0 : (flo > (double)G.gz ? G.gz : (int)flo);
                const int near_hi = fhi < 0.0 ? -1 : (fhi >= (double)G.gz ? G.gz - 1 : (int)fhi);
                const bool ring = max(abs(dx), abs(dy)) == s;
                const size_t col = ((size_t)cxw * G.gy + cyw) * G.gz;
                // on the ring of the shell the whole column dz = -s .. s, inside it the two end cells
                for (int part = 0; part < (ring || s == 0 ? 1 : 2) && ok; part++) {
                    int z0 = ring ? iz - s : (part == 0 ? iz - s : iz + s), z1 = ring ? iz + s : z0;
                    z0 = max(max(z0, 0), near_lo);
                    z1 = min(min(z1, G.gz - 1), near_hi);
                    if (z0 > z1) continue;
                    ok = cut_range(C, F, T, r2max, G, pos, item, start[col + z0], start[col + z1 + 1], sx, sy, s, i, xi, yi, zi,
                                   lane);
                }
            }
        }
    }
    // ---- the closed-surface check: every edge of every vertex has exactly one other vertex on it
    if (ok) {
        bool bad = false;
        for (int v = lane; v < T; v += kWave) {
            const unsigned t = C.tri[v], pl[3] = {t & 255u, (t >> 8) & 255u, t >> 16};
            for (int e = 0; e < 3; e++) {
                int cnt = 0;
                for (int w = 0; w < T; w++) cnt += w != v && has(C.tri[w], pl[e]) && has(C.tri[w], pl[(e + 1) % 3]);
                bad = bad || cnt != 1;
            }
        }
        ok = __ballot(bad) == 0ull;
    }
    int *row = rec + (size_t)i * kRec;
    if (!ok) {
        if (lane == 0) row[0] = -1;
        return;
    }
    // ---- the row: one lane per plane
    bool listed = false;
    int id = 0;
    if (lane < F) {
        id = C.id[lane];
        int first = -1, nv = 0;
        double acc = 0.0;
        const double ax = C.nx[lane], ay = C.ny[lane], az = C.nz[lane];
        for (int v = 0; v < T; v++) {
            const unsigned t = C.tri[v];
            if (!has(t, (unsigned)lane)) continue;
            nv++;
            if (first < 0) { first = v; continue; }
            const double ux = C.px[v] - C.px[first], uy = C.py[v] - C.py[first], uz = C.pz[v] - C.pz[first];
            const unsigned pl[3] = {t & 255u, (t >> 8) & 255u, t >> 16};
            for (int e = 0; e < 3; e++) {                               // the two edges of v on this face
                if (pl[e] == (unsigned)lane) continue;
                for (int w = v + 1; w < T; w++) {
                    const unsigned tw = C.tri[w];
                    if (!has(tw, (unsigned)lane) || !has(tw, pl[e])) continue;
                    const double wx = C.px[w] - C.px[first], wy = C.py[w] - C.py[first], wz = C.pz[w] - C.pz[first];
                    const double kx = uy * wz - uz * wy, ky = uz * wx - ux * wz, kz = ux * wy - uy * wx;
                    acc += fabs(kx * ax + ky * ay + kz * az);
                }
            }
        }
        const double area = 0.5 * acc / sqrt(ax * ax + ay * ay + az * az);
        listed = nv >= 3 && id != 0 && id != i + 1 && !(area <= G.amin);
        C.key_ok[lane] = listed;
        C.key_id[lane] = id;
        C.key_shell[lane] = C.shell[lane];
        C.key_d2[lane] = C.d2[lane];
    }
    __syncthreads();
    // walls first (-5 before -6), then ascending (shell, d2, id); a second image of a listed neighbour is left out
    if (listed)
        for (int k = 0; k < F; k++)
            if (k != lane && C.key_ok[k] && C.key_id[k] == id && row_before(C, k, lane)) listed = false;
    __syncthreads();
    if (lane < F) C.key_ok[lane] = listed;
    __syncthreads();
    if (listed) {
        int rank = 0;
        for (int k = 0; k < F; k++) rank += k != lane && C.key_ok[k] && row_before(C, k, lane);
        row[1 + rank] = id;
    }
    const int cnt = __popcll(__ballot(listed));
    if (lane == 0) row[0] = cnt;
}

// The records into read_cell's (n, D1) column-major int64 matrix: count in column 0, zeros beyond it.  Flagged sites get
// a zero row here and go to the list; a row that does not fit D1 - 1 entries leaves the lowest such site in kGridSite.
__global__ void __launch_bounds__(256) k_tess_rows(int64_t n, int64_t D1, const int *__restrict__ rec, int64_t *__restrict__ nbr,
                                                   int *__restrict__ flagged, int *__restrict__ scalars)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int cnt = 0;
    const int *row = rec + (size_t)(i < n ? i : 0) * kRec;
    if (i < n) {
        cnt = row[0];
        if (cnt < 0) {
            flagged[atomicAdd(&scalars[kFlagged], 1)] = (int)i;
            cnt = 0;
        } else if ((int64_t)cnt > D1 - 1) {
            atomicMin(&scalars[kGridSite], (int)i);
            cnt = 0;
        }
        nbr[i] = cnt;
        for (int64_t q = 1; q < D1; q++) nbr[i + n * q] = q <= cnt ? (int64_t)row[q] : (int64_t)0;
    }
    int mx = cnt;
    for (int off = 32; off >= 1; off >>= 1) mx = max(mx, __shfl_xor(mx, off));
    if ((threadIdx.x & (kWave - 1)) == 0 && mx > 0) atomicMax(&scalars[kMaxCount], mx);
}

// rows (m, D1) column-major of the recomputed sites into the matrix
__global__ void __launch_bounds__(256) k_tess_patch(int64_t n, int64_t D1, int64_t m, const int *__restrict__ sites,
                                                    const int64_t *__restrict__ rows, int64_t *__restrict__ nbr)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= m * D1) return;
    const int64_t k = t % m, q = t / m;
    nbr[(int64_t)sites[k] + n * q] = rows[t];
}

double g_phase_ms[3] = {0, 0, 0};        // of the last tessellation: grid build, cell kernel, rows with any fallback
int64_t g_phase_sites = 0;

int tess_checks(int64_t n, const double *pos, const double *bounds, int64_t D1, const int64_t *nbr)
{
    if (!pos || !bounds || !nbr) return fail(VRT_EINVAL, "NULL argument");
    if (n < 1 || n >= ((int64_t)1 << 30)) return fail(VRT_EINVAL, "n must be in [1, 2^30)");
    if (D1 < 5) return fail(VRT_EINVAL, "D1 must leave room for at least four neighbours");
    if (!(bounds[1] - bounds[0] > 0 && bounds[3] - bounds[2] > 0 && bounds[5] - bounds[4] > 0)) return fail(VRT_EINVAL, "empty box");
    return VRT_OK;
}

inline int grid_blocks(int64_t count) { return (int)((count + 255) / 256); }

// d_pos, d_nbr: device; h_pos: the same positions on the host, or NULL (downloaded if a site is flagged).  The device is
// chosen.  Synchronises st.
int tessellate_device(int64_t n, const double *d_pos, const double *h_pos, const double bounds[6], int64_t D1, int64_t *d_nbr,
                      int64_t *max_count, int64_t *host_sites, hipStream_t st)
{
    TessGeom G;
    G.z_min = bounds[0]; G.z_max = bounds[1]; G.x_min = bounds[2]; G.x_max = bounds[3]; G.y_min = bounds[4]; G.y_max = bounds[5];
    G.Lz = G.z_max - G.z_min; G.Lx = G.x_max - G.x_min; G.Ly = G.y_max - G.y_min;
    // the host's search grid (vrt_tessellate.cpp), with its arithmetic
    const double vol = G.Lx * G.Ly * G.Lz, h = std::cbrt(vol * 4.0 / (double)std::max<int64_t>(n, 1));
    G.gx = std::max(1, (int)(G.Lx / h)); G.gy = std::max(1, (int)(G.Ly / h)); G.gz = std::max(1, (int)(G.Lz / h));
    G.cx = G.Lx / G.gx; G.cy = G.Ly / G.gy; G.cz = G.Lz / G.gz;
    G.cmin = std::min({G.cx, G.cy, G.cz});
    G.smax = std::max({G.gx, G.gy, G.gz});
    const double Lmax = std::max({G.Lx, G.Ly, G.Lz});
    G.eps = 1e-11 * Lmax;
    G.amin = 1e-14 * (G.Lx * G.Ly);
    G.slack = 1e-9 * Lmax;
    G.n = n;
    const size_t ncell = (size_t)G.gx * G.gy * G.gz;
    if (ncell >= ((size_t)1 << 31)) return fail(VRT_EINVAL, "search grid too large");

    DevBuf<int> d_cell, d_count, d_start, d_cur, d_unsorted, d_item, d_rec, d_flagged, d_scalars;
    int rc;
    if ((rc = d_cell.alloc((size_t)n)) || (rc = d_count.alloc(ncell)) || (rc = d_start.alloc(ncell + 1)) ||
        (rc = d_cur.alloc(ncell)) || (rc = d_unsorted.alloc((size_t)n)) || (rc = d_item.alloc((size_t)n)) ||
        (rc = d_rec.alloc((size_t)n * kRec)) || (rc = d_flagged.alloc((size_t)n)) || (rc = d_scalars.alloc(kScalars)))
        return rc;
    Event ev[4];
    for (Event &e : ev)
        if ((rc = e.create())) return rc;
    int sc[kScalars] = {INT_MAX, INT_MAX, 0, 0};
    VRT_HIP_TRY(hipMemcpyAsync(d_scalars, sc, sizeof(sc), hipMemcpyHostToDevice, st));
    VRT_HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(int) * ncell, st));
    VRT_HIP_TRY(hipEventRecord(ev[0], st));
    const int nb = grid_blocks(n);
    hipLaunchKernelGGL(k_tess_bin, dim3(nb), dim3(256), 0, st, G, d_pos, d_cell.get(), d_count.get(), d_scalars.get());
    hipLaunchKernelGGL(k_tess_scan, dim3(1), dim3(1024), 0, st, (int)ncell, d_count.get(), d_start.get(), d_cur.get());
    hipLaunchKernelGGL(k_tess_fill, dim3(nb), dim3(256), 0, st, n, d_cell.get(), d_cur.get(), d_unsorted.get());
    hipLaunchKernelGGL(k_tess_rank, dim3(nb), dim3(256), 0, st, n, d_cell.get(), d_start.get(), d_unsorted.get(), d_item.get());
    VRT_HIP_TRY(hipGetLastError());
    VRT_HIP_TRY(hipEventRecord(ev[1], st));
    VRT_HIP_TRY(hipMemcpyAsync(sc, d_scalars, sizeof(sc), hipMemcpyDeviceToHost, st));
    VRT_HIP_TRY(hipStreamSynchronize(st));
    if (sc[kBadSite] != INT_MAX) return fail(VRT_EINVAL, "site " + std::to_string((int64_t)sc[kBadSite] + 1) + " lies outside the box");

    hipLaunchKernelGGL(k_tess_cells, dim3((unsigned)n), dim3(kWave), 0, st, G, d_pos, d_start.get(), d_item.get(), d_rec.get());
    VRT_HIP_TRY(hipGetLastError());
    VRT_HIP_TRY(hipEventRecord(ev[2], st));
    hipLaunchKernelGGL(k_tess_rows, dim3(nb), dim3(256), 0, st, n, D1, d_rec.get(), d_nbr, d_flagged.get(), d_scalars.get());
    VRT_HIP_TRY(hipGetLastError());
    VRT_HIP_TRY(hipMemcpyAsync(sc, d_scalars, sizeof(sc), hipMemcpyDeviceToHost, st));
    VRT_HIP_TRY(hipStreamSynchronize(st));
    const auto grid_error = [](int64_t site0) {
        return fail(VRT_EGRID, "site " + std::to_string(site0 + 1) + " has more neighbours than the matrix holds");
    };
    if (sc[kGridSite] != INT_MAX) return grid_error(sc[kGridSite]);
    int64_t mx = sc[kMaxCount];
    const int64_t m = sc[kFlagged];
    if (m > 0) {
        // the flagged sites again, on the host, in ascending order
        std::vector<int> ids((size_t)m);
        VRT_HIP_TRY(hipMemcpyAsync(ids.data(), d_flagged, sizeof(int) * (size_t)m, hipMemcpyDeviceToHost, st));
        std::vector<double> pos_copy;
        if (!h_pos) {
            pos_copy.resize((size_t)n * 3);
            VRT_HIP_TRY(hipMemcpyAsync(pos_copy.data(), d_pos, sizeof(double) * 3 * (size_t)n, hipMemcpyDeviceToHost, st));
            h_pos = pos_copy.data();
        }
        VRT_HIP_TRY(hipStreamSynchronize(st));
        std::sort(ids.begin(), ids.end());
        std::vector<int64_t> sites(ids.begin(), ids.end()), rows((size_t)m * (size_t)D1);
        int64_t mx_host = 0;
        if ((rc = tessellate_host_sites(n, h_pos, bounds, D1, m, sites.data(), rows.data(), &mx_host, tessellate_threads(m)))) return rc;
        mx = std::max(mx, mx_host);
        DevBuf<int64_t> d_rows;
        if ((rc = d_rows.alloc(rows.size()))) return rc;
        VRT_HIP_TRY(hipMemcpyAsync(d_flagged, ids.data(), sizeof(int) * (size_t)m, hipMemcpyHostToDevice, st));
        VRT_HIP_TRY(hipMemcpyAsync(d_rows, rows.data(), sizeof(int64_t) * rows.size(), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_tess_patch, dim3(grid_blocks(m * D1)), dim3(256), 0, st, n, D1, m, d_flagged.get(), d_rows.get(), d_nbr);
        VRT_HIP_TRY(hipGetLastError());
        VRT_HIP_TRY(hipEventRecord(ev[3], st));
        VRT_HIP_TRY(hipStreamSynchronize(st));          // rows and ids are read until here
    } else {
        VRT_HIP_TRY(hipEventRecord(ev[3], st));
        VRT_HIP_TRY(hipStreamSynchronize(st));
    }
    for (int k = 0; k < 3; k++) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev[k], ev[k + 1]) == hipSuccess) g_phase_ms[k] = ms;
    }
    g_phase_sites = n;
    if (max_count) *max_count = mx;
    if (host_sites) *host_sites = m;
    return VRT_OK;
}

}  // namespace
}  // namespace vrt

using namespace vrt;

extern "C" int vrt_tessellate_gpu(int device, int64_t n, const double *pos_zxy, const double bounds[6], int64_t D1, int64_t *nbr,
                                  int64_t *max_count, int64_t *host_sites)
{
    return guarded([&]() -> int {
        int rc = tess_checks(n, pos_zxy, bounds, D1, nbr);
        if (rc) return rc;
        if ((rc = use_device(device))) return rc;
        DevBuf<double> d_pos;
        DevBuf<int64_t> d_nbr;
        if ((rc = d_pos.alloc((size_t)n * 3)) || (rc = d_nbr.alloc((size_t)n * (size_t)D1))) return rc;
        if (hipMemcpy(d_pos, pos_zxy, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess)
            return fail(VRT_ENODEVICE, "HIP error uploading the positions");
        int64_t mx = 0, m = 0;
        if ((rc = tessellate_device(n, d_pos, pos_zxy, bounds, D1, d_nbr, &mx, &m, nullptr))) return rc;
        // on an error nbr is left as it was; the columns beyond the longest row are zero
        const size_t filled = (size_t)n * (size_t)std::min<int64_t>(mx + 1, D1);
        if (hipMemcpy(nbr, d_nbr, sizeof(int64_t) * filled, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(VRT_ENODEVICE, "HIP error downloading the neighbour matrix");
        std::fill(nbr + filled, nbr + (size_t)n * (size_t)D1, (int64_t)0);
        if (max_count) *max_count = mx;
        if (host_sites) *host_sites = m;
        return VRT_OK;
    });
}

extern "C" int vrt_tessellate_dev(int device, int64_t n, const double *d_pos_zxy, const double bounds[6], int64_t D1,
                                  int64_t *d_nbr, int64_t *max_count, int64_t *host_sites, void *stream)
{
    return guarded([&]() -> int {
        int rc = tess_checks(n, d_pos_zxy, bounds, D1, d_nbr);
        if (rc) return rc;
        if ((rc = use_device(device))) return rc;
        return tessellate_device(n, d_pos_zxy, nullptr, bounds, D1, d_nbr, max_count, host_sites, (hipStream_t)stream);
    });
}

extern "C" int vrt_tessellate_last_phases(int64_t *n, double *grid_ms, double *cells_ms, double *rows_ms)
{
    if (!n && !grid_ms && !cells_ms && !rows_ms) return fail(VRT_EINVAL, "NULL argument");
    if (n) *n = g_phase_sites;
    if (grid_ms) *grid_ms = g_phase_ms[0];
    if (cells_ms) *cells_ms = g_phase_ms[1];
    if (rows_ms) *rows_ms = g_phase_ms[2];
    return VRT_OK;
}

extern "C" int64_t vrt_tessellate_capacity(void) { return kF; }
