// Stand-alone host program for csrc/vrt_raster_store.h, the owner of a raster Λ-iteration session's S and J, and for the two
// pieces of csrc/vrt_internal.h that every single-device session calls after its update: read_criterion and
// ng_after_update.  Built by tests/test_raster_store_host.py with g++ -fsanitize=address,undefined and run as a child
// process.  The HIP calls behind the store are faked below (device memory is malloc, a copy is memcpy, hipMalloc can be told
// to fail at its k-th call), and so are the three layout launches, as plain loops over the documented layouts: (n, nlam)
// rows in Julia point order (point i = iz + nz (ix + nx iy)), planes [l][iz][iy][ix], bottom planes [l][iy][ix].  The device
// halves of an Ng step are played by the program, which hands out the verdict.  What no GPU test reaches is covered here: an
// allocation that fails at every position in turn during create and during stage, and a rejected step.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "vrt_raster_store.h"

namespace {
std::map<void *, size_t> live_dev;      // address -> bytes
long bad_release = 0, mallocs = 0, fail_at = -1, syncs = 0, to_planes_calls = 0;
size_t last_copy_bytes = 0;
std::string last_error;
int checks = 0;
bool ng_verdict = true, ng_valid = true;        // what the apply kernel and the coefficients of the next due step report
size_t ng_seen_count = 0;                       // what ng_after_iterate was handed last
vrt::NgRange ng_seen_range;
}  // namespace

// ---- the fake runtime ------------------------------------------------------------------------------------------------
extern "C" {
hipError_t hipMalloc(void **p, size_t bytes)
{
    if (mallocs++ == fail_at) { *p = nullptr; return hipErrorOutOfMemory; }
    *p = std::malloc(bytes);
    live_dev[*p] = bytes;
    return hipSuccess;
}
hipError_t hipFree(void *p)
{
    if (!live_dev.erase(p)) { bad_release++; return hipErrorInvalidValue; }
    std::free(p);
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind, hipStream_t)
{
    std::memcpy(dst, src, bytes);
    last_copy_bytes = bytes;
    return hipSuccess;
}
hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind)
{
    std::memcpy(dst, src, bytes);
    return hipSuccess;
}
hipError_t hipMemsetAsync(void *dst, int value, size_t bytes, hipStream_t)
{
    std::memset(dst, value, bytes);
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t) { syncs++; return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t) { return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
hipError_t hipHostFree(void *) { return hipSuccess; }
hipError_t hipGetDevice(int *d) { *d = 0; return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
const char *hipGetErrorString(hipError_t) { return "error"; }
void vrt_plan_destroy(vrt_plan *) {}
void vrt_grid_destroy(vrt_grid *) {}
}

namespace vrt {
void set_error(const std::string &msg) { last_error = msg; }
int fail(int code, const std::string &msg)
{
    last_error = msg;
    return code;
}
void raster_locator_delete(RasterLocator *) {}

int launch_to_planes(const vrt_regular *r, int64_t nlam, const double *in, double *out, hipStream_t)
{
    to_planes_calls++;
    const int64_t nz = r->nz, nx = r->nx, ny = r->ny, vol = nz * nx * ny;
    for (int64_t l = 0; l < nlam; l++)
        for (int64_t iz = 0; iz < nz; iz++)
            for (int64_t iy = 0; iy < ny; iy++)
                for (int64_t ix = 0; ix < nx; ix++) out[l * vol + ix + nx * (iy + ny * iz)] = in[(iz + nz * (ix + nx * iy)) * nlam + l];
    return VRT_OK;
}
int launch_from_planes(const vrt_regular *r, int64_t nlam, const double *in, double *out, hipStream_t)
{
    const int64_t nz = r->nz, nx = r->nx, ny = r->ny, vol = nz * nx * ny;
    for (int64_t l = 0; l < nlam; l++)
        for (int64_t iz = 0; iz < nz; iz++)
            for (int64_t iy = 0; iy < ny; iy++)
                for (int64_t ix = 0; ix < nx; ix++) out[(iz + nz * (ix + nx * iy)) * nlam + l] = in[l * vol + ix + nx * (iy + ny * iz)];
    return VRT_OK;
}
int launch_bottom_planes(const vrt_regular *r, int64_t nlam, const double *B0, double *out, hipStream_t)
{
    const int64_t nz = r->nz, nx = r->nx, ny = r->ny;
    for (int64_t l = 0; l < nlam; l++)
        for (int64_t iy = 0; iy < ny; iy++)
            for (int64_t ix = 0; ix < nx; ix++) out[l * nx * ny + ix + nx * iy] = B0[(nz * (ix + nx * iy)) * nlam + l];
    return VRT_OK;
}

// the phases of vrt_internal.h in the order of vrt_accel.hip's ng_after_iterate; the sums and the apply are the program's:
// x_acc is a marker (-1 everywhere), the verdicts are ng_verdict and ng_valid
int ng_after_iterate(NgState &ng, int64_t iterate, DevBuf<double> &S, size_t alloc_count, const NgRange &rg, hipStream_t st)
{
    ng_seen_count = alloc_count;
    ng_seen_range = rg;
    ng.last_applied = 0;
    const int due = ng_due(ng, iterate);
    if (due == kNgNothing) return VRT_OK;
    if (due != kNgStep) return ng_record(ng, due, S, alloc_count, st);
    if (!ng_take_history(ng)) return VRT_OK;
    ng.last_applied = -1;
    for (size_t i = 0; i < alloc_count; i++) ng.hist[2][i] = -1.0;
    NgPiece piece{&ng, &S, ng_verdict};
    if (ng_commit(&piece, 1, ng_valid)) ng.last_applied = 1;
    return VRT_OK;
}
}  // namespace vrt

using namespace vrt;

namespace {

#define CHECK(cond)                                                                  \
    do {                                                                             \
        checks++;                                                                    \
        if (!(cond)) {                                                               \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);            \
            std::exit(1);                                                            \
        }                                                                            \
    } while (0)

// how many live allocations have `bytes` bytes
long live_of(size_t bytes)
{
    long c = 0;
    for (const auto &kv : live_dev) c += kv.second == bytes;
    return c;
}

// the addresses of everything a store hands out
std::vector<const void *> handles(RasterStore &s)
{
    return {s.S_rows(), s.S_next(), s.J_rows(), s.S_planes(), s.J_planes(), s.I0_planes(), s.zero_plane(), s.ng_S().p};
}

// every byte a store's buffers hold, buffer after buffer
std::vector<char> contents(RasterStore &s)
{
    std::vector<char> all;
    for (const void *h : handles(s)) {
        const char *b = (const char *)h;
        all.insert(all.end(), b, b + live_dev.at(const_cast<void *>(h)));
    }
    return all;
}

struct Raster {
    int64_t nz, nx, ny, nlam;
};

double b0(int64_t i, int64_t l) { return 1.0 + 0.1 * (double)i + 0.001 * (double)l; }

// is `pl` ([l][iz][iy][ix]) the transpose of `rows` ((n, nlam), Julia point order)?  Written out from the layouts' words.
bool planes_of(const Raster &g, const double *pl, const double *rows)
{
    const int64_t vol = g.nz * g.nx * g.ny;
    for (int64_t iy = 0; iy < g.ny; iy++)
        for (int64_t ix = 0; ix < g.nx; ix++)
            for (int64_t iz = 0; iz < g.nz; iz++)
                for (int64_t l = 0; l < g.nlam; l++) {
                    const int64_t point = iz + g.nz * (ix + g.nx * iy), pos = ix + g.nx * (iy + g.ny * iz);
                    if (pl[l * vol + pos] != rows[point * g.nlam + l]) return false;
                }
    return true;
}

void check_raster(const Raster &g)
{
    vrt_regular reg;
    reg.nz = g.nz; reg.nx = g.nx; reg.ny = g.ny;
    const int64_t n = g.nz * g.nx * g.ny, plane = g.nx * g.ny, nlam = g.nlam;
    const size_t rows = (size_t)(n * nlam), row_bytes = rows * sizeof(double);
    const size_t i0_bytes = (size_t)(plane * nlam) * sizeof(double), zero_bytes = (size_t)plane * sizeof(double);
    std::vector<double> B0(rows);
    for (int64_t i = 0; i < n; i++)
        for (int64_t l = 0; l < nlam; l++) B0[(size_t)(i * nlam + l)] = b0(i, l);
    CHECK(live_dev.empty());

    // ---- create: a hipMalloc that fails at every position in turn leaves nothing allocated and a fresh store empty
    long n_alloc = 0;
    for (long k = 0;; k++) {
        RasterStore s;
        mallocs = 0; fail_at = k;
        const int rc = s.create(&reg, nlam, B0.data(), nullptr);
        fail_at = -1;
        if (!rc) { n_alloc = mallocs; break; }
        CHECK(rc == VRT_ENOMEM && live_dev.empty() && bad_release == 0);
        for (const void *h : handles(s)) CHECK(h == nullptr);
        CHECK(s.ng_count() == 0 && k < 16);
    }
    CHECK(n_alloc == 7 && live_dev.empty() && bad_release == 0);   // (the store that came up went out of scope above)

    RasterStore s;
    CHECK(s.create(&reg, nlam, B0.data(), nullptr) == VRT_OK);
    // ---- which buffers exist, and how large: S twice, J, S and J plane-major; the I_0 planes; the zero plane
    CHECK(live_dev.size() == 7 && live_of(row_bytes) == 5 && live_of(i0_bytes) == 1 && live_of(zero_bytes) == 1);
    for (const void *h : handles(s)) CHECK(h != nullptr);
    CHECK(s.S_rows() != s.S_next() && s.ng_S().p == s.S_rows());
    CHECK(live_dev.at((void *)s.I0_planes()) == i0_bytes && live_dev.at((void *)s.zero_plane()) == zero_bytes);
    for (size_t t = 0; t < rows; t++) CHECK(s.S_rows()[t] == B0[t] && s.J_rows()[t] == 0.0);
    CHECK(planes_of(g, s.S_planes(), B0.data()));
    for (int64_t q = 0; q < plane; q++) {
        CHECK(s.zero_plane()[q] == 0.0);
        for (int64_t l = 0; l < nlam; l++) CHECK(s.I0_planes()[l * plane + q] == b0(g.nz * q, l));     // point (iz = 0, q)
    }
    // ... and a create that fails on a store that is up leaves it bit for bit what it was
    {
        const std::vector<const void *> before = handles(s);
        const std::vector<char> bytes_before = contents(s);
        const std::map<void *, size_t> live_before = live_dev;
        std::vector<double> other(rows, 9.0);
        for (long k = 0; k < n_alloc; k++) {
            mallocs = 0; fail_at = k;
            CHECK(s.create(&reg, nlam, other.data(), nullptr) == VRT_ENOMEM);
            fail_at = -1;
            CHECK(handles(s) == before && contents(s) == bytes_before && live_dev == live_before && bad_release == 0);
        }
    }

    // ---- J_home, S_written, download: the update's buffer becomes the current S and the solves' copy follows it
    std::vector<double> S1(rows), J1(rows);
    for (size_t t = 0; t < rows; t++) { S1[t] = 3.0 * B0[t] + 0.5; J1[t] = 0.25 * B0[t]; }
    {
        for (int64_t l = 0; l < nlam; l++)                    // J as the solves leave it, plane-major
            for (int64_t p = 0; p < n; p++) s.J_planes()[l * n + p] = -7.0;
        launch_to_planes(&reg, nlam, J1.data(), s.J_planes(), nullptr);
        CHECK(s.J_home(nullptr) == VRT_OK);
        for (size_t t = 0; t < rows; t++) CHECK(s.J_rows()[t] == J1[t]);
        const double *cur = s.S_rows();
        double *next = s.S_next();
        std::memcpy(next, S1.data(), row_bytes);              // the update's write
        CHECK(s.S_rows() == cur && planes_of(g, s.S_planes(), B0.data()));     // nothing moves before S_written
        CHECK(s.S_written(nullptr) == VRT_OK);
        CHECK(s.S_rows() == next && s.S_next() == cur && s.ng_S().p == next && planes_of(g, s.S_planes(), S1.data()));
        std::vector<double> S(rows, -1.0), J(rows, -1.0);
        const long syncs_before = syncs;
        CHECK(s.download(J.data(), S.data(), nullptr) == VRT_OK && syncs == syncs_before + 1);
        CHECK(S == S1 && J == J1);
        std::vector<double> only(rows, -1.0);
        CHECK(s.download(nullptr, only.data(), nullptr) == VRT_OK && only == S1);
        // another array of the store's shape, home through the store (a line session's Λ*)
        std::vector<double> pl(rows), back(rows, -1.0);
        launch_to_planes(&reg, nlam, B0.data(), pl.data(), nullptr);
        CHECK(s.rows_from_planes(pl.data(), back.data(), nullptr) == VRT_OK && back == B0);
    }

    // ---- stage: a hipMalloc that fails at every position in turn leaves the store's addresses and values unchanged, and
    // every staged buffer is released exactly once
    std::vector<double> S2(rows);
    for (size_t t = 0; t < rows; t++) S2[t] = 2.0 * B0[t] + 1e-9;
    const std::vector<const void *> before = handles(s);
    const std::vector<char> bytes_before = contents(s);
    const std::map<void *, size_t> live_before = live_dev;
    for (long k = 0;; k++) {
        int rc;
        {
            RasterStore::Staged sg;
            mallocs = 0; fail_at = k;
            rc = s.stage(S2.data(), sg, nullptr);
            fail_at = -1;
            CHECK(handles(s) == before && contents(s) == bytes_before);     // untouched until adopt, staged or not
        }
        CHECK(live_dev == live_before && bad_release == 0);
        if (!rc) { CHECK(mallocs == 2); break; }
        CHECK(rc == VRT_ENOMEM && k < 16);
    }
    // ---- adopt: pointer swaps only; the old rows and planes go with the staged set, exactly once
    {
        RasterStore::Staged sg;
        CHECK(s.stage(S2.data(), sg, nullptr) == VRT_OK);
        const void *st_rows = sg.rows.p, *st_planes = sg.planes.p;
        const size_t live_staged = live_dev.size();
        mallocs = 0;
        s.adopt(sg);
        CHECK(mallocs == 0 && live_dev.size() == live_staged);
        const std::vector<const void *> after = handles(s);
        CHECK(after[0] == st_rows && after[3] == st_planes && after[7] == st_rows);
        CHECK(sg.rows.p == before[0] && sg.planes.p == before[3]);
        for (size_t h : {1, 2, 4, 5, 6}) CHECK(after[h] == before[h]);       // the other S buffer, J, I_0, the zero plane stay
    }
    CHECK(live_dev.size() == live_before.size() && bad_release == 0);
    CHECK(!live_dev.count(const_cast<void *>(before[0])) && !live_dev.count(const_cast<void *>(before[3])));
    for (size_t h : {1, 2, 4, 5, 6}) CHECK(live_dev.count(const_cast<void *>(before[h])) == 1);
    {
        std::vector<double> S(rows), J(rows);
        CHECK(s.download(J.data(), S.data(), nullptr) == VRT_OK && S == S2 && J == J1);
        CHECK(planes_of(g, s.S_planes(), S2.data()));
    }

    // ---- what Ng works on: all n nlam doubles, the pairs dense and -- odd -- one more
    CHECK(s.ng_count() == rows);
    const NgRange rg = s.ng_range();
    CHECK(rg.dense == ((n * nlam) & ~(int64_t)1) && rg.tail == ((n * nlam) & 1) && rg.tstride == 1);
    {
        for (size_t t = 0; t < rows; t++) s.ng_S()[t] = 7.0 + (double)t;       // rows changed underneath the planes
        std::vector<double> want(s.ng_S().p, s.ng_S().p + rows);
        bool queued = false;
        CHECK(!planes_of(g, s.S_planes(), want.data()));
        CHECK(s.ng_refresh(nullptr, &queued) == VRT_OK && queued && planes_of(g, s.S_planes(), want.data()));
    }

    // ---- ng_after_update on the store: record, record, record, an accepted step; then a rejected one
    {
        NgState ng;
        ng.order = 2; ng.start = 4; ng.period = 4;
        for (DevBuf<double> &h : ng.hist) CHECK(h.alloc(rows) == VRT_OK);
        for (int it = 1; it <= 3; it++) {
            const long syncs_before = syncs, planes_before = to_planes_calls;
            CHECK(ng_after_update(ng, it, s, nullptr) == VRT_OK && ng.last_applied == 0);
            CHECK(syncs == syncs_before && to_planes_calls == planes_before && ng.hist[3 - it][5] == 12.0);
        }
        CHECK(ng.have == 7u && ng_seen_count == rows && ng_seen_range.dense == rg.dense && ng_seen_range.tail == rg.tail &&
              ng_seen_range.tstride == 1);
        const double *S_before = s.S_rows(), *x3 = ng.hist[2].p;
        long syncs_before = syncs, planes_before = to_planes_calls;
        ng_verdict = true; ng_valid = true;
        CHECK(ng_after_update(ng, 4, s, nullptr) == VRT_OK && ng.last_applied == 1);
        CHECK(s.S_rows() == x3 && ng.hist[2].p == S_before);                 // x_acc's buffer BECAME the store's S
        CHECK(to_planes_calls == planes_before + 1 && syncs == syncs_before + 1);
        for (size_t t = 0; t < rows; t++) CHECK(s.S_rows()[t] == -1.0 && s.S_planes()[t] == -1.0);
        for (int it = 5; it <= 7; it++) CHECK(ng_after_update(ng, it, s, nullptr) == VRT_OK && ng.last_applied == 0);
        const std::vector<const void *> h_before = handles(s);
        syncs_before = syncs; planes_before = to_planes_calls;
        ng_verdict = false;
        CHECK(ng_after_update(ng, 8, s, nullptr) == VRT_OK && ng.last_applied == -1);
        CHECK(handles(s) == h_before && to_planes_calls == planes_before && syncs == syncs_before);
        ng_verdict = true;
    }
    std::printf("ok raster %d x %d x %d, nlam %d\n", (int)g.nz, (int)g.nx, (int)g.ny, (int)nlam);
}

// ---- ng_after_update against a store that only counts: when the refresh is called, and when the stream is synchronised
struct CountingStore {
    DevBuf<double> S;
    size_t count = 0;
    bool queues = true;                 // a RasterStore, a SourceStore in a plane form; false: a SourceStore in rows
    int refreshed = 0;
    DevBuf<double> &ng_S() { return S; }
    size_t ng_count() const { return count; }
    NgRange ng_range() const { return ng_S_range((int64_t)count, 1, false); }
    int ng_refresh(hipStream_t, bool *queued)
    {
        refreshed++;
        *queued = queues;
        return VRT_OK;
    }
};

void check_epilogue()
{
    CountingStore st;
    st.count = 9;
    CHECK(st.S.alloc(st.count) == VRT_OK);
    NgState ng;
    for (DevBuf<double> &h : ng.hist) CHECK(h.alloc(st.count) == VRT_OK);
    auto run = [&](int it, int want_applied, int want_refresh, long want_syncs) {
        const long s0 = syncs;
        const int r0 = st.refreshed;
        ng.last_applied = 5;                                  // (stale: every call sets it)
        CHECK(ng_after_update(ng, it, st, nullptr) == VRT_OK);
        CHECK(ng.last_applied == want_applied && st.refreshed - r0 == want_refresh && syncs - s0 == want_syncs);
    };
    // order 0: nothing but last_applied = 0, whatever the iterate number
    ng.order = 0; ng.start = 4; ng.period = 4;
    ng_seen_count = 0;
    for (int it = 1; it <= 8; it++) run(it, 0, 0, 0);
    CHECK(ng.have == 0 && ng_seen_count == 0);
    ng.order = 2;
    // switched on at iterate 2: x3 is missing, so the step due at 4 is not taken (and uses the history up)
    run(2, 0, 0, 0);
    run(3, 0, 0, 0);
    CHECK(ng.have == 3u);
    run(4, 0, 0, 0);
    CHECK(ng.have == 0);
    // record iterates, then an accepted step: refreshed exactly once, one synchronise
    for (int it = 5; it <= 7; it++) run(it, 0, 0, 0);
    CHECK(ng.have == 7u && ng_seen_count == st.count && ng_seen_range.dense == 8 && ng_seen_range.tail == 1);
    ng_verdict = true; ng_valid = true;
    run(8, 1, 1, 1);
    // a rejected step (a bad verdict; invalid coefficients): no refresh, no synchronise
    for (int it = 9; it <= 11; it++) run(it, 0, 0, 0);
    ng_verdict = false;
    run(12, -1, 0, 0);
    for (int it = 13; it <= 15; it++) run(it, 0, 0, 0);
    ng_verdict = true; ng_valid = false;
    run(16, -1, 0, 0);
    // an accepted step of a store whose refresh queues nothing (rows): called, but no synchronise
    ng_valid = true;
    st.queues = false;
    for (int it = 17; it <= 19; it++) run(it, 0, 0, 0);
    run(20, 1, 1, 0);
    std::printf("ok epilogue\n");
}

void check_read_criterion()
{
    unsigned long long words[3];
    const double crit = 0.015625;
    std::memcpy(&words[0], &crit, sizeof(double));
    words[1] = 0; words[2] = 41;
    double d = -1.0;
    int64_t third = -5;
    long s0 = syncs;
    CHECK(read_criterion(words, 3, nullptr, &d, &third) == VRT_OK && d == crit && third == 41 && syncs == s0 + 1);
    CHECK(last_copy_bytes == 3 * sizeof(words[0]));
    third = -5; d = -1.0;                                     // two words: the third is neither copied nor handed on
    CHECK(read_criterion(words, 2, nullptr, &d, &third) == VRT_OK && d == crit && third == -5);
    CHECK(last_copy_bytes == 2 * sizeof(words[0]));
    CHECK(read_criterion(words, 3, nullptr, &d) == VRT_OK && d == crit);
    words[1] = 1;                                             // the NaN flag: NaN, like Julia's maximum
    CHECK(read_criterion(words, 2, nullptr, &d, &third) == VRT_OK && std::isnan(d) && third == -5);
    std::printf("ok criterion\n");
}

}  // namespace

int main()
{
    check_raster(Raster{5, 3, 3, 3});           // n nlam = 135, odd: ng_range() has a tail
    CHECK(live_dev.empty() && bad_release == 0);
    check_raster(Raster{4, 2, 3, 4});           // 96, even
    CHECK(live_dev.empty() && bad_release == 0);
    {
        // a store that was never created holds nothing
        RasterStore none;
        CHECK(none.ng_count() == 0 && !none.J_rows() && !none.S_planes());
    }
    check_epilogue();
    check_read_criterion();
    CHECK(live_dev.empty() && bad_release == 0);
    std::printf("%d checks passed; no allocation outlived a failed create or stage\n", checks);
    return 0;
}
