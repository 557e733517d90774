// Stand-alone host program for csrc/vrt_source_store.h, the owner of a Λ-iteration session's S and J in its three storage
// forms.  Built by tests/test_source_store_host.py with g++ -fsanitize=address,undefined and run as a child process.  The
// HIP calls behind the store are faked below (device memory is malloc, a copy is memcpy, hipMalloc can be told to fail at
// its k-th call), and so are the few layout and convert launches, on a plan whose sweep orders are the identity (up) and
// the reversal (down).  What no GPU test reaches is covered here: an allocation that fails at every position in turn during
// create and during stage.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "vrt_source_store.h"

namespace {
std::map<void *, size_t> live_dev;      // address -> bytes
long bad_release = 0, mallocs = 0, fail_at = -1;
std::string last_error;
int checks = 0;
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
    return hipSuccess;
}
hipError_t hipMemcpy2DAsync(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height, hipMemcpyKind,
                            hipStream_t)
{
    for (size_t r = 0; r < height; r++) std::memcpy((char *)dst + r * dpitch, (const char *)src + r * spitch, width);
    return hipSuccess;
}
hipError_t hipMemsetAsync(void *dst, int value, size_t bytes, hipStream_t)
{
    std::memset(dst, value, bytes);
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t) { return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
hipError_t hipHostFree(void *) { return hipSuccess; }
hipError_t hipGetDevice(int *d) { *d = 0; return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
const char *hipGetErrorString(hipError_t) { return "error"; }
void vrt_plan_destroy(vrt_plan *) {}
void vrt_grid_destroy(vrt_grid *) {}
int64_t vrt_plan_native_plane_count(const vrt_plan *p, int64_t nlam) { return (nlam + 1) / 2 * 2 * p->g->n; }
}

namespace vrt {
void set_error(const std::string &msg) { last_error = msg; }
int fail(int code, const std::string &msg)
{
    last_error = msg;
    return code;
}
void raster_locator_delete(RasterLocator *) {}
int native_planes_ok(const vrt_plan *, bool) { return VRT_OK; }

// plane sets [pair][pos][2]; position = site in the up order, n - 1 - site in the down order; padding wavelength zero
template <typename T>
int to_planes(const vrt_plan *p, int64_t nlam, int64_t ld, const T *in, T *up, T *down)
{
    const int64_t n = p->g->n, npair = (nlam + 1) / 2;
    for (int64_t q = 0; q < npair; q++)
        for (int64_t i = 0; i < n; i++)
            for (int h = 0; h < 2; h++) {
                const T v = 2 * q + h < nlam ? in[i * ld + 2 * q + h] : (T)0;
                if (up) up[(q * n + i) * 2 + h] = v;
                if (down) down[(q * n + (n - 1 - i)) * 2 + h] = v;
            }
    return VRT_OK;
}
template <typename T>
int from_plane(const vrt_plan *p, int dir, int64_t nlam, int64_t ld, const T *in, T *out, const T *add_down = nullptr)
{
    const int64_t n = p->g->n;
    for (int64_t i = 0; i < n; i++)
        for (int64_t l = 0; l < nlam; l++) {
            T v = in[((l / 2) * n + (dir ? n - 1 - i : i)) * 2 + (l & 1)];
            if (add_down) v += add_down[((l / 2) * n + (n - 1 - i)) * 2 + (l & 1)];
            out[i * ld + l] = v;
        }
    return VRT_OK;
}
int planes_to_native(vrt_plan *p, int64_t nlam, int64_t ld, const double *in, double *up, double *down, hipStream_t) { return to_planes(p, nlam, ld, in, up, down); }
int planes_to_native_f32(vrt_plan *p, int64_t nlam, int64_t ld, const float *in, float *up, float *down, hipStream_t) { return to_planes(p, nlam, ld, in, up, down); }
int plane_from_native(vrt_plan *p, int dir, int64_t nlam, int64_t ld, const double *in, double *out, hipStream_t) { return from_plane(p, dir, nlam, ld, in, out); }
int plane_from_native_f32(vrt_plan *p, int dir, int64_t nlam, int64_t ld, const float *in, float *out, hipStream_t) { return from_plane(p, dir, nlam, ld, in, out); }
int J_from_native(vrt_plan *p, int64_t nlam, int64_t ld, const double *up, const double *down, double *J, hipStream_t) { return from_plane(p, 0, nlam, ld, up, J, down); }
int J_from_native_f32(vrt_plan *p, int64_t nlam, int64_t ld, const float *up, const float *down, float *J, hipStream_t) { return from_plane(p, 0, nlam, ld, up, J, down); }
int launch_round_to_f32(size_t count, const double *src, float *dst, hipStream_t)
{
    for (size_t i = 0; i < count; i++) dst[i] = (float)src[i];
    return VRT_OK;
}
int launch_widen_f32(size_t count, const float *src, double *dst, hipStream_t)
{
    for (size_t i = 0; i < count; i++) dst[i] = (double)src[i];
    return VRT_OK;
}
int launch_ng_mirror(vrt_grid *g, int64_t nlam, const double *up, double *down, hipStream_t)
{
    const int64_t n = g->n, npair = (nlam + 1) / 2;
    for (int64_t q = 0; q < npair; q++)
        for (int64_t i = 0; i < n; i++)
            for (int h = 0; h < 2; h++) down[(q * n + (n - 1 - i)) * 2 + h] = up[(q * n + i) * 2 + h];
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

constexpr int64_t kN = 5;
const char *form_name(SourceStore::Form f) { return f == SourceStore::kRows ? "rows" : f == SourceStore::kPlanes ? "planes" : "planes f32"; }

// how many live allocations have `bytes` bytes
long live_of(size_t bytes)
{
    long c = 0;
    for (const auto &kv : live_dev) c += kv.second == bytes;
    return c;
}

// the addresses of everything a store hands out
std::vector<const void *> handles(const SourceStore &s)
{
    return {s.S_plane(0), s.S_plane(1), s.J_plane(0), s.J_plane(1), s.S_plane<float>(0), s.S_plane<float>(1), s.J_plane<float>(0),
            s.J_plane<float>(1), s.S_new(), s.S_old(), s.J_rows()};
}

// B_0[i, l]: positive, not representable in float (so that the fp32 form's rounding shows)
double b0(int64_t i, int64_t l) { return 1.0 + 0.1 * (double)i + 0.001 * (double)l + 1e-12; }

void check_form(vrt_plan *plan, SourceStore::Form form, int64_t nlam)
{
    const size_t rows = (size_t)(kN * nlam), planes = (size_t)((nlam + 1) / 2 * 2 * kN);
    const bool f32 = form == SourceStore::kPlanesF32;
    const size_t esz = f32 ? sizeof(float) : sizeof(double);
    std::vector<double> B0(rows);
    for (int64_t i = 0; i < kN; i++)
        for (int64_t l = 0; l < nlam; l++) B0[(size_t)(i * nlam + l)] = b0(i, l);
    auto as_kept = [&](double v) { return f32 ? (double)(float)v : v; };
    CHECK(live_dev.empty());

    // ---- create: a hipMalloc that fails at every position in turn leaves nothing allocated and the store what it was
    long n_alloc = 0;
    for (long k = 0;; k++) {
        SourceStore s;
        mallocs = 0; fail_at = k;
        const int rc = s.create(plan, nlam, form, B0.data(), nullptr);
        fail_at = -1;
        if (!rc) { n_alloc = mallocs; break; }
        CHECK(rc == VRT_ENOMEM && live_dev.empty() && bad_release == 0);
        for (const void *h : handles(s)) CHECK(h == nullptr);
        CHECK(k < 16);
    }
    CHECK(live_dev.empty() && bad_release == 0);             // (the store that came up went out of scope above)

    SourceStore s;
    CHECK(s.create(plan, nlam, form, B0.data(), nullptr) == VRT_OK);
    CHECK(s.form() == form && s.two_orders() == (form != SourceStore::kRows));
    // ---- which buffers exist, and how large
    if (form == SourceStore::kRows) {
        CHECK(n_alloc == 3 && live_dev.size() == 3 && live_of(rows * sizeof(double)) == 3);
        CHECK(s.S_new() && s.S_old() && s.J_rows() && !s.S_plane(0) && !s.J_plane(1) && !s.S_plane<float>(0));
        for (size_t t = 0; t < rows; t++) CHECK(s.S_new()[t] == B0[t] && s.S_old()[t] == 0.0 && s.J_rows()[t] == 0.0);
    } else {
        CHECK(live_dev.size() == 4 && live_of(planes * esz) == 4);       // (an odd nlam: the padding plane is there)
        CHECK(n_alloc == (f32 ? 5 : 4));                                 // (float storage: B_0 rounded in scratch that is gone)
        CHECK(!s.S_new() && !s.S_old() && !s.J_rows());
        CHECK(f32 ? (s.S_plane<float>(0) && s.J_plane<float>(1) && !s.S_plane(0)) : (s.S_plane(0) && s.J_plane(1) && !s.S_plane<float>(0)));
        for (int64_t q = 0; q < (nlam + 1) / 2; q++)
            for (int64_t i = 0; i < kN; i++)
                for (int h = 0; h < 2; h++) {
                    const double want = 2 * q + h < nlam ? as_kept(b0(i, 2 * q + h)) : 0.0;
                    const size_t up = (size_t)((q * kN + i) * 2 + h), down = (size_t)((q * kN + (kN - 1 - i)) * 2 + h);
                    if (f32) CHECK(s.S_plane<float>(0)[up] == (float)want && s.S_plane<float>(1)[down] == (float)want && s.J_plane<float>(0)[up] == 0.0f);
                    else CHECK(s.S_plane(0)[up] == want && s.S_plane(1)[down] == want && s.J_plane(0)[up] == 0.0 && s.J_plane(1)[down] == 0.0);
                }
    }
    // ---- what a sweep is handed
    const double w[1] = {1.0};
    const ExecArgs x = s.exec_args(&w, 3, &w, w, nullptr);
    CHECK(x.nlam == nlam && x.f32 == f32 && x.native == (form != SourceStore::kRows) && x.I0[1] == nullptr && x.alpha_mode == 3);
    if (form == SourceStore::kRows) CHECK(x.S == s.S_new() && x.J == s.J_rows() && x.ld == nlam);
    else if (f32) CHECK(x.S_nat[0] == s.S_plane<float>(0) && x.S_nat[1] == s.S_plane<float>(1) && x.J_nat[1] == s.J_plane<float>(1));
    else CHECK(x.S_nat[0] == s.S_plane(0) && x.S_nat[1] == s.S_plane(1) && x.J_nat[0] == s.J_plane(0) && x.J_nat[1] == s.J_plane(1));

    // ---- download: S as kept, into a column block of wider host rows; the scratch is gone afterwards
    {
        const int64_t ld = nlam + 3, col0 = 2;
        std::vector<double> S((size_t)(kN * ld), -1.0), J((size_t)(kN * ld), -1.0);
        const size_t before = live_dev.size();
        CHECK(s.download(J.data(), S.data(), ld, col0, nullptr) == VRT_OK && live_dev.size() == before);
        for (int64_t i = 0; i < kN; i++)
            for (int64_t c = 0; c < ld; c++) {
                const bool in = c >= col0 && c < col0 + nlam;
                CHECK(S[(size_t)(i * ld + c)] == (in ? as_kept(b0(i, c - col0)) : -1.0) && J[(size_t)(i * ld + c)] == (in ? 0.0 : -1.0));
            }
        std::vector<double> dense((size_t)(kN * nlam));
        CHECK(s.download(nullptr, dense.data(), nlam, 0, nullptr) == VRT_OK);
        for (size_t t = 0; t < rows; t++) CHECK(dense[t] == as_kept(B0[t]));
    }

    // ---- stage: a hipMalloc that fails at every position in turn leaves the store's addresses and values unchanged, and
    // every staged buffer is released exactly once
    std::vector<double> S2(rows);
    for (size_t t = 0; t < rows; t++) S2[t] = 2.0 * B0[t] + 1e-9;
    const std::vector<const void *> before = handles(s);
    const std::map<void *, size_t> live_before = live_dev;
    for (long k = 0;; k++) {
        int rc;
        {
            SourceStore::Staged sg;
            mallocs = 0; fail_at = k;
            rc = s.stage(S2.data(), nlam, 0, sg, nullptr);
            fail_at = -1;
            CHECK(handles(s) == before);
        }
        CHECK(live_dev == live_before && bad_release == 0);
        if (!rc) { CHECK(mallocs == (form == SourceStore::kRows ? 1 : f32 ? 4 : 3)); break; }
        CHECK(rc == VRT_ENOMEM && k < 16);
    }
    {
        std::vector<double> dense(rows);
        CHECK(s.download(nullptr, dense.data(), nlam, 0, nullptr) == VRT_OK);
        for (size_t t = 0; t < rows; t++) CHECK(dense[t] == as_kept(B0[t]));
    }
    // ---- adopt: pointer swaps only; the old buffers go with the staged set, exactly once
    {
        SourceStore::Staged sg;
        CHECK(s.stage(S2.data(), nlam, 0, sg, nullptr) == VRT_OK);
        const void *st0 = f32 ? (const void *)sg.Sf[0].p : (const void *)sg.S[0].p;
        const void *st1 = f32 ? (const void *)sg.Sf[1].p : (const void *)sg.S[1].p;
        const size_t live_staged = live_dev.size();
        mallocs = 0;
        s.adopt(sg);
        CHECK(mallocs == 0 && live_dev.size() == live_staged);
        const std::vector<const void *> after = handles(s);
        if (form == SourceStore::kRows) {
            CHECK(s.S_new() == st0 && sg.S[0].p == before[8] && s.S_old() == before[9] && s.J_rows() == before[10]);
        } else {
            const int o = f32 ? 4 : 0;
            CHECK(after[(size_t)o] == st0 && after[(size_t)o + 1] == st1);
            CHECK((f32 ? (const void *)sg.Sf[0].p : (const void *)sg.S[0].p) == before[(size_t)o]);
            CHECK((f32 ? (const void *)sg.Sf[1].p : (const void *)sg.S[1].p) == before[(size_t)o + 1]);
            CHECK(after[(size_t)o + 2] == before[(size_t)o + 2] && after[(size_t)o + 3] == before[(size_t)o + 3]);      // J stays
        }
    }
    CHECK(live_dev.size() == live_before.size() && bad_release == 0);
    for (const void *h : before)
        if (h && h != before[form == SourceStore::kRows ? 8 : f32 ? 4 : 0] && h != before[form == SourceStore::kRows ? 8 : f32 ? 5 : 1])
            CHECK(live_dev.count(const_cast<void *>(h)) == 1);
    {
        std::vector<double> dense(rows);
        CHECK(s.download(nullptr, dense.data(), nlam, 0, nullptr) == VRT_OK);
        for (size_t t = 0; t < rows; t++) CHECK(dense[t] == as_kept(S2[t]));
        if (form != SourceStore::kRows && (nlam & 1))        // the padding wavelength of the staged planes: zero as at create
            for (int64_t i = 0; i < kN; i++) {
                const size_t t = (size_t)(((nlam / 2) * kN + i) * 2 + 1);
                CHECK(f32 ? s.S_plane<float>(0)[t] == 0.0f && s.S_plane<float>(1)[t] == 0.0f : s.S_plane(0)[t] == 0.0 && s.S_plane(1)[t] == 0.0);
            }
    }

    // ---- what Ng works on
    if (f32) {
        CHECK(s.ng_check() == VRT_EINVAL && last_error.find("not on a float-storage session") != std::string::npos);
    } else {
        CHECK(s.ng_check() == VRT_OK);
        const bool sweep = form == SourceStore::kPlanes;
        CHECK(s.ng_S().p == (sweep ? s.S_plane(0) : s.S_new()) && s.ng_count() == (sweep ? planes : rows));
        const NgRange a = s.ng_range(), b = ng_S_range(kN, nlam, sweep);
        CHECK(a.dense == b.dense && a.tail == b.tail && a.tstride == b.tstride);
        if (sweep) {                                         // the down-order copy follows the up-order one, value for value
            for (size_t t = 0; t < planes; t++) s.S_plane(0)[t] = 7.0 + (double)t;
            CHECK(s.mirror_down(nullptr) == VRT_OK);
            std::vector<double> from_down(rows), from_up(rows);
            CHECK(plane_from_native(plan, 1, nlam, nlam, s.S_plane(1), from_down.data(), nullptr) == VRT_OK);
            CHECK(plane_from_native(plan, 0, nlam, nlam, s.S_plane(0), from_up.data(), nullptr) == VRT_OK);
            CHECK(from_down == from_up);
        }
    }

    // ---- the arrays beside S: rows stay rows, planes take the up order (and come back value for value)
    if (!f32) {
        DevBuf<double> a, tmp;
        CHECK(upload(a, B0.data(), rows, nullptr) == VRT_OK);
        const double *was = a.p, *back = nullptr;
        CHECK(s.to_up_order(a, nullptr) == VRT_OK);
        CHECK(form == SourceStore::kRows ? a.p == was : live_dev.at(a.p) == planes * sizeof(double));
        CHECK(s.rows_of(a, tmp, &back, nullptr) == VRT_OK && (form == SourceStore::kRows ? back == a.p && !tmp.p : back == tmp.p));
        for (size_t t = 0; t < rows; t++) CHECK(back[t] == B0[t]);
        DevBuf<double> al;
        int mode = -1;
        CHECK(upload(al, B0.data(), rows, nullptr) == VRT_OK && s.to_sweep_alpha(al, &mode, nullptr) == VRT_OK);
        CHECK(form == SourceStore::kRows ? mode == VRT_ALPHA_SITE_LAM && live_dev.at(al.p) == rows * sizeof(double)
                                         : mode == VRT_ALPHA_SITE_LAM_NATIVE && live_dev.at(al.p) == 2 * planes * sizeof(double));
    } else {
        DevBuf<double> a;
        DevBuf<float> af;
        CHECK(upload(a, B0.data(), rows, nullptr) == VRT_OK && s.to_up_order(a, af, nullptr) == VRT_OK);
        CHECK(!a.p && live_dev.at(af.p) == planes * sizeof(float) && af.p[0] == (float)B0[0]);
        CHECK(s.to_up_order(a, nullptr) == VRT_EINVAL);
    }
    std::printf("ok %s, nlam %d\n", form_name(form), (int)nlam);
}

}  // namespace

int main()
{
    {
        vrt_grid grid;
        grid.n = kN;
        vrt_plan plan;
        plan.g = &grid;
        plan.A = 1;
        CHECK(SourceStore::plan_keeps_planes(&plan));
        plan.A = 0;
        CHECK(!SourceStore::plan_keeps_planes(&plan));
        plan.A = 1; plan.tune.lambda_native = 0;
        CHECK(!SourceStore::plan_keeps_planes(&plan));
        plan.tune.lambda_native = 1; plan.tune.path = 2;
        CHECK(!SourceStore::plan_keeps_planes(&plan));
        plan.tune.path = 0;
        for (SourceStore::Form form : {SourceStore::kRows, SourceStore::kPlanes, SourceStore::kPlanesF32})
            for (int64_t nlam : {3, 4}) {
                check_form(&plan, form, nlam);
                CHECK(live_dev.empty() && bad_release == 0);
            }
        // a store that was never created (a member without wavelengths) holds nothing and has nothing to take home
        SourceStore none;
        double x = -1.0;
        CHECK(none.download(&x, &x, 1, 0, nullptr) == VRT_OK && x == -1.0 && none.ng_count() == 0 && !none.J_rows() && !none.J_plane(0));
    }
    CHECK(live_dev.empty() && bad_release == 0);
    std::printf("%d checks passed; no allocation outlived a failed create or stage\n", checks);
    return 0;
}
