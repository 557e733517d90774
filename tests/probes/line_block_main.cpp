// Stand-alone host program for csrc/vrt_line_block.h, the owner of one wavelength block of a line Λ-iteration session, and
// for csrc/vrt_multi_members.h, the per-device worker protocol of the multi-device object.  Built by
// tests/test_line_block_host.py with g++ -fsanitize=address,undefined and a second time with -fsanitize=thread, and run as
// a child process.  The HIP calls behind the headers are faked below (device memory is malloc, a copy is memcpy, hipMalloc
// can be told to fail at its k-th call, the current device and the error text are per thread as in the library), and so
// are the launches: the layout ones as plain loops on a plan whose sweep orders are the identity (up) and the reversal
// (down), the physics ones as entries in a list of calls.  What no GPU test reaches is covered here: an allocation that
// fails at every position in turn during create, and every way a member's work can end.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <thread>
#include <vector>

#include "vrt_line_block.h"
#include "vrt_multi_members.h"

namespace {
std::map<void *, size_t> live_dev;      // address -> bytes
long bad_release = 0, mallocs = 0, fail_at = -1;
thread_local std::string last_error;    // per thread, as vrt_last_error's
thread_local int current_device = -1;
std::atomic<int> checks{0};
std::vector<std::string> calls;         // the launches of a step, in order
const double *diag_rows = nullptr, *diag_planes = nullptr, *update_diag = nullptr, *small_base = nullptr;
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
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t)
{
    if (kind == hipMemcpyDeviceToDevice) calls.push_back("copy");
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
hipError_t hipGetDevice(int *d) { *d = current_device; return hipSuccess; }
hipError_t hipSetDevice(int d)
{
    if (d == 99) return hipErrorInvalidDevice;       // the one device that does not exist
    current_device = d;
    return hipSuccess;
}
const char *hipGetErrorString(hipError_t) { return "error"; }
void vrt_plan_destroy(vrt_plan *) {}
void vrt_grid_destroy(vrt_grid *) {}
const char *vrt_last_error(void) { return last_error.c_str(); }
int64_t vrt_plan_native_plane_count(const vrt_plan *p, int64_t nlam) { return (nlam + 1) / 2 * 2 * p->g->n; }
int64_t vrt_plan_native_alpha_count(const vrt_plan *p, int64_t nlam) { return (nlam + 1) / 2 * 2 * p->g->n * p->A; }
}

namespace vrt {
void set_error(const std::string &msg) { last_error = msg; }
int fail(int code, const std::string &msg)
{
    last_error = msg;
    return code;
}
void raster_locator_delete(RasterLocator *) {}
int native_planes_ok(const vrt_plan *p, bool) { return p->patch_ok ? VRT_OK : fail(VRT_EINVAL, "no planes"); }
int64_t steps_max_layer(bool) { return 4096; }

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
int launch_ng_mirror(vrt_grid *, int64_t, const double *, double *, hipStream_t) { return VRT_OK; }
template <typename T>
int gather(int64_t rows, int64_t nlam, int64_t ld, const int32_t *order, const double *src, T *dst)
{
    for (int64_t r = 0; r < rows; r++)
        for (int64_t l = 0; l < nlam; l++) dst[r * nlam + l] = (T)src[order[r] * ld + l];
    return VRT_OK;
}
int launch_gather_rows(int64_t rows, int64_t nlam, int64_t ld, const int32_t *order, const double *src, double *dst, hipStream_t) { return gather(rows, nlam, ld, order, src, dst); }
int launch_gather_rows_f32(int64_t rows, int64_t nlam, int64_t ld, const int32_t *order, const double *src, float *dst, hipStream_t) { return gather(rows, nlam, ld, order, src, dst); }

// the launches of a step: names in `calls`, and the arguments the checks below ask about
int launch_line_terms(int64_t, const double *, const double *, const double *, double, double, double, double *, double *, hipStream_t)
{
    calls.push_back("terms");
    return VRT_OK;
}
int launch_line_opacity(vrt_plan *, int64_t nlam, const double *d_lambda, double, double, const double *, const double *, const double *,
                        const double *, const double *, void *, hipStream_t, bool f32_out)
{
    calls.push_back(std::string(f32_out ? "opacity_f32 " : "opacity ") + std::to_string(nlam) + " from " + std::to_string((long)(d_lambda - small_base)));
    return VRT_OK;
}
int launch_line_lambda_diagonal(vrt_plan *, int64_t, const double *, const double *, int64_t, double *d_rows, double *d_up_planes, hipStream_t)
{
    calls.push_back("diagonal");
    diag_rows = d_rows;
    diag_planes = d_up_planes;
    return VRT_OK;
}
int execute_locked(vrt_plan *, const ExecArgs &x)
{
    calls.push_back(x.native ? (x.f32 ? "execute_planes_f32" : "execute_planes") : "execute_rows");
    return VRT_OK;
}
int launch_lambda_update(int64_t, int64_t, int64_t, const double *, const double *, const double *, const double *, double *,
                         unsigned long long *, hipStream_t, const double *d_diag)
{
    calls.push_back("update_rows");
    update_diag = d_diag;
    return VRT_OK;
}
int launch_lambda_update_native(vrt_grid *, int64_t, const double *, const double *, const double *, const double *, double *, double *,
                                unsigned long long *, hipStream_t, const double *dL_up)
{
    calls.push_back("update_planes");
    update_diag = dL_up;
    return VRT_OK;
}
int launch_lambda_update_native_f32(vrt_plan *, int64_t, const float *, const float *, const float *, const double *, float *, float *,
                                    unsigned long long *, hipStream_t)
{
    calls.push_back("update_planes_f32");
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

constexpr int64_t kN = 5, kNlam = 7, kBottom = 2;       // sites, wavelengths of the case, sites that take I_0
const int32_t kOrder[kBottom] = {3, 0};                 // the up order's first sites
size_t base_live = 0;                                   // what the grid itself holds

const char *form_name(SourceStore::Form f) { return f == SourceStore::kRows ? "rows" : f == SourceStore::kPlanes ? "planes" : "planes f32"; }

long live_of(size_t bytes)
{
    long c = 0;
    for (const auto &kv : live_dev) c += kv.second == bytes;
    return c;
}

std::vector<const void *> handles(const LineBlock &b)
{
    return {b.d_B0.p, b.d_I0.p, b.d_native.p, b.f_B0.p, b.f_I0.p, b.f_native.p, b.sj.S_plane(0), b.sj.S_plane<float>(0), b.sj.S_new()};
}

// B_0[i, l]: positive, not representable in float (so that float storage's rounding shows)
double b0(int64_t i, int64_t l) { return 1.0 + 0.1 * (double)i + 0.001 * (double)l + 1e-12; }

void check_create(vrt_plan *plan, SourceStore::Form form, int64_t l0, int64_t l1, const std::vector<double> &B0)
{
    const int64_t nb = l1 - l0;
    const bool f32 = form == SourceStore::kPlanesF32, rows_form = form == SourceStore::kRows;
    const size_t esz = f32 ? sizeof(float) : sizeof(double);
    const size_t rows = (size_t)(kN * nb), planes = (size_t)((nb + 1) / 2 * 2 * kN);
    auto as_kept = [&](double v) { return f32 ? (double)(float)v : v; };
    CHECK(live_dev.size() == base_live);

    // ---- a hipMalloc that fails at every position in turn leaves nothing allocated and a fresh block empty
    long n_alloc = 0;
    for (long k = 0;; k++) {
        LineBlock b;
        mallocs = 0; fail_at = k;
        const int rc = b.create(plan, B0.data(), kNlam, l0, l1, form, nullptr);
        fail_at = -1;
        if (!rc) { n_alloc = mallocs; break; }
        CHECK(rc == VRT_ENOMEM && live_dev.size() == base_live && bad_release == 0);
        for (const void *h : handles(b)) CHECK(h == nullptr);
        CHECK(b.nb() == 0 && !b.f32 && k < 24);
    }
    CHECK(live_dev.size() == base_live && bad_release == 0);     // (the block that came up went out of scope above)

    LineBlock b;
    CHECK(b.create(plan, B0.data(), kNlam, l0, l1, form, nullptr) == VRT_OK);
    CHECK(b.l0 == l0 && b.l1 == l1 && b.nb() == nb && b.f32 == f32);
    const size_t mine = live_dev.size() - base_live;
    if (nb == 0) {
        // the placeholders of a member without wavelengths: one element each of B_0, I_0 and α, and no store
        CHECK(n_alloc == 3 && mine == 3 && b.d_B0.p && (f32 ? b.f_I0.p && b.f_native.p && !b.d_I0.p : b.d_I0.p && b.d_native.p && !b.f_I0.p));
        CHECK(live_dev.at(b.d_B0.p) == sizeof(double) && live_dev.at(const_cast<void *>(b.I0())) == esz && live_dev.at(b.alpha()) == esz);
        CHECK(!b.sj.S_new() && !b.sj.S_plane(0) && !b.sj.S_plane<float>(0) && b.sj.ng_count() == 0);
    } else {
        // ---- which buffers exist, and how large: the store's, B_0 in its order, I_0 and α in the storage type
        const size_t nI0 = (size_t)(kBottom * nb) * esz, nnat = planes * (size_t)plan->A * esz;
        CHECK(mine == (rows_form ? 6u : 7u));
        CHECK(live_dev.at(const_cast<void *>(b.I0())) == nI0 && live_dev.at(b.alpha()) == nnat);
        CHECK(f32 ? !b.d_B0.p && !b.d_I0.p && !b.d_native.p && live_dev.at(b.f_B0.p) == planes * sizeof(float)
                  : !b.f_B0.p && !b.f_I0.p && !b.f_native.p && live_dev.at(b.d_B0.p) == (rows_form ? rows : planes) * sizeof(double));
        CHECK(live_of((rows_form ? rows : planes) * esz) >= (rows_form ? 4 : 5));
        CHECK(b.sj.form() == form);
        // S = the block's columns of B_0, as kept; J = 0
        std::vector<double> S((size_t)(kN * nb), -1.0), J((size_t)(kN * nb), -1.0);
        CHECK(b.sj.download(J.data(), S.data(), nb, 0, nullptr) == VRT_OK);
        for (int64_t i = 0; i < kN; i++)
            for (int64_t c = 0; c < nb; c++) CHECK(S[(size_t)(i * nb + c)] == as_kept(b0(i, l0 + c)) && J[(size_t)(i * nb + c)] == 0.0);
        // I_0: the rows of the up order's first sites, in the storage type
        for (int64_t r = 0; r < kBottom; r++)
            for (int64_t c = 0; c < nb; c++) {
                const double want = as_kept(b0(kOrder[r], l0 + c));
                CHECK(f32 ? (double)b.f_I0.p[r * nb + c] == want : b.d_I0.p[r * nb + c] == want);
            }
        // B_0 in the store's order: rows as they are, or the up-order plane set with a zero padding wavelength
        for (int64_t i = 0; i < kN; i++)
            for (int64_t c = 0; c < (rows_form ? nb : (nb + 1) / 2 * 2); c++) {
                const double want = c < nb ? as_kept(b0(i, l0 + c)) : 0.0;
                const size_t t = rows_form ? (size_t)(i * nb + c) : (size_t)(((c / 2) * kN + i) * 2 + (c & 1));
                CHECK(f32 ? (double)b.f_B0.p[t] == want : b.d_B0.p[t] == want);
            }
    }
    // ---- a create that fails on a block that is up leaves it what it was
    {
        const std::vector<const void *> before = handles(b);
        const std::map<void *, size_t> live_before = live_dev;
        for (long k = 0; k < n_alloc; k++) {
            mallocs = 0; fail_at = k;
            CHECK(b.create(plan, B0.data(), kNlam, 0, 2, form, nullptr) == VRT_ENOMEM);
            fail_at = -1;
            CHECK(handles(b) == before && live_dev == live_before && bad_release == 0 && b.l0 == l0 && b.l1 == l1);
        }
    }

    // ---- step: the launches of one iterate up to the update, in order, with and without Λ*
    LineCaseDev line;
    line.n = kN; line.nlam = kNlam;
    CHECK(line.d_small.alloc((size_t)kNlam) == VRT_OK);       // (the wavelengths: the opacity launch is handed those from l0)
    small_base = line.d_small;
    const double w[1] = {1.0};
    double diag_buf[1] = {0.0};
    for (double *d_diag : {(double *)nullptr, diag_buf}) {
        if (d_diag && f32) continue;                          // (the sessions refuse the operator on float storage)
        calls.clear();
        diag_rows = diag_planes = update_diag = diag_buf + 1;
        RatesJ J;
        CHECK(b.step(plan, line, nullptr, w, nullptr, d_diag, nullptr, &J) == VRT_OK);
        std::vector<std::string> want;
        if (nb && rows_form) want.push_back("copy");          // S_old = copy(S_new)
        want.push_back("terms");
        if (nb) {
            want.push_back(std::string(f32 ? "opacity_f32 " : "opacity ") + std::to_string(nb) + " from " + std::to_string(l0));
            if (d_diag) want.push_back("diagonal");
            want.push_back(rows_form ? "execute_rows" : f32 ? "execute_planes_f32" : "execute_planes");
            want.push_back(rows_form ? "update_rows" : f32 ? "update_planes_f32" : "update_planes");
        }
        CHECK(calls == want);
        if (nb && d_diag) CHECK(update_diag == d_diag && (rows_form ? diag_rows == d_diag && !diag_planes : diag_planes == d_diag && !diag_rows));
        if (nb && !d_diag && !f32) CHECK(update_diag == nullptr);
        // where the rates read J
        if (!nb) CHECK(J.rows == nullptr && J.ld == 1 && !J.up && !J.up_f);
        else if (rows_form) CHECK(J.rows == b.sj.J_rows() && J.ld == nb && !J.up && !J.up_f);
        else if (f32) CHECK(J.up_f == b.sj.J_plane<float>(0) && J.down_f == b.sj.J_plane<float>(1) && J.plan == plan && !J.rows && !J.up);
        else CHECK(J.up == b.sj.J_plane(0) && J.down == b.sj.J_plane(1) && J.grid == plan->g && !J.rows && !J.up_f);
    }
    std::printf("ok block [%d, %d) %s\n", (int)l0, (int)l1, form_name(form));
}

void check_plan_ok()
{
    vrt_grid grid;
    grid.n = kN;
    vrt_plan plan;
    plan.g = &grid;
    plan.A = 3; plan.n_angles_user = 3; plan.patch_ok = true;
    CHECK(line_session_plan_ok(&plan, false) == VRT_OK && line_session_plan_ok(&plan, true) == VRT_OK);
    plan.n_angles_user = 4;                                   // a θ = 90 direction
    CHECK(line_session_plan_ok(&plan, false) == VRT_EINVAL && last_error.find("every angle active") != std::string::npos);
    plan.n_angles_user = 3; plan.tune.lambda_native = 0;
    CHECK(line_session_plan_ok(&plan, false) == VRT_OK);
    CHECK(line_session_plan_ok(&plan, true) == VRT_EINVAL && last_error.find("float-storage line session") != std::string::npos);
    plan.tune.lambda_native = 1; plan.tune.path = 3;
    CHECK(line_session_plan_ok(&plan, false) == VRT_OK && line_session_plan_ok(&plan, true) == VRT_EINVAL);
    plan.tune.path = 4;
    CHECK(line_session_plan_ok(&plan, true) == VRT_OK);
    plan.patch_ok = false;                                    // no layer path at all
    CHECK(line_session_plan_ok(&plan, false) == VRT_EINVAL && last_error.find("the line session needs a layer path") != std::string::npos);
    std::printf("ok plan checks\n");
}

// ---- the member protocol, with three members that are nothing but what on_members asks of one
struct FakeMember {
    int device = 0, rc = VRT_OK;
    std::string err;
    std::mutex mu;
    std::mutex &plan_mutex() { return mu; }
};

void check_members()
{
    std::vector<FakeMember> m(3);
    const std::thread::id main_thread = std::this_thread::get_id();
    struct Seen {
        bool called = false, own_thread = false, locked = false;
        int device = -2;
    };
    Seen seen[3];
    auto reset = [&] {
        for (int d = 0; d < 3; d++) { m[(size_t)d].device = 10 + d; m[(size_t)d].rc = 77; m[(size_t)d].err = "stale"; seen[d] = Seen(); }
    };
    // what a body sees: its thread, the current device, and whether another thread can take the member's plan mutex
    auto look = [&](int d, FakeMember &me) {
        Seen &s = seen[d];
        s.called = true;
        s.own_thread = std::this_thread::get_id() != main_thread;
        s.device = current_device;
        std::thread([&] {
            s.locked = !me.mu.try_lock();
            if (!s.locked) me.mu.unlock();
        }).join();
    };

    // every member runs, on a thread of its own, its device current; the plan mutex held only when asked for
    for (int options : {0, (int)kLockPlan}) {
        reset();
        last_error = "untouched";
        CHECK(on_members(m, options, every_member, [&](int d, FakeMember &me) { look(d, me); return (int)VRT_OK; }) == VRT_OK);
        for (int d = 0; d < 3; d++)
            CHECK(seen[d].called && seen[d].own_thread && seen[d].device == 10 + d && seen[d].locked == (options == kLockPlan) && m[(size_t)d].rc == VRT_OK);
        CHECK(last_error == "untouched");
        for (FakeMember &me : m) { CHECK(me.mu.try_lock()); me.mu.unlock(); }      // (released afterwards)
    }
    // kNoDevice: nothing is made current for the body
    reset();
    CHECK(on_members(m, kNoDevice, every_member, [&](int d, FakeMember &me) { look(d, me); return (int)VRT_OK; }) == VRT_OK);
    for (int d = 0; d < 3; d++) CHECK(seen[d].called && seen[d].device == -1);
    // a skipped member's body is never called, and its code is cleared all the same
    reset();
    CHECK(on_members(m, kLockPlan, [](int d) { return d == 0; }, [&](int d, FakeMember &me) { look(d, me); return (int)VRT_OK; }) == VRT_OK);
    CHECK(!seen[0].called && seen[1].called && seen[2].called && m[0].rc == VRT_OK);
    // a body that fails on member 1 only: its code, and its text -- set in the worker thread -- behind the device's number
    reset();
    last_error = "the caller's";
    CHECK(on_members(m, 0, every_member, [&](int d, FakeMember &me) {
              look(d, me);
              return d == 1 ? fail(VRT_EINVAL, "the text of member 1") : (int)VRT_OK;
          }) == VRT_EINVAL);
    CHECK(last_error == "device 11: the text of member 1" && seen[1].own_thread);
    CHECK(m[0].rc == VRT_OK && m[1].rc == VRT_EINVAL && m[2].rc == VRT_OK && m[1].err == "the text of member 1");
    // two members fail: the report names the lower index
    reset();
    CHECK(on_members(m, 0, every_member, [&](int d, FakeMember &) {
              return d == 0 ? (int)VRT_OK : fail(d == 1 ? VRT_ENOMEM : VRT_ENODEVICE, "member " + std::to_string(d) + " failed");
          }) == VRT_ENOMEM);
    CHECK(last_error == "device 11: member 1 failed" && m[2].rc == VRT_ENODEVICE && m[2].err == "member 2 failed");
    // a body that throws: VRT_ENOMEM, whatever the others return
    reset();
    CHECK(on_members(m, kLockPlan, every_member, [&](int d, FakeMember &) -> int {
              if (d == 2) throw std::bad_alloc();
              return d == 0 ? fail(VRT_EINVAL, "member 0 failed") : (int)VRT_OK;
          }) == VRT_ENOMEM);
    CHECK(last_error == "out of host memory in a device worker");
    for (FakeMember &me : m) { CHECK(me.mu.try_lock()); me.mu.unlock(); }          // (the thrower's lock is released)
    // a device that cannot be made current: reported like a failing body, which never runs there
    reset();
    m[1].device = 99;
    CHECK(on_members(m, 0, every_member, [&](int d, FakeMember &me) { look(d, me); return (int)VRT_OK; }) == VRT_ENODEVICE);
    CHECK(last_error == "device 99: hipSetDevice failed" && !seen[1].called && seen[0].called && seen[2].called);
    std::printf("ok members\n");
}

}  // namespace

int main()
{
    {
        vrt_grid grid;
        grid.n = kN;
        grid.up.n1 = kBottom;
        CHECK(grid.up.d_order.alloc(kBottom) == VRT_OK);
        std::memcpy(grid.up.d_order.p, kOrder, sizeof(kOrder));
        vrt_plan plan;
        plan.g = &grid;
        plan.A = 3; plan.n_angles_user = 3; plan.patch_ok = true;
        base_live = live_dev.size();
        std::vector<double> B0((size_t)(kN * kNlam));
        for (int64_t i = 0; i < kN; i++)
            for (int64_t l = 0; l < kNlam; l++) B0[(size_t)(i * kNlam + l)] = b0(i, l);
        for (SourceStore::Form form : {SourceStore::kRows, SourceStore::kPlanes, SourceStore::kPlanesF32}) {
            check_create(&plan, form, 1, 4, B0);                  // n nb = 15, odd
            check_create(&plan, form, 2, 6, B0);                  // 20, even
            check_create(&plan, form, 6, 7, B0);                  // one wavelength
            check_create(&plan, form, 3, 3, B0);                  // a member without wavelengths
            CHECK(live_dev.size() == base_live && bad_release == 0);
        }
    }
    CHECK(live_dev.empty() && bad_release == 0);
    check_plan_ok();
    check_members();
    std::printf("%d checks passed; no allocation outlived a failed create\n", checks.load());
    return 0;
}
