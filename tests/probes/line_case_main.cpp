// Stand-alone host program for csrc/vrt_line_case.h: the argument checks of a vrt_line_case, the one writer and the one
// reader of the wavelength-sized vector lambda | planck2 | sigma_bf1 | sigma_bf2, and LineCaseDev, the owner of the line
// case a Λ-iteration session uploads.  Built by tests/test_line_case_host.py with g++ -fsanitize=address,undefined and run
// as a child process.  The HIP calls behind upload() and DevBuf are faked below (device memory is malloc, a copy is memcpy,
// hipMalloc can be told to fail at its k-th call); the two launches the owner forwards to record what they were handed.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "vrt_line_case.h"

namespace {
std::map<void *, size_t> live_dev;      // address -> bytes
long bad_release = 0, mallocs = 0, fail_at = -1;
std::string last_error;
int checks = 0;

struct TermsCall {
    int64_t n;
    const double *gamma_static, *gamma_unsold, *pops;
    double strength_const, Bij, Bji;
    double *gamma, *strength;
} terms_call;
struct OpacityCall {
    vrt_plan *plan;
    int64_t nlam;
    const double *lambda, *velocity, *doppler, *gamma, *strength, *alpha_cont;
    double lambda0, c0;
    void *out;
    bool f32;
} opacity_call;
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
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
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
int launch_line_terms(int64_t n, const double *d_gamma_static, const double *d_gamma_unsold, const double *d_pops,
                      double strength_const, double Bij, double Bji, double *d_gamma, double *d_strength, hipStream_t)
{
    terms_call = TermsCall{n, d_gamma_static, d_gamma_unsold, d_pops, strength_const, Bij, Bji, d_gamma, d_strength};
    return VRT_OK;
}
int launch_line_opacity(vrt_plan *p, int64_t nlam, const double *d_lambda, double lambda0, double c0, const double *d_velocity,
                        const double *d_doppler, const double *d_gamma, const double *d_strength, const double *d_alpha_cont,
                        void *d_out, hipStream_t, bool f32_out)
{
    opacity_call = OpacityCall{p, nlam, d_lambda, d_velocity, d_doppler, d_gamma, d_strength, d_alpha_cont, lambda0, c0, d_out, f32_out};
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

const char *kNlamText = "nlam must be >= 2";
const char *kNullText = "NULL array in the line case";
const char *kBlockText = "each wavelength block needs at least two wavelengths inside [0, nlam)";
const char *kPositiveText = "lambda0 and c0 must be positive";

bool refused(const vrt_line_case &lc, const char *text)
{
    last_error.clear();
    return check_line_case(&lc) == VRT_EINVAL && last_error == text;
}
bool accepted(const vrt_line_case &lc)
{
    last_error.clear();
    return check_line_case(&lc) == VRT_OK && last_error.empty();
}

// the fifteen arrays of a line case, in the order of the struct
typedef const double *vrt_line_case::*ArrayField;
const ArrayField kArrays[15] = {&vrt_line_case::lambda,       &vrt_line_case::velocity,     &vrt_line_case::doppler_width,
                                &vrt_line_case::gamma_static, &vrt_line_case::gamma_unsold, &vrt_line_case::alpha_cont,
                                &vrt_line_case::eps,          &vrt_line_case::temperature,  &vrt_line_case::atom_density,
                                &vrt_line_case::B0,           &vrt_line_case::lte_populations, &vrt_line_case::C,
                                &vrt_line_case::planck2,      &vrt_line_case::sigma_bf1,    &vrt_line_case::sigma_bf2};

// A case of n sites whose every array holds values of its own (array a, element i: 1000 (a + 1) + i), so that an array in
// another's place shows; the scalars are all different too.
struct HostCase {
    std::vector<std::vector<double>> arrays;
    vrt_line_case lc;
    HostCase(int64_t n, int64_t nlam, const int64_t blocks[6])
    {
        const size_t sn = (size_t)n, nl = (size_t)nlam;
        const size_t len[15] = {nl, 3 * sn, sn, sn, sn, sn, sn, sn, sn, sn * nl, 3 * sn, 9 * sn, nl, (size_t)(blocks[3] - blocks[2]),
                                (size_t)(blocks[5] - blocks[4])};
        std::memset(&lc, 0, sizeof(lc));
        lc.nlam = nlam;
        for (int q = 0; q < 6; q++) lc.blocks[q] = blocks[q];
        arrays.resize(15);
        for (int a = 0; a < 15; a++) {
            arrays[(size_t)a].resize(len[a]);
            for (size_t i = 0; i < len[a]; i++) arrays[(size_t)a][i] = 1000.0 * (a + 1) + (double)i;
            lc.*kArrays[a] = arrays[(size_t)a].data();
        }
        lc.lambda0 = 11; lc.c0 = 12; lc.strength_const = 13; lc.Bij = 14; lc.Bji = 15;
        lc.sigma_bb_const = 16; lc.hc_over_kB = 17; lc.pref_ij = 18; lc.pref_ji = 19;
    }
};

void check_the_checks()
{
    const int64_t smallest[6] = {0, 2, 2, 4, 4, 6};
    HostCase hc(1, 6, smallest);
    CHECK(accepted(hc.lc));                                  // the smallest valid case
    for (int a = 0; a < 15; a++) {                           // each array NULL in turn: the one NULL text
        vrt_line_case lc = hc.lc;
        lc.*kArrays[a] = nullptr;
        CHECK(refused(lc, kNullText));
    }
    {
        vrt_line_case lc = hc.lc;
        lc.nlam = 1;
        CHECK(refused(lc, kNlamText));
        lc.nlam = 0;
        CHECK(refused(lc, kNlamText));
        lc.nlam = 2;                                         // passes the nlam test: the blocks are what is wrong with it
        CHECK(refused(lc, kBlockText));
        for (int b = 0; b < 3; b++) { lc.blocks[2 * b] = 0; lc.blocks[2 * b + 1] = 2; }
        CHECK(accepted(lc));
        lc.lambda = nullptr; lc.nlam = 1;                    // the order of the checks: nlam, arrays, blocks, λ_0 and c_0
        CHECK(refused(lc, kNlamText));
        lc.nlam = 2; lc.blocks[1] = 3; lc.lambda0 = 0;
        CHECK(refused(lc, kNullText));
        lc.lambda = hc.lc.lambda;
        CHECK(refused(lc, kBlockText));
        lc.blocks[1] = 2;
        CHECK(refused(lc, kPositiveText));
    }
    for (int b = 0; b < 3; b++) {
        vrt_line_case lc = hc.lc;
        lc.blocks[2 * b] = -1;
        CHECK(refused(lc, kBlockText));
        lc = hc.lc;
        lc.blocks[2 * b + 1] = lc.nlam + 1;
        CHECK(refused(lc, kBlockText));
        lc = hc.lc;
        lc.blocks[2 * b + 1] = lc.blocks[2 * b] + 1;         // a length of 1
        CHECK(refused(lc, kBlockText));
        lc.blocks[2 * b + 1] = lc.blocks[2 * b];             // and of 0
        CHECK(refused(lc, kBlockText));
        lc.blocks[2 * b + 1] = lc.blocks[2 * b] + 2;         // a length of 2
        CHECK(accepted(lc));
        lc.blocks[2 * b] = 0; lc.blocks[2 * b + 1] = lc.nlam;        // the whole range
        CHECK(accepted(lc));
        last_error.clear();
        CHECK(check_blocks(lc.blocks, lc.nlam) == VRT_OK && check_blocks(lc.blocks, lc.nlam - 1) == VRT_EINVAL && last_error == kBlockText);
    }
    for (double bad : {0.0, -1.0, (double)NAN}) {
        vrt_line_case lc = hc.lc;
        lc.lambda0 = bad;
        CHECK(refused(lc, kPositiveText));
        lc = hc.lc;
        lc.c0 = bad;
        CHECK(refused(lc, kPositiveText));
    }
    {
        vrt_line_case lc = hc.lc;                            // overlapping blocks pass, as they always did
        const int64_t overlap[6] = {0, 4, 2, 5, 3, 6};
        for (int q = 0; q < 6; q++) lc.blocks[q] = overlap[q];
        CHECK(accepted(lc));
    }
    std::printf("ok checks\n");
}

// unequal continuum blocks (2 and 3 wavelengths): every view pointer lands on the element that was written
void check_small()
{
    const int64_t nlam = 9, blocks[6] = {0, 4, 4, 6, 6, 9};
    HostCase hc(1, nlam, blocks);
    const vrt_line_case &lc = hc.lc;
    const std::vector<double> small = pack_small(nlam, blocks, lc.lambda, lc.planck2, lc.sigma_bf1, lc.sigma_bf2);
    CHECK(small.size() == (size_t)(2 * nlam + 2 + 3));
    const SmallView v = small_view(small.data(), nlam, blocks);
    CHECK(v.lambda == small.data() && v.planck2 == small.data() + nlam && v.sigma_bf1 == small.data() + 2 * nlam);
    CHECK(v.sigma_bf2 == small.data() + 2 * nlam + (blocks[3] - blocks[2]));
    for (int64_t l = 0; l < nlam; l++) CHECK(v.lambda[l] == lc.lambda[l] && v.planck2[l] == lc.planck2[l]);
    for (int64_t l = 0; l < 2; l++) CHECK(v.sigma_bf1[l] == lc.sigma_bf1[l]);
    for (int64_t l = 0; l < 3; l++) CHECK(v.sigma_bf2[l] == lc.sigma_bf2[l]);
    CHECK(v.sigma_bf2 + 3 == small.data() + small.size());
    std::printf("ok small\n");
}

size_t doubles_at(const double *p) { return live_dev.count((void *)p) ? live_dev.at((void *)p) / sizeof(double) : 0; }
bool holds(const double *dev, const double *host, size_t count) { return doubles_at(dev) == count && !std::memcmp(dev, host, sizeof(double) * count); }

std::vector<const double *> handles(const LineCaseDev &d)
{
    return {d.d_small,       d.d_velocity, d.d_doppler, d.d_gamma_static, d.d_gamma_unsold, d.d_alpha_cont, d.d_eps,
            d.d_temperature, d.d_atom,     d.d_lte,     d.d_C,            d.d_gamma,        d.d_strength,   d.d_R};
}

void check_owner()
{
    const int64_t n = 5, nlam = 9, blocks[6] = {0, 4, 4, 6, 6, 9};
    const size_t sn = (size_t)n;
    HostCase hc(n, nlam, blocks);
    const vrt_line_case &lc = hc.lc;
    CHECK(live_dev.empty());
    // ---- an allocation that fails at every position in turn: nothing stays allocated, the owner holds nothing
    long n_alloc = 0;
    for (long k = 0;; k++) {
        LineCaseDev d;
        mallocs = 0; fail_at = k;
        const int rc = d.create(&lc, n, nullptr);
        fail_at = -1;
        if (!rc) { n_alloc = mallocs; break; }
        CHECK(rc == VRT_ENOMEM && live_dev.empty() && bad_release == 0 && d.n == 0 && d.nlam == 0);
        for (const double *h : handles(d)) CHECK(h == nullptr);
        CHECK(k < 32);
    }
    CHECK(n_alloc == 14 && live_dev.empty() && bad_release == 0);        // (the owner that came up went out of scope above)

    LineCaseDev d;
    CHECK(d.create(&lc, n, nullptr) == VRT_OK && live_dev.size() == 14);
    // ---- every buffer: its length and what it holds
    const std::vector<double> small = pack_small(nlam, blocks, lc.lambda, lc.planck2, lc.sigma_bf1, lc.sigma_bf2);
    CHECK(d.n == n && d.nlam == nlam);
    CHECK(holds(d.d_small, small.data(), (size_t)(2 * nlam + 5)));
    CHECK(holds(d.d_velocity, lc.velocity, 3 * sn) && holds(d.d_doppler, lc.doppler_width, sn));
    CHECK(holds(d.d_gamma_static, lc.gamma_static, sn) && holds(d.d_gamma_unsold, lc.gamma_unsold, sn));
    CHECK(holds(d.d_alpha_cont, lc.alpha_cont, sn) && holds(d.d_eps, lc.eps, sn) && holds(d.d_temperature, lc.temperature, sn));
    CHECK(holds(d.d_atom, lc.atom_density, sn) && holds(d.d_lte, lc.lte_populations, 3 * sn) && holds(d.d_C, lc.C, 9 * sn));
    CHECK(doubles_at(d.d_gamma) == sn && doubles_at(d.d_strength) == sn && doubles_at(d.d_R) == 9 * sn);
    // ---- the constants, filled in one place
    for (int q = 0; q < 6; q++) CHECK(d.k.blocks[q] == blocks[q]);
    CHECK(d.k.lambda0 == 11 && d.k.c0 == 12 && d.k.strength_const == 13 && d.k.Bij == 14 && d.k.Bji == 15 && d.k.sigma_bb_const == 16 &&
          d.k.hc_over_kB == 17 && d.k.pref_ij == 18 && d.k.pref_ji == 19);
    // ---- a create that fails on an owner that is up leaves it what it was
    {
        const std::vector<const double *> before = handles(d);
        const std::map<void *, size_t> live_before = live_dev;
        for (long k = 0; k < n_alloc; k++) {
            mallocs = 0; fail_at = k;
            CHECK(d.create(&lc, n, nullptr) == VRT_ENOMEM);
            fail_at = -1;
            CHECK(handles(d) == before && live_dev == live_before && bad_release == 0);
        }
    }
    // ---- the two launches it forwards to
    double pops[1], out[1];
    vrt_plan *plan = reinterpret_cast<vrt_plan *>(out);      // (an address only: the fake launch does not look into it)
    CHECK(d.terms(pops, nullptr) == VRT_OK);
    CHECK(terms_call.n == n && terms_call.gamma_static == d.d_gamma_static && terms_call.gamma_unsold == d.d_gamma_unsold &&
          terms_call.pops == pops && terms_call.strength_const == 13 && terms_call.Bij == 14 && terms_call.Bji == 15 &&
          terms_call.gamma == d.d_gamma && terms_call.strength == d.d_strength);
    for (int64_t l0 : {0, 3}) {                              // a block of the wavelengths: an offset into λ, nothing else moves
        CHECK(d.opacity(plan, 4, l0, out, nullptr, l0 != 0) == VRT_OK);
        CHECK(opacity_call.plan == plan && opacity_call.nlam == 4 && opacity_call.lambda == d.d_small + l0 && *opacity_call.lambda == lc.lambda[l0]);
        CHECK(opacity_call.lambda0 == 11 && opacity_call.c0 == 12 && opacity_call.velocity == d.d_velocity && opacity_call.doppler == d.d_doppler &&
              opacity_call.gamma == d.d_gamma && opacity_call.strength == d.d_strength && opacity_call.alpha_cont == d.d_alpha_cont &&
              opacity_call.out == out && opacity_call.f32 == (l0 != 0));
    }
    // ---- the inputs of a rate launch
    const RatesIn in = d.rates_in();
    CHECK(in.n == n && in.nlam == nlam && !std::memcmp(&in.k, &d.k, sizeof(LineConstants)));
    CHECK(in.small.lambda == d.d_small && *in.small.planck2 == lc.planck2[0] && *in.small.sigma_bf1 == lc.sigma_bf1[0] &&
          *in.small.sigma_bf2 == lc.sigma_bf2[0] && in.small.sigma_bf2[2] == lc.sigma_bf2[2]);
    CHECK(in.doppler == d.d_doppler && in.gamma == d.d_gamma && in.temperature == d.d_temperature && in.lte == d.d_lte && in.C == d.d_C &&
          in.atom_density == d.d_atom);
    // ---- where J comes from: one of the three, the others empty
    const float f[1] = {0};
    const vrt_grid *grid = reinterpret_cast<const vrt_grid *>(f);
    RatesJ J = RatesJ::from_rows(pops, 7);
    CHECK(J.rows == pops && J.ld == 7 && !J.up && !J.down && !J.grid && !J.up_f && !J.down_f && !J.plan);
    J = RatesJ::from_planes(grid, pops, out);
    CHECK(!J.rows && J.up == pops && J.down == out && J.grid == grid && !J.up_f && !J.down_f && !J.plan);
    J = RatesJ::from_planes_f32(plan, f, f + 1);
    CHECK(!J.rows && !J.up && !J.down && !J.grid && J.up_f == f && J.down_f == f + 1 && J.plan == plan);
    std::printf("ok owner, %ld allocations\n", n_alloc);
}

}  // namespace

int main()
{
    check_the_checks();
    check_small();
    check_owner();
    CHECK(live_dev.empty() && bad_release == 0);
    std::printf("%d checks passed; no allocation outlived a failed create\n", checks);
    return 0;
}
