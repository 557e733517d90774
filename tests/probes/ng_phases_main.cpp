// Stand-alone host program for the phases of the Ng step that csrc/vrt_internal.h shares between the single-device sessions
// (ng_after_iterate) and the multi-device session (vrt_multi.cpp): ng_due (the schedule), ng_record, ng_take_history,
// ng_add_sums, ng_commit, ng_S_range.  Built by tests/test_accel_session_multi_host.py with g++ -fsanitize=address,undefined
// and run as a child process.  The few HIP calls behind them are faked below (device memory is malloc, a copy is memcpy);
// the device halves of a step (the sums, the apply) are played by the program itself, which hands out the verdicts -- a
// REJECTED step, which no physical case provokes reliably, is covered here: one member of three reports a bad verdict and
// no member's S handle may have been swapped.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "vrt_internal.h"

namespace {
std::set<void *> live_dev;
long bad_release = 0;
std::string last_error;
int checks = 0;
}  // namespace

// ---- the fake runtime ------------------------------------------------------------------------------------------------
extern "C" {
hipError_t hipMalloc(void **p, size_t bytes)
{
    *p = std::malloc(bytes);
    live_dev.insert(*p);
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

// the header's words, written out independently: the first step after iterate `start`, then every `period` further ones;
// the three iterates before a due one are kept as x3, x2, x1
int expected_action(int start, int period, int iterate)
{
    int next = start;
    while (next < iterate) next += period;
    const int to_go = next - iterate;
    return to_go == 0 ? kNgStep : (to_go <= 3 ? to_go : kNgNothing);
}

void check_schedule()
{
    const int settings[][2] = {{4, 4}, {4, 5}, {5, 7}, {9, 4}, {6, 11}};
    for (const auto &sp : settings) {
        NgState ng;
        ng.order = 2; ng.start = sp[0]; ng.period = sp[1];
        for (int it = 1; it <= 60; it++) CHECK(ng_due(ng, it) == expected_action(sp[0], sp[1], it));
        ng.order = 0;
        for (int it = 1; it <= 60; it++) CHECK(ng_due(ng, it) == kNgNothing);
    }
    NgState ng;
    ng.order = 2; ng.start = 4; ng.period = 4;
    const int want[12] = {3, 2, 1, kNgStep, 3, 2, 1, kNgStep, 3, 2, 1, kNgStep};
    for (int it = 1; it <= 12; it++) CHECK(ng_due(ng, it) == want[it - 1]);
    std::printf("ok schedule\n");
}

void check_ranges()
{
    NgRange r = ng_S_range(5, 3, true);          // one full pair plane, then the first halves of the last plane's pairs
    CHECK(r.dense == 10 && r.tail == 5 && r.tstride == 2);
    r = ng_S_range(5, 4, true);
    CHECK(r.dense == 20 && r.tail == 0);
    r = ng_S_range(5, 1, true);
    CHECK(r.dense == 0 && r.tail == 5 && r.tstride == 2);
    r = ng_S_range(5, 3, false);
    CHECK(r.dense == 14 && r.tail == 1 && r.tstride == 1);
    r = ng_S_range(5, 4, false);
    CHECK(r.dense == 20 && r.tail == 0 && r.tstride == 1);
    std::printf("ok ranges\n");
}

void check_sum_order()
{
    // ((1e16 + 1) + 1) = 1e16, but 1e16 + (1 + 1) = 1e16 + 2: the result tells the order
    const double parts[3][5] = {{1e16, 1, 2, 3, 4}, {1.0, 1, 2, 3, 4}, {1.0, 1, 2, 3, 4}};
    double total[5] = {-7, -7, -7, -7, -7};      // (stale values: the first member's sums are copied, not added)
    for (int d = 0; d < 3; d++) ng_add_sums(total, parts[d], d == 0);
    volatile double left = 1e16;
    left = left + 1.0;
    left = left + 1.0;
    CHECK(total[0] == left && total[0] != 1e16 + 2.0);
    CHECK(total[1] == 3 && total[2] == 6 && total[3] == 9 && total[4] == 12);
    std::printf("ok order of addition\n");
}

// three members with blocks of 4, 4 and 3 "wavelengths" of two sites
struct Member {
    size_t count;
    DevBuf<double> S;
    NgState ng;
};

void plain_update(std::vector<Member> &ms, int iterate)
{
    for (size_t d = 0; d < ms.size(); d++)
        for (size_t i = 0; i < ms[d].count; i++) ms[d].S[i] = 100.0 * iterate + 10.0 * (double)d + (double)i;
}

// one iterate of a session: the plain update, then the phases; `verdicts` are what the members' apply kernels would report
// (the program writes a marker into every x_acc buffer first, as the kernel writes x_acc whatever its verdict is)
int after_iterate(std::vector<Member> &ms, const NgState &settings, int iterate, const std::vector<bool> &verdicts, bool coeffs_valid)
{
    plain_update(ms, iterate);
    const int due = ng_due(settings, iterate);
    if (due == kNgNothing) return 0;
    if (due != kNgStep) {
        for (Member &m : ms) CHECK(ng_record(m.ng, due, m.S, m.count, nullptr) == VRT_OK);
        return 0;
    }
    bool complete = true;
    for (Member &m : ms)
        if (!ng_take_history(m.ng)) complete = false;
    for (Member &m : ms) CHECK(m.ng.have == 0);                 // used up either way
    if (!complete) return 0;
    std::vector<NgPiece> pieces;
    for (size_t d = 0; d < ms.size(); d++) {
        for (size_t i = 0; i < ms[d].count; i++) ms[d].ng.hist[2][i] = -1.0;
        pieces.push_back(NgPiece{&ms[d].ng, &ms[d].S, (bool)verdicts[d]});
    }
    return ng_commit(pieces.data(), (int)pieces.size(), coeffs_valid) ? 1 : -1;
}

void check_all_or_nothing()
{
    std::vector<Member> ms(3);
    const size_t counts[3] = {8, 8, 6};
    NgState settings;
    settings.order = 2; settings.start = 4; settings.period = 4;
    for (size_t d = 0; d < 3; d++) {
        ms[d].count = counts[d];
        CHECK(ms[d].S.alloc(counts[d]) == VRT_OK);
        for (DevBuf<double> &h : ms[d].ng.hist) CHECK(h.alloc(counts[d]) == VRT_OK);
    }
    auto handles = [&] {
        std::vector<double *> h;
        for (Member &m : ms) { h.push_back(m.S.p); for (DevBuf<double> &b : m.ng.hist) h.push_back(b.p); }
        return h;
    };
    const std::vector<bool> all_good = {true, true, true};
    // iterates 1..3 record x3, x2, x1 of every member
    for (int it = 1; it <= 3; it++) {
        CHECK(after_iterate(ms, settings, it, all_good, true) == 0);
        for (Member &m : ms) CHECK(m.ng.have == (7u & ~((1u << (3 - it)) - 1u)));
    }
    for (size_t d = 0; d < 3; d++)
        for (int k = 0; k < 3; k++) CHECK(ms[d].ng.hist[k][1] == 100.0 * (3 - k) + 10.0 * (double)d + 1.0);      // hist[k] = x_{k+1}
    // iterate 4: the middle member's verdict is bad -> rejected, and NO member's S handle was swapped
    std::vector<double *> before = handles();
    CHECK(after_iterate(ms, settings, 4, {true, false, true}, true) == -1);
    CHECK(handles() == before);
    for (size_t d = 0; d < 3; d++)
        for (size_t i = 0; i < ms[d].count; i++) CHECK(ms[d].S[i] == 400.0 + 10.0 * (double)d + (double)i);      // the plain update's S
    // iterate 8: the last member alone is bad; iterate 12: the first
    for (int it = 5; it <= 7; it++) CHECK(after_iterate(ms, settings, it, all_good, true) == 0);
    CHECK(after_iterate(ms, settings, 8, {true, true, false}, true) == -1 && handles() == before);
    for (int it = 9; it <= 11; it++) CHECK(after_iterate(ms, settings, it, all_good, true) == 0);
    CHECK(after_iterate(ms, settings, 12, {false, true, true}, true) == -1 && handles() == before);
    // iterate 16: every verdict good but the coefficients invalid (a singular system) -> rejected as well
    for (int it = 13; it <= 15; it++) CHECK(after_iterate(ms, settings, it, all_good, true) == 0);
    CHECK(after_iterate(ms, settings, 16, all_good, false) == -1 && handles() == before);
    // iterate 20: accepted -> EVERY member's x_acc buffer is its S now, and its old S buffer the oldest history slot
    for (int it = 17; it <= 19; it++) CHECK(after_iterate(ms, settings, it, all_good, true) == 0);
    CHECK(after_iterate(ms, settings, 20, all_good, true) == 1);
    std::vector<double *> after = handles();
    for (size_t d = 0; d < 3; d++) {
        CHECK(after[4 * d] == before[4 * d + 3] && after[4 * d + 3] == before[4 * d]);
        CHECK(after[4 * d + 1] == before[4 * d + 1] && after[4 * d + 2] == before[4 * d + 2]);
        CHECK(ms[d].S[0] == -1.0 && ms[d].ng.hist[2][0] == 2000.0 + 10.0 * (double)d);
    }
    // a history dropped on the way (what *_set_state does) makes the next due iterate take no step at all
    CHECK(after_iterate(ms, settings, 21, all_good, true) == 0);
    for (Member &m : ms) m.ng.have = 0;
    CHECK(after_iterate(ms, settings, 22, all_good, true) == 0 && after_iterate(ms, settings, 23, all_good, true) == 0);
    before = handles();
    CHECK(after_iterate(ms, settings, 24, all_good, true) == 0 && handles() == before);
    // ... and so does a history that ONE member lacks
    for (int it = 25; it <= 27; it++) CHECK(after_iterate(ms, settings, it, all_good, true) == 0);
    ms[1].ng.have = 3u;
    CHECK(after_iterate(ms, settings, 28, all_good, true) == 0 && handles() == before);
    std::printf("ok all or nothing\n");
}

}  // namespace

int main()
{
    check_schedule();
    check_ranges();
    check_sum_order();
    check_all_or_nothing();
    CHECK(live_dev.empty() && bad_release == 0);
    std::printf("%d checks passed; no S handle moved on a rejected step\n", checks);
    return 0;
}
