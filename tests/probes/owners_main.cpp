// Stand-alone host program for the owner types of csrc/vrt_internal.h (DevBuf, DevWork, HostBuf, Stream, Event), built by
// tests/test_host.py with g++ -fsanitize=address,undefined and run as a child process.  The HIP calls the owners use are
// faked below: memory is malloc with a live counter, streams and events are counted dummy handles, and a switch makes the
// next allocation fail with out-of-memory.  Every check ends with all live counts at zero; a double release trips the
// counters (and the sanitizer), a missed one leaves a count behind.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <set>
#include <string>
#include <utility>

#include "vrt_internal.h"

namespace {
std::set<void *> live_dev, live_host, live_stream, live_event;
long n_malloc = 0, n_free = 0, bad_release = 0;
bool fail_next_alloc = false;
std::string last_error;
int checks = 0;

void *new_handle(std::set<void *> &live)
{
    void *h = std::malloc(1);
    live.insert(h);
    return h;
}
hipError_t release(std::set<void *> &live, void *h)
{
    if (!live.erase(h)) { bad_release++; return hipErrorInvalidValue; }     // released twice, or never handed out
    std::free(h);
    return hipSuccess;
}
}  // namespace

// ---- the fake runtime ------------------------------------------------------------------------------------------------
extern "C" {
hipError_t hipMalloc(void **p, size_t bytes)
{
    if (fail_next_alloc) { fail_next_alloc = false; *p = nullptr; return hipErrorOutOfMemory; }
    *p = std::malloc(bytes);
    live_dev.insert(*p);
    n_malloc++;
    return hipSuccess;
}
hipError_t hipFree(void *p) { n_free++; return release(live_dev, p); }
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned)
{
    if (fail_next_alloc) { fail_next_alloc = false; *p = nullptr; return hipErrorOutOfMemory; }
    *p = std::malloc(bytes);
    live_host.insert(*p);
    return hipSuccess;
}
hipError_t hipHostFree(void *p) { return release(live_host, p); }
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { *s = (hipStream_t)new_handle(live_stream); return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t s) { return release(live_stream, (void *)s); }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { *e = (hipEvent_t)new_handle(live_event); return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t e) { return release(live_event, (void *)e); }
hipError_t hipGetDevice(int *d) { *d = 0; return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
const char *hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : "error"; }
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

size_t live_total() { return live_dev.size() + live_host.size() + live_stream.size() + live_event.size(); }

#define CHECK(cond)                                                                  \
    do {                                                                             \
        checks++;                                                                    \
        if (!(cond)) {                                                               \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);            \
            std::exit(1);                                                            \
        }                                                                            \
    } while (0)

// what every owner has in common: `make` fills one, `live` is its counter
template <typename Owner, typename Make>
void check_owner(const char *name, Make make, const std::set<void *> &live)
{
    {   // destruction releases exactly once; an empty one releases nothing
        Owner a, empty;
        CHECK(make(a) == VRT_OK && live.size() == 1);
    }
    CHECK(live.empty() && bad_release == 0);
    {   // move construction
        Owner a;
        CHECK(make(a) == VRT_OK);
        Owner b(std::move(a));
        CHECK(live.size() == 1);
    }
    CHECK(live.empty() && bad_release == 0);
    {   // move assignment onto an empty and onto a non-empty target
        Owner a, b, c;
        CHECK(make(a) == VRT_OK && make(c) == VRT_OK && live.size() == 2);
        b = std::move(a);
        CHECK(live.size() == 2);
        c = std::move(b);
        CHECK(live.size() == 2);              // (the target's old object went to the source, which still owns it)
    }
    CHECK(live.empty() && bad_release == 0);
    {   // reset() is idempotent; creating again releases what was held
        Owner a;
        CHECK(make(a) == VRT_OK && make(a) == VRT_OK && live.size() == 1);
        a.reset();
        CHECK(live.empty());
        a.reset();
        CHECK(live.empty() && bad_release == 0);
    }
    CHECK(live_total() == 0 && bad_release == 0);
    std::printf("ok %s\n", name);
}

void check_work()
{
    DevWork<double> w;
    CHECK(w.grow(100) == VRT_OK && w.cap == 100 && w.get() && live_dev.size() == 1);
    double *first = w;
    const long mallocs = n_malloc, frees = n_free;
    CHECK(w.grow(100) == VRT_OK && w.grow(7) == VRT_OK && w.get() == first && w.cap == 100);       // large enough: kept
    CHECK(n_malloc == mallocs && n_free == frees);
    CHECK(w.grow(101) == VRT_OK && w.cap == 101 && live_dev.size() == 1);                           // too small: freed, then
    CHECK(n_malloc == mallocs + 1 && n_free == frees + 1 && !live_dev.count(first));                //   allocated
    fail_next_alloc = true;
    CHECK(w.grow(1000) == VRT_ENOMEM && w.cap == 0 && w.get() == nullptr && live_dev.empty());      // failed: nothing held
    CHECK(last_error.find("hipMalloc") != std::string::npos);
    CHECK(w.grow(5) == VRT_OK && w.cap == 5 && live_dev.size() == 1);                               // and usable again
    DevWork<double> v(std::move(w));
    CHECK(v.cap == 5 && v.get() && w.get() == nullptr && live_dev.size() == 1);
    std::printf("ok DevWork::grow\n");
}

// one owner of each kind, as the handles hold them
struct Handle {
    DevBuf<int> table;
    DevWork<double> work;
    HostBuf<char> pinned;
    Stream stream;
    Event event;
};

int half_built(bool fail_midway, Handle **out)
{
    std::unique_ptr<Handle> h(new Handle());
    int rc;
    if ((rc = h->table.alloc(10)) || (rc = h->work.grow(20)) || (rc = h->pinned.alloc(30)) || (rc = h->stream.create()) ||
        (rc = h->event.create()))
        return rc;
    CHECK(live_total() == 5);
    fail_next_alloc = fail_midway;
    DevBuf<int> late;
    if ((rc = late.alloc(40))) return rc;           // (dropped halfway through "construction": everything above goes)
    *out = h.release();
    return VRT_OK;
}

}  // namespace

int main()
{
    check_owner<DevBuf<int>>("DevBuf", [](DevBuf<int> &b) { return b.alloc(3); }, live_dev);
    check_owner<DevWork<double>>("DevWork", [](DevWork<double> &w) { w.reset(); return w.grow(3); }, live_dev);
    check_owner<HostBuf<char>>("HostBuf", [](HostBuf<char> &b) { return b.alloc(3); }, live_host);
    check_owner<Stream>("Stream", [](Stream &s) { return s.create(); }, live_stream);
    check_owner<Event>("Event", [](Event &e) { return e.create(hipEventDisableTiming); }, live_event);
    check_work();
    CHECK(live_total() == 0);
    {
        DevBuf<int> b;
        fail_next_alloc = true;
        CHECK(b.alloc(1) == VRT_ENOMEM && b.get() == nullptr);
        HostBuf<int> hb;
        fail_next_alloc = true;
        CHECK(hb.alloc(1) == VRT_ENODEVICE && hb.p == nullptr && live_total() == 0);
    }
    Handle *h = nullptr;
    CHECK(half_built(true, &h) == VRT_ENOMEM && h == nullptr && live_total() == 0);
    CHECK(half_built(false, &h) == VRT_OK && h && live_total() == 5);
    delete h;
    CHECK(live_total() == 0 && bad_release == 0);
    std::printf("%d checks passed; all live counts are zero (device %zu, host %zu, streams %zu, events %zu)\n", checks,
                live_dev.size(), live_host.size(), live_stream.size(), live_event.size());
    return 0;
}
