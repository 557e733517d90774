// Internal declarations of libvrt_hip.so (not part of the C ABI; see include/voronoirt.h).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "voronoirt.h"

namespace vrt {

void set_error(const std::string &msg);
int fail(int code, const std::string &msg);

// Host checks of a session state handed back by the caller (*_set_source, *_set_state), before the device is touched:
// S finite and > 0 (the criterion divides by it), populations finite and >= 0.  The three *_lambda_set_state entries call
// check_state_pointers (a session and at least one of the two arrays; the session is not dereferenced), then check_state
// on the arrays that were given: S (nlam, n), populations (n, 3).
int check_source(const double *S, int64_t count);
int check_state_pointers(const void *session, const double *S, const double *populations);
int check_state(int64_t n, int64_t nlam, const double *S, const double *populations);

#define VRT_HIP_TRY(expr)                                                                  \
    do {                                                                                   \
        hipError_t _e = (expr);                                                            \
        if (_e != hipSuccess)                                                              \
            return ::vrt::fail(VRT_ENODEVICE, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

// Restores the caller's current HIP device when an entry point returns (a multi-GPU host such as
// torch keeps its own notion of the current device; the library must not change it behind its back).
struct DeviceScope {
    int prev = -1;
    DeviceScope() { if (hipGetDevice(&prev) != hipSuccess) prev = -1; }
    ~DeviceScope()
    {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
    DeviceScope(const DeviceScope &) = delete;
    DeviceScope &operator=(const DeviceScope &) = delete;
};

// The body of an extern "C" entry point that allocates, locks or touches the device: it runs under a DeviceScope, and
// no exception crosses the C boundary (std::bad_alloc is VRT_ENOMEM, anything else VRT_EINVAL).  The entry point
// returns that code, or `on_error` when it gives one (the int64_t queries: -1).
template <typename Body>
inline auto guarded(Body body, int64_t on_error = 0) -> decltype(body())
{
    DeviceScope scope;
    int rc;
    try {
        return body();
    } catch (const std::bad_alloc &) {
        rc = fail(VRT_ENOMEM, "out of host memory");
    } catch (...) {
        rc = fail(VRT_EINVAL, "unexpected exception");
    }
    return on_error ? on_error : rc;
}

// The device checks of the entry points: use_device for a handle's device (vrt_api.cpp), use_current_device for the
// *_dev calls that run on the caller's current device.  Both clear an error an earlier call left behind.
int use_device(int device);
int use_current_device();

// Device memory for `count` elements (at least one); *p is NULL on failure.  Out of memory is VRT_ENOMEM, any other
// error VRT_ENODEVICE.  The only place the library calls hipMalloc.
template <typename T>
inline int dev_alloc(T **p, size_t count)
{
    *p = nullptr;
    const hipError_t e = hipMalloc((void **)p, std::max<size_t>(count, 1) * sizeof(T));
    if (e == hipSuccess) return VRT_OK;
    *p = nullptr;
    return fail(e == hipErrorOutOfMemory ? VRT_ENOMEM : VRT_ENODEVICE, std::string("hipMalloc: ") + hipGetErrorString(e));
}

// ---- owners: whoever holds one of these releases it exactly once, when it goes out of scope.  All are move-only.  A
// handle (vrt_grid, vrt_plan, ...) is a struct of them and has no free list of its own; its *_destroy entry point makes
// the handle's device current and deletes it.  They are the only callers of hipFree, hipHostMalloc / hipHostFree and of
// the create / destroy calls of streams and events.

// Device memory: alloc() frees what it held; converts to T* wherever a raw (borrowed) pointer is wanted.
template <typename T>
struct DevBuf {
    T *p = nullptr;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(o.p) { o.p = nullptr; }
    DevBuf &operator=(DevBuf &&o) noexcept { std::swap(p, o.p); return *this; }
    ~DevBuf() { reset(); }
    void reset()
    {
        if (p) (void)hipFree((void *)p);
        p = nullptr;
    }
    int alloc(size_t count) { reset(); return dev_alloc(&p, count); }
    T *get() const { return p; }
    operator T *() const { return p; }
};

// `count` doubles of a host array into d (allocated here), enqueued on `st`
inline int upload(DevBuf<double> &d, const double *h, size_t count, hipStream_t st)
{
    int rc = d.alloc(count);
    if (rc) return rc;
    VRT_HIP_TRY(hipMemcpyAsync(d, h, sizeof(double) * count, hipMemcpyHostToDevice, st));
    return VRT_OK;
}

// Grow-only workspace: a buffer of fewer than `count` elements is freed and `count` allocated (cap = 0 on failure).
template <typename T>
struct DevWork {
    DevBuf<T> buf;
    size_t cap = 0;
    int grow(size_t count)
    {
        if (buf.p && count <= cap) return VRT_OK;
        reset();
        const int rc = buf.alloc(count);
        if (!rc) cap = count;
        return rc;
    }
    void reset() { buf.reset(); cap = 0; }
    T *get() const { return buf.p; }
    operator T *() const { return buf.p; }
};

// Columns [l0, l1) of host rows (rows, ld) into the dense device block (rows, l1 - l0) at `d`, enqueued on `st`
// (a template only so that a host program which never stages anything need not fake the 2D copy)
template <typename T>
inline int copy_cols(T *d, const T *h, size_t rows, int64_t ld, int64_t l0, int64_t l1, hipStream_t st)
{
    const size_t w = sizeof(T) * (size_t)(l1 - l0);
    if (!w || !rows) return VRT_OK;
    VRT_HIP_TRY(hipMemcpy2DAsync(d, w, h + l0, sizeof(T) * (size_t)ld, w, rows, hipMemcpyHostToDevice, st));
    return VRT_OK;
}
// ... with `d` made large enough first: a DevBuf is allocated, a DevWork grows
template <typename T> inline int reserve(DevBuf<T> &d, size_t count) { return d.alloc(count); }
template <typename T> inline int reserve(DevWork<T> &d, size_t count) { return d.grow(count); }
template <typename Buf>
inline int upload_cols(Buf &d, const double *h, size_t rows, int64_t ld, int64_t l0, int64_t l1, hipStream_t st)
{
    const int rc = reserve(d, rows * (size_t)(l1 - l0));
    return rc ? rc : copy_cols<double>(d, h, rows, ld, l0, l1, st);
}

// Pinned (or, with hipHostMallocMapped, mapped) host memory.
template <typename T>
struct HostBuf {
    T *p = nullptr;
    HostBuf() = default;
    HostBuf(HostBuf &&o) noexcept : p(o.p) { o.p = nullptr; }
    HostBuf &operator=(HostBuf &&o) noexcept { std::swap(p, o.p); return *this; }
    ~HostBuf() { reset(); }
    void reset()
    {
        if (p) (void)hipHostFree((void *)p);
        p = nullptr;
    }
    int alloc(size_t count, unsigned flags = hipHostMallocDefault)
    {
        reset();
        const hipError_t e = hipHostMalloc((void **)&p, std::max<size_t>(count, 1) * sizeof(T), flags);
        if (e == hipSuccess) return VRT_OK;
        p = nullptr;
        return fail(VRT_ENODEVICE, std::string("hipHostMalloc: ") + hipGetErrorString(e));
    }
    operator T *() const { return p; }
};

struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(Stream &&o) noexcept : s(o.s) { o.s = nullptr; }
    Stream &operator=(Stream &&o) noexcept { std::swap(s, o.s); return *this; }
    ~Stream() { reset(); }
    void reset()
    {
        if (s) (void)hipStreamDestroy(s);
        s = nullptr;
    }
    int create(unsigned flags = hipStreamNonBlocking)
    {
        reset();
        const hipError_t e = hipStreamCreateWithFlags(&s, flags);
        if (e == hipSuccess) return VRT_OK;
        s = nullptr;
        return fail(VRT_ENODEVICE, std::string("hipStreamCreateWithFlags: ") + hipGetErrorString(e));
    }
    operator hipStream_t() const { return s; }
};

struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event &&o) noexcept : e(o.e) { o.e = nullptr; }
    Event &operator=(Event &&o) noexcept { std::swap(e, o.e); return *this; }
    ~Event() { reset(); }
    void reset()
    {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
    int create(unsigned flags = hipEventDefault)      // (timing events: the default; the rest pass hipEventDisableTiming)
    {
        reset();
        const hipError_t err = hipEventCreateWithFlags(&e, flags);
        if (err == hipSuccess) return VRT_OK;
        e = nullptr;
        return fail(VRT_ENODEVICE, std::string("hipEventCreateWithFlags: ") + hipGetErrorString(err));
    }
    operator hipEvent_t() const { return e; }
};

// Runs body(t) for t = 0 .. count-1 on `count` host threads.  A worker must not throw (an exception that leaves a
// std::thread's function is std::terminate for the whole host process -- Julia or Python): every body runs inside a
// try block, and a thread that cannot be created has its share done by the calling thread.  Returns false when a
// body threw (std::bad_alloc in practice: the callers report VRT_ENOMEM).
template <typename Body>
inline bool run_workers(int count, Body body)
{
    std::vector<char> threw((size_t)std::max(count, 1), 0);
    auto guarded = [&](int t) {
        try {
            body(t);
        } catch (...) {
            threw[(size_t)t] = 1;
        }
    };
    std::vector<std::thread> pool;
    try {
        pool.reserve((size_t)std::max(count, 1));
    } catch (...) {
    }
    for (int t = 0; t < count; t++) {
        try {
            pool.emplace_back(guarded, t);
        } catch (...) {
            guarded(t);
        }
    }
    for (auto &th : pool) th.join();
    for (int t = 0; t < count; t++)
        if (threw[(size_t)t]) return false;
    return true;
}

constexpr int kMaxAngles = 64;          // active angles per plan (kernel-argument weight table)
constexpr int64_t kMaxGuess = 70;       // read_cell's neighbour cap, voronoi_utils.jl:42
constexpr int32_t kNoUpwind = -1;

// One sweep direction of the grid (up: from the z_min wall, down: from the z_max wall).
struct Direction {
    std::vector<int32_t> layer_of;   // BFS layer per site, 1-based (voronoi_utils.jl:93-174)
    std::vector<int64_t> perm;       // stable sortperm, 1-based site ids (:72,77)
    std::vector<int64_t> reduced;    // reduce_layers offsets, 1-based, r[end] = n (:253-269)
    int64_t n1 = 0;                  // reduced[1] - 1: sites that receive I_0
    DevBuf<int32_t> d_order;         // device copy of perm, 0-based int32: sweep position -> site
    DevBuf<int32_t> d_rank;          // inverse: site -> sweep position
    DevBuf<int32_t> d_lay;           // 0-based layer boundaries: layer l = [lay[l-1], lay[l]), L+1 entries
    // STORAGE order of the layer-tile path: layers contiguous exactly like the sweep order, but
    // inside a layer the sites are sorted in strips of rows (vrt_grid.cpp; VRT_STORE_ORDER=morton: along a Morton curve over (x, y)) so that spatial
    // neighbours (and therefore upwind gathers) share cache lines; the never-visited last site
    // perm[n] stays at position n-1.  The Gauss-Seidel ORDER is unaffected (it lives in the schedule).
    std::vector<int32_t> store;      // storage position -> site (0-based)
    DevBuf<int32_t> d_store;
    DevBuf<int32_t> d_srank;         // site -> storage position
};

struct PlanCacheEntry;

// Host <-> device lanes of the host-pointer entry points (vrt_lambda.cpp: vrt_plan_execute_line): per lane a copy stream
// and two pinned staging buffers, filled / drained by a host thread of its own, so that the caller's pageable arrays
// travel at PCIe speed (a pageable hipMemcpy stages through ONE thread: 0.4 GB of S took 20 ms each way)
struct CopyLane {
    Stream st;
    HostBuf<char> pin[2];
    Event ev[2];
};
constexpr size_t kCopyChunk = (size_t)8 << 20;      // bytes per staging buffer

// Tuning options of a plan (vrt_plan_set_option / vrt_grid_set_option).  Defaults; an environment variable of the
// option's name presets it, read ONCE when the plan is created (never during an execute).  Results do not
// depend on any of them (the parity tests run the paths and shapes against each other).
struct Tuning {
    int path = 0;                 // VRT_PATH: 0 auto, 1 levels, 2 tiles, 3 steps, 4 patches
    int step_K = 0;               // VRT_STEP_K: sites per thread of the layer-step level kernels (0: fewest that fit)
    int step_single = 0;          // VRT_STEP_SINGLE: 1 = the single-wavelength level kernel on any grid
    int step_pairs = 0;           // VRT_STEP_PAIRS: wavelength pairs per coefficient thread (0: 4 to 6)
    int step_xcd = 2;             // VRT_STEP_XCD: block -> XCD map of the coefficient kernel
    int step_streams = 2;         // VRT_STEP_STREAMS: internal streams of the layer paths (1..4)
    int step_level_map = 1;       // VRT_STEP_LEVEL_MAP: level workgroups of an angle on one XCD
    int step_group_dir = 1;       // VRT_STEP_GROUP_DIR: one direction per stream when balanced
    int tile_wide = 1;            // VRT_TILE_WIDE, VRT_TILE_PRE: variants of the persistent tile path
    int tile_pre = 1;
    int patch_K = 1, patch_NT = 512;   // VRT_PATCH_K, VRT_PATCH_NT: entries per thread, threads (plan creation only)
    int patch_own = 0;            // VRT_PATCH_OWN: owned sites per patch at most (0: as many as fit; creation only)
    int patch_Q = 1;              // VRT_PATCH_Q: wavelength pairs a patch workgroup solves at a time
    int pair_block = 1;           // VRT_PAIR_BLOCK: wavelength pairs of a site kept side by side in the patch path's
                                  //   storage layout, 1 / 2 / 4 / 8 / 16 (vrt_device.h; creation only: the native
                                  //   per-angle alpha of the plan is laid out with it)
    int patch_quad = 1;           // VRT_PATCH_QUAD: fp32 storage in blocks of >= 2 pairs, four wavelengths per lane
                                  //   (k_patch_quad; creation only: the native float alpha is laid out with it)
    int patch_lean = 1;           // VRT_PATCH_LEAN: the 64-register form of the (1, 1, NT) kernel (four workgroups per CU;
                                  //   default for two and more wavelength pairs)
    int patch_chain = 2;          // VRT_PATCH_CHAIN: every layer inside ONE chained launch (k_patch_chain) instead of one launch
                                  //   per layer and direction: 0 never, 1 wherever it exists, 2 = auto: where a layer
                                  //   alone cannot fill the chip (patch_shape)
    int chain_pairs = 9;          // VRT_CHAIN_PAIRS: wavelength-pair blocks an item of the chained launch solves at most
    int chain_spin = 2048;        // VRT_CHAIN_SPIN: polls (x 1024) after which a waiting workgroup gives up (~2 s)
    int chain_dataflag = 2;       // VRT_CHAIN_DATAFLAG: the chained launch's intensities as their own flags: 0 never, 1 wherever
                                  //   the kernel exists, 2 auto (one or two wavelength pairs: the planes are filled per step)
    int patch_split = 0;          // VRT_PATCH_SPLIT: workgroups per item of a per-layer launch, fixed (0: from VRT_PATCH_TARGET)
    int patch_target = 0;         // VRT_PATCH_TARGET: workgroups per launch aimed at when the pair steps of an item are split
                                  //   (0: a balanced split chosen per launch, launch_patch_layer)
    int patch_order = 1;          // VRT_PATCH_ORDER: dispatch order of the patch blocks of a per-layer launch: 0 = the workgroups of an
                                  //   item side by side (interleaved), 1 = share-major, every item's longest share first
                                  //   (vrt_patch.hip: patch_block_of; default since profiles/order/INDEX.md)
    int patch_reduce_ride = 0;    // VRT_PATCH_REDUCE_RIDE: 1 = the J reduction of a per-layer launch in its patch blocks' start-up (a
                                  //   launch without patch rows, or whose patch grid cannot take it at four elements per
                                  //   thread, keeps its reduction rows), 0 = reduction rows always (vrt_patch.hip: ride_slice).
                                  //   Default 0: on C4 riding runs at 6.849 ms against 6.613 with rows (profiles/reduce_ride/INDEX.md)
    int patch_timeline = 0;       // VRT_PATCH_TIMELINE: the blocks of the per-layer launches leave their start and end stamps
                                  //   (-DVRT_DIAG build only: tools/patch_timeline.py)
    int chain_static = 1;         // VRT_CHAIN_STATIC: the progress-word form of the chained launch maps block -> item statically (0: tickets)
    int lambda_native = 1;        // VRT_LAMBDA_NATIVE: the Λ-iteration session keeps S and J in sweep order between its steps
                                  //   (read when a session is created; 0: the caller's layout, two layout changes per iteration)
    int debug_flags = 0, debug_skip_levels = 0, tile_debug = 0;   // timing diagnostics (-DVRT_DIAG build only)
};
void tuning_from_env(Tuning &t);
// VRT_OK, or VRT_EINVAL for an unknown name / bad value; `created`: the plan exists already (creation-only options fail)
int tuning_set(Tuning &t, const char *name, const char *value, bool created);

// The arguments of one execute, filled in by its entry point (vrt_plan_execute[_dev][_f32], vrt_plan_execute_native_dev[_f32],
// the Λ-iteration and the multi-device session).  Caller-layout calls pass S, J and I_out as (n, ld) rows; native calls
// (vrt_plan_execute_native_dev) pass S and J as per-direction sweep-order planes (index 0 up, 1 down), read and written in
// place by the layer paths.  Pointers are device pointers; double, or float when f32.
struct ExecArgs {
    int64_t nlam = 0, ld = 0;
    const void *S = nullptr;                      // caller layout
    const void *S_nat[2] = {nullptr, nullptr};    // sweep order (native)
    const void *alpha = nullptr;
    int alpha_mode = 0;
    const void *I0[2] = {nullptr, nullptr};       // boundary intensities of the up / down sweeps
    const double *weights = nullptr;              // host, per user angle
    void *J = nullptr;                            // caller layout
    void *J_nat[2] = {nullptr, nullptr};          // sweep order (native)
    void *I_out = nullptr;                        // caller layout, per user angle
    bool native = false;
    bool f32 = false;                             // fp32 storage of S, α, I, J (arithmetic stays fp64)
    hipStream_t st = nullptr;
    bool wants_J() const { return native ? J_nat[0] != nullptr : J != nullptr; }
};
inline ExecArgs caller_args(int64_t nlam, int64_t ld, const void *S, const void *alpha, int alpha_mode, const void *I0_up,
                            const void *I0_down, const double *weights, void *J, void *I_out, hipStream_t st, bool f32)
{
    ExecArgs x;
    x.nlam = nlam; x.ld = ld;
    x.S = S;
    x.alpha = alpha; x.alpha_mode = alpha_mode;
    x.I0[0] = I0_up; x.I0[1] = I0_down;
    x.weights = weights;
    x.J = J; x.I_out = I_out;
    x.f32 = f32;
    x.st = st;
    return x;
}
inline ExecArgs native_args(int64_t nlam, const void *S_up, const void *S_down, const void *alpha, int alpha_mode,
                            const void *I0_up, const void *I0_down, const double *weights, void *J_up, void *J_down,
                            hipStream_t st, bool f32)
{
    ExecArgs x = caller_args(nlam, (nlam + 1) / 2 * 2, nullptr, alpha, alpha_mode, I0_up, I0_down, weights, nullptr, nullptr,
                             st, f32);     // (ld: the planes' wavelength count, padded to whole pairs)
    x.S_nat[0] = S_up; x.S_nat[1] = S_down;
    x.J_nat[0] = J_up; x.J_nat[1] = J_down;
    x.native = true;
    return x;
}

// ---- the chained launch of the fused patch path: everything a plan keeps for it (vrt_patch.hip: launch_patch_chain) ----
// One item set on the device: eight XCD queues of items and the dependency lists they point into, built for one
// (pair count, block, split, reduce) combination (vrt_patch.cpp: build_chain_items).
struct ChainItems {
    int npair = -1, lgB = -1, nsplit = -1, reduce = -1;
    DevBuf<int4> items;
    DevBuf<int32_t> deps;
    int q_off[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};      // queue x: items [q_off[x], q_off[x + 1])
    bool segments_even = false;          // every queue holds the same number of items in every segment (build_chain_items)
};
struct ChainLaunch {
    // The item sets this plan has run, most recently used first: sets[0] is the one in use.  A caller that alternates
    // wavelength counts, or J and no J, switches between them instead of rebuilding (and freeing: a device synchronisation).
    static constexpr size_t kSets = 4;
    std::vector<ChainItems> sets;
    DevWork<uint32_t> progress;          // one word per (split, patch); they only grow
    bool progress_fresh = false;         //   allocated since the last launch: zero them on the launch stream
    DevBuf<uint32_t> ctrl;               // queue heads and the give-up word (chain_ctrl_words() of them)
    HostBuf<uint32_t> h_status;          // mapped host word: a launch gave up
    uint32_t *d_status = nullptr;        //   its device address (borrowed from h_status)
    DevBuf<char> d_args;                 // the launch's argument block (ChainDev)
    HostBuf<char> h_args_pinned;         //   and its staging copy
    std::vector<char> h_args;            //   what the device copy holds
    Event args_ev;                       //   the last copy out of the staging copy
    bool args_ev_valid = false;
    uint32_t epoch = 0;                  // counts the launches; stale progress words compare as "behind"

    // The control words, or NULL before the plan's first chained launch.
    uint32_t *ctrl_words() const { return ctrl; }
    // The set of this combination to the front: one of the sets, or -- after the least recently used of kSets has gone
    // (freeing it waits for the device) -- what make(ChainItems &) builds.  A make that fails leaves the sets as they were.
    template <typename Make>
    int select(int npair, int lgB, int nsplit, bool reduce, Make make)
    {
        for (size_t c = 0; c < sets.size(); c++)
            if (sets[c].npair == npair && sets[c].lgB == lgB && sets[c].nsplit == nsplit && sets[c].reduce == (reduce ? 1 : 0)) {
                std::rotate(sets.begin(), sets.begin() + (long)c, sets.begin() + (long)c + 1);
                return VRT_OK;
            }
        sets.reserve(kSets);
        if (sets.size() == kSets) sets.pop_back();
        ChainItems cs;
        if (int rc = make(cs)) return rc;
        cs.npair = npair; cs.lgB = lgB; cs.nsplit = nsplit; cs.reduce = reduce ? 1 : 0;
        sets.insert(sets.begin(), std::move(cs));
        return VRT_OK;
    }
};

}  // namespace vrt

namespace vrt {
struct RasterLocator;                // vrt_raster.hip: cell list and seeds of the nearest-site walk, workspaces
void raster_locator_delete(RasterLocator *L);
struct RasterLocatorDelete { void operator()(RasterLocator *L) const { raster_locator_delete(L); } };
}

struct vrt_grid {
    int device = 0;
    int64_t n = 0;
    int64_t D = 0;                   // maximum(neighbours[:,1])
    double bounds[6] = {0, 0, 0, 0, 0, 0};
    std::vector<double> pos;         // (3, n) z,x,y
    std::vector<int32_t> rowptr;     // CSR over the neighbour lists, n+1
    std::vector<int32_t> col;        // 1-based ids, walls <= 0, row order preserved
    vrt::Direction up, down;
    // device mirrors
    vrt::DevBuf<double> d_pos;
    vrt::DevBuf<int32_t> d_rowptr, d_col;
    vrt::DevBuf<double> d_lz, d_lx, d_ly;      // Delaunay lines, CSR-packed SoA
    vrt::Stream stream;
    vrt::DevBuf<unsigned long long> d_scalars; // scratch of the Λ-iteration epilogue's reduction (kUpdateWords)
    vrt::DevBuf<double> d_small;               // wavelength-sized host arrays of the physics kernels (λ, 2hc²/λ⁵, σ_bf)
    size_t small_cap = 0;
    vrt::HostBuf<double> h_small;              // pinned staging buffer of the same capacity
    vrt::Event small_ev;                       // last kernel that read d_small
    bool small_ev_valid = false;
    vrt::Event small_copy_ev;                  // last copy out of h_small
    bool small_copy_valid = false;
    // options applied to the single-solve plans cached below (vrt_grid_set_option)
    std::vector<std::pair<std::string, std::string>> options;
    // cache of single-angle plans for vrt_delaunay_up/down
    std::mutex mu;
    std::vector<std::unique_ptr<vrt::PlanCacheEntry>> cache;    // (declared after the device mirrors: the plans go first)
    // nearest-site search of the raster resampling (built on first use, under mu); cells per axis, 0 = auto
    std::unique_ptr<vrt::RasterLocator, vrt::RasterLocatorDelete> locator;
    int64_t nearest_cells = 0;
};

struct vrt_plan {
    vrt_grid *g = nullptr;              // borrowed: the caller keeps the grid alive for as long as the plan
    int device = 0;                     // of the grid (kept here: destroying the plan must not look into a grid that may be gone)
    vrt::Tuning tune;
    int n_sweeps = 3;
    int64_t n_angles_user = 0;
    int A = 0;                          // active angles (k[0] != 0)
    std::vector<int> user_of_active;    // active index -> user angle index
    std::vector<int> dir_of_active;     // +1 up, -1 down
    std::vector<double> k;              // (3, A)
    // per-angle upwind tables, [A][n]
    vrt::DevBuf<int32_t> d_up1, d_up2;              // 0-based ids, kNoUpwind if none
    vrt::DevBuf<double> d_d1, d_d2;                  // dot products (smallest_angle's `dots`)
    vrt::DevBuf<double> d_w1, d_w2;                  // dot_weights, irregular_ray_tracing.jl:51
    vrt::DevBuf<double> d_r1, d_r2;                  // euclidean path lengths, :66
    // level schedule, merged over the active angles
    vrt::DevBuf<uint32_t> d_node_site;  // site id (0-based)
    vrt::DevBuf<uint32_t> d_node_meta;  // active angle | zero-read flags
    vrt::DevBuf<int32_t> d_node_u1, d_node_u2;            // the node's upwind site ids (copied next to it)
    std::vector<int64_t> level_off;     // nodes of level t are [level_off[t], level_off[t+1])
    bool level_ready = false;           // the level schedule is built on first use
    std::vector<int32_t> h_up1, h_up2;  // host copies of the upwind ids (schedule building)
    int64_t n_nodes = 0;
    // per-direction lists of active angle indices (for the boundary kernel)
    vrt::DevBuf<int32_t> d_angles_up, d_angles_down;
    int n_up = 0, n_down = 0;
    std::vector<int64_t> skip_site;     // per active angle: never-updated site perm[n] (0-based)
    // workspaces (grow-only)
    vrt::DevWork<double> d_I;
    int64_t I_ld = 0;
    vrt::DevWork<double> d_stage[6];    // S, alpha, I0up, I0down, J, I_out
    // layer paths (vrt_layers.hip, vrt_tables.hip): tables in storage order, per-layer level counts
    bool tile_ok = false;
    bool step_tables_ready = false;      // t_self ... t_code_ss exist (ensure_step_tables)
    int tile_K = 8;                      // sites per thread of the 1024-thread workgroup
    int tile_max_layers = 0;
    int64_t tile_max_layer_size = 0;
    int64_t tile_visits = 0;
    vrt::DevBuf<int32_t> t_u1, t_u2;
    vrt::DevBuf<double> t_w1, t_w2, t_r1, t_r2;
    vrt::DevBuf<uint32_t> t_vis, t_loc;
    // layer-step level kernel: sites of a layer dealt to threads sorted by visit pattern
    vrt::DevBuf<int32_t> t_self;         // [A][n] sorted index (absolute) -> storage position
    vrt::DevBuf<uint32_t> t_vis_s, t_loc_s;            // t_vis / t_loc in sorted order
    vrt::DevBuf<uint32_t> t_gpos;        // [A][n] compact in-layer coupling list (k_gpos)
    vrt::DevBuf<int32_t> t_rank_s;       // [A][n] storage position -> sorted index (inverse of t_self)
    vrt::DevBuf<uint32_t> t_loc_ss;      // [A][n] upwind tile slots of the sorted entries, in SORTED terms
    vrt::DevBuf<uint32_t> t_code_ss;     // [A][n] two-launch tile path: upwind slot + kind codes (layers <= 4096 sites)
    vrt::DevBuf<int32_t> d_nlev, d_angle_dir;
    std::vector<int64_t> angle_visits;   // surviving visits per active angle (task cost)
    std::vector<int32_t> h_task_map;     // block -> angle | wavelength << 8
    vrt::DevWork<int32_t> d_task_map;
    int task_map_nlam = -1;
    vrt::DevWork<double> ws_S[2], ws_A[2], ws_J[2];
    vrt::DevWork<double> ws_AA;
    vrt::DevWork<double> ws_cg[2];           // layer-step coefficient buffers: constant terms, compact couplings
    // layer-step path: internal streams and the angle groups they advance through the layers
    int step_groups = 0;
    vrt::DevBuf<int32_t> d_step_angles;
    std::vector<int> step_group_off;
    std::vector<double> angle_mean_levels;   // mean in-layer level count per active angle (level-kernel task cost)
    vrt::DevBuf<int32_t> d_level_map;    // block -> task of the layer-step level kernels, per stream group (build_level_map)
    std::vector<int> level_map_off;      //   offsets of the groups' maps (+ end); 8 ceil-blocks each
    int level_map_units = 0, level_map_groups = 0;
    std::vector<int32_t> h_step_angles;  // host copy of d_step_angles
    // fused patch path (vrt_patch.hip): per-angle patch schedules, concatenated over the active angles
    bool patch_ok = false;
    int lg_pair_block = 0;           // log2 of the pairs per block of the patch path's storage layout (vrt_device.h)
    int patch_cap = 0, patch_K = 0, patch_NT = 0;   // entries per patch <= cap = K * NT (fixed at creation)
    int64_t n_patches = 0, n_patch_entries = 0, n_patch_visits = 0;
    std::vector<int32_t> h_patch_first;  // [A][tile_max_layers + 2]: index of the first patch of (angle, layer)
    std::vector<int4> h_patch_rec;       // per patch: first entry, entries, first owned position, owned sites
    vrt::DevBuf<int32_t> e_pos, e_u1, e_u2;
    vrt::DevBuf<uint32_t> e_vis, e_loc;
    vrt::DevBuf<double> e_w1, e_w2, e_r1, e_r2;
    std::vector<int2> h_patch_rec2;      // per patch: levels, active angle
    std::vector<int64_t> h_patch_dep_off;   // per patch: the patches (plan-wide indices) whose stored intensities it gathers
    std::vector<int32_t> h_patch_deps;      //   (vrt_patch.cpp: dep_list) -- what the chained launch waits on
    vrt::ChainLaunch chain;              // chained launch (vrt_patch.hip: k_patch_chain)
    vrt::DevBuf<int4> d_patch_work;      // work lists of the launches: two int4 per slot (ensure_patch_work, PatchArgs::wrec)
    std::vector<int64_t> patch_work_off; //   [group][layer] offsets into it
    int patch_work_groups = 0;
    int64_t patch_work_padding = 0;      //   slots of it that hold no patch (a layer's items are dealt to 8 runs of one length)
    vrt::DevBuf<unsigned long long> d_patch_tl;   // timeline of the -DVRT_DIAG build (VRT_PATCH_TIMELINE): three words per block
    std::vector<int64_t> patch_tl_launches;       //   kPatchTimelineRec numbers per recorded launch of the last sweep
    int64_t patch_tl_blocks = 0;                  //   blocks recorded so far
    int64_t patch_rode_launches = 0, patch_rode_chunks = 0;   // per-layer launches of the last sweep whose reduction rode in their
                                                  //   patch blocks, and the most chunks a block of them took (vrt_plan_patch_ride_stats)
    vrt::Stream step_stream[4];
    vrt::Event step_fork, step_join[4];
    int last_path = 0;                   // path of the last execute (vrt_plan_last_path): 1 levels, 2 tiles, 3 steps, 4 patches
    vrt::Event ev0, ev1;
    bool ev_valid = false;
    std::vector<vrt::CopyLane> copy_lanes;      // host-pointer entry points (ensure_copy_lanes)
    vrt::Event copy_done;
    int64_t last_launches = 0;
    std::mutex mu;
};

namespace vrt {

struct PlanDelete { void operator()(vrt_plan *p) const { vrt_plan_destroy(p); } };   // (makes the plan's device current)
using PlanPtr = std::unique_ptr<vrt_plan, PlanDelete>;
struct GridDelete { void operator()(vrt_grid *g) const { vrt_grid_destroy(g); } };
using GridPtr = std::unique_ptr<vrt_grid, GridDelete>;

struct PlanCacheEntry {
    double k[3];
    int n_sweeps;
    PlanPtr plan;
    int users;          // single solves running on the plan right now (guarded by the grid's mutex)
};

// ---- host-side grid preparation (vrt_grid.cpp) ---------------------------------------------
int parse_neighbour_file(const char *path, int64_t n, std::vector<int64_t> &matrix, int64_t &D1);
int build_grid_host(vrt_grid *g, int64_t n, const double *pos, const int64_t *nbr, int64_t D1,
                    const double bounds[6]);

// ---- in-process tessellation (vrt_tessellate.cpp) ------------------------------------------------
int tessellate_host(int64_t n, const double *pos, const double bounds[6], int64_t D1, int64_t *nbr_out,
                    int64_t *max_count, int nthreads);
// host threads for `count` cells: the hardware's, at most 64, at least one per 256 cells
inline int tessellate_threads(int64_t count)
{
    const unsigned hw = std::thread::hardware_concurrency();
    return (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)(hw ? hw : 4), 64, count / 256 + 1}));
}
// the same cells for the m listed sites only (0-based ids, any order): rows_out (m, D1) column-major, row k of sites[k];
// what the device tessellation (vrt_tessellate.hip) recomputes its flagged sites with
int tessellate_host_sites(int64_t n, const double *pos, const double bounds[6], int64_t D1, int64_t m, const int64_t *sites,
                          int64_t *rows_out, int64_t *max_count, int nthreads);

// ---- schedule (vrt_schedule.cpp) -------------------------------------------------------------
struct AngleSchedule {
    std::vector<uint32_t> site;      // live nodes sorted by level
    std::vector<uint8_t> zflags;     // bit0: I(upwind 1) reads as zero, bit1: upwind 2
    std::vector<int64_t> level_off;  // per-angle level offsets (level 1 first)
    int64_t bad_site = -1;           // visited site without an upwind neighbour
};
void build_angle_schedule(const Direction &dir, bool ascending, int64_t n, int n_sweeps,
                          const int32_t *up1, const int32_t *up2, AngleSchedule &out);
struct LayerSchedule {
    std::vector<uint32_t> vis;       // per site (original id): 4 x 8-bit in-layer visit levels
    std::vector<int32_t> nlev;       // per layer (index = 1-based layer): number of levels
    int64_t n_visits = 0;
    int64_t max_layer_size = 0;
    int64_t bad_site = -1;
    bool ok = false;                 // fits the tile kernel's encoding
};
void build_layer_schedule(const Direction &dir, bool ascending, int64_t n, int n_sweeps,
                          const int32_t *up1, const int32_t *up2, LayerSchedule &out);
void build_sorted_slots(const Direction &dir, int64_t n, const std::vector<uint32_t> &vis_site,
                        std::vector<int32_t> &self);
// Patch schedule of the fused layer kernel (vrt_patch.cpp): every layer cut into ranges of
// consecutive storage positions, each with the in-layer dependency cone of its sites.
struct PatchSchedule {
    std::vector<int32_t> layer_patch_off;   // patches of layer l (1-based): [off[l], off[l+1]); L + 2 entries
    std::vector<int32_t> patch_own_lo;      // first owned storage position
    std::vector<int32_t> patch_own_cnt;     // owned sites (consecutive storage positions)
    std::vector<int32_t> patch_nlev;        // in-layer levels the patch has to run
    std::vector<int64_t> patch_ent_off;     // entries of patch q: [off[q], off[q+1]); owned first, then the halo
    std::vector<int32_t> entry_pos;         // storage position of the entry's site
    std::vector<uint32_t> entry_vis;        // up to 4 x 8-bit visit levels the patch executes for it, increasing
    std::vector<uint32_t> entry_loc;        // patch-local tile slots of its two upwinds, 16 bits each; 0xFFFF: reads 0
    std::vector<int64_t> dep_off;           // patches of EARLIER layers whose stored intensities patch q gathers:
    std::vector<int32_t> dep_list;          //   dep_list[dep_off[q] .. dep_off[q+1]), sorted (chained launch: what q waits for)
    int64_t n_visits = 0;                   // visits executed over all patches (halo visits counted per patch)
    int64_t n_live = 0;                     // live visits of the unsplit schedule
    int64_t max_entries = 0;
    int64_t bad_site = -1;
    bool ok = false;
};
// `threads`: host threads the layers of the angle are dealt to (they are analysed independently); may throw std::bad_alloc
void build_patch_schedule(const Direction &dir, bool ascending, int64_t n, int n_sweeps, const int32_t *up1,
                          const int32_t *up2, int own_target, int entry_cap, PatchSchedule &out, int threads = 1,
                          LayerSchedule *layers = nullptr);
// (`layers`: also filled with what build_layer_schedule returns for the angle -- the same analysis, done layer by layer
//  here -- whenever its packed encoding fits; !layers->ok with bad_site < 0 means "ask build_layer_schedule")

// ---- device launchers (vrt_kernels.hip) ------------------------------------------------------
int launch_delaunay_lines(vrt_grid *g);
int launch_upwind_table(vrt_plan *p, int a);
struct SweepArgs {
    int64_t n, nlam, ldS, ldA, ldI;
    const void *S, *alpha;     // double, or float when f32
    int alpha_mode;
    void *I;
    bool f32 = false;          // fp32 storage of S, α, I, J (arithmetic stays fp64)
};
int launch_boundary(vrt_plan *p, const SweepArgs &sa, const void *dI0_up, const void *dI0_down,
                    hipStream_t st);
int launch_sweep_levels(vrt_plan *p, const SweepArgs &sa, hipStream_t st, int64_t *launches);
int launch_reduce_J(vrt_plan *p, const SweepArgs &sa, const double *weights_active, void *dJ,
                    int64_t ldJ, hipStream_t st);
int launch_copy_I_out(vrt_plan *p, const SweepArgs &sa, void *dI_out, int64_t ldO, hipStream_t st);

constexpr size_t kUpdateWords = 3;   // a grid's d_scalars: the criterion's maximum, its NaN flag, the continuum's thick count
                                     //   (the line ALI updates: the entries that fell back to the plain update)
// The words of an update, home: the criterion's scalar (NaN like Julia's maximum) and, if asked for, the third word.
// `words`: 2 or 3, as many as the update defined (a plain line update clears and writes two: its third is never read, and
// *third stays what it was).  Synchronises `st`.
inline int read_criterion(const unsigned long long *d_result, size_t words, hipStream_t st, double *max_rel_change,
                          int64_t *third = nullptr)
{
    unsigned long long h[kUpdateWords] = {0, 0, 0};
    VRT_HIP_TRY(hipMemcpyAsync(h, d_result, words * sizeof(h[0]), hipMemcpyDeviceToHost, st));
    VRT_HIP_TRY(hipStreamSynchronize(st));
    double d;
    std::memcpy(&d, &h[0], sizeof(double));
    *max_rel_change = h[1] ? std::nan("") : d;
    if (third && words > 2) *third = (int64_t)h[2];
    return VRT_OK;
}
int launch_axpy(size_t count, const double *d_src, double *d_dst, hipStream_t st);
int launch_gather_rows(int64_t rows, int64_t nlam, int64_t ld, const int32_t *d_order, const double *d_src, double *d_dst,
                       hipStream_t st);
int launch_gather_rows_f32(int64_t rows, int64_t nlam, int64_t ld, const int32_t *d_order, const double *d_src, float *d_dst,
                           hipStream_t st);                                            // the same rows, rounded to float
int launch_round_to_f32(size_t count, const double *d_src, float *d_dst, hipStream_t st);    // dst = (float)src
int launch_widen_f32(size_t count, const float *d_src, double *d_dst, hipStream_t st);       // dst = (double)src, exact
// d_diag: Λ* of this iterate's α in the layout of the other arrays (the ALI update; d_result then has a third word, the
// entries that fell back to the plain update), or NULL: the plain update, two words
int launch_lambda_update(int64_t n, int64_t nlam, int64_t ld, const double *dJ, const double *dB,
                         const double *deps, const double *dS_old, double *dS_new,
                         unsigned long long *d_result, hipStream_t st, const double *d_diag = nullptr);
// the same on sweep-order planes (J_up, J_down in, B in the up order, S_up updated in place, S_down written; Λ* up order)
int launch_lambda_update_native(vrt_grid *g, int64_t nlam, const double *dJ_up, const double *dJ_down, const double *dB_up,
                                const double *deps, double *dS_up, double *dS_down, unsigned long long *d_result, hipStream_t st,
                                const double *dL_up = nullptr);
// Λ* of the line case (vrt_line_ali.hip) from the plan's native per-angle α: into (n, ld) rows, or into an up-order plane
// set (a plan whose double planes exist: native_planes_ok).  Caller holds p->mu and has chosen the device.
int launch_line_lambda_diagonal(vrt_plan *p, int64_t nlam, const double *d_alpha_native, const double *weights, int64_t ld,
                                double *d_rows, double *d_up_planes, hipStream_t st);
// the same on the plan's FLOAT plane sets (pair blocks of native_lg(p, true); the roundings: include/voronoirt.h)
int launch_lambda_update_native_f32(vrt_plan *p, int64_t nlam, const float *dJ_up, const float *dJ_down, const float *dB_up,
                                    const double *deps, float *dS_up, float *dS_down, unsigned long long *d_result, hipStream_t st);

// ---- physics either side of the formal solve (vrt_physics.hip) -------------------------------------
int launch_line_opacity(vrt_plan *p, int64_t nlam, const double *d_lambda, double lambda0, double c0,
                        const double *d_velocity, const double *d_doppler, const double *d_gamma,
                        const double *d_strength, const double *d_alpha_cont, void *d_out, hipStream_t st,
                        bool f32_out = false);
int launch_line_terms(int64_t n, const double *d_gamma_static, const double *d_gamma_unsold, const double *d_pops,
                      double strength_const, double Bij, double Bji, double *d_gamma, double *d_strength, hipStream_t st);
// (the rate launches and their named arguments: vrt_line_case.h)

// ---- entry-point internals shared with vrt_lambda.cpp (vrt_api.cpp) ---------------------------------
// one execute (caller holds p->mu): checks the arguments, chooses the path, runs it
int execute_locked(vrt_plan *p, const ExecArgs &x);

// ---- layer paths (vrt_tables.hip, vrt_layers.hip) ----------------------------------------------------------
int ensure_step_tables(vrt_plan *p);     // sorted-slot tables of the steps / tiles paths, on first use (vrt_api.cpp)
int launch_permute_table(vrt_plan *p, int a, const uint32_t *d_vis_site);
int launch_sorted_tables(vrt_plan *p, int a);
int launch_gpos(vrt_plan *p, int a);
// log2 of the pairs per block of the plan's NATIVE per-angle alpha (and of every plane of the patch path)
// (fp32 storage: at least two pairs, so that k_patch_quad can take them as one 16-byte access)
inline int native_lg(const vrt_plan *p, bool f32)
{
    if (!p->patch_ok) return 0;
    return f32 && p->tune.patch_quad != 0 && p->patch_K == 1 ? std::max(p->lg_pair_block, 1) : p->lg_pair_block;
}
int alpha_to_native(vrt_plan *p, int64_t nlam, int64_t ld, const void *dalpha, void *out, hipStream_t st, bool f32);
// sweep-order S and J (per direction [pairs][n][2] in that direction's storage order)
int native_planes_ok(const vrt_plan *p, bool f32 = false);
int planes_to_native_f32(vrt_plan *p, int64_t nlam, int64_t ld, const float *din, float *out_up, float *out_down, hipStream_t st);
int plane_from_native_f32(vrt_plan *p, int dir_index, int64_t nlam, int64_t ld, const float *din, float *dout, hipStream_t st);
int J_from_native_f32(vrt_plan *p, int64_t nlam, int64_t ld, const float *dJ_up, const float *dJ_down, float *dJ, hipStream_t st);
int planes_to_native(vrt_plan *p, int64_t nlam, int64_t ld, const double *din, double *out_up, double *out_down, hipStream_t st);
int plane_from_native(vrt_plan *p, int dir_index, int64_t nlam, int64_t ld, const double *din, double *dout, hipStream_t st);
int J_from_native(vrt_plan *p, int64_t nlam, int64_t ld, const double *dJ_up, const double *dJ_down, double *dJ, hipStream_t st);
// one execute on a layer path (2 tiles, 3 steps, 4 patches) that choose_path (vrt_api.cpp) chose for `x`
int execute_layers(vrt_plan *p, const ExecArgs &x, int path);
int64_t steps_max_layer(bool f32);   // largest layer the layer-step level kernels hold
// the per-angle native α of the line case exists on the layer paths only; `who`: the subject of the refusal
inline int line_path_ok(const vrt_plan *p, const char *who)
{
    if (!p->patch_ok && (!p->tile_ok || p->tile_max_layer_size > steps_max_layer(false)))
        return fail(VRT_EINVAL, std::string(who) + " needs a layer path (at most 4 visits per site and 255 levels per layer)");
    return VRT_OK;
}

// ---- fused patch path (vrt_patch.hip) ----------------------------------------------------------------
struct TileArgs;
struct PatchReduce;
bool patch_shape_exists(int K, int Q, int NT);
// The kernel shape of a patch launch of `npair` wavelength pairs: THE place that decides it (vrt_patch.cpp).  Q_asked:
// pairs a workgroup is asked to solve at a time (the plan's VRT_PATCH_Q; 1 for a launch that only reduces).
// lgB: log2 of the pairs per block of the planes (native_lg); quad: fp32 storage, k_patch_quad, two neighbouring pairs of a
// block per workgroup; lean: k_patch_lean, the 64-register form of the (1, 1, NT) kernel; lgS: log2 of the sibling
// workgroups per pair block; Q: pairs a workgroup solves at a time; chain: every layer inside ONE chained launch
// (k_patch_chain); chain_dataflag: ... with the intensities as their own flags (chain_data_wait).
struct PatchShape {
    int lgB = 0, quad = 0, lean = 0, lgS = 0, Q = 1;
    bool chain = false, chain_dataflag = false;
};
PatchShape patch_shape(const vrt_plan *p, int npair, bool f32, int Q_asked);
// The plan's patch index as the item builders read it (vrt_patch.cpp; nothing of it is copied).
struct PatchIndex {
    const std::vector<int32_t> &first;      // h_patch_first
    const std::vector<int4> &rec;           // h_patch_rec
    const std::vector<int2> &rec2;          // h_patch_rec2
    const std::vector<int64_t> &dep_off;    // h_patch_dep_off
    const std::vector<int32_t> &deps;       // h_patch_deps
    const std::vector<int> &dir_of_active;
    const std::vector<int64_t> *reduced[2]; // the directions' reduce_layers offsets (0 up, 1 down)
    int max_layers;                         // tile_max_layers
    int64_t n;
};
// Work lists of the per-layer launches, two int4 per slot (PatchArgs::wrec): `off` [group][layer] (+ end) in slots,
// `padding` the slots that hold no patch.
void build_patch_work(const PatchIndex &ix, int G, const std::vector<int32_t> &group_angles, const std::vector<int> &group_off,
                      std::vector<int4> &work, std::vector<int64_t> &off, int64_t &padding);
// Items of the chained launch, three int4 each, queue x at [set.q_off[x], set.q_off[x + 1]); `deps`: the patches' dependency
// lists with those of the J_dir items behind them; set.segments_even: every queue holds the same number of items in every
// (layer, direction) and J_dir segment.
int build_chain_items(const PatchIndex &ix, int nblock, int nsplit, bool with_reduce, std::vector<int4> &items,
                      std::vector<int32_t> &deps, ChainItems &set);
int launch_patch_entries(vrt_plan *p, int a, int64_t first, int64_t count);
int ensure_patch_work(vrt_plan *p, int G, const std::vector<int32_t> &group_angles, const std::vector<int> &group_off);
int launch_patch_layer(vrt_plan *p, const TileArgs &ta, int npair, int layer, int group, const PatchShape &shape, hipStream_t st,
                       bool f32, const PatchReduce *reduce);
// numbers per launch of the timeline: layer, stream group, gridDim.x, gridDim.y, work-list rows, splits, log2 siblings,
// order, patch rows, reduction blocks, first block in the stamps, pair steps of an item
constexpr int kPatchTimelineRec = 12;
void patch_timeline_begin(vrt_plan *p);          // a sweep of per-layer launches starts: forget the last one's records
int patch_timeline_read(vrt_plan *p, int64_t cap_launches, int64_t cap_blocks, int64_t *launches, uint64_t *stamps, int64_t *counts);
// the grid of a per-layer launch and, with `blocks`, what each of its blocks does (vrt_patch_dispatch_map)
int patch_dispatch_map(int order, int nrow, int nsplit, int lg_siblings, int64_t nred, int steps, int64_t *dims, int32_t *blocks);
// which pair elements the blocks of a launch's patch grid reduce in the riding form (vrt_patch_ride_map)
int patch_ride_map(int order, int nrow, int nsplit, int lg_siblings, int npair, int lg_block, int NT, int64_t n, const int32_t *lo,
                   const int32_t *hi, int64_t first_block, int64_t nblocks, int64_t *dims, int64_t *elems);
// ctrl_zeroed: the launch's control words (chain_ctrl_words() of them at p->chain.ctrl_words()) were zeroed on `st` by the caller
int launch_patch_chain(vrt_plan *p, const TileArgs &ta, int npair, const PatchShape &shape, hipStream_t st, bool f32,
                       const PatchReduce *reduce, bool ctrl_zeroed = false);
int chain_ctrl_words();
int patch_chain_check(vrt_plan *p);

// ---- Ng acceleration of the Λ-iteration sessions (vrt_accel.hip) ----------------------------------------
// the elements of an S array that take part: `dense` contiguous doubles (even), then `tail` doubles `tstride` apart
struct NgRange {
    int64_t dense = 0, tail = 0, tstride = 1;
};
// what a session keeps while acceleration is on (order 0: nothing allocated)
struct NgState {
    int order = 0, start = 0, period = 0;
    DevBuf<double> hist[3];                             // S after the 1, 2, 3 iterates before the next due step (x1, x2, x3)
    unsigned have = 0;                                  // bit d-1: hist[d-1] holds its iterate
    DevBuf<double> d_ws;                                // partial sums, sums, verdict
    int last_applied = 0;                               // of the last iterate: 1 taken, 0 none due, -1 rejected
    double last_sums[5] = {0, 0, 0, 0, 0}, last_coeffs[2] = {0, 0};
};
// the physical entries of a session's S of `nlam` wavelengths at `n` sites: a sweep-order plane set is every full pair
// plane dense, then the first halves of an odd nlam's last plane (stride 2; the padding wavelength is never touched);
// the caller's layout is n nlam contiguous doubles
inline NgRange ng_S_range(int64_t n, int64_t nlam, bool sweep_order)
{
    NgRange rg;
    if (sweep_order) { rg.dense = (nlam / 2) * 2 * n; rg.tail = nlam & 1 ? n : 0; rg.tstride = 2; }
    else { rg.dense = (n * nlam) & ~(int64_t)1; rg.tail = (n * nlam) & 1; rg.tstride = 1; }
    return rg;
}
int ng_check_settings(int order, int start, int period);
int ng_configure(NgState &ng, int order, int start, int period, size_t alloc_count);
void ng_release(NgState &ng);
// The device halves of a step on one array (they synchronise `st`): the five sums of x0 .. x3 into sums[5]; x_acc of
// (a, b) into `out` with *ok = every x_acc finite and > 0.  d_ws: the NgState's workspace.  ng_coefficients: host only.
int ng_sums(const NgRange &rg, const double *x0, const double *x1, const double *x2, const double *x3, double *d_ws,
            double sums[5], hipStream_t st);
bool ng_coefficients(const double sums[5], double coeffs[2]);
int ng_apply(const NgRange &rg, double a, double b, const double *x0, const double *x1, const double *x2, double *out,
             double *d_ws, bool *ok, hipStream_t st);
// ---- the phases of what follows a plain update, shared by the sessions that hold S in one array (ng_after_iterate) and
// the multi-device session, whose S is one array per member (vrt_multi.cpp): due -> record | history, sums, apply, commit.
// They are host code and live here, so that a host-only build runs them too (tests/probes/ng_phases_main.cpp).
enum { kNgNothing = 0, kNgRecord1 = 1, kNgRecord2 = 2, kNgRecord3 = 3, kNgStep = 4 };
// what iterate number `iterate` (1-based) calls for -- THE schedule: with d iterates to go until the next due one,
// d = 1, 2, 3 -> S is kept as x_d (kNgRecord1..3 = d); d = 0 -> kNgStep; anything else, or order 0 -> kNgNothing
inline int ng_due(const NgState &ng, int64_t iterate)
{
    if (!ng.order) return kNgNothing;
    const int64_t d = iterate < ng.start ? ng.start - iterate : (ng.period - (iterate - ng.start) % ng.period) % ng.period;
    return d == 0 ? kNgStep : (d <= 3 ? (int)d : kNgNothing);
}
// S kept as x_d, enqueued on `st`.  alloc_count: doubles of an S buffer (padding included, copied along).
inline int ng_record(NgState &ng, int d, const double *S, size_t alloc_count, hipStream_t st)
{
    VRT_HIP_TRY(hipMemcpyAsync(ng.hist[d - 1], S, sizeof(double) * alloc_count, hipMemcpyDeviceToDevice, st));
    ng.have |= 1u << (d - 1);
    return VRT_OK;
}
// a step is due: the history is used up either way; false when it was not complete (switched on too late, or dropped by
// *_set_state): nothing is due then
inline bool ng_take_history(NgState &ng)
{
    const bool complete = ng.have == 7u;
    ng.have = 0;
    return complete;
}
// the session's sums from its members': added in the order of the calls, the first one copied
inline void ng_add_sums(double total[5], const double part[5], bool first)
{
    for (int k = 0; k < 5; k++) total[k] = first ? part[k] : total[k] + part[k];
}
// One array of S with its history and the verdict of its apply (x_acc stands in ng->hist[2], x3's buffer).
struct NgPiece {
    NgState *ng;
    DevBuf<double> *S;
    bool good;
};
// ALL OR NOTHING: with valid coefficients and every verdict good, every piece's x_acc buffer BECOMES its S (true);
// otherwise no S changes (false).  Every verdict is looked at before the first swap.
inline bool ng_commit(NgPiece *pieces, int count, bool coeffs_valid)
{
    if (!coeffs_valid) return false;
    for (int i = 0; i < count; i++)
        if (!pieces[i].good) return false;
    for (int i = 0; i < count; i++) std::swap(*pieces[i].S, pieces[i].ng->hist[2]);
    return true;
}
int ng_after_iterate(NgState &ng, int64_t iterate, DevBuf<double> &S, size_t alloc_count, const NgRange &rg, hipStream_t st);
// What follows the update of iterate number `iterate` in a session whose S stands behind a store (SourceStore, RasterStore):
// acceleration off -> no step; otherwise ng_after_iterate on the store's S, and after an accepted step the store makes
// again what follows S (its down-order copy, its plane-major copy); `st` is synchronised only where that queued work.
template <typename Store>
inline int ng_after_update(NgState &ng, int64_t iterate, Store &store, hipStream_t st)
{
    if (!ng.order) {
        ng.last_applied = 0;
        return VRT_OK;
    }
    int rc = ng_after_iterate(ng, iterate, store.ng_S(), store.ng_count(), store.ng_range(), st);
    if (rc || ng.last_applied != 1) return rc;
    bool queued = false;
    if ((rc = store.ng_refresh(st, &queued)) || !queued) return rc;
    VRT_HIP_TRY(hipStreamSynchronize(st));
    return VRT_OK;
}
int ng_report(const NgState &ng, int *applied, double sums[5], double coeffs[2]);
int launch_ng_mirror(vrt_grid *g, int64_t nlam, const double *dS_up, double *dS_down, hipStream_t st);
// the multi-device session's acceleration (vrt_multi.cpp); the C entries of voronoirt_multi_accel.h are built into the
// companion library libvrt_hip_multi_accel.so (vrt_multi_accel.cpp) and forward to these
int multi_lambda_set_acceleration(vrt_multi_lambda *s, int order, int start, int period);
int multi_lambda_last_acceleration(const vrt_multi_lambda *s, int *applied, double sums[5], double coeffs[2]);

}  // namespace vrt
