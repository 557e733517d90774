// Multi-device object of the C ABI: ONE host process (the reference's Julia driver is one)
// uses several GPUs of a node.  The object owns a grid + plan per device and, when the devices are distinct,
// an in-process RCCL communicator (ncclCommInitAll; the library is dlopen'ed on first use, libvrt_hip.so does
// not link it).  The angle x wavelength loop of J_λ_voronoi (src/lambda_iteration.jl:84-111) is sharded the
// way voronoirt_amd/distributed.py shards it across processes:
//   "lambda"  nλ >= devices: contiguous wavelength blocks (51 over 8 -> 7,7,7,6,6,6,6,6), every device solves
//             all angles of its block and owns whole rows J[l, :]: no exchange, the blocks go home by strided copies
//   "angle"   nλ < devices (or forced): the angles are dealt to the devices (ups and downs separately), the
//             partial J's are summed by ONE RCCL all-reduce -- the north star's scheme
// Two handles on the SAME device (rehearsal on a one-GPU box; RCCL refuses that) sum through a kernel instead.
#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <thread>

#include "vrt_internal.h"
#include "vrt_line_case.h"
#include "vrt_source_store.h"

using namespace vrt;

namespace {

// The few RCCL entry points this file calls, declared here: librccl is dlopen'ed on first use, and the library builds
// (and serves one device) on a ROCm installation without the RCCL development headers.  The values are NCCL's ABI.
typedef struct ncclComm *ncclComm_t;
typedef int ncclResult_t;
constexpr ncclResult_t ncclSuccess = 0;
constexpr int ncclDouble = 8, ncclSum = 0;

struct Rccl {
    void *lib = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Reduce)(const void *, void *, size_t, int, int, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    bool load()
    {
        if (lib) return true;
        for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (lib) break;
        }
        if (!lib) return false;
        CommInitAll = (decltype(CommInitAll))dlsym(lib, "ncclCommInitAll");
        CommDestroy = (decltype(CommDestroy))dlsym(lib, "ncclCommDestroy");
        AllReduce = (decltype(AllReduce))dlsym(lib, "ncclAllReduce");
        Reduce = (decltype(Reduce))dlsym(lib, "ncclReduce");
        GroupStart = (decltype(GroupStart))dlsym(lib, "ncclGroupStart");
        GroupEnd = (decltype(GroupEnd))dlsym(lib, "ncclGroupEnd");
        GetErrorString = (decltype(GetErrorString))dlsym(lib, "ncclGetErrorString");
        return CommInitAll && CommDestroy && AllReduce && Reduce && GroupStart && GroupEnd && GetErrorString;
    }
};

// One device's share.  Its members go in reverse order of declaration -- workspaces, stream, the part plan, the
// all-angle plan, then the grid the plans borrow -- after the destructor made the device current and gave back the
// communicator.
struct Member {
    int device = 0;
    GridPtr grid;
    PlanPtr plan_all;                      // every angle (lambda mode)
    PlanPtr plan_part;                     // this device's angles (angle mode), built on first use
    std::vector<int> my_angles;
    Stream stream;
    DevWork<double> dS, dA, dU, dD, dJ, dV;
    ncclComm_t comm = nullptr;             // RCCL rank of this device (NULL: the same-device rehearsal, or one device)
    ncclResult_t (*comm_destroy)(ncclComm_t) = nullptr;
    int rc = VRT_OK;
    std::string err;
    ~Member()
    {
        if (!grid && !stream) return;      // never got a device (creation failed there)
        (void)hipSetDevice(device);
        if (comm && comm_destroy) (void)comm_destroy(comm);
    }
};

}  // namespace

struct vrt_multi {
    std::vector<Member> m;
    int64_t n = 0, n_angles = 0;
    int n_sweeps = 3;
    std::vector<double> k;
    std::vector<int> dirs;
    bool distinct = true;                   // all devices different: RCCL; otherwise the same-device rehearsal
    Rccl rccl;
    bool uses_rccl() const { return !m.empty() && m[0].comm; }
    int shard = 0;                          // 0 auto, 1 lambda, 2 angle
    int last_shard = 0;
    std::mutex mu;
};

struct MultiDelete { void operator()(vrt_multi *mm) const { vrt_multi_destroy(mm); } };

// contiguous block partition: the first n_units % world ranks get one extra unit (distributed.partition)
static void block_of(int64_t n_units, int world, int rank, int64_t &start, int64_t &stop)
{
    const int64_t base = n_units / world, extra = n_units % world;
    start = rank * base + std::min<int64_t>(rank, extra);
    stop = start + base + (rank < extra ? 1 : 0);
}

extern "C" {

int vrt_multi_create(int n_devices, const int *devices, int64_t n, const double *pos_zxy, const int64_t *nbr, int64_t D1,
                     const double bounds[6], int64_t n_angles, const double *k, const int *dirs, int n_sweeps,
                     vrt_multi **out)
{
    if (!out) return fail(VRT_EINVAL, "out is NULL");
    *out = nullptr;
    if (!devices || !pos_zxy || !nbr || !bounds || !k) return fail(VRT_EINVAL, "NULL argument");
    if (n_devices < 1 || n_devices > 64) return fail(VRT_EINVAL, "need 1 <= n_devices <= 64");
    if (n_angles < 1) return fail(VRT_EINVAL, "n_angles must be >= 1");
    return guarded([&] {
        std::unique_ptr<vrt_multi, MultiDelete> mm(new vrt_multi());
        mm->n = n;
        mm->n_angles = n_angles;
        mm->n_sweeps = n_sweeps;
        mm->k.assign(k, k + 3 * n_angles);
        mm->dirs.resize((size_t)n_angles);
        for (int64_t a = 0; a < n_angles; a++)
            mm->dirs[(size_t)a] = dirs ? (dirs[a] > 0 ? 1 : (dirs[a] < 0 ? -1 : 0))
                                       : (std::fabs(k[3 * a]) < 1e-12 ? 0 : (k[3 * a] < 0 ? 1 : -1));
        mm->m = std::vector<Member>((size_t)n_devices);
        for (int d = 0; d < n_devices; d++) {
            mm->m[(size_t)d].device = devices[d];
            for (int e = 0; e < d; e++)
                if (devices[e] == devices[d]) mm->distinct = false;
        }
        // one grid + all-angle plan per device, built concurrently (plan creation is host-side schedule work)
        if (!run_workers(n_devices, [&](int d) {
                Member &me = mm->m[(size_t)d];
                vrt_grid *grid = nullptr;
                vrt_plan *plan = nullptr;
                me.rc = vrt_grid_create(n, pos_zxy, nbr, D1, bounds, me.device, &grid);
                me.grid.reset(grid);
                if (!me.rc) me.rc = vrt_plan_create_ex(grid, n_angles, k, mm->dirs.data(), n_sweeps, &plan);
                me.plan_all.reset(plan);
                if (!me.rc && (hipSetDevice(me.device) != hipSuccess || me.stream.create()))
                    me.rc = fail(VRT_ENODEVICE, "cannot create a stream");
                if (me.rc) me.err = vrt_last_error();
            }))
            return fail(VRT_ENOMEM, "out of host memory while creating the per-device plans");
        for (const Member &me : mm->m)
            if (me.rc) return fail(me.rc, "device " + std::to_string(me.device) + ": " + me.err);
        // angles of the "angle" mode: ups and downs dealt round-robin separately (distributed.angle_assignment)
        {
            int ju = 0, jd = 0;
            for (int64_t a = 0; a < n_angles; a++) {
                if (mm->dirs[(size_t)a] > 0) mm->m[(size_t)(ju++ % n_devices)].my_angles.push_back((int)a);
                else if (mm->dirs[(size_t)a] < 0) mm->m[(size_t)((n_devices - 1 - (jd++ % n_devices)))].my_angles.push_back((int)a);
            }
            for (Member &me : mm->m) std::sort(me.my_angles.begin(), me.my_angles.end());
        }
        // VRT_MULTI_FORCE_RCCL=1: a communicator also for ONE device (a one-rank ncclCommInitAll), so that the RCCL legs of this
        // file -- ncclReduce of the angle shards, ncclAllReduce of the rate-integral shares, the group calls -- execute on a
        // one-GPU box too (tests/test_physics.py); read here, once per object
        const char *force = std::getenv("VRT_MULTI_FORCE_RCCL");
        const bool force_rccl = force && force[0] == '1';
        if (mm->distinct && (n_devices > 1 || force_rccl)) {
            if (!mm->rccl.load()) return fail(VRT_ENODEVICE, "cannot load librccl.so (needed for more than one device)");
            std::vector<ncclComm_t> comms((size_t)n_devices, nullptr);
            const ncclResult_t r = mm->rccl.CommInitAll(comms.data(), n_devices, devices);
            if (r != ncclSuccess) return fail(VRT_ENODEVICE, std::string("ncclCommInitAll: ") + mm->rccl.GetErrorString(r));
            for (int d = 0; d < n_devices; d++) {
                mm->m[(size_t)d].comm = comms[(size_t)d];
                mm->m[(size_t)d].comm_destroy = mm->rccl.CommDestroy;
            }
        }
        *out = mm.release();
        return VRT_OK;
    });
}

int vrt_multi_set_shard(vrt_multi *mm, const char *mode)
{
    if (!mm || !mode) return fail(VRT_EINVAL, "NULL argument");
    return guarded([&] {
        const std::string s(mode);
        std::lock_guard<std::mutex> lock(mm->mu);
        if (s == "auto") mm->shard = 0;
        else if (s == "lambda") mm->shard = 1;
        else if (s == "angle") mm->shard = 2;
        else return fail(VRT_EINVAL, "shard must be auto, lambda or angle");
        return VRT_OK;
    });
}

int vrt_multi_last_shard(const vrt_multi *mm) { return mm ? mm->last_shard : 0; }
int vrt_multi_uses_rccl(const vrt_multi *mm) { return mm && mm->uses_rccl() ? 1 : 0; }

int vrt_multi_execute(vrt_multi *mm, int64_t nlam, int64_t ld, const double *S, const double *alpha, int alpha_mode,
                      const double *I0_up, const double *I0_down, const double *weights, double *J)
{
    if (!mm || !S || !alpha || !weights || !J) return fail(VRT_EINVAL, "NULL argument");
    if (nlam < 1 || ld < nlam) return fail(VRT_EINVAL, "need nlam >= 1 and ld >= nlam");
    if (alpha_mode < 0 || alpha_mode > 2) return fail(VRT_EINVAL, "bad alpha_mode (host arrays: 0, 1 or 2)");
    return guarded([&] {
        std::lock_guard<std::mutex> lock(mm->mu);
        const int W = (int)mm->m.size();
        const int64_t n = mm->n, A = mm->n_angles;
        int shard = mm->shard;
        if (shard == 0) shard = nlam >= W ? 1 : 2;
        if (shard == 2 && W > A) return fail(VRT_EINVAL, "more devices than angles");
        mm->last_shard = shard;
        const int64_t n1u = mm->m[0].grid->up.n1, n1d = mm->m[0].grid->down.n1;
        // angle mode: the devices' partial plans
        if (shard == 2)
            for (Member &me : mm->m)
                if (!me.plan_part && !me.my_angles.empty()) {
                    std::vector<double> kk;
                    std::vector<int> dd;
                    for (int a : me.my_angles) {
                        kk.insert(kk.end(), mm->k.begin() + 3 * a, mm->k.begin() + 3 * a + 3);
                        dd.push_back(mm->dirs[(size_t)a]);
                    }
                    vrt_plan *part = nullptr;
                    int rc = vrt_plan_create_ex(me.grid.get(), (int64_t)me.my_angles.size(), kk.data(), dd.data(), mm->n_sweeps, &part);
                    me.plan_part.reset(part);
                    if (rc) return rc;
                }
        auto work = [&](int d) {
            Member &me = mm->m[(size_t)d];
            me.rc = VRT_OK;
            auto chk = [&](hipError_t e, const char *what) {
                if (e != hipSuccess && !me.rc) {
                    me.rc = VRT_ENODEVICE;
                    me.err = std::string(what) + ": " + hipGetErrorString(e);
                }
            };
            chk(hipSetDevice(me.device), "hipSetDevice");
            if (me.rc) return;
            hipStream_t st = me.stream;
            int64_t l0 = 0, l1 = nlam;
            if (shard == 1) block_of(nlam, W, d, l0, l1);
            const int64_t nb = l1 - l0;
            const size_t w8 = sizeof(double);
            if (nb <= 0 || (shard == 2 && me.my_angles.empty())) {       // nothing to do here: contributes zeros in angle mode
                if (shard == 2) {
                    if ((me.rc = me.dJ.grow((size_t)n * (size_t)nlam))) { me.err = vrt_last_error(); return; }
                    chk(hipMemsetAsync(me.dJ, 0, w8 * (size_t)n * (size_t)nlam, st), "hipMemsetAsync");
                    chk(hipStreamSynchronize(st), "hipStreamSynchronize");      // another member's stream reads these zeros
                }
                return;
            }
            vrt_plan *plan = shard == 1 ? me.plan_all.get() : me.plan_part.get();
            const int64_t nA = shard == 1 ? A : (int64_t)me.my_angles.size();
            // S block (nb, n) dense on the device
            if ((me.rc = me.dS.grow((size_t)n * (size_t)nb)) || (me.rc = me.dJ.grow((size_t)n * (size_t)nb))) {
                me.err = vrt_last_error();
                return;
            }
            chk(hipMemcpy2DAsync(me.dS, w8 * (size_t)nb, S + l0, w8 * (size_t)ld, w8 * (size_t)nb, (size_t)n, hipMemcpyHostToDevice, st), "upload S");
            // alpha
            const double *dA = nullptr;
            if (alpha_mode == VRT_ALPHA_SITE) {
                if ((me.rc = me.dA.grow((size_t)n))) { me.err = vrt_last_error(); return; }
                chk(hipMemcpyAsync(me.dA, alpha, w8 * (size_t)n, hipMemcpyHostToDevice, st), "upload alpha");
            } else if (alpha_mode == VRT_ALPHA_SITE_LAM) {
                if ((me.rc = me.dA.grow((size_t)n * (size_t)nb))) { me.err = vrt_last_error(); return; }
                chk(hipMemcpy2DAsync(me.dA, w8 * (size_t)nb, alpha + l0, w8 * (size_t)ld, w8 * (size_t)nb, (size_t)n, hipMemcpyHostToDevice, st), "upload alpha");
            } else {
                if ((me.rc = me.dA.grow((size_t)nA * (size_t)n * (size_t)nb))) { me.err = vrt_last_error(); return; }
                for (int64_t j = 0; j < nA; j++) {
                    const int64_t a = shard == 1 ? j : me.my_angles[(size_t)j];
                    chk(hipMemcpy2DAsync(me.dA + (size_t)j * (size_t)n * (size_t)nb, w8 * (size_t)nb,
                                         alpha + (size_t)a * (size_t)n * (size_t)ld + l0, w8 * (size_t)ld, w8 * (size_t)nb, (size_t)n,
                                         hipMemcpyHostToDevice, st), "upload alpha");
                }
            }
            dA = me.dA;
            double *dU = nullptr, *dD = nullptr;
            if (I0_up && n1u) {
                if ((me.rc = me.dU.grow((size_t)n1u * (size_t)nb))) { me.err = vrt_last_error(); return; }
                chk(hipMemcpy2DAsync(me.dU, w8 * (size_t)nb, I0_up + l0, w8 * (size_t)nlam, w8 * (size_t)nb, (size_t)n1u, hipMemcpyHostToDevice, st), "upload I0");
                dU = me.dU;
            }
            if (I0_down && n1d) {
                if ((me.rc = me.dD.grow((size_t)n1d * (size_t)nb))) { me.err = vrt_last_error(); return; }
                chk(hipMemcpy2DAsync(me.dD, w8 * (size_t)nb, I0_down + l0, w8 * (size_t)nlam, w8 * (size_t)nb, (size_t)n1d, hipMemcpyHostToDevice, st), "upload I0");
                dD = me.dD;
            }
            if (me.rc) return;
            std::vector<double> wv;
            if (shard == 1) wv.assign(weights, weights + A);
            else
                for (int a : me.my_angles) wv.push_back(weights[a]);
            me.rc = vrt_plan_execute_dev(plan, nb, nb, me.dS, dA, alpha_mode, dU, dD, wv.data(), me.dJ, nullptr, st);
            if (me.rc) { me.err = vrt_last_error(); return; }
            if (shard == 1)     // the device owns rows l0..l1 of J: straight home
                chk(hipMemcpy2DAsync(J + l0, w8 * (size_t)ld, me.dJ, w8 * (size_t)nb, w8 * (size_t)nb, (size_t)n, hipMemcpyDeviceToHost, st), "download J");
            chk(hipStreamSynchronize(st), "hipStreamSynchronize");
            // (a chained sweep that gave up waiting: reported by THIS call, whose J it spoiled)
            if (!me.rc && (me.rc = patch_chain_check(plan))) me.err = vrt_last_error();
        };
        if (!run_workers(W, work)) return fail(VRT_ENOMEM, "out of host memory in a device worker");
        for (const Member &me : mm->m)
            if (me.rc) return fail(me.rc, "device " + std::to_string(me.device) + ": " + me.err);
        if (shard == 2) {
            // J = Σ over the devices' partial sums, wanted on ONE device only (the host array is filled from device 0):
            // one RCCL reduce to rank 0 over xGMI -- half the bytes of an all-reduce -- or, on a shared device, adds
            const size_t cnt = (size_t)n * (size_t)nlam;
            if (mm->uses_rccl()) {
                // (nothing may return between GroupStart and GroupEnd: an open group poisons every later call)
                ncclResult_t r = mm->rccl.GroupStart();
                hipError_t he = hipSuccess;
                for (int d = 0; d < W && r == ncclSuccess && he == hipSuccess; d++) {
                    Member &me = mm->m[(size_t)d];
                    he = hipSetDevice(me.device);
                    if (he == hipSuccess)
                        r = mm->rccl.Reduce(me.dJ, me.dJ, cnt, ncclDouble, ncclSum, 0, mm->m[(size_t)d].comm, me.stream);
                }
                const ncclResult_t r2 = mm->rccl.GroupEnd();
                if (he != hipSuccess) return fail(VRT_ENODEVICE, std::string("hipSetDevice: ") + hipGetErrorString(he));
                if (r != ncclSuccess || r2 != ncclSuccess)
                    return fail(VRT_ENODEVICE, std::string("ncclReduce: ") + mm->rccl.GetErrorString(r != ncclSuccess ? r : r2));
                for (Member &me : mm->m) {
                    VRT_HIP_TRY(hipSetDevice(me.device));
                    VRT_HIP_TRY(hipStreamSynchronize(me.stream));
                }
            } else {
                Member &m0 = mm->m[0];
                VRT_HIP_TRY(hipSetDevice(m0.device));
                (void)hipGetLastError();
                for (int d = 1; d < W; d++)
                    if (int rc = launch_axpy(cnt, mm->m[(size_t)d].dJ, m0.dJ, m0.stream)) return rc;     // same device: plain adds
            }
            Member &m0 = mm->m[0];
            VRT_HIP_TRY(hipSetDevice(m0.device));
            VRT_HIP_TRY(hipMemcpy2DAsync(J, sizeof(double) * (size_t)ld, m0.dJ, sizeof(double) * (size_t)nlam,
                                         sizeof(double) * (size_t)nlam, (size_t)n, hipMemcpyDeviceToHost, m0.stream));
            VRT_HIP_TRY(hipStreamSynchronize(m0.stream));
        }
        return VRT_OK;
    });
}

// ---- the line case across several devices ---------------------------------------------------------------------------
// vrt_multi_execute_line: J_λ_voronoi of the line case (src/lambda_iteration.jl:72-111) from host arrays, the wavelengths
// in contiguous blocks over the devices: every device makes the per-angle α_tot of ITS wavelengths itself
// (vrt_line_opacity's kernel), so the (nλ, n, n_angles) array neither exists on the host nor crosses PCIe, and owns
// whole rows J[l, :] -- no exchange.
int vrt_multi_execute_line(vrt_multi *mm, int64_t nlam, int64_t ld, const double *lambda, double lambda0, double c0,
                           const double *velocity, const double *doppler_width, const double *gamma,
                           const double *line_strength, const double *alpha_cont, const double *S, const double *I0_up,
                           const double *I0_down, const double *weights, double *J)
{
    if (!mm || !lambda || !velocity || !doppler_width || !gamma || !line_strength || !alpha_cont || !S || !weights || !J)
        return fail(VRT_EINVAL, "NULL argument");
    if (nlam < 1 || ld < nlam) return fail(VRT_EINVAL, "need nlam >= 1 and ld >= nlam");
    if (!(lambda0 > 0) || !(c0 > 0)) return fail(VRT_EINVAL, "lambda0 and c0 must be positive");
    return guarded([&] {
        std::lock_guard<std::mutex> lock(mm->mu);
        const int W = (int)mm->m.size();
        const int64_t n = mm->n;
        const int64_t n1u = mm->m[0].grid->up.n1, n1d = mm->m[0].grid->down.n1;
        mm->last_shard = 1;
        auto work = [&](int d) {
            Member &me = mm->m[(size_t)d];
            me.rc = VRT_OK;
            auto chk = [&](hipError_t e, const char *what) {
                if (e != hipSuccess && !me.rc) {
                    me.rc = VRT_ENODEVICE;
                    me.err = std::string(what) + ": " + hipGetErrorString(e);
                }
            };
            int64_t l0, l1;
            block_of(nlam, W, d, l0, l1);
            const int64_t nb = l1 - l0;
            if (nb <= 0) return;
            chk(hipSetDevice(me.device), "hipSetDevice");
            if (me.rc) return;
            hipStream_t st = me.stream;
            vrt_plan *plan = me.plan_all.get();
            std::lock_guard<std::mutex> plock(plan->mu);
            const size_t w8 = sizeof(double), sn = (size_t)n;
            const size_t nnat = (size_t)vrt_plan_native_alpha_count(plan, nb);
            // S | seven per-site vectors + the block's wavelengths | native alpha | J
            if ((me.rc = me.dS.grow(sn * (size_t)nb)) || (me.rc = me.dJ.grow(sn * (size_t)nb)) ||
                (me.rc = me.dA.grow(nnat)) || (me.rc = me.dV.grow(7 * sn + (size_t)nb))) {
                me.err = vrt_last_error();
                return;
            }
            double *d_vel = me.dV, *d_dop = me.dV + 3 * sn, *d_gam = me.dV + 4 * sn, *d_str = me.dV + 5 * sn, *d_ac = me.dV + 6 * sn,
                   *d_lam = me.dV + 7 * sn;
            chk(hipMemcpy2DAsync(me.dS, w8 * (size_t)nb, S + l0, w8 * (size_t)ld, w8 * (size_t)nb, sn, hipMemcpyHostToDevice, st), "upload S");
            chk(hipMemcpyAsync(d_vel, velocity, w8 * 3 * sn, hipMemcpyHostToDevice, st), "upload velocity");
            chk(hipMemcpyAsync(d_dop, doppler_width, w8 * sn, hipMemcpyHostToDevice, st), "upload doppler");
            chk(hipMemcpyAsync(d_gam, gamma, w8 * sn, hipMemcpyHostToDevice, st), "upload gamma");
            chk(hipMemcpyAsync(d_str, line_strength, w8 * sn, hipMemcpyHostToDevice, st), "upload strength");
            chk(hipMemcpyAsync(d_ac, alpha_cont, w8 * sn, hipMemcpyHostToDevice, st), "upload alpha_cont");
            chk(hipMemcpyAsync(d_lam, lambda + l0, w8 * (size_t)nb, hipMemcpyHostToDevice, st), "upload lambda");
            double *dU = nullptr, *dD = nullptr;
            if (I0_up && n1u) {
                if ((me.rc = me.dU.grow((size_t)n1u * (size_t)nb))) { me.err = vrt_last_error(); return; }
                chk(hipMemcpy2DAsync(me.dU, w8 * (size_t)nb, I0_up + l0, w8 * (size_t)nlam, w8 * (size_t)nb, (size_t)n1u, hipMemcpyHostToDevice, st), "upload I0");
                dU = me.dU;
            }
            if (I0_down && n1d) {
                if ((me.rc = me.dD.grow((size_t)n1d * (size_t)nb))) { me.err = vrt_last_error(); return; }
                chk(hipMemcpy2DAsync(me.dD, w8 * (size_t)nb, I0_down + l0, w8 * (size_t)nlam, w8 * (size_t)nb, (size_t)n1d, hipMemcpyHostToDevice, st), "upload I0");
                dD = me.dD;
            }
            if (me.rc) return;
            if ((me.rc = launch_line_opacity(plan, nb, d_lam, lambda0, c0, d_vel, d_dop, d_gam, d_str, d_ac, me.dA, st)) ||
                (me.rc = execute_locked(plan, caller_args(nb, nb, me.dS, me.dA, VRT_ALPHA_ANGLE_NATIVE, dU, dD, weights, me.dJ, nullptr, st, false)))) {
                me.err = vrt_last_error();
                return;
            }
            chk(hipMemcpy2DAsync(J + l0, w8 * (size_t)ld, me.dJ, w8 * (size_t)nb, w8 * (size_t)nb, sn, hipMemcpyDeviceToHost, st), "download J");
            chk(hipStreamSynchronize(st), "hipStreamSynchronize");
            if (!me.rc && (me.rc = patch_chain_check(plan))) me.err = vrt_last_error();
        };
        if (!run_workers(W, work)) return fail(VRT_ENOMEM, "out of host memory in a device worker");
        for (const Member &me : mm->m)
            if (me.rc) return fail(me.rc, "device " + std::to_string(me.device) + ": " + me.err);
        return VRT_OK;
    });
}

}  // extern "C"

// ---- Λ-iteration session across several devices (BASELINE configs[3]; src/lambda_iteration.jl:205-300) ---------------
// Every device owns a contiguous block of the wavelengths (91 over 8 -> 12,12,12,11,11,11,11,11) and the whole per-site
// state.  Per iteration it runs, for ITS wavelengths: the line terms of the current populations, α_tot of every
// angle, the sweep, S_new with its share of the convergence maximum, and its share of the six λ-integrals of the
// radiative rates (rates.jl:154-201).  The shares are summed by ONE all-reduce of 6 n doubles over xGMI (SURVEY 8e:
// "only R and one scalar are reduced"); J never travels.  Every device then solves the statistical equilibrium of
// every site itself (populations.jl:191-221), so the next iteration's opacity needs no further exchange.  A member's S and
// J live in a SourceStore (vrt_source_store.h), in rows or in sweep order, all members alike.  Float storage
// (vrt_multi_lambda_create_f32): every member's store is kPlanesF32 and f_B0, f_I0 and f_native replace d_B0, d_I0 and
// d_native -- no member holds a double array of size nλ_block·n or nλ_block·n·angles; the shares, the all-reduce and the
// statistical equilibrium are the same doubles.
struct LambdaMember {
    int device = 0;
    int64_t l0 = 0, l1 = 0;
    LineCaseDev line;                   // the whole case (every site, ALL wavelengths), γ, the line strength and R (vrt_line_case.h)
    DevBuf<double> d_B0, d_I0, d_native;   // this block's columns (B_0 in the store's order: rows, or its up-order plane set)
    DevBuf<float> f_B0, f_I0, f_native;    // float storage: B_0 rounded once in the up order, I_0, the native α
    DevBuf<double> d_pops, d_shares;
    DevBuf<unsigned long long> d_scalars;
    Event ev;
    SourceStore sj;                     // the block's S and J, as the one-device session keeps them (a member without
                                        // wavelengths: never created, holds nothing)
    NgState ng;                         // this block's history and workspace (vrt_multi_lambda_set_acceleration; off: nothing)
    ~LambdaMember() { (void)hipSetDevice(device); }    // (its own copy: the vrt_multi may be gone already); then the members go
};

struct vrt_multi_lambda {
    vrt_multi *mm = nullptr;            // borrowed
    int64_t n = 0, nlam = 0;
    std::vector<double> weights;
    std::vector<LambdaMember> lm;
    bool f32 = false;                   // float storage, every member (a member without wavelengths has no store to ask)
    int iterations = 0;
    NgState ng;                         // the settings and the last report; the buffers are the members'
    bool ng_torn = false;               // an accepted step whose down-order copy could not be rewritten: S is inconsistent
};

namespace {

// columns [l0, l1) of a host array (rows, nlam) into a dense device block (rows, l1 - l0)
int dupload_cols(DevBuf<double> &d, const double *h, size_t rows, int64_t nlam, int64_t l0, int64_t l1, hipStream_t st)
{
    const size_t nb = (size_t)(l1 - l0);
    int rc = d.alloc(rows * nb);
    if (rc || nb == 0) return rc;
    VRT_HIP_TRY(hipMemcpy2DAsync(d, sizeof(double) * nb, h + l0, sizeof(double) * (size_t)nlam, sizeof(double) * nb, rows, hipMemcpyHostToDevice, st));
    return VRT_OK;
}

// ---- Ng acceleration of the session (vrt_multi_lambda_set_acceleration): the phases of vrt_internal.h, each over every
// member that holds wavelengths, on the S of its store.

// body(d, member, its share of the session) -> rc on every member with wavelengths, one host thread each, the member's
// device current and its plan locked
template <typename Body>
int ng_on_members(vrt_multi_lambda *s, Body body)
{
    vrt_multi *mm = s->mm;
    auto work = [&](int d) {
        Member &me = mm->m[(size_t)d];
        LambdaMember &l = s->lm[(size_t)d];
        me.rc = VRT_OK;
        if (l.l1 <= l.l0) return;
        if (hipSetDevice(me.device) != hipSuccess) { me.rc = VRT_ENODEVICE; me.err = "hipSetDevice"; return; }
        std::lock_guard<std::mutex> plock(me.plan_all->mu);
        if ((me.rc = body(d, me, l))) me.err = vrt_last_error();
    };
    if (!run_workers((int)mm->m.size(), work)) return fail(VRT_ENOMEM, "out of host memory in a device worker");
    for (const Member &me : mm->m)
        if (me.rc) return fail(me.rc, "device " + std::to_string(me.device) + ": " + me.err);
    return VRT_OK;
}

// After the plain update of iterate s->iterations (every stream is synchronised, mm->mu is held).  A due step: every member's
// five sums, added on the host in member order; ONE (a, b); x_acc of every member into its oldest history buffer; and only
// with every verdict in and good do the buffers become the members' S.
int multi_ng_after_iterate(vrt_multi_lambda *s)
{
    const int W = (int)s->lm.size();
    s->ng.last_applied = 0;
    const int due = ng_due(s->ng, s->iterations);
    if (due == kNgNothing) return VRT_OK;
    if (due != kNgStep)
        return ng_on_members(s, [&](int, Member &me, LambdaMember &l) {
            int rc = ng_record(l.ng, due, l.sj.ng_S(), l.sj.ng_count(), me.stream);
            if (!rc && hipStreamSynchronize(me.stream) != hipSuccess) rc = fail(VRT_ENODEVICE, "copying S into the history failed");
            return rc;
        });
    bool complete = true;
    for (LambdaMember &l : s->lm)
        if (l.l1 > l.l0 && !ng_take_history(l.ng)) complete = false;
    if (!complete) return VRT_OK;               // switched on too late for this one, or the state was replaced: nothing due
    std::vector<double> part(5 * (size_t)W, 0.0);
    int rc = ng_on_members(s, [&](int d, Member &me, LambdaMember &l) {
        return ng_sums(l.sj.ng_range(), l.sj.ng_S(), l.ng.hist[0], l.ng.hist[1], l.ng.hist[2],
                       l.ng.d_ws, &part[5 * (size_t)d], me.stream);
    });
    if (rc) return rc;
    // ((s_0 + s_1) + s_2) + ... over the members that hold wavelengths: never the order in which the workers finished
    std::vector<NgPiece> pieces;
    std::vector<int> piece_of((size_t)W, -1);
    for (int d = 0; d < W; d++) {
        LambdaMember &l = s->lm[(size_t)d];
        if (l.l1 <= l.l0) continue;
        ng_add_sums(s->ng.last_sums, &part[5 * (size_t)d], pieces.empty());
        piece_of[(size_t)d] = (int)pieces.size();
        pieces.push_back(NgPiece{&l.ng, &l.sj.ng_S(), false});
    }
    s->ng.last_applied = -1;
    const bool valid = ng_coefficients(s->ng.last_sums, s->ng.last_coeffs);
    if (valid) {
        const double a = s->ng.last_coeffs[0], b = s->ng.last_coeffs[1];
        rc = ng_on_members(s, [&](int d, Member &me, LambdaMember &l) {
            return ng_apply(l.sj.ng_range(), a, b, l.sj.ng_S(), l.ng.hist[0], l.ng.hist[1], l.ng.hist[2],
                            l.ng.d_ws, &pieces[(size_t)piece_of[(size_t)d]].good, me.stream);
        });
        if (rc) return rc;
    }
    if (!ng_commit(pieces.data(), (int)pieces.size(), valid)) return VRT_OK;
    if (s->lm[0].sj.two_orders()) {             // (every member with wavelengths keeps the form of the first)
        // the down-order copies from the new up-order ones, value for value
        rc = ng_on_members(s, [&](int, Member &me, LambdaMember &l) {
            int r = l.sj.mirror_down(me.stream);
            if (!r && hipStreamSynchronize(me.stream) != hipSuccess) r = fail(VRT_ENODEVICE, "rewriting the down-order S failed");
            return r;
        });
        if (rc) {                               // the up-order copies are x_acc, a down-order copy is not: no further iterate
            s->ng_torn = true;
            return rc;
        }
    }
    s->ng.last_applied = 1;
    return VRT_OK;
}

}  // namespace

extern "C" {

static int multi_lambda_create(vrt_multi *mm, const vrt_line_case *lc, const double *weights, vrt_multi_lambda **out, bool f32)
{
    if (!out) return fail(VRT_EINVAL, "out is NULL");
    *out = nullptr;
    if (!mm || !lc || !weights) return fail(VRT_EINVAL, "NULL argument");
    if (int rc = check_line_case(lc)) return rc;
    const int64_t nlam = lc->nlam;
    return guarded([&] {
        std::lock_guard<std::mutex> lock(mm->mu);
        const int W = (int)mm->m.size();
        for (const Member &me : mm->m) {
            const vrt_plan *p = me.plan_all.get();
            if (int rc = line_path_ok(p, "the line session")) return rc;
            if (p->A != (int)p->n_angles_user)
                return fail(VRT_EINVAL, "per-angle alpha needs every angle active (no θ = 90 direction)");
            if (f32) {                                  // float planes exist on the patch path only: no fp64 fallback
                if (int rc = native_planes_ok(p, true)) return rc;
                if (p->tune.lambda_native == 0 || (p->tune.path != 0 && p->tune.path != 4))
                    return fail(VRT_EINVAL, "the float-storage line session keeps S and J in the patch path's sweep order: not with VRT_LAMBDA_NATIVE=0 or a VRT_PATH other than patches");
            }
        }
        std::unique_ptr<vrt_multi_lambda> s(new vrt_multi_lambda());
        s->mm = mm;
        s->f32 = f32;
        s->n = mm->n;
        s->nlam = nlam;
        s->weights.assign(weights, weights + mm->n_angles);
        s->lm = std::vector<LambdaMember>((size_t)W);
        // every member keeps its block in sweep order, or none does (VRT_LAMBDA_NATIVE, all plans fit)
        SourceStore::Form form = f32 ? SourceStore::kPlanesF32 : SourceStore::kPlanes;
        for (const Member &me : mm->m)
            if (!f32 && !SourceStore::plan_keeps_planes(me.plan_all.get())) form = SourceStore::kRows;
        const size_t n = (size_t)mm->n;
        std::vector<int> rcs((size_t)W, VRT_OK);
        std::vector<std::string> errs((size_t)W);
        auto work = [&](int d) {
            Member &me = mm->m[(size_t)d];
            LambdaMember &l = s->lm[(size_t)d];
            l.device = me.device;
            block_of(nlam, W, d, l.l0, l.l1);
            const size_t nb = (size_t)(l.l1 - l.l0);
            int rc = VRT_OK;
            if (hipSetDevice(me.device) != hipSuccess) { rcs[(size_t)d] = VRT_ENODEVICE; errs[(size_t)d] = "hipSetDevice"; return; }
            hipStream_t st = me.stream;
            vrt_grid *g = me.grid.get();
#define VRT_S(expr) do { if (!rc) rc = (expr); } while (0)
            VRT_S(l.line.create(lc, mm->n, st));
            VRT_S(upload(l.d_pops, lc->lte_populations, 3 * n, st));               // populations = copy(LTE_pops), :232
            VRT_S(dupload_cols(l.d_B0, lc->B0, n, nlam, l.l0, l.l1, st));
            if (nb) VRT_S(l.sj.create(me.plan_all.get(), (int64_t)nb, form, l.d_B0, st));      // S_new = B_0, S_old = zero(S_new), :236-240
            VRT_S(l.d_shares.alloc(6 * n));
            VRT_S(l.d_scalars.alloc(2));
            VRT_S(l.ev.create(hipEventDisableTiming));
            // I_0 = B_λ of the bottom layer (:99-101) and α_tot of every angle in the sweep's storage type; B_0 into the store's order
            const size_t nnat = nb ? (size_t)vrt_plan_native_alpha_count(me.plan_all.get(), (int64_t)nb) : 1;
            if (f32) {
                VRT_S(l.f_I0.alloc((size_t)g->up.n1 * nb));
                VRT_S(l.f_native.alloc(nnat));
                if (nb) {
                    VRT_S(launch_gather_rows_f32(g->up.n1, (int64_t)nb, (int64_t)nb, g->up.d_order, l.d_B0, l.f_I0, st));
                    VRT_S(l.sj.to_up_order(l.d_B0, l.f_B0, st));         // (rounded once; the staged doubles go)
                }
            } else {
                VRT_S(l.d_I0.alloc((size_t)g->up.n1 * nb));
                VRT_S(l.d_native.alloc(nnat));
                if (nb) {
                    VRT_S(launch_gather_rows(g->up.n1, (int64_t)nb, (int64_t)nb, g->up.d_order, l.d_B0, l.d_I0, st));
                    VRT_S(l.sj.to_up_order(l.d_B0, st));
                }
            }
#undef VRT_S
            if (!rc && hipStreamSynchronize(st) != hipSuccess) rc = fail(VRT_ENODEVICE, "uploading the line case failed");
            if (rc) { rcs[(size_t)d] = rc; errs[(size_t)d] = vrt_last_error(); }
        };
        const bool ok = run_workers(W, work);
        for (int d = 0; d < W; d++)
            if (!ok || rcs[(size_t)d]) {
                const int rc = ok ? rcs[(size_t)d] : VRT_ENOMEM;
                return fail(rc, ok ? "device " + std::to_string(mm->m[(size_t)d].device) + ": " + errs[(size_t)d] : "out of host memory");
            }
        *out = s.release();
        return VRT_OK;
    });
}

int vrt_multi_lambda_create(vrt_multi *mm, const vrt_line_case *lc, const double *weights, vrt_multi_lambda **out)
{
    return multi_lambda_create(mm, lc, weights, out, false);
}

int vrt_multi_lambda_create_f32(vrt_multi *mm, const vrt_line_case *lc, const double *weights, vrt_multi_lambda **out)
{
    return multi_lambda_create(mm, lc, weights, out, true);
}

int vrt_multi_lambda_storage(const vrt_multi_lambda *s)
{
    return !s ? fail(VRT_EINVAL, "NULL session") : s->f32 ? 4 : 8;
}

int vrt_multi_lambda_iterate(vrt_multi_lambda *s, double *max_rel_change)
{
    if (!s || !max_rel_change) return fail(VRT_EINVAL, "NULL argument");
    return guarded([&] {
        vrt_multi *mm = s->mm;
        std::lock_guard<std::mutex> lock(mm->mu);
        if (s->ng_torn)
            return fail(VRT_ENODEVICE, "an accepted Ng step failed while rewriting the down-order S: the session's S is inconsistent, "
                                       "replace it with vrt_multi_lambda_set_state or destroy the session");
        const int W = (int)mm->m.size();
        const int64_t n = s->n;
        // ---- every device: its wavelengths' share of the iteration, enqueued on its stream ----------------------------
        auto work = [&](int d) {
            Member &me = mm->m[(size_t)d];
            LambdaMember &l = s->lm[(size_t)d];
            me.rc = VRT_OK;
            const int64_t nb = l.l1 - l.l0;
            if (hipSetDevice(me.device) != hipSuccess) { me.rc = VRT_ENODEVICE; me.err = "hipSetDevice"; return; }
            hipStream_t st = me.stream;
            vrt_plan *p = me.plan_all.get();
            vrt_grid *g = me.grid.get();
            std::lock_guard<std::mutex> plock(p->mu);
            int rc = VRT_OK;
            SourceStore &sj = l.sj;
            if (nb == 0 && hipMemsetAsync(l.d_scalars, 0, 2 * sizeof(unsigned long long), st) != hipSuccess)
                rc = fail(VRT_ENODEVICE, "hipMemsetAsync");
            if (nb > 0 && sj.form() == SourceStore::kRows &&
                hipMemcpyAsync(sj.S_old(), sj.S_new(), sizeof(double) * (size_t)n * (size_t)nb, hipMemcpyDeviceToDevice, st) != hipSuccess)
                rc = fail(VRT_ENODEVICE, "hipMemcpyAsync");                                                      // S_old = copy(S_new), :258
            // γ and the line strength of the current populations (:72-75, line.jl:219-225), α_tot of every angle (:89-96)
            if (!rc) rc = l.line.terms(l.d_pops, st);
            if (!rc && nb > 0) {
                void *alpha = s->f32 ? (void *)l.f_native.get() : (void *)l.d_native.get();
                const void *I0 = s->f32 ? (const void *)l.f_I0.get() : (const void *)l.d_I0.get();
                rc = l.line.opacity(p, nb, l.l0, alpha, st, s->f32);
                // J_λ of this block (:84-111)
                if (!rc) rc = execute_locked(p, sj.exec_args(alpha, VRT_ALPHA_ANGLE_NATIVE, I0, s->weights.data(), st));
                // S_new = (1 - ε) J + ε B_0 and this block's share of the criterion (:261-263, :325-349); in sweep order the
                // update reads the old S where it writes the new
                if (!rc && sj.form() == SourceStore::kPlanesF32)      // (the roundings: include/voronoirt.h)
                    rc = launch_lambda_update_native_f32(p, nb, sj.J_plane<float>(0), sj.J_plane<float>(1), l.f_B0, l.line.d_eps,
                                                         sj.S_plane<float>(0), sj.S_plane<float>(1), l.d_scalars, st);
                else if (!rc && sj.form() == SourceStore::kPlanes)
                    rc = launch_lambda_update_native(g, nb, sj.J_plane(0), sj.J_plane(1), l.d_B0, l.line.d_eps, sj.S_plane(0), sj.S_plane(1), l.d_scalars, st);
                else if (!rc)
                    rc = launch_lambda_update(n, nb, nb, sj.J_rows(), l.d_B0, l.line.d_eps, sj.S_old(), sj.S_new(), l.d_scalars, st);
            }
            // this block's share of the six rate integrals (rates.jl:154-201), from J in rows or in its planes
            // (a member without wavelengths: an empty range of rows)
            const RatesJ J = sj.form() == SourceStore::kPlanesF32 ? RatesJ::from_planes_f32(p, sj.J_plane<float>(0), sj.J_plane<float>(1))
                             : sj.form() == SourceStore::kPlanes ? RatesJ::from_planes(g, sj.J_plane(0), sj.J_plane(1))
                                                                 : RatesJ::from_rows(sj.J_rows(), std::max<int64_t>(nb, 1));
            if (!rc) rc = launch_rates_partial(l.line.rates_in(), J, l.l0, l.l1, l.d_shares, st);
            if (rc) { me.rc = rc; me.err = vrt_last_error(); }
        };
        if (!run_workers(W, work)) return fail(VRT_ENOMEM, "out of host memory in a device worker");
        for (const Member &me : mm->m)
            if (me.rc) return fail(me.rc, "device " + std::to_string(me.device) + ": " + me.err);
        // ---- the shares summed over the devices: ONE all-reduce of 6 n doubles (in place), stream-ordered ---------------
        const size_t cnt = 6 * (size_t)n;
        if (mm->uses_rccl()) {
            ncclResult_t r = mm->rccl.GroupStart();
            hipError_t he = hipSuccess;
            for (int d = 0; d < W && r == ncclSuccess && he == hipSuccess; d++) {
                he = hipSetDevice(mm->m[(size_t)d].device);
                if (he == hipSuccess)
                    r = mm->rccl.AllReduce(s->lm[(size_t)d].d_shares, s->lm[(size_t)d].d_shares, cnt, ncclDouble, ncclSum, mm->m[(size_t)d].comm, mm->m[(size_t)d].stream);
            }
            const ncclResult_t r2 = mm->rccl.GroupEnd();
            if (he != hipSuccess) return fail(VRT_ENODEVICE, std::string("hipSetDevice: ") + hipGetErrorString(he));
            if (r != ncclSuccess || r2 != ncclSuccess)
                return fail(VRT_ENODEVICE, std::string("ncclAllReduce: ") + mm->rccl.GetErrorString(r != ncclSuccess ? r : r2));
        } else if (W > 1) {
            // handles on ONE device (rehearsal): member 0 adds the others' shares behind their streams, the others copy the sum
            Member &m0 = mm->m[0];
            VRT_HIP_TRY(hipSetDevice(m0.device));
            for (int d = 1; d < W; d++) {
                VRT_HIP_TRY(hipEventRecord(s->lm[(size_t)d].ev, mm->m[(size_t)d].stream));
                VRT_HIP_TRY(hipStreamWaitEvent(m0.stream, s->lm[(size_t)d].ev, 0));
                if (int rc = launch_axpy(cnt, s->lm[(size_t)d].d_shares, s->lm[0].d_shares, m0.stream)) return rc;
            }
            VRT_HIP_TRY(hipEventRecord(s->lm[0].ev, m0.stream));
            for (int d = 1; d < W; d++) {
                VRT_HIP_TRY(hipStreamWaitEvent(mm->m[(size_t)d].stream, s->lm[0].ev, 0));
                VRT_HIP_TRY(hipMemcpyAsync(s->lm[(size_t)d].d_shares, s->lm[0].d_shares, sizeof(double) * cnt, hipMemcpyDeviceToDevice, mm->m[(size_t)d].stream));
            }
        }
        // ---- every device: R and the populations of every site; the criterion's scalars come home -----------------------
        std::vector<unsigned long long> h((size_t)(2 * W), 0);
        for (int d = 0; d < W; d++) {
            Member &me = mm->m[(size_t)d];
            LambdaMember &l = s->lm[(size_t)d];
            VRT_HIP_TRY(hipSetDevice(me.device));
            (void)hipGetLastError();
            if (int rc = launch_populations_from_shares(n, l.d_shares, l.line.d_C, l.line.d_atom, l.line.d_R, l.d_pops, me.stream)) return rc;
            VRT_HIP_TRY(hipMemcpyAsync(h.data() + 2 * d, l.d_scalars, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, me.stream));
        }
        double worst = 0.0;
        bool is_nan = false;
        for (int d = 0; d < W; d++) {
            VRT_HIP_TRY(hipSetDevice(mm->m[(size_t)d].device));
            VRT_HIP_TRY(hipStreamSynchronize(mm->m[(size_t)d].stream));
            if (int rcc = patch_chain_check(mm->m[(size_t)d].plan_all.get())) return rcc;     // this iteration's sweep gave up on that device
            double v;
            std::memcpy(&v, &h[(size_t)(2 * d)], sizeof(double));
            worst = std::max(worst, v);
            is_nan = is_nan || h[(size_t)(2 * d + 1)] != 0;
        }
        *max_rel_change = is_nan ? std::nan("") : worst;
        s->iterations++;
        if (s->ng.order) return multi_ng_after_iterate(s);       // history copies or the step, on the S of the plain update
        s->ng.last_applied = 0;
        return VRT_OK;
    });
}

}  // extern "C"

// (the C entries vrt_multi_lambda_set_acceleration / _last_acceleration call these two: vrt_multi_accel.cpp)
int vrt::multi_lambda_set_acceleration(vrt_multi_lambda *s, int order, int start, int period)
{
    if (!s) return fail(VRT_EINVAL, "NULL session");
    int rc = ng_check_settings(order, start, period);
    if (rc) return rc;
    if (s->f32)                                 // the Ng kernels and NgRange: the [pair][pos][2] double layout
        return fail(VRT_EINVAL, "vrt_multi_lambda_set_acceleration: not on a float-storage session (the Ng kernels work on double planes)");
    return guarded([&] {
        vrt_multi *mm = s->mm;
        std::lock_guard<std::mutex> lock(mm->mu);
        const int W = (int)mm->m.size();
        s->ng.last_applied = 0;
        // every member with wavelengths: three copies of ITS block of S and a workspace (order 0: released)
        for (int d = 0; d < W && !rc; d++) {
            Member &me = mm->m[(size_t)d];
            LambdaMember &l = s->lm[(size_t)d];
            if (l.l1 <= l.l0) continue;
            if (hipSetDevice(me.device) != hipSuccess) { rc = fail(VRT_ENODEVICE, "hipSetDevice failed"); break; }
            std::lock_guard<std::mutex> plock(me.plan_all->mu);
            rc = ng_configure(l.ng, order, start, period, l.sj.ng_count());
        }
        if (rc) {
            // one member could not: no member keeps a history, and the session goes on as a plain one
            for (int d = 0; d < W; d++) {
                (void)hipSetDevice(mm->m[(size_t)d].device);
                (void)ng_configure(s->lm[(size_t)d].ng, 0, 0, 0, 0);
            }
            order = 0;
        }
        s->ng.order = order;
        s->ng.start = order ? start : 0;
        s->ng.period = order ? period : 0;
        return rc;
    });
}

int vrt::multi_lambda_last_acceleration(const vrt_multi_lambda *s, int *applied, double sums[5], double coeffs[2])
{
    if (!s || !applied) return fail(VRT_EINVAL, "NULL argument");
    return ng_report(s->ng, applied, sums, coeffs);
}

extern "C" {

int vrt_multi_lambda_get(vrt_multi_lambda *s, double *J, double *S, double *populations, double *R, double *gamma)
{
    if (!s) return fail(VRT_EINVAL, "NULL session");
    return guarded([&] {
        vrt_multi *mm = s->mm;
        std::lock_guard<std::mutex> lock(mm->mu);
        const size_t n = (size_t)s->n, w8 = sizeof(double);
        for (size_t d = 0; d < mm->m.size(); d++) {
            const LambdaMember &l = s->lm[d];
            VRT_HIP_TRY(hipSetDevice(mm->m[d].device));
            {   // this block's columns, in the caller's layout
                std::lock_guard<std::mutex> plock(mm->m[d].plan_all->mu);
                if (int rc = l.sj.download(J, S, s->nlam, l.l0, mm->m[d].stream)) return rc;
            }
            if (d == 0) {
                if (populations) VRT_HIP_TRY(hipMemcpy(populations, l.d_pops, w8 * 3 * n, hipMemcpyDeviceToHost));
                if (R) VRT_HIP_TRY(hipMemcpy(R, l.line.d_R, w8 * 9 * n, hipMemcpyDeviceToHost));
                if (gamma) VRT_HIP_TRY(hipMemcpy(gamma, l.line.d_gamma, w8 * n, hipMemcpyDeviceToHost));
            }
        }
        return VRT_OK;
    });
}

int vrt_multi_lambda_set_state(vrt_multi_lambda *s, const double *S, const double *populations)
{
    int rc = check_state_pointers(s, S, populations);
    if (rc || (rc = check_state(s->n, s->nlam, S, populations))) return rc;
    return guarded([&] {
        vrt_multi *mm = s->mm;
        std::lock_guard<std::mutex> lock(mm->mu);
        const int W = (int)mm->m.size();
        const size_t n = (size_t)s->n;
        // staged copies beside the session, one set per device: it is untouched until every one of them is complete
        struct Staged {
            int device = 0;
            SourceStore::Staged S;
            DevBuf<double> pops;
            ~Staged() { (void)hipSetDevice(device); }        // then the members go, on their device
        };
        std::vector<Staged> staged((size_t)W);
        std::vector<int> rcs((size_t)W, VRT_OK);
        std::vector<std::string> errs((size_t)W);
        auto work = [&](int d) {
            Member &me = mm->m[(size_t)d];
            const LambdaMember &l = s->lm[(size_t)d];
            Staged &sg = staged[(size_t)d];
            sg.device = me.device;
            const int64_t nb = l.l1 - l.l0;
            if (hipSetDevice(me.device) != hipSuccess) { rcs[(size_t)d] = VRT_ENODEVICE; errs[(size_t)d] = "hipSetDevice"; return; }
            hipStream_t st = me.stream;
            vrt_plan *p = me.plan_all.get();
            std::lock_guard<std::mutex> plock(p->mu);
            int rc = VRT_OK;
            if (S && nb > 0) rc = l.sj.stage(S, s->nlam, l.l0, sg.S, st);      // this block's columns
            if (!rc && populations) rc = upload(sg.pops, populations, 3 * n, st);       // every device holds a full copy
            if (!rc && hipStreamSynchronize(st) != hipSuccess) rc = fail(VRT_ENODEVICE, "uploading the state failed");
            if (rc) { rcs[(size_t)d] = rc; errs[(size_t)d] = vrt_last_error(); }
        };
        const bool ok = run_workers(W, work);
        for (int d = 0; d < W; d++)
            if (!ok || rcs[(size_t)d]) {
                const int rc = ok ? rcs[(size_t)d] : VRT_ENOMEM;
                return fail(rc, ok ? "device " + std::to_string(mm->m[(size_t)d].device) + ": " + errs[(size_t)d] : "out of host memory");
            }
        for (int d = 0; d < W; d++) {
            LambdaMember &l = s->lm[(size_t)d];
            Staged &sg = staged[(size_t)d];
            if (S && l.l1 > l.l0) l.sj.adopt(sg.S);
            if (populations) std::swap(l.d_pops, sg.pops);
            l.ng.have = 0;                                   // iterates of another state are no history of this one
        }
        s->ng.last_applied = 0;
        if (S) s->ng_torn = false;                           // both sweep-order copies of every member are new
        return (int)VRT_OK;
    });
}

void vrt_multi_lambda_destroy(vrt_multi_lambda *s)
{
    DeviceScope scope;
    delete s;
}

void vrt_multi_destroy(vrt_multi *mm)
{
    DeviceScope scope;
    delete mm;
}

}  // extern "C"
