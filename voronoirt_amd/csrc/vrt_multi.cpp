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
// Every piece of per-device work -- create, the two executes, the session's create, iterate, set_state and the Ng phases --
// is a body handed to on_members (vrt_multi_members.h): a host thread per member, its device current, its plan locked
// where the body sweeps, the first failing member reported as "device N: ...".  Both collectives go through rccl_group,
// host columns reach a device through upload_cols (vrt_internal.h), and a session member's wavelengths are a LineBlock
// (vrt_line_block.h), the one the single-device session holds.
#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "vrt_internal.h"
#include "vrt_line_block.h"
#include "vrt_multi_members.h"

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
    int rc = VRT_OK;                       // on_members: of the last piece of work here, and its text
    std::string err;
    std::mutex &plan_mutex() { return plan_all->mu; }
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

// ONE RCCL group call over every member: call(d, member) -> ncclResult_t queues the member's collective (`what`, for the
// error text) with its device current.  Nothing returns between GroupStart and GroupEnd: an open group poisons every
// later call.
template <typename Call>
static int rccl_group(vrt_multi *mm, const char *what, Call call)
{
    ncclResult_t r = mm->rccl.GroupStart();
    hipError_t he = hipSuccess;
    for (size_t d = 0; d < mm->m.size() && r == ncclSuccess && he == hipSuccess; d++) {
        he = hipSetDevice(mm->m[d].device);
        if (he == hipSuccess) r = call((int)d, mm->m[d]);
    }
    const ncclResult_t r2 = mm->rccl.GroupEnd();
    if (he != hipSuccess) return fail(VRT_ENODEVICE, std::string("hipSetDevice: ") + hipGetErrorString(he));
    if (r != ncclSuccess || r2 != ncclSuccess)
        return fail(VRT_ENODEVICE, std::string(what) + ": " + mm->rccl.GetErrorString(r != ncclSuccess ? r : r2));
    return VRT_OK;
}

// I_0 of one sweep direction for an execute: columns [l0, l1) of the host rows (n1, nlam) into the member's workspace;
// *dev stays NULL without the array or without sites that take it
static int stage_I0(DevWork<double> &d, const double *I0, int64_t n1, int64_t nlam, int64_t l0, int64_t l1, hipStream_t st,
                    double **dev)
{
    *dev = nullptr;
    if (!I0 || !n1) return VRT_OK;
    const int rc = upload_cols(d, I0, (size_t)n1, nlam, l0, l1, st);
    if (!rc) *dev = d;
    return rc;
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
        // (kNoDevice: vrt_grid_create is the call that finds out whether the device exists)
        int rc = on_members(mm->m, kNoDevice, every_member, [&](int, Member &me) {
            vrt_grid *grid = nullptr;
            vrt_plan *plan = nullptr;
            int r = vrt_grid_create(n, pos_zxy, nbr, D1, bounds, me.device, &grid);
            me.grid.reset(grid);
            if (!r) r = vrt_plan_create_ex(grid, n_angles, k, mm->dirs.data(), n_sweeps, &plan);
            me.plan_all.reset(plan);
            if (!r && (hipSetDevice(me.device) != hipSuccess || me.stream.create())) r = fail(VRT_ENODEVICE, "cannot create a stream");
            return r;
        });
        if (rc) return rc;
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
        // lambda mode: the member's block of the wavelengths (a member without one sits the call out); angle mode: all of them
        auto block = [&](int d, int64_t &l0, int64_t &l1) {
            l0 = 0, l1 = nlam;
            if (shard == 1) block_of(nlam, W, d, l0, l1);
            return l1 > l0;
        };
        int rc = on_members(mm->m, 0, [&](int d) { int64_t l0, l1; return !block(d, l0, l1); }, [&](int d, Member &me) {
            hipStream_t st = me.stream;
            int64_t l0, l1;
            block(d, l0, l1);
            const size_t sn = (size_t)n, nb = (size_t)(l1 - l0), w8 = sizeof(double);
            int rc;
            if (shard == 2 && me.my_angles.empty()) {                    // no angle here: its partial J is zero
                if ((rc = me.dJ.grow(sn * nb))) return rc;
                VRT_HIP_TRY(hipMemsetAsync(me.dJ, 0, w8 * sn * nb, st));
                VRT_HIP_TRY(hipStreamSynchronize(st));                   // another member's stream reads these zeros
                return (int)VRT_OK;
            }
            vrt_plan *plan = shard == 1 ? me.plan_all.get() : me.plan_part.get();
            const size_t nA = shard == 1 ? (size_t)A : me.my_angles.size();
            // the block (nb, n) of S and of α dense on the device
            if ((rc = upload_cols(me.dS, S, sn, ld, l0, l1, st)) || (rc = me.dJ.grow(sn * nb))) return rc;
            if (alpha_mode == VRT_ALPHA_SITE) rc = upload_cols(me.dA, alpha, 1, (int64_t)sn, 0, (int64_t)sn, st);
            else if (alpha_mode == VRT_ALPHA_SITE_LAM) rc = upload_cols(me.dA, alpha, sn, ld, l0, l1, st);
            else {
                rc = me.dA.grow(nA * sn * nb);
                for (size_t j = 0; j < nA && !rc; j++) {
                    const size_t a = shard == 1 ? j : (size_t)me.my_angles[j];
                    rc = copy_cols<double>(me.dA + j * sn * nb, alpha + a * sn * (size_t)ld, sn, ld, l0, l1, st);
                }
            }
            double *dU, *dD;
            if (rc || (rc = stage_I0(me.dU, I0_up, n1u, nlam, l0, l1, st, &dU)) || (rc = stage_I0(me.dD, I0_down, n1d, nlam, l0, l1, st, &dD)))
                return rc;
            std::vector<double> wv;
            if (shard == 1) wv.assign(weights, weights + A);
            else
                for (int a : me.my_angles) wv.push_back(weights[a]);
            if ((rc = vrt_plan_execute_dev(plan, (int64_t)nb, (int64_t)nb, me.dS, me.dA, alpha_mode, dU, dD, wv.data(), me.dJ, nullptr, st)))
                return rc;
            if (shard == 1)     // the device owns rows l0..l1 of J: straight home
                VRT_HIP_TRY(hipMemcpy2DAsync(J + l0, w8 * (size_t)ld, me.dJ, w8 * nb, w8 * nb, sn, hipMemcpyDeviceToHost, st));
            VRT_HIP_TRY(hipStreamSynchronize(st));
            return patch_chain_check(plan);      // (a chained sweep that gave up waiting: reported by THIS call, whose J it spoiled)
        });
        if (rc) return rc;
        if (shard == 2) {
            // J = Σ over the devices' partial sums, wanted on ONE device only (the host array is filled from device 0):
            // one RCCL reduce to rank 0 over xGMI -- half the bytes of an all-reduce -- or, on a shared device, adds
            const size_t cnt = (size_t)n * (size_t)nlam;
            if (mm->uses_rccl()) {
                if ((rc = rccl_group(mm, "ncclReduce", [&](int, Member &me) {
                        return mm->rccl.Reduce(me.dJ, me.dJ, cnt, ncclDouble, ncclSum, 0, me.comm, me.stream);
                    })))
                    return rc;
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
        auto block = [&](int d, int64_t &l0, int64_t &l1) {
            block_of(nlam, W, d, l0, l1);
            return l1 > l0;
        };
        return on_members(mm->m, kLockPlan, [&](int d) { int64_t l0, l1; return !block(d, l0, l1); }, [&](int d, Member &me) {
            hipStream_t st = me.stream;
            vrt_plan *plan = me.plan_all.get();
            int64_t l0, l1;
            block(d, l0, l1);
            const size_t w8 = sizeof(double), sn = (size_t)n, nb = (size_t)(l1 - l0);
            // S | seven per-site vectors + the block's wavelengths | native alpha | J
            int rc;
            if ((rc = upload_cols(me.dS, S, sn, ld, l0, l1, st)) || (rc = me.dJ.grow(sn * nb)) ||
                (rc = me.dA.grow((size_t)vrt_plan_native_alpha_count(plan, (int64_t)nb))) || (rc = me.dV.grow(7 * sn + nb)))
                return rc;
            double *d_vel = me.dV, *d_dop = me.dV + 3 * sn, *d_gam = me.dV + 4 * sn, *d_str = me.dV + 5 * sn, *d_ac = me.dV + 6 * sn,
                   *d_lam = me.dV + 7 * sn;
            const struct { double *dev; const double *host; size_t count; } vectors[] = {
                {d_vel, velocity, 3 * sn}, {d_dop, doppler_width, sn}, {d_gam, gamma, sn}, {d_str, line_strength, sn},
                {d_ac, alpha_cont, sn}, {d_lam, lambda + l0, nb}};
            for (const auto &v : vectors) VRT_HIP_TRY(hipMemcpyAsync(v.dev, v.host, w8 * v.count, hipMemcpyHostToDevice, st));
            double *dU, *dD;
            if ((rc = stage_I0(me.dU, I0_up, n1u, nlam, l0, l1, st, &dU)) || (rc = stage_I0(me.dD, I0_down, n1d, nlam, l0, l1, st, &dD)) ||
                (rc = launch_line_opacity(plan, (int64_t)nb, d_lam, lambda0, c0, d_vel, d_dop, d_gam, d_str, d_ac, me.dA, st)) ||
                (rc = execute_locked(plan, caller_args((int64_t)nb, (int64_t)nb, me.dS, me.dA, VRT_ALPHA_ANGLE_NATIVE, dU, dD, weights, me.dJ, nullptr, st, false))))
                return rc;
            VRT_HIP_TRY(hipMemcpy2DAsync(J + l0, w8 * (size_t)ld, me.dJ, w8 * nb, w8 * nb, sn, hipMemcpyDeviceToHost, st));
            VRT_HIP_TRY(hipStreamSynchronize(st));
            return patch_chain_check(plan);
        });
    });
}

}  // extern "C"

// ---- Λ-iteration session across several devices (BASELINE configs[3]; src/lambda_iteration.jl:205-300) ---------------
// Every device owns a contiguous block of the wavelengths (91 over 8 -> 12,12,12,11,11,11,11,11) and the whole per-site
// state.  Per iteration it runs, for ITS wavelengths: the line terms of the current populations, α_tot of every
// angle, the sweep, S_new with its share of the convergence maximum, and its share of the six λ-integrals of the
// radiative rates (rates.jl:154-201).  The shares are summed by ONE all-reduce of 6 n doubles over xGMI (SURVEY 8e:
// "only R and one scalar are reduced"); J never travels.  Every device then solves the statistical equilibrium of
// every site itself (populations.jl:191-221), so the next iteration's opacity needs no further exchange.  A member's
// wavelengths are a LineBlock (vrt_line_block.h) -- S and J in rows or in sweep order, B_0, I_0 and the native α, all
// members alike -- and LineBlock::step is its iterate up to the update, the one the single-device session runs.  Float
// storage (vrt_multi_lambda_create_f32): no member holds a double array of size nλ_block·n or nλ_block·n·angles; the
// shares, the all-reduce and the statistical equilibrium are the same doubles.
struct LambdaMember {
    int device = 0;
    LineCaseDev line;                   // the whole case (every site, ALL wavelengths), γ, the line strength and R (vrt_line_case.h)
    LineBlock blk;                      // this device's wavelengths [blk.l0, blk.l1) (none: placeholders and no store)
    DevBuf<double> d_pops, d_shares;
    DevBuf<unsigned long long> d_scalars;
    Event ev;
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

// ---- Ng acceleration of the session (vrt_multi_lambda_set_acceleration): the phases of vrt_internal.h, each over every
// member that holds wavelengths, on the S of its store.

// body(d, member, its share of the session) -> rc on every member with wavelengths, its plan locked (on_members)
template <typename Body>
int ng_on_members(vrt_multi_lambda *s, Body body)
{
    return on_members(s->mm->m, kLockPlan, [&](int d) { return s->lm[(size_t)d].blk.nb() == 0; },
                      [&](int d, Member &me) { return body(d, me, s->lm[(size_t)d]); });
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
            int rc = ng_record(l.ng, due, l.blk.sj.ng_S(), l.blk.sj.ng_count(), me.stream);
            if (!rc && hipStreamSynchronize(me.stream) != hipSuccess) rc = fail(VRT_ENODEVICE, "copying S into the history failed");
            return rc;
        });
    bool complete = true;
    for (LambdaMember &l : s->lm)
        if (l.blk.nb() > 0 && !ng_take_history(l.ng)) complete = false;
    if (!complete) return VRT_OK;               // switched on too late for this one, or the state was replaced: nothing due
    std::vector<double> part(5 * (size_t)W, 0.0);
    int rc = ng_on_members(s, [&](int d, Member &me, LambdaMember &l) {
        return ng_sums(l.blk.sj.ng_range(), l.blk.sj.ng_S(), l.ng.hist[0], l.ng.hist[1], l.ng.hist[2],
                       l.ng.d_ws, &part[5 * (size_t)d], me.stream);
    });
    if (rc) return rc;
    // ((s_0 + s_1) + s_2) + ... over the members that hold wavelengths: never the order in which the workers finished
    std::vector<NgPiece> pieces;
    std::vector<int> piece_of((size_t)W, -1);
    for (int d = 0; d < W; d++) {
        LambdaMember &l = s->lm[(size_t)d];
        if (l.blk.nb() == 0) continue;
        ng_add_sums(s->ng.last_sums, &part[5 * (size_t)d], pieces.empty());
        piece_of[(size_t)d] = (int)pieces.size();
        pieces.push_back(NgPiece{&l.ng, &l.blk.sj.ng_S(), false});
    }
    s->ng.last_applied = -1;
    const bool valid = ng_coefficients(s->ng.last_sums, s->ng.last_coeffs);
    if (valid) {
        const double a = s->ng.last_coeffs[0], b = s->ng.last_coeffs[1];
        rc = ng_on_members(s, [&](int d, Member &me, LambdaMember &l) {
            return ng_apply(l.blk.sj.ng_range(), a, b, l.blk.sj.ng_S(), l.ng.hist[0], l.ng.hist[1], l.ng.hist[2],
                            l.ng.d_ws, &pieces[(size_t)piece_of[(size_t)d]].good, me.stream);
        });
        if (rc) return rc;
    }
    if (!ng_commit(pieces.data(), (int)pieces.size(), valid)) return VRT_OK;
    if (s->lm[0].blk.sj.two_orders()) {             // (every member with wavelengths keeps the form of the first)
        // the down-order copies from the new up-order ones, value for value
        rc = ng_on_members(s, [&](int, Member &me, LambdaMember &l) {
            int r = l.blk.sj.mirror_down(me.stream);
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
        for (const Member &me : mm->m)
            if (int rc = line_session_plan_ok(me.plan_all.get(), f32)) return rc;
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
        for (int d = 0; d < W; d++) s->lm[(size_t)d].device = mm->m[(size_t)d].device;      // (what a member's destructor needs)
        int rc = on_members(mm->m, 0, every_member, [&](int d, Member &me) {
            LambdaMember &l = s->lm[(size_t)d];
            hipStream_t st = me.stream;
            int64_t l0, l1;
            block_of(nlam, W, d, l0, l1);
            int rc;
            if ((rc = l.line.create(lc, mm->n, st)) ||
                (rc = upload(l.d_pops, lc->lte_populations, 3 * n, st)) ||           // populations = copy(LTE_pops), :232
                (rc = l.blk.create(me.plan_all.get(), lc->B0, nlam, l0, l1, form, st)) || (rc = l.d_shares.alloc(6 * n)) ||
                (rc = l.d_scalars.alloc(2)) || (rc = l.ev.create(hipEventDisableTiming)))
                return rc;
            if (hipStreamSynchronize(st) != hipSuccess) return fail(VRT_ENODEVICE, "uploading the line case failed");
            return (int)VRT_OK;
        });
        if (rc) return rc;
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
        int rc = on_members(mm->m, kLockPlan, every_member, [&](int d, Member &me) {
            LambdaMember &l = s->lm[(size_t)d];
            hipStream_t st = me.stream;
            if (l.blk.nb() == 0)                 // no update writes its words
                VRT_HIP_TRY(hipMemsetAsync(l.d_scalars, 0, 2 * sizeof(unsigned long long), st));
            // α of the current populations, the sweep and the update with this block's share of the criterion: the block's
            RatesJ J;
            int rc = l.blk.step(me.plan_all.get(), l.line, l.d_pops, s->weights.data(), l.d_scalars, nullptr, st, &J);
            // this block's share of the six rate integrals (rates.jl:154-201), from J in the store's form
            return rc ? rc : launch_rates_partial(l.line.rates_in(), J, l.blk.l0, l.blk.l1, l.d_shares, st);
        });
        if (rc) return rc;
        // ---- the shares summed over the devices: ONE all-reduce of 6 n doubles (in place), stream-ordered ---------------
        const size_t cnt = 6 * (size_t)n;
        if (mm->uses_rccl()) {
            if ((rc = rccl_group(mm, "ncclAllReduce", [&](int d, Member &me) {
                    double *shares = s->lm[(size_t)d].d_shares;
                    return mm->rccl.AllReduce(shares, shares, cnt, ncclDouble, ncclSum, me.comm, me.stream);
                })))
                return rc;
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
            if (l.blk.nb() == 0) continue;
            if (hipSetDevice(me.device) != hipSuccess) { rc = fail(VRT_ENODEVICE, "hipSetDevice failed"); break; }
            std::lock_guard<std::mutex> plock(me.plan_all->mu);
            rc = ng_configure(l.ng, order, start, period, l.blk.sj.ng_count());
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
                if (int rc = l.blk.sj.download(J, S, s->nlam, l.blk.l0, mm->m[d].stream)) return rc;
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
        for (int d = 0; d < W; d++) staged[(size_t)d].device = mm->m[(size_t)d].device;
        rc = on_members(mm->m, kLockPlan, every_member, [&](int d, Member &me) {
            const LineBlock &b = s->lm[(size_t)d].blk;
            Staged &sg = staged[(size_t)d];
            hipStream_t st = me.stream;
            int rc = VRT_OK;
            if (S && b.nb() > 0) rc = b.sj.stage(S, s->nlam, b.l0, sg.S, st);            // this block's columns
            if (!rc && populations) rc = upload(sg.pops, populations, 3 * n, st);       // every device holds a full copy
            if (!rc && hipStreamSynchronize(st) != hipSuccess) rc = fail(VRT_ENODEVICE, "uploading the state failed");
            return rc;
        });
        if (rc) return rc;
        for (int d = 0; d < W; d++) {
            LambdaMember &l = s->lm[(size_t)d];
            Staged &sg = staged[(size_t)d];
            if (S && l.blk.nb() > 0) l.blk.sj.adopt(sg.S);
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
