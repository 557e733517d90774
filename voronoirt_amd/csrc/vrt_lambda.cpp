// Host-pointer entry points of the line case: what a single-process host WITHOUT device arrays of its own
// (the reference's Julia driver) calls instead of shipping α_tot (nλ, n, n_angles) through PCIe.
//   vrt_line_terms_dev     γ and the line strength from the current populations (device pointers)
//   vrt_plan_execute_line  the body of J_λ_voronoi, line case (src/lambda_iteration.jl:72-111): per-site line
//                          vectors + S in, J out; α_tot is made on the device and never exists on the host
//   vrt_lambda_*           Λ_voronoi's loop (src/lambda_iteration.jl:205-300) with library-owned device state:
//                          per iteration only the criterion's scalar comes back.  S, J, B_0, I_0 and the native α of
//                          all wavelengths are ONE LineBlock (vrt_line_block.h), which also runs an iterate up to the
//                          update; the session follows with the rates, the populations and the criterion
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <thread>

#include "vrt_internal.h"
#include "vrt_line_block.h"

using namespace vrt;

namespace {

// ---- pageable host arrays at PCIe speed: lanes of (host thread, copy stream, two pinned staging buffers) ----------------
struct CopyJob {
    const char *host_src = nullptr;     // upload: rows of `width` bytes, `hstride` apart
    char *host_dst = nullptr;           // download
    char *dev = nullptr;                // dense on the device: rows x width bytes
    size_t rows = 0, width = 0, hstride = 0;
};

int ensure_copy_lanes(vrt_plan *p, int lanes)
{
    if ((int)p->copy_lanes.size() >= lanes && p->copy_done) return VRT_OK;
    int rc;
    if (!p->copy_done && (rc = p->copy_done.create(hipEventDisableTiming))) return rc;
    while ((int)p->copy_lanes.size() < lanes) {
        CopyLane l;
        if ((rc = l.st.create())) return rc;
        for (int b = 0; b < 2; b++)
            if ((rc = l.pin[b].alloc(kCopyChunk)) || (rc = l.ev[b].create(hipEventDisableTiming))) return rc;
        p->copy_lanes.push_back(std::move(l));
    }
    return VRT_OK;
}

// rows x width bytes per job <= kCopyChunk
void split_jobs(std::vector<CopyJob> &jobs, const void *host, void *dev, size_t rows, size_t width, size_t hstride, bool download)
{
    const size_t per = std::max<size_t>(1, kCopyChunk / std::max<size_t>(width, 1));
    for (size_t r0 = 0; r0 < rows; r0 += per) {
        CopyJob j;
        j.rows = std::min(per, rows - r0);
        j.width = width;
        j.hstride = hstride;
        j.dev = (char *)dev + r0 * width;
        if (download) j.host_dst = (char *)const_cast<void *>(host) + r0 * hstride;
        else j.host_src = (const char *)host + r0 * hstride;
        jobs.push_back(j);
    }
}

void rows_copy(char *dst, size_t dstride, const char *src, size_t sstride, size_t rows, size_t width)
{
    if (dstride == width && sstride == width) { std::memcpy(dst, src, rows * width); return; }
    for (size_t r = 0; r < rows; r++) std::memcpy(dst + r * dstride, src + r * sstride, width);
}

// every lane takes the jobs lane, lane + L, ...; uploads leave on the lanes' streams (`st` then waits for them), downloads
// start behind `after` (an event of the producing stream) and are complete in host memory on return
int run_copy_jobs(vrt_plan *p, const std::vector<CopyJob> &jobs, bool download, hipEvent_t after, hipStream_t st, int device)
{
    const int L = (int)p->copy_lanes.size();
    std::vector<int> rcs((size_t)L, VRT_OK);
    auto lane_work = [&](int li) {
        CopyLane &l = p->copy_lanes[(size_t)li];
        if (hipSetDevice(device) != hipSuccess) { rcs[(size_t)li] = VRT_ENODEVICE; return; }
        auto ok = [&](hipError_t e) { if (e != hipSuccess) rcs[(size_t)li] = VRT_ENODEVICE; return e == hipSuccess; };
        if (download && after && !ok(hipStreamWaitEvent(l.st, after, 0))) return;
        // (the staging buffers may still feed the last transfers of an EARLIER call: those first)
        for (int b = 0; b < 2; b++)
            if (!ok(hipEventSynchronize(l.ev[b]))) return;
        int pending[2] = {-1, -1};
        int slot = 0;
        for (size_t k = (size_t)li; k < jobs.size(); k += (size_t)L, slot ^= 1) {
            const CopyJob &j = jobs[k];
            const size_t bytes = j.rows * j.width;
            if (pending[slot] >= 0) {                        // the buffer's previous transfer: finished (and, downloading, taken home)
                if (!ok(hipEventSynchronize(l.ev[slot]))) return;
                if (download) {
                    const CopyJob &o = jobs[(size_t)pending[slot]];
                    rows_copy(o.host_dst, o.hstride, l.pin[slot], o.width, o.rows, o.width);
                }
            }
            if (download) {
                if (!ok(hipMemcpyAsync(l.pin[slot], j.dev, bytes, hipMemcpyDeviceToHost, l.st))) return;
            } else {
                rows_copy(l.pin[slot], j.width, j.host_src, j.hstride, j.rows, j.width);
                if (!ok(hipMemcpyAsync(j.dev, l.pin[slot], bytes, hipMemcpyHostToDevice, l.st))) return;
            }
            if (!ok(hipEventRecord(l.ev[slot], l.st))) return;
            pending[slot] = (int)k;
        }
        for (int b = 0; b < 2; b++) {                        // drain (oldest first: the slot that is next in turn)
            const int sl = slot ^ b;
            if (pending[sl] < 0) continue;
            if (download) {
                if (!ok(hipEventSynchronize(l.ev[sl]))) return;
                const CopyJob &o = jobs[(size_t)pending[sl]];
                rows_copy(o.host_dst, o.hstride, l.pin[sl], o.width, o.rows, o.width);
            }
        }
    };
    if (!run_workers(L, lane_work)) return fail(VRT_ENOMEM, "out of host memory in a copy lane");
    for (int li = 0; li < L; li++)
        if (rcs[(size_t)li]) return fail(rcs[(size_t)li], "a host <-> device copy lane failed");
    if (!download)
        for (int li = 0; li < L; li++) {                     // `st` follows the uploads
            CopyLane &l = p->copy_lanes[(size_t)li];
            for (int b = 0; b < 2; b++) VRT_HIP_TRY(hipStreamWaitEvent(st, l.ev[b], 0));
        }
    return VRT_OK;
}

}  // namespace

struct vrt_lambda {
    vrt_plan *p = nullptr;              // borrowed: the caller keeps the plan alive for as long as the session
    int device = 0;                     // of the plan's grid (kept here: destroying the session must not look into a plan that may be gone)
    int64_t n = 0, nlam = 0;
    std::vector<double> weights;
    // device state
    LineCaseDev line;                   // the uploaded case, γ, the line strength and R (vrt_line_case.h)
    DevBuf<double> d_pops, d_pops_new;
    DevBuf<unsigned long long> d_scalars;
    int iterations = 0;
    // every wavelength: S and J in rows or in sweep order (VRT_LAMBDA_NATIVE, default), B_0, I_0 and the native α.  Float
    // storage (vrt_lambda_create_f32): no double array of size nλ·n or nλ·n·angles exists in such a session
    LineBlock blk;
    NgState ng;                         // vrt_lambda_set_acceleration (off: nothing allocated, nothing run)
    // vrt_lambda_use_operator (0: nothing allocated, nothing run): Λ* of the current iterate's α in the store's form
    // (rows, or one up-order plane set), rewritten by every iterate -- no operator state survives an iterate
    int op = 0;
    DevBuf<double> d_diag;
    int64_t fallback_last = 0;          // entries of the last iterate that took the plain update (den not > 0)
};

struct LambdaDelete { void operator()(vrt_lambda *s) const { vrt_lambda_destroy(s); } };

extern "C" {

int vrt_line_terms_dev(vrt_grid *g, const double *d_gamma_static, const double *d_gamma_unsold,
                       const double *d_populations, double strength_const, double Bij, double Bji, double *d_gamma,
                       double *d_line_strength, void *stream)
{
    if (!g || !d_populations) return fail(VRT_EINVAL, "NULL argument");
    if (d_gamma && (!d_gamma_static || !d_gamma_unsold)) return fail(VRT_EINVAL, "gamma needs gamma_static and gamma_unsold");
    return guarded([&] {
        int rc = use_device(g->device);
        if (rc) return rc;
        return launch_line_terms(g->n, d_gamma_static, d_gamma_unsold, d_populations, strength_const, Bij, Bji, d_gamma,
                                 d_line_strength, (hipStream_t)stream);
    });
}

int vrt_plan_execute_line(vrt_plan *p, int64_t nlam, int64_t ld, const double *lambda, double lambda0, double c0,
                          const double *velocity, const double *doppler_width, const double *gamma,
                          const double *line_strength, const double *alpha_cont, const double *S, const double *I0_up,
                          const double *I0_down, const double *weights, double *J)
{
    if (!p || !lambda || !velocity || !doppler_width || !gamma || !line_strength || !alpha_cont || !S || !weights || !J)
        return fail(VRT_EINVAL, "NULL argument");
    if (nlam < 1 || ld < nlam) return fail(VRT_EINVAL, "need nlam >= 1 and ld >= nlam");
    if (!(lambda0 > 0) || !(c0 > 0)) return fail(VRT_EINVAL, "lambda0 and c0 must be positive");
    return guarded([&] {
        std::lock_guard<std::mutex> lock(p->mu);
        vrt_grid *g = p->g;
        int rc = use_device(g->device);
        if (rc) return rc;
        if ((rc = line_path_ok(p, "the line entry"))) return rc;
        if (p->A != (int)p->n_angles_user)
            return fail(VRT_EINVAL, "per-angle alpha needs every angle active (no θ = 90 direction)");
        const size_t n = (size_t)g->n, nl = (size_t)nlam, nS = n * nl;           // dense (n, nlam) on the device
        const size_t nU = (size_t)g->up.n1 * nl, nD = (size_t)g->down.n1 * nl;
        hipStream_t st = g->stream;
        // staging: S | J in the plan's stage buffers; the seven per-site vectors + λ in stage 1; α_tot native in ws_AA
        const size_t vecs = 7 * n + nl;                  // velocity (3n), ΔλD, γ, strength, α_cont, λ
        if ((rc = p->d_stage[0].grow(nS))) return rc;
        if ((rc = p->d_stage[1].grow(vecs))) return rc;
        if ((rc = p->d_stage[4].grow(nS))) return rc;
        const size_t nnat = (size_t)vrt_plan_native_alpha_count(p, nlam);
        if ((rc = p->ws_AA.grow(nnat))) return rc;
        double *dv = p->d_stage[1];
        double *d_vel = dv, *d_dop = dv + 3 * n, *d_gam = dv + 4 * n, *d_str = dv + 5 * n, *d_ac = dv + 6 * n, *d_lam = dv + 7 * n;
        double *dU = nullptr, *dD = nullptr;
        if (I0_up && nU) {
            if ((rc = p->d_stage[2].grow(nU))) return rc;
            dU = p->d_stage[2];
        }
        if (I0_down && nD) {
            if ((rc = p->d_stage[3].grow(nD))) return rc;
            dD = p->d_stage[3];
        }
        // The caller's arrays are pageable: they cross PCIe through copy lanes (a host thread, a copy stream and two pinned
        // buffers each).  Order: the per-site vectors -> the opacity kernel starts while S is still on its way -> sweep ->
        // J comes home in chunks.  Only the nlam columns of S and J are touched (ld >= nlam: the padding stays the caller's).
        unsigned hw = std::thread::hardware_concurrency();
        const int lanes = (int)std::max(2u, std::min(8u, (hw ? hw : 8u) / 2));
        if ((rc = ensure_copy_lanes(p, lanes))) return rc;
        const size_t w8 = sizeof(double);
#ifdef VRT_DIAG
        const auto t0 = std::chrono::steady_clock::now();
#endif
        std::vector<CopyJob> jobs;
        split_jobs(jobs, velocity, d_vel, 1, w8 * 3 * n, w8 * 3 * n, false);
        split_jobs(jobs, doppler_width, d_dop, 1, w8 * n, w8 * n, false);
        split_jobs(jobs, gamma, d_gam, 1, w8 * n, w8 * n, false);
        split_jobs(jobs, line_strength, d_str, 1, w8 * n, w8 * n, false);
        split_jobs(jobs, alpha_cont, d_ac, 1, w8 * n, w8 * n, false);
        // (a 1-row job wider than a staging buffer is cut by bytes: rows of 1 MiB)
        {
            std::vector<CopyJob> cut;
            for (const CopyJob &j : jobs)
                if (j.rows == 1 && j.width > kCopyChunk) {
                    const size_t piece = (size_t)1 << 20;
                    split_jobs(cut, j.host_src, j.dev, j.width / piece, piece, piece, false);
                    const size_t done = j.width / piece * piece;
                    if (done < j.width) split_jobs(cut, j.host_src + done, j.dev + done, 1, j.width - done, j.width - done, false);
                } else
                    cut.push_back(j);
            jobs.swap(cut);
        }
        split_jobs(jobs, lambda, d_lam, 1, w8 * nl, w8 * nl, false);
        if ((rc = run_copy_jobs(p, jobs, false, nullptr, st, g->device))) return rc;
#ifdef VRT_DIAG
        const auto t1 = std::chrono::steady_clock::now();
#endif
        // α_tot of every angle straight into the native layout (lambda_iteration.jl:72-80, :89, :93-96)
        if ((rc = launch_line_opacity(p, nlam, d_lam, lambda0, c0, d_vel, d_dop, d_gam, d_str, d_ac, p->ws_AA, st))) return rc;
        jobs.clear();
        split_jobs(jobs, S, p->d_stage[0], n, w8 * nl, w8 * (size_t)ld, false);
        if (dU) split_jobs(jobs, I0_up, dU, (size_t)g->up.n1, w8 * nl, w8 * nl, false);
        if (dD) split_jobs(jobs, I0_down, dD, (size_t)g->down.n1, w8 * nl, w8 * nl, false);
        if ((rc = run_copy_jobs(p, jobs, false, nullptr, st, g->device))) return rc;
#ifdef VRT_DIAG
        const auto t2 = std::chrono::steady_clock::now();
#endif
        // (the execute reuses ws_AA only for the CALLER-layout per-angle alpha, not for the native one)
        rc = execute_locked(p, caller_args(nlam, nlam, p->d_stage[0], p->ws_AA, VRT_ALPHA_ANGLE_NATIVE, dU, dD, weights,
                                           p->d_stage[4], nullptr, st, false));
        if (rc) return rc;
        VRT_HIP_TRY(hipEventRecord(p->copy_done, st));
#ifdef VRT_DIAG
        const auto t3 = std::chrono::steady_clock::now();
        (void)hipStreamSynchronize(st);
        const auto t4 = std::chrono::steady_clock::now();
#endif
        jobs.clear();
        split_jobs(jobs, J, p->d_stage[4], n, w8 * nl, w8 * (size_t)ld, true);
        if ((rc = run_copy_jobs(p, jobs, true, p->copy_done, st, g->device))) return rc;
#ifdef VRT_DIAG
        {
            const auto t5 = std::chrono::steady_clock::now();
            auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
            std::fprintf(stderr, "[vrt execute_line] lanes %d: vectors up %.1f ms, S staged %.1f ms, launches %.1f ms, wait for the sweep %.1f ms, J down %.1f ms\n",
                         lanes, ms(t0, t1), ms(t1, t2), ms(t2, t3), ms(t3, t4), ms(t4, t5));
        }
#endif
        VRT_HIP_TRY(hipStreamSynchronize(st));
        return patch_chain_check(p);         // a chained sweep that gave up waiting: THIS call's J is invalid
    });
}

static int lambda_create(vrt_plan *p, const vrt_line_case *lc, const double *weights, vrt_lambda **out, bool f32)
{
    if (!out) return fail(VRT_EINVAL, "out is NULL");
    *out = nullptr;
    if (!p || !lc || !weights) return fail(VRT_EINVAL, "NULL argument");
    if (int rc = check_line_case(lc)) return rc;
    const int64_t nlam = lc->nlam;
    return guarded([&] {
        std::lock_guard<std::mutex> lock(p->mu);
        vrt_grid *g = p->g;
        int rc = use_device(g->device);
        if (rc) return rc;
        if ((rc = line_session_plan_ok(p, f32))) return rc;
        std::unique_ptr<vrt_lambda, LambdaDelete> s(new vrt_lambda());
        s->p = p;
        s->device = g->device;
        s->n = g->n;
        s->nlam = nlam;
        s->weights.assign(weights, weights + p->n_angles_user);
        const size_t n = (size_t)g->n;
        hipStream_t st = g->stream;
        const SourceStore::Form form = f32 ? SourceStore::kPlanesF32
                                           : SourceStore::plan_keeps_planes(p) ? SourceStore::kPlanes : SourceStore::kRows;
        if ((rc = s->line.create(lc, g->n, st)) || (rc = s->blk.create(p, lc->B0, nlam, 0, nlam, form, st)) ||
            (rc = upload(s->d_pops, lc->lte_populations, 3 * n, st)) ||      // populations = copy(LTE_pops), :232
            (rc = s->d_pops_new.alloc(3 * n)) || (rc = s->d_scalars.alloc(kUpdateWords)))
            return rc;
        if (hipStreamSynchronize(st) != hipSuccess)                         // the host arrays may go after return
            return fail(VRT_ENODEVICE, "uploading the line case failed");
        *out = s.release();
        return VRT_OK;
    });
}

int vrt_lambda_create(vrt_plan *p, const vrt_line_case *lc, const double *weights, vrt_lambda **out)
{
    return lambda_create(p, lc, weights, out, false);
}

int vrt_lambda_create_f32(vrt_plan *p, const vrt_line_case *lc, const double *weights, vrt_lambda **out)
{
    return lambda_create(p, lc, weights, out, true);
}

int vrt_lambda_storage(const vrt_lambda *s)
{
    return !s ? fail(VRT_EINVAL, "NULL session") : s->blk.sj.form() == SourceStore::kPlanesF32 ? 4 : 8;
}

int vrt_lambda_iterate(vrt_lambda *s, double *max_rel_change)
{
    if (!s || !max_rel_change) return fail(VRT_EINVAL, "NULL argument");
    return guarded([&] {
        vrt_plan *p = s->p;
        std::lock_guard<std::mutex> lock(p->mu);
        vrt_grid *g = p->g;
        int rc = use_device(g->device);
        if (rc) return rc;
        hipStream_t st = g->stream;
        // α, Λ* with the operator on (d_diag is NULL otherwise), the sweep and the update: the block's
        RatesJ J;
        if ((rc = s->blk.step(p, s->line, s->d_pops, s->weights.data(), s->d_scalars, s->d_diag, st, &J))) return rc;
        // R, populations (:269, :274) from the same J
        if ((rc = launch_rates_populations(s->line.rates_in(), J, s->line.d_R, s->d_pops_new, st))) return rc;
        std::swap(s->d_pops, s->d_pops_new);
        double crit;
        int64_t fallback = 0;                                // (the third word: the ALI update's, in the same copy)
        if ((rc = read_criterion(s->d_scalars, s->op ? 3 : 2, st, &crit, &fallback))) return rc;
        if ((rc = patch_chain_check(p))) return rc;          // a chained sweep that gave up: THIS iteration's results are invalid
        *max_rel_change = crit;
        s->fallback_last = fallback;
        s->iterations++;
        // history copy or Ng step on the S of the plain update (the up-order copy); an accepted x_acc becomes that copy and
        // the down-order copy is rewritten from it, value for value
        return ng_after_update(s->ng, s->iterations, s->blk.sj, st);
    });
}

int vrt_lambda_set_acceleration(vrt_lambda *s, int order, int start, int period)
{
    if (!s) return fail(VRT_EINVAL, "NULL session");
    int rc = ng_check_settings(order, start, period);
    if (rc) return rc;
    return guarded([&] {
        vrt_plan *p = s->p;
        std::lock_guard<std::mutex> lock(p->mu);
        if ((rc = s->blk.sj.ng_check()) || (rc = use_device(p->g->device))) return rc;
        return ng_configure(s->ng, order, start, period, s->blk.sj.ng_count());
    });
}

int vrt_lambda_use_operator(vrt_lambda *s, int op)
{
    if (!s) return fail(VRT_EINVAL, "NULL session");
    if (op != 0 && op != 1) return fail(VRT_EINVAL, "operator must be 0 (plain) or 1 (diagonal)");
    return guarded([&] {
        vrt_plan *p = s->p;
        std::lock_guard<std::mutex> lock(p->mu);
        if (s->blk.sj.form() == SourceStore::kPlanesF32)
            return fail(VRT_EINVAL, "vrt_lambda_use_operator: not on a float-storage session (the ALI update works on double arrays)");
        int rc = use_device(p->g->device);
        if (rc) return rc;
        if (op == s->op) return (int)VRT_OK;
        if (op) {
            if ((rc = s->blk.sj.alloc_beside(s->d_diag))) return rc;
        } else
            s->d_diag.reset();
        s->op = op;
        s->fallback_last = 0;
        return (int)VRT_OK;
    });
}

int vrt_lambda_get_operator(const vrt_lambda *s, int *op, int64_t *fallback_entries_last_iterate)
{
    if (!s || !op) return fail(VRT_EINVAL, "NULL argument");
    *op = s->op;
    if (fallback_entries_last_iterate) *fallback_entries_last_iterate = s->fallback_last;
    return VRT_OK;
}

int vrt_lambda_last_acceleration(const vrt_lambda *s, int *applied, double sums[5], double coeffs[2])
{
    if (!s || !applied) return fail(VRT_EINVAL, "NULL argument");
    return ng_report(s->ng, applied, sums, coeffs);
}

int vrt_lambda_get(vrt_lambda *s, double *J, double *S, double *populations, double *R, double *gamma)
{
    if (!s) return fail(VRT_EINVAL, "NULL session");
    return guarded([&] {
        vrt_plan *p = s->p;
        std::lock_guard<std::mutex> lock(p->mu);
        int rc = use_device(p->g->device);
        if (rc) return rc;
        const size_t n = (size_t)s->n;
        if ((rc = s->blk.sj.download(J, S, s->nlam, 0, p->g->stream))) return rc;
        if (populations) VRT_HIP_TRY(hipMemcpy(populations, s->d_pops, sizeof(double) * 3 * n, hipMemcpyDeviceToHost));
        if (R) VRT_HIP_TRY(hipMemcpy(R, s->line.d_R, sizeof(double) * 9 * n, hipMemcpyDeviceToHost));
        if (gamma) VRT_HIP_TRY(hipMemcpy(gamma, s->line.d_gamma, sizeof(double) * n, hipMemcpyDeviceToHost));
        return VRT_OK;
    });
}

int vrt_lambda_set_state(vrt_lambda *s, const double *S, const double *populations)
{
    int rc = check_state_pointers(s, S, populations);
    if (rc || (rc = check_state(s->n, s->nlam, S, populations))) return rc;
    return guarded([&] {
        vrt_plan *p = s->p;
        std::lock_guard<std::mutex> lock(p->mu);
        if ((rc = use_device(p->g->device))) return rc;
        hipStream_t st = p->g->stream;
        // staged copies beside the session: it is untouched until every one of them is complete
        SourceStore::Staged staged;
        DevBuf<double> pops;
        if (S && (rc = s->blk.sj.stage(S, s->nlam, 0, staged, st))) return rc;
        if (populations && (rc = upload(pops, populations, 3 * (size_t)s->n, st))) return rc;
        VRT_HIP_TRY(hipStreamSynchronize(st));               // the host arrays may go after return
        if (S) s->blk.sj.adopt(staged);
        if (populations) std::swap(s->d_pops, pops);
        s->ng.have = 0;                                      // iterates of another state are no history of this one
        s->ng.last_applied = 0;
        return VRT_OK;
    });
}

void vrt_lambda_destroy(vrt_lambda *s)
{
    DeviceScope scope;
    if (s) (void)hipSetDevice(s->device);
    delete s;
}

}  // extern "C"
