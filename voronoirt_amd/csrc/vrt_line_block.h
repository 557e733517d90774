// One block of consecutive wavelengths of a line Λ-iteration session on a vrt_plan, and what one iterate does with it up
// to the rate integrals.  vrt_lambda (vrt_lambda.cpp) holds ONE block of all its wavelengths; every member of
// vrt_multi_lambda (vrt_multi.cpp) holds the block [l0, l1) of its device.  The block owns S and J (a SourceStore), B_0 in
// the store's order, I_0 of the up sweeps and the native per-angle α, the last three as doubles or -- float storage -- as
// floats.  What is NOT here: the line case (LineCaseDev, whole in every session), the populations, the criterion's words,
// Λ* (the caller's, handed to step) and everything after the update: the one-device session goes on with
// launch_rates_populations, the multi-device one with launch_rates_partial and the all-reduce.  Inline host code, like
// vrt_source_store.h: tests/probes/line_block_main.cpp compiles it against a fake runtime.
#pragma once

#include "vrt_line_case.h"
#include "vrt_source_store.h"

namespace vrt {

// Can a line session (float storage: f32) be made on this plan?
inline int line_session_plan_ok(const vrt_plan *p, bool f32)
{
    if (int rc = line_path_ok(p, "the line session")) return rc;
    if (p->A != (int)p->n_angles_user)
        return fail(VRT_EINVAL, "per-angle alpha needs every angle active (no θ = 90 direction)");
    if (!f32) return VRT_OK;
    if (int rc = native_planes_ok(p, true)) return rc;      // float planes exist on the patch path only: no fp64 fallback
    if (p->tune.lambda_native == 0 || (p->tune.path != 0 && p->tune.path != 4))
        return fail(VRT_EINVAL, "the float-storage line session keeps S and J in the patch path's sweep order: not with VRT_LAMBDA_NATIVE=0 or a VRT_PATH other than patches");
    return VRT_OK;
}

struct LineBlock {
    int64_t l0 = 0, l1 = 0;             // the block's wavelengths among the case's
    bool f32 = false;                   // float storage (kept here: an empty block has no store to ask)
    SourceStore sj;                     // S and J of the block (an empty block: never created, holds nothing)
    DevBuf<double> d_B0, d_I0, d_native;    // B_0 in the store's order (rows, or its up-order plane set), I_0, the native α
    DevBuf<float> f_B0, f_I0, f_native;     // float storage: these replace the three above (B_0 rounded once)

    int64_t nb() const { return l1 - l0; }
    // in the storage type, as a sweep takes them
    void *alpha() const { return f32 ? (void *)f_native.get() : (void *)d_native.get(); }
    const void *I0() const { return f32 ? (const void *)f_I0.get() : (const void *)d_I0.get(); }

    // Columns [l0, l1) of the host rows B0 (n, nlam): S = B_0 (S_new = B_0, S_old = zero(S_new), lambda_iteration.jl:236-240),
    // I_0 = B_λ of the bottom layer (:99-101) gathered in the storage type, room for the native α, and B_0 put into the
    // store's order; enqueued on `st` (B0 may go once it is synchronised).  An empty block holds one-element placeholders
    // and no store.  A block that fails to come up holds nothing, and `*this` is what it was.
    int create(vrt_plan *p, const double *B0, int64_t nlam, int64_t l0_, int64_t l1_, SourceStore::Form form, hipStream_t st)
    {
        LineBlock t;
        t.l0 = l0_; t.l1 = l1_; t.f32 = form == SourceStore::kPlanesF32;
        const vrt_grid *g = p->g;
        const int64_t nb = t.nb();
        int rc;
        if ((rc = upload_cols(t.d_B0, B0, (size_t)g->n, nlam, l0_, l1_, st))) return rc;
        if (nb && (rc = t.sj.create(p, nb, form, t.d_B0, st))) return rc;
        const size_t nI0 = (size_t)g->up.n1 * (size_t)nb, nnat = nb ? (size_t)vrt_plan_native_alpha_count(p, nb) : 1;
        if ((rc = t.f32 ? t.f_I0.alloc(nI0) : t.d_I0.alloc(nI0)) || (rc = t.f32 ? t.f_native.alloc(nnat) : t.d_native.alloc(nnat)))
            return rc;
        if (nb) {
            rc = t.f32 ? launch_gather_rows_f32(g->up.n1, nb, nb, g->up.d_order, t.d_B0, t.f_I0, st)
                       : launch_gather_rows(g->up.n1, nb, nb, g->up.d_order, t.d_B0, t.d_I0, st);
            if (rc || (rc = t.sj.to_up_order(t.d_B0, t.f_B0, st))) return rc;      // (float storage: the staged doubles go)
        }
        *this = std::move(t);
        return VRT_OK;
    }

    // One iterate from the populations `d_pops` up to the update, enqueued on `st` (the caller holds p->mu):
    //   S_old = copy(S_new) in rows (:258); γ and the line strength of d_pops (:72-75, line.jl:219-225) and α_tot of
    //   every angle (:89-96); with d_diag, Λ* of that α into it (vrt_line_ali.hip: rows, or one up-order plane set);
    //   J_λ (:84-111); S_new = (1 - ε) J + ε B_0 and the criterion's words into d_scalars (:261-263, :325-349) -- in sweep
    //   order the update reads the old S where it writes the new, and with d_diag it is the ALI update (a third word).
    // *J: where the rate integrals read this block's J.  An empty block runs the line terms and nothing else; its J is an
    // empty range of rows.
    int step(vrt_plan *p, LineCaseDev &line, const double *d_pops, const double *weights, unsigned long long *d_scalars,
             double *d_diag, hipStream_t st, RatesJ *J)
    {
        const int64_t n = line.n, nb_ = nb();
        const bool rows = sj.form() == SourceStore::kRows;
        int rc;
        if (nb_ > 0 && rows)
            VRT_HIP_TRY(hipMemcpyAsync(sj.S_old(), sj.S_new(), sizeof(double) * (size_t)n * (size_t)nb_, hipMemcpyDeviceToDevice, st));
        if ((rc = line.terms(d_pops, st))) return rc;
        *J = RatesJ::from_rows(nullptr, std::max<int64_t>(nb_, 1));
        if (nb_ == 0) return VRT_OK;
        if ((rc = line.opacity(p, nb_, l0, alpha(), st, f32))) return rc;
        if (d_diag && (rc = launch_line_lambda_diagonal(p, nb_, d_native, weights, nb_, rows ? d_diag : nullptr,
                                                        rows ? nullptr : d_diag, st)))
            return rc;
        if ((rc = execute_locked(p, sj.exec_args(alpha(), VRT_ALPHA_ANGLE_NATIVE, I0(), weights, st)))) return rc;
        switch (sj.form()) {
        case SourceStore::kPlanesF32:                        // (the roundings: include/voronoirt.h)
            *J = RatesJ::from_planes_f32(p, sj.J_plane<float>(0), sj.J_plane<float>(1));
            return launch_lambda_update_native_f32(p, nb_, sj.J_plane<float>(0), sj.J_plane<float>(1), f_B0, line.d_eps,
                                                   sj.S_plane<float>(0), sj.S_plane<float>(1), d_scalars, st);
        case SourceStore::kPlanes:
            *J = RatesJ::from_planes(p->g, sj.J_plane(0), sj.J_plane(1));
            return launch_lambda_update_native(p->g, nb_, sj.J_plane(0), sj.J_plane(1), d_B0, line.d_eps, sj.S_plane(0),
                                               sj.S_plane(1), d_scalars, st, d_diag);
        case SourceStore::kRows:
            *J = RatesJ::from_rows(sj.J_rows(), nb_);
            return launch_lambda_update(n, nb_, nb_, sj.J_rows(), d_B0, line.d_eps, sj.S_old(), sj.S_new(), d_scalars, st, d_diag);
        }
        return VRT_OK;
    }
};

}  // namespace vrt
