// The source function S and the mean intensity J of a device-resident Λ-iteration session on a vrt_plan: vrt_lambda
// (vrt_lambda.cpp) and every member of vrt_multi_lambda (vrt_multi.cpp) -- inside their LineBlock, vrt_line_block.h -- and
// vrt_continuum (vrt_continuum.hip) keep theirs in a SourceStore.  The storage form is chosen once, at create, and is the store's business from then on:
//   kRows       the caller's layout, (n, nlam) rows of doubles: S_new, S_old and J (VRT_LAMBDA_NATIVE=0, or a plan without
//               sweep-order planes: two layout changes per sweep)
//   kPlanes     sweep order, doubles: one plane set ([pairs][n][2], vrt_plan_native_plane_count) of S and of J per
//               direction.  The update writes S where the sweep reads it and the sweep reduces J where the update and the
//               rate integrals read it; the up-order S is THE S (what Ng works on and what goes home), the down-order
//               one its copy, value for value.  The padding wavelength of an odd nlam is zero.
//   kPlanesF32  the same plane sets as floats in the pair blocks of the plan's float layout (the patch path only); what
//               goes home is widened on the device, what comes in is rounded to float once
// A session sees the form only where it must pick a kernel (one switch in its iterate).  Inline host code, like the Ng
// phases of vrt_internal.h: tests/probes/source_store_main.cpp compiles it against a fake runtime.
#pragma once

#include <type_traits>

#include "vrt_internal.h"

namespace vrt {

struct SourceStore {
    enum Form { kRows, kPlanes, kPlanesF32 };

    // Does a session on this plan keep sweep-order planes (kPlanes) rather than rows?  (The line sessions refuse a plan with
    // an inactive angle before they ask, so `A > 0` is the continuum's guard and always true for them.)
    static bool plan_keeps_planes(const vrt_plan *p)
    {
        return p->tune.lambda_native != 0 && p->A > 0 && native_planes_ok(p) == VRT_OK && p->tune.path != 1 && p->tune.path != 2;
    }

    // A host S staged beside a store (stage), complete once `st` is synchronised; adopt() then makes it the store's.
    struct Staged {
        DevBuf<double> rows, S[2];
        DevBuf<float> rows_f, Sf[2];
    };

    Form form() const { return form_; }
    bool two_orders() const { return form_ != kRows; }      // a down-order copy of S follows the up-order one

    // S = B_0 (device rows (n, nlam)), J = 0 and -- rows -- S_old = 0, enqueued on `st`.  A store that fails to come up
    // holds nothing, and `*this` is what it was.
    int create(vrt_plan *p, int64_t nlam, Form form, const double *d_B0, hipStream_t st)
    {
        SourceStore t;
        t.p_ = p; t.n_ = p->g->n; t.nlam_ = nlam; t.form_ = form;
        t.rows_ = (size_t)t.n_ * (size_t)nlam;
        t.planes_ = form == kRows ? 0 : (size_t)vrt_plan_native_plane_count(p, nlam);
        int rc = t.fill(d_B0, st);
        if (rc) return rc;
        *this = std::move(t);
        return VRT_OK;
    }

    // ---- what a sweep, an update and the rate integrals are handed ---------------------------------------------------
    // one sweep from the current S into J; I_0 of the down sweeps is zero in every session
    ExecArgs exec_args(const void *alpha, int alpha_mode, const void *I0_up, const double *weights, hipStream_t st) const
    {
        if (form_ == kRows)
            return caller_args(nlam_, nlam_, S_[0], alpha, alpha_mode, I0_up, nullptr, weights, J_[0], nullptr, st, false);
        if (form_ == kPlanesF32)
            return native_args(nlam_, Sf_[0], Sf_[1], alpha, alpha_mode, I0_up, nullptr, weights, Jf_[0], Jf_[1], st, true);
        return native_args(nlam_, S_[0], S_[1], alpha, alpha_mode, I0_up, nullptr, weights, J_[0], J_[1], st, false);
    }
    // planes (T: double, or float in kPlanesF32): 0 up, 1 down
    template <typename T = double> T *S_plane(int dir) const { return pick<T>(S_, Sf_, dir, form_ != kRows); }
    template <typename T = double> T *J_plane(int dir) const { return pick<T>(J_, Jf_, dir, form_ != kRows); }
    // rows; NULL in the plane forms, as the launches that take either expect
    double *S_new() const { return form_ == kRows ? S_[0].p : nullptr; }
    double *S_old() const { return form_ == kRows ? S_[1].p : nullptr; }
    double *J_rows() const { return form_ == kRows ? J_[0].p : nullptr; }
    void swap_rows() { std::swap(S_[0].p, S_[1].p); }       // an update that wrote S_old: the two change roles

    // ---- arrays that stand beside S in an update: B_0, ε, Λ* -----------------------------------------------------------
    // The up-order plane set of (n, nlam) device rows into `up`, enqueued on `st`.  kRows: `up` stays empty, the update
    // reads the rows as they are.
    int up_order_of(const double *rows, DevBuf<double> &up, hipStream_t st) const
    {
        if (form_ == kRows) return VRT_OK;
        if (form_ == kPlanesF32) return fail(VRT_EINVAL, "a float-storage store has no double planes");
        int rc = up.alloc(planes_);
        return rc ? rc : planes_to_native(p_, nlam_, nlam_, rows, up, nullptr, st);
    }
    // Room for an array that a kernel writes in this store's form (a line session's Λ*): rows, or one up-order plane set
    int alloc_beside(DevBuf<double> &a) const
    {
        if (form_ == kPlanesF32) return fail(VRT_EINVAL, "a float-storage store has no double planes");
        return a.alloc(form_ == kRows ? rows_ : planes_);
    }
    // The same in place: `a` holds rows and -- kPlanes -- is replaced by its up-order plane set.  kPlanesF32: rounded to
    // float once, the up-order plane set of that in `af`, `a` released.  Synchronises `st` where a buffer goes.
    int to_up_order(DevBuf<double> &a, DevBuf<float> &af, hipStream_t st) const
    {
        int rc;
        if (form_ == kPlanesF32) {
            DevBuf<float> rf, up;
            if ((rc = rf.alloc(rows_)) || (rc = up.alloc(planes_))) return rc;
            if ((rc = launch_round_to_f32(rows_, a, rf, st))) return rc;
            if ((rc = planes_to_native_f32(p_, nlam_, nlam_, rf, up, nullptr, st))) return rc;
            VRT_HIP_TRY(hipStreamSynchronize(st));
            af = std::move(up);
            a.reset();
            return VRT_OK;
        }
        DevBuf<double> up;
        if ((rc = up_order_of(a, up, st)) || !up) return rc;
        VRT_HIP_TRY(hipStreamSynchronize(st));
        a = std::move(up);
        return VRT_OK;
    }
    int to_up_order(DevBuf<double> &a, hipStream_t st) const
    {
        if (form_ == kPlanesF32) return fail(VRT_EINVAL, "a float-storage store has no double planes");
        DevBuf<float> none;
        return to_up_order(a, none, st);
    }
    // α per (site, wavelength) as the sweeps of this form take it; `a` holds rows.  kRows: it stays (VRT_ALPHA_SITE_LAM);
    // kPlanes: both orders, one behind the other (VRT_ALPHA_SITE_LAM_NATIVE).  Synchronises `st` where a buffer goes.
    int to_sweep_alpha(DevBuf<double> &a, int *alpha_mode, hipStream_t st) const
    {
        *alpha_mode = VRT_ALPHA_SITE_LAM;
        if (form_ == kRows) return VRT_OK;
        if (form_ == kPlanesF32) return fail(VRT_EINVAL, "a float-storage store has no double planes");
        DevBuf<double> both;
        int rc = both.alloc(2 * planes_);
        if (rc) return rc;
        if ((rc = planes_to_native(p_, nlam_, nlam_, a, both, both + planes_, st))) return rc;
        VRT_HIP_TRY(hipStreamSynchronize(st));
        a = std::move(both);
        *alpha_mode = VRT_ALPHA_SITE_LAM_NATIVE;
        return VRT_OK;
    }
    // the way back, value for value: *rows is `a` itself (kRows), or `tmp`, filled on `st` from a's up-order plane set
    int rows_of(const double *a, DevBuf<double> &tmp, const double **rows, hipStream_t st) const
    {
        *rows = a;
        if (form_ == kRows) return VRT_OK;
        if (form_ == kPlanesF32) return fail(VRT_EINVAL, "a float-storage store has no double planes");
        int rc = tmp.alloc(rows_);
        if (rc) return rc;
        *rows = tmp;
        return plane_from_native(p_, 0, nlam_, nlam_, a, tmp, st);
    }

    // ---- home and back ----------------------------------------------------------------------------------------------
    // J and / or S into columns [col0, col0 + nlam) of host rows `ld` doubles apart; complete on return.  The plane forms
    // go through scratch that exists only here; float planes are widened on the device (exact).
    int download(double *J, double *S, int64_t ld, int64_t col0, hipStream_t st) const
    {
        if ((!J && !S) || !rows_) return VRT_OK;
        if (form_ == kRows) {
            if (J) VRT_HIP_TRY(copy_cols(J, ld, col0, J_[0], false, st));
            if (S) VRT_HIP_TRY(copy_cols(S, ld, col0, S_[0], false, st));
            VRT_HIP_TRY(hipStreamSynchronize(st));
            return VRT_OK;
        }
        DevBuf<float> tf;
        DevBuf<double> tmp;
        int rc;
        if (form_ == kPlanesF32 && (rc = tf.alloc(rows_))) return rc;
        if ((rc = tmp.alloc(rows_))) return rc;
        for (int which = 0; which < 2; which++) {
            double *host = which == 0 ? J : S;
            if (!host) continue;
            if (form_ == kPlanesF32) {
                rc = which == 0 ? J_from_native_f32(p_, nlam_, nlam_, Jf_[0], Jf_[1], tf, st)
                                : plane_from_native_f32(p_, 0, nlam_, nlam_, Sf_[0], tf, st);
                if (!rc) rc = launch_widen_f32(rows_, tf, tmp, st);
            } else
                rc = which == 0 ? J_from_native(p_, nlam_, nlam_, J_[0], J_[1], tmp, st)
                                : plane_from_native(p_, 0, nlam_, nlam_, S_[0], tmp, st);
            if (rc) return rc;
            VRT_HIP_TRY(copy_cols(host, ld, col0, tmp, false, st));
            VRT_HIP_TRY(hipStreamSynchronize(st));           // (tmp is written again, then goes)
        }
        return VRT_OK;
    }

    // Columns [col0, col0 + nlam) of a host S (rows `ld` doubles apart) into `sg`, in this store's form: rounded to float
    // if it keeps floats, both orders if it keeps planes, the padding wavelength of an odd nlam zero as at create.
    // Enqueued on `st`; the store itself is not touched.
    int stage(const double *S, int64_t ld, int64_t col0, Staged &sg, hipStream_t st) const
    {
        DevBuf<double> &rows = form_ == kRows ? sg.S[0] : sg.rows;
        int rc = rows.alloc(rows_);
        if (rc) return rc;
        VRT_HIP_TRY(copy_cols(const_cast<double *>(S), ld, col0, rows, true, st));
        if (form_ == kPlanesF32) {
            if ((rc = sg.rows_f.alloc(rows_)) || (rc = sg.Sf[0].alloc(planes_)) || (rc = sg.Sf[1].alloc(planes_))) return rc;
            if ((rc = launch_round_to_f32(rows_, rows, sg.rows_f, st))) return rc;
            return planes_to_native_f32(p_, nlam_, nlam_, sg.rows_f, sg.Sf[0], sg.Sf[1], st);
        }
        if (form_ == kPlanes) {
            if ((rc = sg.S[0].alloc(planes_)) || (rc = sg.S[1].alloc(planes_))) return rc;
            return planes_to_native(p_, nlam_, nlam_, rows, sg.S[0], sg.S[1], st);
        }
        return VRT_OK;
    }
    // a staged S whose copies are complete becomes the store's (pointer swaps only); the old one goes with `sg`
    void adopt(Staged &sg)
    {
        const int orders = form_ == kRows ? 1 : 2;
        for (int d = 0; d < orders; d++) {
            if (form_ == kPlanesF32) std::swap(Sf_[d], sg.Sf[d]);
            else std::swap(S_[d], sg.S[d]);
        }
    }

    // ---- what Ng acceleration works on: THE S, its doubles (padding included), which of them are physical -----------------
    int ng_check() const
    {
        if (form_ == kPlanesF32)                             // the Ng kernels and NgRange: the [pair][pos][2] double layout
            return fail(VRT_EINVAL, "vrt_lambda_set_acceleration: not on a float-storage session (the Ng kernels work on double planes)");
        return VRT_OK;
    }
    DevBuf<double> &ng_S() { return S_[0]; }
    size_t ng_count() const { return form_ == kRows ? rows_ : planes_; }
    NgRange ng_range() const { return ng_S_range(n_, nlam_, form_ != kRows); }
    // after an accepted step (two_orders() only): the down-order copy rewritten from the up-order one, enqueued on `st`
    int mirror_down(hipStream_t st) { return launch_ng_mirror(p_->g, nlam_, S_[0], S_[1], st); }
    // ... as ng_after_update (vrt_internal.h) asks for it: rows have nothing that follows S, and queue nothing
    int ng_refresh(hipStream_t st, bool *queued)
    {
        *queued = two_orders();
        return *queued ? mirror_down(st) : VRT_OK;
    }

private:
    vrt_plan *p_ = nullptr;             // borrowed, as the session borrows it
    int64_t n_ = 0, nlam_ = 0;
    Form form_ = kRows;
    size_t rows_ = 0, planes_ = 0;      // elements of a rows array, of one plane set
    DevBuf<double> S_[2], J_[2];        // planes: [0] up, [1] down; rows: S_new, S_old and J, -
    DevBuf<float> Sf_[2], Jf_[2];

    template <typename T>
    static T *pick(const DevBuf<double> *d, const DevBuf<float> *f, int i, bool have)
    {
        if (!have) return nullptr;
        if constexpr (std::is_same<T, float>::value) return f[i].p;
        else return d[i].p;
    }

    // columns [col0, col0 + nlam) of host rows <-> dense device rows (n, nlam), on `st`
    hipError_t copy_cols(double *host, int64_t ld, int64_t col0, double *dev, bool to_device, hipStream_t st) const
    {
        const size_t w = sizeof(double) * (size_t)nlam_, pitch = sizeof(double) * (size_t)ld;
        const hipMemcpyKind kind = to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
        if (ld == nlam_) return to_device ? hipMemcpyAsync(dev, host, w * (size_t)n_, kind, st) : hipMemcpyAsync(host, dev, w * (size_t)n_, kind, st);
        return to_device ? hipMemcpy2DAsync(dev, w, host + col0, pitch, w, (size_t)n_, kind, st)
                         : hipMemcpy2DAsync(host + col0, pitch, dev, w, w, (size_t)n_, kind, st);
    }

    int fill(const double *d_B0, hipStream_t st)
    {
        int rc;
        if (form_ == kRows) {
            if ((rc = S_[0].alloc(rows_)) || (rc = S_[1].alloc(rows_)) || (rc = J_[0].alloc(rows_))) return rc;
            if (!rows_) return VRT_OK;
            VRT_HIP_TRY(hipMemcpyAsync(S_[0], d_B0, sizeof(double) * rows_, hipMemcpyDeviceToDevice, st));
            VRT_HIP_TRY(hipMemsetAsync(S_[1], 0, sizeof(double) * rows_, st));
            VRT_HIP_TRY(hipMemsetAsync(J_[0], 0, sizeof(double) * rows_, st));
            return VRT_OK;
        }
        if (form_ == kPlanesF32) {
            // B_0 rounded to float once, then both orders; the caller-layout float copy is staging only
            DevBuf<float> B0f;
            if ((rc = B0f.alloc(rows_))) return rc;
            if ((rc = launch_round_to_f32(rows_, d_B0, B0f, st))) return rc;
            for (int d = 0; d < 2; d++) {
                if ((rc = Sf_[d].alloc(planes_)) || (rc = Jf_[d].alloc(planes_))) return rc;
                VRT_HIP_TRY(hipMemsetAsync(Jf_[d], 0, sizeof(float) * planes_, st));
            }
            if ((rc = planes_to_native_f32(p_, nlam_, nlam_, B0f, Sf_[0], Sf_[1], st))) return rc;
            VRT_HIP_TRY(hipStreamSynchronize(st));           // (B0f goes here)
            return VRT_OK;
        }
        for (int d = 0; d < 2; d++) {
            if ((rc = S_[d].alloc(planes_)) || (rc = J_[d].alloc(planes_))) return rc;
            VRT_HIP_TRY(hipMemsetAsync(J_[d], 0, sizeof(double) * planes_, st));
        }
        return planes_to_native(p_, nlam_, nlam_, d_B0, S_[0], S_[1], st);
    }
};

}  // namespace vrt
