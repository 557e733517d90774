// The source function S and the mean intensity J of a device-resident Λ-iteration session on a vrt_regular:
// vrt_regular_lambda (vrt_regular_lambda.hip) and vrt_regular_continuum (vrt_continuum.hip) keep theirs in a RasterStore.
// One storage form: S and J as (n, nlam) rows in Julia point order for the pointwise steps (the update, the rate integrals,
// Ng), and plane-major ([l][iz][iy][ix]) for the solves -- the current S's copy, which follows every change of S, and the J
// the solves reduce, which goes home to the rows once per iterate.  Beside them what the solves start from: the bottom
// planes of B_0 ([l][iy][ix], I_0 of the up solves) and one plane of zeros (the down solves).
// Inline host code, like SourceStore (vrt_source_store.h): tests/probes/raster_store_main.cpp compiles it against a fake
// runtime.
#pragma once

#include "vrt_regular.h"

namespace vrt {

struct RasterStore {
    // A host S staged beside a store (stage), complete once `st` is synchronised; adopt() then makes it the store's.
    struct Staged {
        DevBuf<double> rows, planes;
    };

    // S = B_0 (device rows (n, nlam)) in rows and planes, J = 0, the zero plane and B_0's bottom planes, enqueued on `st`.
    // A store that fails to come up holds nothing, and `*this` is what it was.
    int create(const vrt_regular *r, int64_t nlam, const double *d_B0, hipStream_t st)
    {
        RasterStore t;
        t.r_ = r; t.n_ = r->nz * r->nx * r->ny; t.nlam_ = nlam;
        t.rows_ = (size_t)t.n_ * (size_t)nlam;
        t.plane_ = (size_t)(r->nx * r->ny);
        int rc = t.fill(d_B0, st);
        if (rc) return rc;
        *this = std::move(t);
        return VRT_OK;
    }

    // ---- what a J pass and an update are handed -----------------------------------------------------------------------
    const double *S_planes() const { return S_pl_; }          // the current S, plane-major
    double *J_planes() const { return J_pl_; }                // where the solves reduce J
    const double *I0_planes() const { return I0_pl_; }
    const double *zero_plane() const { return zero_; }
    double *J_rows() const { return J_; }
    const double *S_rows() const { return S_[cur_]; }         // the current S
    double *S_next() const { return S_[cur_ ^ 1]; }           // where an update writes the new one

    // J of the solves into the rows
    int J_home(hipStream_t st) { return launch_from_planes(r_, nlam_, J_pl_, J_, st); }
    // an update that wrote S_next() is queued: that buffer is the current S, and the solves' copy follows it
    int S_written(hipStream_t st)
    {
        cur_ ^= 1;
        return launch_to_planes(r_, nlam_, S_[cur_], S_pl_, st);
    }
    // another plane-major array of the store's shape into rows (a line session's Λ*; the session owns both)
    int rows_from_planes(const double *pl, double *rows, hipStream_t st) const { return launch_from_planes(r_, nlam_, pl, rows, st); }

    // ---- home and back ----------------------------------------------------------------------------------------------
    // J and / or S into dense host rows; synchronises `st` first, complete on return
    int download(double *J, double *S, hipStream_t st) const
    {
        VRT_HIP_TRY(hipStreamSynchronize(st));
        if (J) VRT_HIP_TRY(hipMemcpy(J, J_, sizeof(double) * rows_, hipMemcpyDeviceToHost));
        if (S) VRT_HIP_TRY(hipMemcpy(S, S_[cur_], sizeof(double) * rows_, hipMemcpyDeviceToHost));
        return VRT_OK;
    }
    // A host S (dense rows) and its plane-major copy into `sg`, enqueued on `st`; the store itself is not touched.
    int stage(const double *S, Staged &sg, hipStream_t st) const
    {
        int rc;
        if ((rc = sg.rows.alloc(rows_)) || (rc = sg.planes.alloc(rows_))) return rc;
        VRT_HIP_TRY(hipMemcpyAsync(sg.rows, S, sizeof(double) * rows_, hipMemcpyHostToDevice, st));
        return launch_to_planes(r_, nlam_, sg.rows, sg.planes, st);
    }
    // a staged S whose copies are complete becomes the store's (pointer swaps only); the old one goes with `sg`
    void adopt(Staged &sg)
    {
        std::swap(S_[cur_], sg.rows);
        std::swap(S_pl_, sg.planes);
    }

    // ---- what Ng acceleration works on (the names of SourceStore: ng_after_update, vrt_internal.h) ---------------------------
    DevBuf<double> &ng_S() { return S_[cur_]; }
    size_t ng_count() const { return rows_; }
    NgRange ng_range() const { return ng_S_range(n_, nlam_, false); }
    // after an accepted step: the solves' copy made again from the rows, enqueued on `st`
    int ng_refresh(hipStream_t st, bool *queued)
    {
        *queued = true;
        return launch_to_planes(r_, nlam_, S_[cur_], S_pl_, st);
    }

private:
    const vrt_regular *r_ = nullptr;    // borrowed, as the session borrows it
    int64_t n_ = 0, nlam_ = 0;
    size_t rows_ = 0, plane_ = 0;       // elements of an (n, nlam) array, points of one xy plane
    DevBuf<double> S_[2], J_;           // rows; S_[cur_]: the current S
    int cur_ = 0;
    DevBuf<double> S_pl_, J_pl_, I0_pl_, zero_;     // plane-major, wavelength slowest

    int fill(const double *d_B0, hipStream_t st)
    {
        int rc;
        if ((rc = S_[0].alloc(rows_)) || (rc = S_[1].alloc(rows_)) || (rc = J_.alloc(rows_)) || (rc = S_pl_.alloc(rows_)) ||
            (rc = J_pl_.alloc(rows_)) || (rc = I0_pl_.alloc(plane_ * (size_t)nlam_)) || (rc = zero_.alloc(plane_)))
            return rc;
        VRT_HIP_TRY(hipMemcpyAsync(S_[0], d_B0, sizeof(double) * rows_, hipMemcpyDeviceToDevice, st));
        // (J is that of "no iteration yet": zeros)
        VRT_HIP_TRY(hipMemsetAsync(J_, 0, sizeof(double) * rows_, st));
        VRT_HIP_TRY(hipMemsetAsync(zero_, 0, sizeof(double) * plane_, st));
        if ((rc = launch_to_planes(r_, nlam_, d_B0, S_pl_, st))) return rc;
        return launch_bottom_planes(r_, nlam_, d_B0, I0_pl_, st);
    }
};

}  // namespace vrt
