// The line case of a Λ-iteration session: the atmosphere and atom data of a vrt_line_case that a session uploads once
// and reads in every iterate.  vrt_lambda (vrt_lambda.cpp), every member of vrt_multi_lambda (vrt_multi.cpp) and
// vrt_regular_lambda (vrt_regular_lambda.hip) keep theirs in a LineCaseDev; the argument checks, the layout of the
// wavelength-sized vector and the named arguments of the rate launches (vrt_physics.hip) stand here too, once.
// What is NOT here: B_0, I_0 and the native α (their shape differs per session; the Voronoi sessions keep them in a
// LineBlock, vrt_line_block.h, beside S and J), the populations, the criterion's
// scalars, the shares, events and Ng state, and every step of an iterate beyond the two launches that read nothing but
// this data and the current populations.  Inline host code, like vrt_source_store.h: tests/probes/line_case_main.cpp
// compiles it against a fake runtime.
#pragma once

#include "vrt_internal.h"

namespace vrt {

// ---- argument checks ----------------------------------------------------------------------------------------------------
inline int check_blocks(const int64_t blocks[6], int64_t nlam)
{
    for (int b = 0; b < 3; b++)
        if (blocks[2 * b] < 0 || blocks[2 * b + 1] > nlam || blocks[2 * b + 1] - blocks[2 * b] < 2)
            return fail(VRT_EINVAL, "each wavelength block needs at least two wavelengths inside [0, nlam)");
    return VRT_OK;
}

inline int check_line_case(const vrt_line_case *lc)
{
    if (lc->nlam < 2) return fail(VRT_EINVAL, "nlam must be >= 2");
    if (!lc->lambda || !lc->velocity || !lc->doppler_width || !lc->gamma_static || !lc->gamma_unsold || !lc->alpha_cont ||
        !lc->eps || !lc->temperature || !lc->atom_density || !lc->B0 || !lc->lte_populations || !lc->C || !lc->planck2 ||
        !lc->sigma_bf1 || !lc->sigma_bf2)
        return fail(VRT_EINVAL, "NULL array in the line case");
    if (int rc = check_blocks(lc->blocks, lc->nlam)) return rc;
    if (!(lc->lambda0 > 0) || !(lc->c0 > 0)) return fail(VRT_EINVAL, "lambda0 and c0 must be positive");
    return VRT_OK;
}

// ---- the wavelength-sized vector lambda | planck2 | sigma_bf1 | sigma_bf2 -------------------------------------------------
// lambda and planck2 of all nlam wavelengths, σ_bf per wavelength of the two bound-free blocks.  pack_small writes it,
// small_view reads it (host or device address alike); nothing else knows the offsets.
inline std::vector<double> pack_small(int64_t nlam, const int64_t blocks[6], const double *lambda, const double *planck2,
                                      const double *sigma_bf1, const double *sigma_bf2)
{
    std::vector<double> small;
    small.insert(small.end(), lambda, lambda + nlam);
    small.insert(small.end(), planck2, planck2 + nlam);
    small.insert(small.end(), sigma_bf1, sigma_bf1 + (blocks[3] - blocks[2]));
    small.insert(small.end(), sigma_bf2, sigma_bf2 + (blocks[5] - blocks[4]));
    return small;
}

struct SmallView {
    const double *lambda = nullptr, *planck2 = nullptr, *sigma_bf1 = nullptr, *sigma_bf2 = nullptr;
};
inline SmallView small_view(const double *small, int64_t nlam, const int64_t blocks[6])
{
    SmallView v;
    v.lambda = small;
    v.planck2 = small + nlam;
    v.sigma_bf1 = small + 2 * nlam;
    v.sigma_bf2 = v.sigma_bf1 + (blocks[3] - blocks[2]);
    return v;
}

// ---- the constants of a line case -------------------------------------------------------------------------------------
struct LineConstants {
    int64_t blocks[6] = {0, 0, 0, 0, 0, 0};     // [lo, hi) of the bb, bf-level-1, bf-level-2 wavelength blocks
    double lambda0 = 0, c0 = 0, strength_const = 0, Bij = 0, Bji = 0, sigma_bb_const = 0, hc_over_kB = 0, pref_ij = 0,
           pref_ji = 0;
};
inline LineConstants line_constants(const vrt_line_case *lc)
{
    LineConstants k;
    for (int q = 0; q < 6; q++) k.blocks[q] = lc->blocks[q];
    k.lambda0 = lc->lambda0; k.c0 = lc->c0; k.strength_const = lc->strength_const; k.Bij = lc->Bij; k.Bji = lc->Bji;
    k.sigma_bb_const = lc->sigma_bb_const; k.hc_over_kB = lc->hc_over_kB; k.pref_ij = lc->pref_ij; k.pref_ji = lc->pref_ji;
    return k;
}

// ---- what the rate launches are handed (vrt_physics.hip) ------------------------------------------------------------------
// the inputs: n sites, all nlam wavelengths (of the rates: strength_const, Bij and Bji are not read)
struct RatesIn {
    int64_t n = 0, nlam = 0;
    LineConstants k;
    SmallView small;                    // device
    const double *doppler = nullptr, *gamma = nullptr, *temperature = nullptr, *lte = nullptr, *C = nullptr,
                 *atom_density = nullptr;       // device, per site
};
// where J comes from: one of the three
struct RatesJ {
    const double *rows = nullptr;       // (nlam, n) in the sites' own order, `ld` values per site
    int64_t ld = 0;
    const double *up = nullptr, *down = nullptr;        // per sweep direction in sweep order (either may be NULL), ...
    const vrt_grid *grid = nullptr;                     // ... the orders of this grid
    const float *up_f = nullptr, *down_f = nullptr;     // the same plane sets as floats, in the pair blocks ...
    const vrt_plan *plan = nullptr;                     // ... of this plan's float layout

    static RatesJ from_rows(const double *J, int64_t ld) { RatesJ j; j.rows = J; j.ld = ld; return j; }
    static RatesJ from_planes(const vrt_grid *g, const double *J_up, const double *J_down)
    {
        RatesJ j; j.up = J_up; j.down = J_down; j.grid = g; return j;
    }
    static RatesJ from_planes_f32(const vrt_plan *p, const float *J_up, const float *J_down)
    {
        RatesJ j; j.up_f = J_up; j.down_f = J_down; j.plan = p; return j;
    }
};
// R (9 n) and the populations (3 n) of every site from J (rates.jl:154-201, populations.jl:191-221)
int launch_rates_populations(const RatesIn &in, const RatesJ &J, double *d_R, double *d_populations, hipStream_t st);
// one device's share of the six rate integrals: wavelengths [l0, l1) of the nlam; J holds those columns only (plane sets:
// l1 - l0 wavelengths at local index l - l0, float ones in the pair blocks the plan gives l1 - l0 wavelengths)
int launch_rates_partial(const RatesIn &in, const RatesJ &J, int64_t l0, int64_t l1, double *d_shares, hipStream_t st);
// R and the populations from the summed shares
int launch_populations_from_shares(int64_t n, const double *d_shares, const double *d_C, const double *d_atom_density,
                                   double *d_R, double *d_populations, hipStream_t st);

// ---- the uploaded line case -------------------------------------------------------------------------------------------
struct LineCaseDev {
    int64_t n = 0, nlam = 0;
    LineConstants k;
    DevBuf<double> d_small;             // pack_small's vector, of ALL nlam wavelengths
    DevBuf<double> d_velocity;          // 3 n
    DevBuf<double> d_doppler, d_gamma_static, d_gamma_unsold, d_alpha_cont, d_eps, d_temperature, d_atom;      // n each
    DevBuf<double> d_lte, d_C;          // 3 n, 9 n
    // per-site work arrays of an iterate: γ and the line strength of the current populations, the rates
    DevBuf<double> d_gamma, d_strength, d_R;            // n, n, 9 n

    // The uploads through `st`, complete on return (the host arrays may go), and the work arrays allocated.  An owner that
    // fails to come up holds nothing, and `*this` is what it was.
    int create(const vrt_line_case *lc, int64_t n_sites, hipStream_t st)
    {
        LineCaseDev t;
        t.n = n_sites; t.nlam = lc->nlam; t.k = line_constants(lc);
        const size_t sn = (size_t)n_sites;
        const std::vector<double> small = pack_small(lc->nlam, lc->blocks, lc->lambda, lc->planck2, lc->sigma_bf1, lc->sigma_bf2);
        int rc;
        if ((rc = upload(t.d_small, small.data(), small.size(), st)) || (rc = upload(t.d_velocity, lc->velocity, 3 * sn, st)) ||
            (rc = upload(t.d_doppler, lc->doppler_width, sn, st)) || (rc = upload(t.d_gamma_static, lc->gamma_static, sn, st)) ||
            (rc = upload(t.d_gamma_unsold, lc->gamma_unsold, sn, st)) || (rc = upload(t.d_alpha_cont, lc->alpha_cont, sn, st)) ||
            (rc = upload(t.d_eps, lc->eps, sn, st)) || (rc = upload(t.d_temperature, lc->temperature, sn, st)) ||
            (rc = upload(t.d_atom, lc->atom_density, sn, st)) || (rc = upload(t.d_lte, lc->lte_populations, 3 * sn, st)) ||
            (rc = upload(t.d_C, lc->C, 9 * sn, st)) || (rc = t.d_gamma.alloc(sn)) || (rc = t.d_strength.alloc(sn)) ||
            (rc = t.d_R.alloc(9 * sn)))
            return rc;
        VRT_HIP_TRY(hipStreamSynchronize(st));               // (`small` goes here)
        *this = std::move(t);
        return VRT_OK;
    }

    // γ and the line strength of the populations `d_pops` (n, 3) into d_gamma and d_strength
    int terms(const double *d_pops, hipStream_t st)
    {
        return launch_line_terms(n, d_gamma_static, d_gamma_unsold, d_pops, k.strength_const, k.Bij, k.Bji, d_gamma, d_strength, st);
    }
    // α_tot of every angle of `plan` for the nb wavelengths from l0, from the γ and strength of the last terms(), into the
    // plan's native layout (doubles, or floats with f32)
    int opacity(vrt_plan *plan, int64_t nb, int64_t l0, void *d_out, hipStream_t st, bool f32 = false)
    {
        return launch_line_opacity(plan, nb, d_small + l0, k.lambda0, k.c0, d_velocity, d_doppler, d_gamma, d_strength,
                                   d_alpha_cont, d_out, st, f32);
    }
    // the inputs of a rate launch: γ is that of the last terms()
    RatesIn rates_in() const
    {
        RatesIn in;
        in.n = n; in.nlam = nlam; in.k = k;
        in.small = small_view(d_small, nlam, k.blocks);
        in.doppler = d_doppler; in.gamma = d_gamma; in.temperature = d_temperature; in.lte = d_lte; in.C = d_C;
        in.atom_density = d_atom;
        return in;
    }
};

}  // namespace vrt
