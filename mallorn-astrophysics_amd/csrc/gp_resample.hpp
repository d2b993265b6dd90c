// gp_resample.hpp -- GP-resampled copies ("GP-resampled copies"): a copy keeps the rows (t, band, err) an
// augmentation plan gave it and gets fluxes drawn from its SOURCE's 2-D GP posterior at another redshift.  Two passes around
// the points stage of gp.hpp (which runs in fit mode on the source batch):
//   query   row i of copy c of source o asks the GP at t* = (t_i - shift_c - t_ref_o) / s_c and lambda* = lambda_band(i) / s_c,
//           s_c = (1 + z_new_c) / (1 + z_old_o); t_ref the source's reference time in the origin's frame
//   write   flux = dim_c (mu* + sd n1) + err_i noise_c n2,  err_out = sqrt(err_i^2 (1 + noise_c^2) + (dim_c sd)^2),
//           sd = sqrt(max(var*, 0)); n1, n2 standard normals, the caller's or Philox streams 4 and 5 of augment.hpp
// The copies of source o are objects o k .. o k + k - 1 of the copy batch, so the points of source o are the rows of its
// copies one after the other and point r IS row r of the copy batch: q_off[o] = copy_offsets[o k].
// This recipe has no counterpart in the reference; its arithmetic is defined here.  Plain fp64, no fused operations.
#pragma once
#include "augment.hpp"
#include "gp.hpp"

namespace lcfe {

enum { AUG_STREAM_GP_N1 = 4, AUG_STREAM_GP_N2 = 5 };

struct GpResSource {
    const int64_t* offsets;
    const double *t, *f, *e;
    const uint8_t* b;
    const double* z_old;        // [n_src]
};
struct GpResCopies {
    const int64_t* offsets;     // [n_src * k + 1]
    const double *t, *e;
    const uint8_t* b;
    int k;
};
struct GpResPlan {              // one entry per copy
    const double *z_new, *dim, *noise, *shift;
    const uint64_t* seed;
};

// The source's reference time, the time the points stage's origin stands for: under GP_GRID_FROM_PEAK the time of the gp2d
// set's peak row (gp_object: first maximum of the r rows in file order, NaN fluxes skipped; of all rows without an r row),
// under GP_GRID_FROM_FIRST the first valid observation.  NaN where there is none.  Uniform over the wave.
template <class W>
LCFE_FN double gp_res_tref(const GpResSource& S, int64_t o, int origin) {
    const int64_t r0 = S.offsets[o];
    const int n = (int)(S.offsets[o + 1] - r0);
    const ObjIn L{S.t + r0, S.f + r0, S.e + r0, S.b + r0, n, qnan()};
    const int lane = W::lane();
    if (origin == GP_GRID_FROM_FIRST) {
        double m = __builtin_inf();
        int have = 0;
        for (int i = lane; i < n; i += W::LANES)
            if (gp_row_valid(L, i)) { m = fmin(m, L.t[i]); have = 1; }
        m = W::min(m);
        return (W::sum(have) > 0) ? m : qnan();
    }
    int nr = 0;
    for (int i = lane; i < n; i += W::LANES) nr += (L.b[i] == 2);
    const bool use_r = W::sum(nr) > 0;
    double best = -__builtin_inf();
    for (int i = lane; i < n; i += W::LANES)
        if ((!use_r || L.b[i] == 2) && !is_nan(L.f[i])) best = fmax(best, L.f[i]);
    best = W::max(best);
    int cand = 0x7fffffff;
    for (int i = lane; i < n; i += W::LANES)
        if ((!use_r || L.b[i] == 2) && L.f[i] == best) cand = (i < cand) ? i : cand;
    const int pk = W::min(cand);
    return (pk == 0x7fffffff) ? qnan() : L.t[pk];
}

// Query pass for source o: q_t and q_lam of the rows of its k copies, and q_off[o] (the last source also writes the end).
// A row of an unknown filter asks for NaN; so does every row of a source without a reference time.
template <class W>
LCFE_FN void gp_res_query_object(const GpResSource& S, const GpResCopies& C, const GpResPlan& P, int64_t o, int64_t n_src, int origin,
                                 int64_t* q_off, double* q_t, double* q_lam) {
    const double tref = gp_res_tref<W>(S, o, origin), zo = S.z_old[o];
    for (int c = 0; c < C.k; ++c) {
        const int64_t oc = o * C.k + c;
        const double s = (1.0 + P.z_new[oc]) / (1.0 + zo), sh = P.shift[oc];
        for (int64_t r = C.offsets[oc] + W::lane(); r < C.offsets[oc + 1]; r += W::LANES) {
            const int b = C.b[r];
            q_t[r] = (b < 6) ? (C.t[r] - sh - tref) / s : qnan();
            q_lam[r] = (b < 6) ? gp_wavelength(b) / s : qnan();
        }
    }
    if (W::lane() == 0) {
        q_off[o] = C.offsets[o * C.k];
        if (o == n_src - 1) q_off[n_src] = C.offsets[n_src * C.k];
    }
}

// Write pass for copy oc: one lane per row.  n1 / n2 null: Philox streams 4 and 5, counter = the row's index in the copy.
template <class W>
LCFE_FN void gp_res_write_copy(const GpResCopies& C, const GpResPlan& P, int64_t oc, const double* mean, const double* var, const double* n1,
                               const double* n2, const int32_t* src_status, int nst, double* flux_out, double* err_out, int32_t* status_out) {
    const double dim = P.dim[oc], noise = P.noise[oc];
    const uint64_t seed = P.seed[oc];
    const int64_t r0 = C.offsets[oc];
    for (int64_t r = r0 + W::lane(); r < C.offsets[oc + 1]; r += W::LANES) {
        const double mu = mean[r], v = var[r], e = C.e[r];
        double f = qnan(), eo = qnan();
        if (!is_nan(mu) && !is_nan(v)) {
            const double a = n1 ? n1[r] : aug_normal(seed, r - r0, AUG_STREAM_GP_N1);
            const double b = n2 ? n2[r] : aug_normal(seed, r - r0, AUG_STREAM_GP_N2);
            const double sd = sqrt((v > 0.0) ? v : 0.0), ds = dim * sd;
            f = dim * (mu + sd * a) + (e * noise) * b;
            eo = sqrt((e * e) * (1.0 + noise * noise) + ds * ds);
        }
        flux_out[r] = f;
        err_out[r] = eo;
    }
    if (W::lane() == 0) status_out[oc] = src_status[(oc / C.k) * nst];
}

}  // namespace lcfe
