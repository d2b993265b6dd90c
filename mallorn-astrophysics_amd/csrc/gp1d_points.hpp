// gp1d_points.hpp -- posterior mean and standard deviation of the per-band GP (gp1d.hpp) at a caller's times
// (reference: src/features/gaussian_process.py, interpolate_at_times -> GaussianProcessRegressor.predict(return_std=True)).
// lcfe_gp1d_points_device of lcfe.hip runs it as the tail of gp1d_band in the band fit's own workgroup; the host
// simulation (tests/hostsim/gp1d_points.cpp) runs the same templates on one lane, so this header stays host-compilable.
//
// For a query t* of a fitted band:  x* = clip((t* - t_min) / t_range, 0, 1),
//     mean = k*' K^-1 y ,   k*_i = c exp(-(x* - x_i)^2 / (2 l^2))          (no white term in the cross kernel)
//     std  = sqrt(max(c + s2 - k*' K^-1 k*, 0))                             (kernel_.diag(X*) carries the WhiteKernel)
// in the reference's units (standardised flux).  The stage is the 2-D GP's (gp_grid_stage of gp.hpp: 16 query columns per
// pass, their kernel values in the pivot panel that is idle after the sweep, the mean as a dot with K^-1 y) with a third
// column source, Gp1dPointSpec, whose model forms the quadratic form itself with one refinement step (see `refine`).
#pragma once
#include "gp1d.hpp"

namespace lcfe {

constexpr int GP1D_NBAND = 4;            // g, r, i, z: band codes 1..4
constexpr int GP1D_NTHETA = 3;           // (log c, log l, log s2)
constexpr int GP1D_NNORM = 4;            // (t_min, t_range, f_mean, f_std) of a band

// The queries of ONE band of one light curve: column g is query perm[g] of the object's list (times q_t in MJD), and its
// results go to that slot -- the caller's order.  (t_min, t_range, ell) are the band's and the evaluation's.  A query with
// a non-finite time has no column.
struct Gp1dPointSpec {
    const double* q_t;                   // the object's queries
    const int* perm;                     // the band's queries, stable in the caller's order
    int n;
    double t_min, t_range, ell;
    LCFE_FN int size() const { return n; }
    // tp = x* / l, the abscissa against S.sm.r[i] = x_i / l (scikit-learn: cdist(X / length_scale, Y / length_scale))
    LCFE_FN bool column(int g, double, double& tp, double& lp) const {
        const double tq = q_t[perm[g]];
        lp = 0.0;
        double x = (tq - t_min) / t_range;
        x = (x < 0.0) ? 0.0 : ((x > 1.0) ? 1.0 : x);                   // np.clip(target_norm, 0, 1)
        tp = x / ell;
        return finite_d(tq);
    }
};

// the stage's model for that source; its parameter vector is (0, log c, log l, log s2): m0 = l, m1 = s2
template <>
struct GpStageModel<Gp1dPointSpec> {
    template <class LDS>
    LCFE_FN static double kval(const LDS& S, int i, double tp, double, double c, double, double) {
        const double q = tp - S.sm.r[i];
        return c * exp(-0.5 * (q * q));
    }
    LCFE_FN static double prior(double c, double, double s2) { return c + s2; }
    // y_var[y_var < 0] = 0 (sklearn/gaussian_process/_gpr.py), then sqrt
    LCFE_FN static double spread(double v, double) { return sqrt((v < 0.0) ? 0.0 : v); }
    LCFE_FN static int slot(const Gp1dPointSpec& G, int g) { return G.perm[g]; }

    // K(i, j) as gp1d_eval fills it
    template <class LDS>
    LCFE_FN static double kmat(const LDS& S, int i, int j, double c, double s2) {
        const double q = S.sm.r[i] - S.sm.r[j];
        const double k = c * exp(-0.5 * (q * q));
        return (i == j) ? k + (s2 + S.e2[i]) : k;
    }
    // The quadratic form with one step of refinement on w = K^-1 k*.  The sweep's explicit inverse carries an error of
    // eps cond(K) that is not a backward error, and k*' A k* summed over the tiles cancels from terms of c^2 |A_ij| down to
    // c: at the kernel's bounds (cond(K) ~ 1e7) both lose what scikit-learn's triangular solves keep (measured: up to 54
    // times the bound derived from scikit-learn's own deviation; with the correction added to the tile sum still 3.7 times
    // at 767 rows).  With w^ = -A k* stored, r = k* - K w^ (K from the kernel again) and ry = y - K alpha^
    // (Gp1dPointsTail::posterior leaves it in S.y),
    //     k*' K^-1 k* = k*' w^ + w^' r + O(r' K^-1 r) ,   k*' K^-1 y = k*' alpha^ + w^' ry + O(r' K^-1 ry)
    // for ANY w^ near K^-1 k* -- provided both terms use the SAME w^, which is why the leading term is the dot with the
    // stored w^ and not the stage's tile sum.  q = -(k*' w^ + w^' r) stands for k*' A k*, dm = w^' ry joins the mean.
    // w^ lives in S.t, which this model does not read (its abscissae are S.sm.r).  O(n^2) kernel values per column.
    static constexpr bool kRefine = true;
    template <class W, class LDS, class KP>
    LCFE_FN static void refine(LDS& S, KP A, int n, const double* Kp, int g, double c, double, double s2, double& q, double& dm) {
        const int lane = W::lane();
        for (int i = lane; i < n; i += W::LANES) {
            double s = 0.0;
            for (int j = 0; j < n; ++j) s += ((j <= i) ? A[tri_index(i, j)] : A[tri_index(j, i)]) * Kp[(j << 4) + g];
            S.t[i] = -s;
        }
        W::sync();
        double a = 0.0, b = 0.0;
        for (int i = lane; i < n; i += W::LANES) {
            double s = 0.0;
            for (int j = 0; j < n; ++j) s += kmat(S, i, j, c, s2) * S.t[j];
            a += S.t[i] * ((Kp[(i << 4) + g] - s) + Kp[(i << 4) + g]);       // w^_i (r_i + k*_i)
            b += S.t[i] * S.y[i];
        }
        q = -W::sum(a);
        dm = W::sum(b);
        W::sync();
    }
};

// gp1d_band's tail: the band's posterior at its queries.  mean / sd are the object's slices (NaN until written), theta_in
// the caller's theta of this band (given mode), theta_out and norm this band's slots.
template <class KP>
struct Gp1dPointsTail {
    static constexpr bool kOn = true;
    bool given;
    KP K;                                // the matrix the caller's evaluation works on
    const double* theta_in;              // [3]
    double *theta_out, *norm;            // [3], [4]
    const double* q_t;
    const int* perm;
    int nq;
    double *mean, *sd;

    // the band is prepared (it has a fit in the reference): its normalisation
    template <class W, class LDS>
    LCFE_FN void prepared(LDS&, int, double t_min, double t_range, double f_mean, double f_std) const {
        if (W::lane() == 0) { norm[0] = t_min; norm[1] = t_range; norm[2] = f_mean; norm[3] = f_std; }
    }

    // x: the winning theta (fit mode: the working set holds the LAST evaluation's state, so evaluate once more at x) or
    // the caller's (given mode: just evaluated).  A failed factorisation leaves NaN: predict would raise.
    template <class W, int NP, class LDS, class Ev>
    LCFE_FN void posterior(LDS& S, int n, const double* x, double fx, Ev&& ev, double t_min, double t_range) const {
        if (W::lane() == 0) { theta_out[0] = x[0]; theta_out[1] = x[1]; theta_out[2] = x[2]; }
        if (nq == 0) return;
        if (!given) {
            double gv[3];
            ev(x, n, fx, gv);
        }
        if (!finite_d(fx)) return;
        // ry = y - K alpha^ into S.y (the band's last use of y): what the stage's refinement step reads
        {
            const double c = exp(x[0]), s2 = exp(x[2]);
            for (int i = W::lane(); i < n; i += W::LANES) {
                double s = 0.0;
                for (int j = 0; j < n; ++j) s += GpStageModel<Gp1dPointSpec>::kmat(S, i, j, c, s2) * S.alpha[j];
                S.y[i] -= s;                                              // (row i's own entry: nobody else reads it)
            }
            W::sync();
        }
        const double p[4] = {0.0, x[0], x[1], x[2]};
        const Gp1dPointSpec G{q_t, perm, nq, t_min, t_range, exp(x[1])};
        gp_grid_stage<W, NP>(S, K, n, p, 1.0, 0.0, G, mean, sd);
    }
};

}  // namespace lcfe
