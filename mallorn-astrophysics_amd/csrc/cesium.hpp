// cesium.hpp -- Cesium-style variability features (reference: src/features/cesium_features.py,
// extract_cesium_features_single) -> 80 columns: per band u..y the 13 columns of extract_cesium_features_single_band
// (Stetson J and K, beyond 1 / 2 sigma, five flux-percentile ratios, percent amplitude, maximum slope, weighted linear
// trend, Anderson-Darling statistic), then cesium_stetson_j_consistency (g, r, i) and cesium_avg_beyond_1std.
//
// One light curve per wavefront, lanes over the rows of a band's time-sorted segment.  ONE rank-counting scan per band
// gives, for every row, the number of fluxes below it and the number not above it: the 24 order statistics behind the
// twelve percentiles and the two behind the median are picked from those intervals, and the Anderson-Darling sum uses the
// same counts as each row's rank -- no sorted copy of the band is made (see cesium_band).
#pragma once
#include "stage.hpp"
#include "stat.hpp"      // np_lerp

namespace lcfe {

constexpr int CESIUM_NCOL = 80;
constexpr int CESIUM_NBAND = 13;      // columns per band
constexpr int CESIUM_NQ = 12;         // percentiles per band: 40 60 32.5 67.5 25 75 17.5 82.5 10 90 5 95
constexpr int CESIUM_NSEL = 2 * CESIUM_NQ + 2;

template <int CAP>
struct CesiumLds {
    unsigned long long keys[CAP];     // sort keys of a band's fluxes
    int rk[CAP];                      // per row of the band: (#fluxes < own) + (#fluxes <= own)
    double sel[CESIUM_NSEL];
    double out[CESIUM_NCOL];
};

// erfcx(y) = exp(y^2) erfc(y) for y >= 1 / sqrt(2): Laplace's continued fraction 1 / sqrt(pi) / (y + (1/2) / (y + (2/2) /
// (y + (3/2) / ...))), evaluated from the tail.  180 / y^2 + 14 terms reach 3e-16 relative (measured against a 40-digit
// evaluation at y = 0.7071 ... 27: 356 terms are needed at 0.7071, 183 at 1, 29 at 3, 9 at 10).
LCFE_FN double erfcx_tail(double y) {
    const double c = 180.0 / (y * y);
    const int n = ((c < 400.0) ? (int)c : 400) + 14;
    double r = 0.0;
    for (int k = n; k >= 1; --k) r = (0.5 * k) / (y + r);
    return 0.5641895835477563 / (y + r);
}

// log of the standard normal CDF at w and at -w (scipy.special.log_ndtr: norm.logcdf / norm.logsf).  Of the two arguments
// at most one lies below -1; there log(erfc) would lose the tail (erfc underflows at 38 and its library versions are not
// held to a RELATIVE error), so log Phi(-a) = log(erfcx(a / sqrt 2) / 2) - a^2 / 2.  The other one follows from it, or --
// for |w| <= 1 -- both come from log1p(-erfc / 2), where erfc's absolute error is all that counts.
LCFE_FN void log_ndtr_both(double w, double& lcdf, double& lsf) {
    const double a = fabs(w);
    const double RSQRT2 = 0.70710678118654752440;
    double lo, hi;                                      // log Phi(-a), log Phi(a)
    if (a > 1.0) {
        lo = log(0.5 * erfcx_tail(a * RSQRT2)) - 0.5 * a * a;
        hi = log1p(-exp(lo));
    } else {
        lo = log1p(-0.5 * erfc(-a * RSQRT2));
        hi = log1p(-0.5 * erfc(a * RSQRT2));
    }
    lcdf = (w < 0) ? lo : hi;
    lsf = (w < 0) ? hi : lo;
}
LCFE_FN double log_ndtr(double x) {
    double a, b;
    log_ndtr_both(x, a, b);
    return a;
}

// the 13 columns of one band (t, f, e: its time-sorted segment of n >= 5 rows) -> o[0..13) (lane 0 writes)
template <class W, int CAP>
LCFE_FN void cesium_band(const double* t, const double* f, const double* e, int n, CesiumLds<CAP>& S, double* o) {
    const int lane = W::lane();
    const double dn = (double)n;
    // ---- pass 1: plain sums
    double a_f = 0, a_t = 0, a_w = 0, a_wf = 0, mx = -__builtin_inf();
    bool nanf = false;
    for (int i = lane; i < n; i += W::LANES) {
        const double fi = f[i], ei = e[i];
        const double w = 1.0 / ((ei > 0) ? ei * ei : 1.0);                 // :58, :256
        a_f += fi; a_t += t[i]; a_w += w; a_wf += w * fi;
        mx = (fi > mx) ? fi : mx;
        nanf = nanf || is_nan(fi);
    }
    const double mean = W::sum(a_f) / dn;                                  // :52, :126
    const double t_mean = W::sum(a_t) / dn;                                // :261
    const double w_sum = W::sum(a_w);                                      // :62, :265
    const double f_w = W::sum(a_wf) / w_sum;                               // :267
    mx = W::max(mx);
    const bool any_nan = W::any(nanf);
    // ---- pass 2: residual sums
    const double c = sqrt(dn / (dn - 1.0));                                // :55
    double a_j = 0, a_ad = 0, a_d2 = 0, a_var = 0, a_wt = 0;
    for (int i = lane; i < n; i += W::LANES) {
        const double fi = f[i], ei = e[i];
        const double w = 1.0 / ((ei > 0) ? ei * ei : 1.0);
        const double d = c * (fi - mean) / ((ei > 0) ? ei : 1.0);
        const double sg = is_nan(d) ? d : ((d > 0) ? 1.0 : ((d < 0) ? -1.0 : 0.0));     // np.sign
        a_j += w * d * sg;                                                 // :61
        a_ad += fabs(d);                                                   // :97
        a_d2 += d * d;                                                     // :98
        a_var += (fi - mean) * (fi - mean);                                // np.std, ddof 0
        a_wt += w * (t[i] - t_mean);                                       // :266
    }
    const double num_j = W::sum(a_j);
    const double k_num = W::sum(a_ad) / dn, k_den = sqrt(W::sum(a_d2) / dn);
    const double sd = sqrt(W::sum(a_var) / dn);
    const double t_w = W::sum(a_wt) / w_sum;
    const double stetson_j = (w_sum == 0) ? qnan() : num_j / w_sum;        // :64-67
    const double stetson_k = (k_den == 0) ? qnan() : k_num / k_den;        // :100-103
    // ---- pass 3: counts beyond 1 / 2 sigma, the regression sums, the largest slope, the mean of the standardised fluxes
    int n1 = 0, n2 = 0;
    double a_num = 0, a_den = 0, a_x = 0, ms = -__builtin_inf();
    bool nans = false;
    for (int i = lane; i < n; i += W::LANES) {
        const double fi = f[i], ei = e[i];
        const double w = 1.0 / ((ei > 0) ? ei * ei : 1.0);
        const double dev = fabs(fi - mean) / sd;                           // :132
        n1 += (dev > 1.0) ? 1 : 0;
        n2 += (dev > 2.0) ? 1 : 0;
        const double tc = (t[i] - t_mean) - t_w;
        a_num += w * tc * (fi - f_w);                                      // :269
        a_den += w * (tc * tc);                                            // :270
        a_x += (fi - mean) / sd;                                           // :300
        if (i + 1 < n) {
            double dt = t[i + 1] - t[i];
            dt = (dt > 0) ? dt : 1.0;                                      // :229
            const double sl = fabs((f[i + 1] - fi) / dt);                  // :231
            nans = nans || is_nan(sl);
            ms = (sl > ms) ? sl : ms;
        }
    }
    n1 = W::sum(n1); n2 = W::sum(n2);
    const double beyond1 = (sd == 0) ? 0.0 : (double)n1 / dn;              // :129-133
    const double beyond2 = (sd == 0) ? 0.0 : (double)n2 / dn;
    const double lt_num = W::sum(a_num), lt_den = W::sum(a_den);
    const double trend = (lt_den == 0) ? qnan() : lt_num / lt_den;         // :272-275
    ms = W::max(ms);
    const double max_slope = W::any(nans) ? qnan() : ms;                   // np.max: a NaN wins
    const double xbar = W::sum(a_x) / dn;
    // ---- Anderson-Darling, scipy.stats.anderson(x, 'norm'): the ddof-1 deviation of the standardised fluxes ...
    double a_s = 0;
    for (int i = lane; i < n; i += W::LANES) {
        const double x = (f[i] - mean) / sd;
        a_s += (x - xbar) * (x - xbar);
    }
    const double s1 = sqrt(W::sum(a_s) / (dn - 1.0));
    // ---- ... the rank counts (with them the percentiles and the median) ...
    int ranks[CESIUM_NSEL];
    double gam[CESIUM_NQ];
    const double Q[CESIUM_NQ] = {40.0, 60.0, 32.5, 67.5, 25.0, 75.0, 17.5, 82.5, 10.0, 90.0, 5.0, 95.0};
#pragma unroll
    for (int q = 0; q < CESIUM_NQ; ++q) {
        const double quant = Q[q] / 100.0;
        const double vi = n * quant + (1.0 - quant) - 1.0;                 // numpy _compute_virtual_index, alpha = beta = 1
        int lo = (int)floor(vi), hi = lo + 1;
        lo = lo < 0 ? 0 : (lo > n - 1 ? n - 1 : lo);
        hi = hi < 0 ? 0 : (hi > n - 1 ? n - 1 : hi);
        ranks[2 * q] = lo;
        ranks[2 * q + 1] = hi;
        gam[q] = vi - floor(vi);
    }
    ranks[2 * CESIUM_NQ] = (n - 1) / 2;
    ranks[2 * CESIUM_NQ + 1] = n / 2;
    wave_select_ranks<W, CESIUM_NSEL, true>(f, n, S.keys, ranks, S.sel, S.rk);
    double p[CESIUM_NQ];
#pragma unroll
    for (int q = 0; q < CESIUM_NQ; ++q) p[q] = any_nan ? qnan() : np_lerp(S.sel[2 * q], S.sel[2 * q + 1], gam[q]);
    const double span = p[11] - p[10];                                     // :168
    const double a0 = S.sel[2 * CESIUM_NQ], a1 = S.sel[2 * CESIUM_NQ + 1];
    const double median = any_nan ? qnan() : ((n & 1) ? a0 : (a0 + a1) / 2.0);
    const double pct_amp = (median == 0) ? qnan() : ((any_nan ? qnan() : mx) - median) / fabs(median);      // :194-197
    // ---- ... and the sum over the rows: A2 = -N - sum_i (2 i - 1) / N (logcdf(w_(i)) + logsf(w_(N + 1 - i))) over the ascending
    // w_(i); collected per row, a row of rank i carries (2 i - 1) / N logcdf(w) + (2 (N + 1 - i) - 1) / N logsf(w).  Equal values
    // have equal w, so only the sum of their ranks counts: each takes the mean rank, 2 i - 1 = #less + #less-or-equal.
    double a_a2 = 0;
    for (int i = lane; i < n; i += W::LANES) {
        const double x = (f[i] - mean) / sd;
        const double w = (x - xbar) / s1;
        double lc, ls;
        log_ndtr_both(w, lc, ls);
        const double r2 = (double)S.rk[i];
        a_a2 += r2 / dn * lc + (2.0 * dn - r2) / dn * ls;
    }
    const double ad = -dn - W::sum(a_a2);
    if (lane == 0) {
        o[0] = stetson_j;
        o[1] = stetson_k;
        o[2] = beyond1;
        o[3] = beyond2;
#pragma unroll
        for (int q = 0; q < 5; ++q) o[4 + q] = (span == 0) ? qnan() : (p[2 * q + 1] - p[2 * q]) / span;     // :170-173
        o[9] = pct_amp;
        o[10] = max_slope;
        o[11] = trend;
        o[12] = ad;
    }
    W::sync();
}

template <class W, int CAP>
LCFE_FN void cesium_object(const ObjLds<CAP>& L, CesiumLds<CAP>& S) {
    const int lane = W::lane();
    for (int k = 0; k < 6; ++k) {
        const int s = uniform_int(L.boff[k]), n = uniform_int(L.boff[k + 1]) - s;
        double* o = S.out + CESIUM_NBAND * k;
        if (n < 5) {                                                       // :367-376
            if (lane == 0)
                for (int c = 0; c < CESIUM_NBAND; ++c) o[c] = qnan();
            continue;
        }
        cesium_band<W, CAP>(L.bt + s, L.bf + s, L.be + s, n, S, o);
    }
    W::sync();
    if (lane == 0) {
        // Stetson J consistency over g, r, i (:391-400): np.std / np.mean(np.abs) of the values that are not NaN
        double v[3], sum = 0, suma = 0;
        int m = 0;
        for (int k = 1; k <= 3; ++k) {
            const double x = S.out[CESIUM_NBAND * k];
            if (!is_nan(x)) { v[m++] = x; sum += x; suma += fabs(x); }
        }
        double cons = qnan();
        if (m >= 2) {
            const double mu = sum / m;
            double q = 0;
            for (int i = 0; i < m; ++i) q += (v[i] - mu) * (v[i] - mu);
            cons = sqrt(q / m) / (suma / m);
        }
        // mean of the bands' beyond_1std that are not NaN (:403-412)
        double sb = 0;
        int mb = 0;
        for (int k = 0; k < 6; ++k) {
            const double x = S.out[CESIUM_NBAND * k + 2];
            if (!is_nan(x)) { sb += x; ++mb; }
        }
        S.out[78] = cons;
        S.out[79] = (mb > 0) ? sb / mb : qnan();
    }
    W::sync();
}

template <class W, class G, int CAP>   // RunSet's hook (feature_sets.hpp); G: policy of one per-band pass or fit
LCFE_FN int run_object(const ObjLds<CAP>& L, const ObjIn&, CesiumLds<CAP>& S, int32_t*) { cesium_object<W, CAP>(L, S); return 0; }

}  // namespace lcfe
