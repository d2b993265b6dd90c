// advanced.hpp -- the "advanced" features (reference: src/features/advanced_features.py,
// extract_advanced_features_single :476-622) -> 50 columns in the order the reference's dict is built: absolute
// magnitudes (:36-89), Mexican-hat power spectra of the r and g bands (:92-192), FLEET widths (:195-277), pre-peak
// colours (:280-329), autocorrelation of the r band (:332-381), early / late ratios (:384-437), higher-order statistics
// (:440-473), peak lags and peak flux ratios (:586-620).
//
// Inputs are the views of stage.hpp.  `band_data` (:490-498) is a band's time-sorted segment when it has >= 3 rows.  The
// reference sorts with pandas' unstable default, so the order of equal times inside a band is undefined there; here it is
// the staged (time, file index) order.
//
// The hot path is the Mexican-hat pair sum: all pairs i < j of a band, four scales.  The pairs are dealt to the lanes by
// the round-robin schedule q -> (i, (i + d) mod m), d = q / m + 1, i = q mod m, q < m (m - 1) / 2, which visits every
// unordered pair once; a pair's time difference and squared flux difference are computed once and serve the four scales.
// Lanes of one trip share d, so their time differences are alike and the `dt / scale < 5` branches are mostly uniform:
// the wavefront skips the exponentials of the short scales for the distant pairs.
#pragma once
#include "fits.hpp"      // wave_median
#include "stage.hpp"
#include "tde.hpp"       // wave_linfit, wave_moments, wave_compact

namespace lcfe {

constexpr int ADVANCED_NCOL = 50;
// longest 1-day grid of the r band the autocorrelation walks (days of time span).  The grid is never stored -- every
// term interpolates its own values -- so this bounds run time only: a wavefront takes about 2^16 trips.  Beyond it the
// three ACF columns are NaN and the status word is -100.
constexpr double ADVANCED_ACF_MAX_DAYS = 4194304.0;

template <int CAP>
struct AdvancedLds {
    double xs[CAP], ys[CAP];
    unsigned long long keys[CAP];
    double slot[4];
    double out[ADVANCED_NCOL + 2];
};

// number of elements < x / <= x of an ascending array
LCFE_FN int count_lt(const double* t, int m, double x) {
    int lo = 0, hi = m;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (t[mid] < x) lo = mid + 1; else hi = mid; }
    return lo;
}
LCFE_FN int count_le(const double* t, int m, double x) {
    int lo = 0, hi = m;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (t[mid] <= x) lo = mid + 1; else hi = mid; }
    return lo;
}

// np.interp(x, t, f) for t[0] <= x on an ascending t (the branches of numpy's compiled loop, as in research_mhps)
LCFE_FN double np_interp_at(const double* t, const double* f, int m, double x) {
    const int lo = count_le(t, m, x) - 1;                           // last j with t[j] <= x
    if (lo >= m - 1) return f[m - 1];
    if (t[lo] == x) return f[lo];
    const double slope = (f[lo + 1] - f[lo]) / (t[lo + 1] - t[lo]);
    double v = slope * (x - t[lo]) + f[lo];
    if (is_nan(v)) {
        v = slope * (x - t[lo + 1]) + f[lo + 1];
        if (is_nan(v) && f[lo] == f[lo + 1]) v = f[lo];
    }
    return v;
}

// luminosity distance in Mpc of compute_absolute_magnitude (:58-74); NaN unless z > 0 (:50).  For z >= 0.1 the reference
// calls scipy.integrate.quad on 1 / E(z): QUADPACK stops after its first 21-point Gauss-Kronrod rule up to z = 4.75, and
// one rule on [0, z] stays within 1.1e-10 relative of its result up to z = 10 (tests/test_advanced_cpu.py checks both).
// Beyond z = 10 this single rule deviates from the reference's adaptive result.
template <class W>
LCFE_FN double advanced_lum_distance(double z) {
    if (!(z > 0)) return qnan();
    const double c = 299792.458, H0 = 70.0;                         // :61-62
    if (z < 0.1) return c * z / H0;                                 // :65
    // QUADPACK qk21: Kronrod abscissae and weights on [-1, 1]
    const double XGK[11] = {0.995657163025808080735527280689003, 0.973906528517171720077964012084452,
                            0.930157491355708226001207180059508, 0.865063366688984510732096688423493,
                            0.780817726586416897063717578345042, 0.679409568299024406234327365114874,
                            0.562757134668604683339000099272694, 0.433395394129247190799265943165784,
                            0.294392862701460198131126603103866, 0.148874338981631210884826001129720, 0.0};
    const double WGK[11] = {0.011694638867371874278064396062192, 0.032558162307964727478818972459390,
                            0.054755896574351996031381300244580, 0.075039674810919952767043140916190,
                            0.093125454583697605535065465083366, 0.109387158802297641899210590325805,
                            0.123491976262065851077958109585166, 0.134709217311473325928054001771707,
                            0.142775938577060080797094273138717, 0.147739104901338491374841515972068,
                            0.149445554002916905664936468389821};
    const double h = 0.5 * z;                                       // centre and half length of [0, z]
    double part = 0;
    for (int k = W::lane(); k < 21; k += W::LANES) {
        const int q = (k <= 10) ? k : 20 - k;
        const double x = (k <= 10) ? h - h * XGK[q] : h + h * XGK[q];
        const double a = 1 + x;
        part += WGK[q] / sqrt(0.3 * (a * a * a) + 0.7);             // :71
    }
    return (c / H0) * (1 + z) * (W::sum(part) * h);                 // :74
}

// compute_absolute_magnitude (:36-89) with the distance of advanced_lum_distance
LCFE_FN double advanced_abs_mag(double flux, double z, double d_l) {
    if (!(flux > 0) || !(z > 0)) return qnan();                     // :50 (flux <= 0, NaN flux, NaN z, z <= 0)
    const double m_ab = -2.5 * log10(flux * 1e-6) + 8.90;           // :56
    if (!(d_l > 0)) return qnan();                                  // :77-80
    const double mu = 5 * log10(d_l) + 25;
    const double k_corr = -2.5 * log10(1 + z);                      // :85
    return m_ab - mu - k_corr;
}

// compute_mhps_features (:92-192) of one band of band_data -> o6.  `nf` = m doubles of wave-shared scratch.
template <class W>
LCFE_FN void advanced_mhps(const double* t, const double* f, int m, double* nf, double* o6) {
    const int lane = W::lane();
    double r[4] = {qnan(), qnan(), qnan(), qnan()};
    if (m >= 5) {                                                   // :107
        double s = 0;
        for (int i = lane; i < m; i += W::LANES) s += f[i];
        const double mean = W::sum(s) / m;                          // :116
        if (!(mean == 0)) {                                         // :117 (a NaN mean goes on and makes every term NaN)
            for (int i = lane; i < m; i += W::LANES) nf[i] = (f[i] - mean) / mean;   // :119
            W::sync();
            const double SC[4] = {10.0, 30.0, 100.0, 365.0};        // :162-167
            double acc[4] = {0, 0, 0, 0};
            int cnt[4] = {0, 0, 0, 0};
            const int total = m * (m - 1) / 2;                      // m <= 16384
            for (int q = lane; q < total; q += W::LANES) {
                const int row = q / m, i = q - row * m;
                int j = i + row + 1;
                if (j >= m) j -= m;
                const double dt = fabs(t[j] - t[i]);                // :131
                const double df = nf[j] - nf[i], d2 = df * df;      // :137 (f2 - f1)^2
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double tn = dt / SC[k];                   // :132, an IEEE division: the cut below is the reference's
                    if (tn < 5) {                                   // :135
                        const double kernel = (1 - tn * tn) * exp(-(tn * tn) / 2);   // :136
                        acc[k] += d2 * fabs(kernel);
                        ++cnt[k];
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double a = W::sum(acc[k]);
                const int c = W::sum(cnt[k]);
                if (c > 0) r[k] = sqrt(a / c);                      // :140-142
            }
            W::sync();
        }
    }
    if (lane == 0) {
        for (int k = 0; k < 4; ++k) o6[k] = r[k];
        o6[4] = (!is_nan(r[0]) && !is_nan(r[2]) && r[2] > 0) ? r[0] / r[2] : qnan();   // :176-182
        o6[5] = (!is_nan(r[1]) && !is_nan(r[3]) && r[3] > 0) ? r[1] / r[3] : qnan();   // :184-190
    }
}

// one side of fit_fleet_model (:238-264): rows [a, b) of the band, dt = sign * (t - pt) -> tau or NaN
template <class W, int CAP>
LCFE_FN double advanced_fleet_side(const double* t, const double* f, int a, int b, double pt, double pf, double sign,
                                   AdvancedLds<CAP>& S) {
    const int lane = W::lane();
    if (b - a < 3) return qnan();                                   // :240, :255
    int cnt = 0;
    bool bad = false;
    for (int base = a; base < b; base += W::LANES) {
        const int i = base + lane;
        const bool sel = i < b && f[i] > 0;                         // :243, :257
        const double lr = sel ? log(f[i] / pf) : 0.0;               // :245, :259
        bad = bad || (sel && !__builtin_isfinite(lr));
        cnt = wave_compact<W>(sel, sel ? sign * (t[i] - pt) : 0.0, lr, S.xs, S.ys, cnt);
    }
    W::sync();
    double tau = qnan();
    // np.polyfit returns NaN coefficients for a non-finite ordinate; `slope < 0` is then False
    const bool any_bad = W::any(bad);
    if (cnt >= 3 && !any_bad) {                                     // :244, :258
        double mean, var, mn, mx;
        wave_moments<W>(S.xs, cnt, mean, var, mn, mx);
        if (sqrt(var) > 0) {                                        // :247, :261 np.std(dt) > 0
            double slope, icpt;
            wave_linfit<W>(S.xs, S.ys, cnt, slope, icpt);           // :249, :262
            if (slope < 0) tau = -1 / slope;                        // :250-251
        }
    }
    W::sync();
    return tau;
}

// fit_fleet_model (:195-277) of one band of band_data whose first maximum is row p -> o3 (fleet_chi2 is never set)
template <class W, int CAP>
LCFE_FN void advanced_fleet(const double* t, const double* f, int m, int p, AdvancedLds<CAP>& S, double* o3) {
    double width = qnan(), asym = qnan();
    if (m >= 5) {                                                   // :213
        const double pt = t[p], pf = f[p];                          // :222-224
        if (!(pf <= 0)) {                                           // :226 (a NaN peak goes on; its log ratios are NaN)
            const int nr = uniform_int(count_lt(t, m, pt)), f0 = uniform_int(count_le(t, m, pt));   // :230-231
            const double rise = advanced_fleet_side<W, CAP>(t, f, 0, nr, pt, pf, -1.0, S);
            const double fall = advanced_fleet_side<W, CAP>(t, f, f0, m, pt, pf, 1.0, S);
            if (!is_nan(rise) && !is_nan(fall)) {                   // :267-275
                width = (rise + fall) / 2;
                asym = (rise > 0) ? fall / rise : qnan();
            } else if (!is_nan(fall)) width = fall;
            else if (!is_nan(rise)) width = rise;
        }
    }
    if (W::lane() == 0) { o3[0] = width; o3[1] = asym; o3[2] = qnan(); }
}

// compute_pre_peak_colors (:280-329) for the pair (k1, k2) -> mean, slope.  The reference walks the band-1 rows before
// the peak in file order and takes, per row, the first minimum of |t2 - t1| among the band-2 rows before the peak, in
// file order too.  Here the band-1 rows are walked in (time, file index) order -- the mean's summation order and the
// origin of the slope's abscissa change, which is rounding only -- and the partner is found by a binary search in the
// time-sorted band 2, equidistant candidates decided by the smaller file index, which IS the reference's first minimum.
// Differences: a non-finite colour makes the slope NaN (np.polyfit returns NaN coefficients); colours that all share
// one time (possible with tied times only) make np.polyfit raise in the reference and give a NaN slope here.
template <class W, int CAP>
LCFE_FN void advanced_pre_peak_pair(const ObjLds<CAP>& L, int k1, int k2, double pk, AdvancedLds<CAP>& S, double& mean_out,
                                    double& slope_out) {
    const int lane = W::lane();
    mean_out = qnan();
    slope_out = qnan();
    const int s1 = uniform_int(L.boff[k1]), s2 = uniform_int(L.boff[k2]);
    const double* t1 = L.bt + s1;
    const double* f1 = L.bf + s1;
    const double* t2 = L.bt + s2;
    const double* f2 = L.bf + s2;
    const unsigned short* x2 = L.bidx + s2;
    const int n1 = uniform_int(count_lt(t1, uniform_int(L.boff[k1 + 1]) - s1, pk));    // :298-299 rows with t < peak_time
    const int n2 = uniform_int(count_lt(t2, uniform_int(L.boff[k2 + 1]) - s2, pk));
    if (n1 < 2 || n2 < 2) return;                                   // :301
    int cnt = 0;
    bool bad = false;
    for (int base = 0; base < n1; base += W::LANES) {
        const int i = base + lane;
        bool ok = false;
        double a = 0, col = 0;
        if (i < n1) {
            a = t1[i];
            const int lo = count_le(t2, n2, a) - 1, hi = lo + 1;    // the neighbours of `a` in band 2
            const double dl = (lo >= 0) ? fabs(t2[lo] - a) : __builtin_inf(), dr = (hi < n2) ? fabs(t2[hi] - a) : __builtin_inf();
            int bj = -1, bfi = 0x7fffffff;                          // :313 np.argmin: the first minimum in file order
            if (dl <= dr)
                for (int j = lo; j >= 0 && t2[j] == t2[lo]; --j)
                    if ((int)x2[j] < bfi) { bfi = x2[j]; bj = j; }
            if (dr <= dl)
                for (int j = hi; j < n2 && t2[j] == t2[hi]; ++j)
                    if ((int)x2[j] < bfi) { bfi = x2[j]; bj = j; }
            const double d = (dl < dr) ? dl : dr;
            if (bj >= 0 && d < 5 && f1[i] > 0) {                    // :315
                const double fb = f2[bj];
                if (fb > 0) { ok = true; col = -2.5 * log10(f1[i] / fb); }   // :317-318
            }
        }
        bad = bad || (ok && !__builtin_isfinite(col));
        cnt = wave_compact<W>(ok, a, col, S.xs, S.ys, cnt);
    }
    W::sync();
    const bool any_bad = W::any(bad);
    if (cnt >= 2) {                                                 // :322
        double s = 0;
        for (int i = lane; i < cnt; i += W::LANES) s += S.ys[i];
        mean_out = W::sum(s) / cnt;                                 // :323
        if (cnt >= 3 && !any_bad) {                                 // :325
            const double x0 = S.xs[0];
            W::sync();
            for (int i = lane; i < cnt; i += W::LANES) S.xs[i] -= x0;   // :326 times - times[0]
            W::sync();
            double slope, icpt;
            wave_linfit<W>(S.xs, S.ys, cnt, slope, icpt);
            slope_out = slope * 10;                                 // :327 per 10 days
        }
    }
    W::sync();
}

// compute_autocorrelation_features (:332-381) on the time-sorted r band -> o3; false if the grid is beyond
// ADVANCED_ACF_MAX_DAYS.  flux_grid = np.interp on t_grid = np.arange(t_min, t_max, 1.0) is never stored: the mean, the
// standard deviation and the two lag sums each interpolate the values they need.
template <class W>
LCFE_FN bool advanced_acf(const double* t, const double* f, int m, double* o3) {
    const int lane = W::lane();
    double a10 = qnan(), a30 = qnan(), ratio = qnan();
    bool fits = true;
    if (m >= 10) {                                                  // :344
        const double span = t[m - 1] - t[0];                        // :348-349
        if (span >= 30) {                                           // :351 (a NaN span makes the reference's arange raise)
            const double nd = ceil(span);                           // len(np.arange(t_min, t_max, 1.0)) >= 30 > 20 (:357)
            fits = nd <= ADVANCED_ACF_MAX_DAYS;
            if (fits) {
                const long long N = (long long)nd;
                // np.arange fills start, start + step, then start + k * delta with delta = (start + step) - start
                const double t0 = t[0], second = t0 + 1.0, delta = second - t0;
                auto grid = [&](long long k) {
                    const double x = (k == 0) ? t0 : ((k == 1) ? second : t0 + (double)k * delta);
                    return np_interp_at(t, f, m, x);                // :361
                };
                double s = 0;
                for (long long k = lane; k < N; k += W::LANES) s += grid(k);
                const double mean = W::sum(s) / (double)N;          // :364
                double q = 0;
                for (long long k = lane; k < N; k += W::LANES) { const double d = grid(k) - mean; q += d * d; }
                const double den = sqrt(W::sum(q) / (double)N) + 1e-10;
                double c10 = 0, c30 = 0;                            // :368 np.correlate(g, g, 'full')[n - 1 + lag]
                for (long long k = lane; k + 10 < N; k += W::LANES) {
                    const double g0 = (grid(k) - mean) / den;
                    c10 += g0 * ((grid(k + 10) - mean) / den);
                    if (k + 30 < N) c30 += g0 * ((grid(k + 30) - mean) / den);
                }
                a10 = W::sum(c10) / (double)N;                      // :371-372
                c30 = W::sum(c30);
                if (N > 30) a30 = c30 / (double)N;                  // :374-375
                if (!is_nan(a10) && !is_nan(a30) && fabs(a30) > 0.01) ratio = a10 / a30;   // :377-379
            }
        }
    }
    if (lane == 0) { o3[0] = a10; o3[1] = a30; o3[2] = ratio; }
    return fits;
}

// compute_higher_order_stats (:440-473) of m wave-shared values -> o3 (skewness, kurtosis, biweight midvariance)
template <class W, int CAP>
LCFE_FN void advanced_hos(const double* x, int m, AdvancedLds<CAP>& S, double* o3) {
    const int lane = W::lane();
    double sk = qnan(), ku = qnan(), bw = qnan();
    if (m >= 5) {                                                   // :452
        // scipy.stats.skew / kurtosis (1.15.3, bias=True, fisher=True): central moments about np.mean in a second pass;
        // NaN where m2 <= (eps * mean)^2, "the data are constant to rounding".  A NaN or an infinite value propagates.
        double s = 0;
        for (int i = lane; i < m; i += W::LANES) s += x[i];
        const double mean = W::sum(s) / m;
        double q2 = 0, q3 = 0, q4 = 0;
        for (int i = lane; i < m; i += W::LANES) {
            const double d = x[i] - mean, d2 = d * d;
            q2 += d2;
            q3 += d2 * d;
            q4 += d2 * d2;
        }
        const double m2 = W::sum(q2) / m, m3 = W::sum(q3) / m, m4 = W::sum(q4) / m;
        const double tiny = 2.220446049250313e-16 * mean;
        if (!(m2 <= tiny * tiny)) {
            sk = m3 / (m2 * sqrt(m2));                              // m3 / m2**1.5
            ku = m4 / (m2 * m2) - 3;
        }
        const double med = wave_median<W>(x, m, S.slot, S.keys);    // :459
        for (int i = lane; i < m; i += W::LANES) S.xs[i] = fabs(x[i] - med);
        W::sync();
        const double mad = wave_median<W>(S.xs, m, S.slot, S.keys); // :460
        if (mad > 0) {                                              // :462
            int nv = 0;
            double num = 0, den = 0;
            for (int i = lane; i < m; i += W::LANES) {
                const double d = x[i] - med, u = d / (9 * mad);     // :463
                if (fabs(u) < 1) {                                  // :464
                    const double u2 = u * u, w = 1 - u2, w2 = w * w;
                    ++nv;
                    num += d * d * (w2 * w2);                       // :467
                    den += w * (1 - 5 * u2);                        // :468
                }
            }
            nv = W::sum(nv);
            num = W::sum(num);
            den = W::sum(den);
            const double denom = den * den;
            if (nv >= 3 && denom > 0) bw = m * num / denom;         // :466, :470-471
        }
        W::sync();
    }
    if (lane == 0) { o3[0] = sk; o3[1] = ku; o3[2] = bw; }
}

// All 50 columns of one staged object into S.out; returns the status word (0, or -100: r band beyond the ACF grid)
template <class W, int CAP>
LCFE_FN int advanced_object(const ObjLds<CAP>& L, double z, AdvancedLds<CAP>& S) {
    const int lane = W::lane();
    double* o = S.out;
    const int n = uniform_int(L.n);
    // band_data (:490-498) of g, r, i: first maximum (np.argmax: the first NaN wins, so f[p] is also np.max) and mean
    int bs[3], bm[3], bp[3];
    double pt[3], pf[3], mean[3];
    bool have[3];
    for (int b = 0; b < 3; ++b) {
        bs[b] = uniform_int(L.boff[b + 1]);
        bm[b] = uniform_int(L.boff[b + 2]) - bs[b];
        have[b] = bm[b] >= 3;                                       // :493
        bp[b] = -1;
        pt[b] = pf[b] = mean[b] = qnan();
        if (have[b]) {
            const double* f = L.bf + bs[b];
            bp[b] = uniform_int(wave_argmax_first<W>(f, bm[b]));
            pt[b] = L.bt[bs[b] + bp[b]];
            pf[b] = f[bp[b]];
            double s = 0;
            for (int i = lane; i < bm[b]; i += W::LANES) s += f[i];
            mean[b] = W::sum(s) / bm[b];
        }
    }
    // absolute magnitudes (:507-516)
    const double d_l = advanced_lum_distance<W>(z);
    if (lane == 0)
        for (int b = 0; b < 3; ++b) {
            o[2 * b] = have[b] ? advanced_abs_mag(pf[b], z, d_l) : qnan();
            o[2 * b + 1] = have[b] ? advanced_abs_mag(mean[b], z, d_l) : qnan();
        }
    // Mexican-hat power spectra: r, then g (:520-539)
    for (int q = 0; q < 2; ++q) {
        const int b = 1 - q;
        advanced_mhps<W>(L.bt + bs[b], L.bf + bs[b], have[b] ? bm[b] : 0, S.xs, o + 6 + 6 * q);
        W::sync();
    }
    // FLEET: r, then g (:542-550)
    for (int q = 0; q < 2; ++q) {
        const int b = 1 - q;
        advanced_fleet<W, CAP>(L.bt + bs[b], L.bf + bs[b], have[b] ? bm[b] : 0, bp[b], S, o + 18 + 3 * q);
    }
    // pre-peak colours against the r peak (:500-504, :553)
    {
        double m_gr = qnan(), s_gr = qnan(), m_ri = qnan(), s_ri = qnan();
        if (have[1] && !is_nan(pt[1])) {                            // :293
            advanced_pre_peak_pair<W, CAP>(L, 1, 2, pt[1], S, m_gr, s_gr);
            advanced_pre_peak_pair<W, CAP>(L, 2, 3, pt[1], S, m_ri, s_ri);
        }
        if (lane == 0) { o[24] = m_gr; o[25] = m_ri; o[26] = s_gr; o[27] = s_ri; }   // :286-291
    }
    // autocorrelation of the r band (:557-564)
    const bool fits = advanced_acf<W>(L.bt + bs[1], L.bf + bs[1], have[1] ? bm[1] : 0, o + 28);
    // early / late thirds of the time range of ALL rows (:384-437)
    {
        double lo = __builtin_inf(), hi = -__builtin_inf();
        for (int i = lane; i < n; i += W::LANES) { const double v = L.t[i]; lo = (v < lo) ? v : lo; hi = (v > hi) ? v : hi; }
        const double tmin = W::min(lo), tmax = W::max(hi);
        const double range = tmax - tmin;                           // :402
        const double early_end = tmin + range / 3, late_start = tmax - range / 3;   // :403-404
        for (int b = 0; b < 3; ++b) {
            double fr = qnan(), vr = qnan();
            if (n >= 10 && bm[b] >= 5) {                            // :395, :409
                const double* t = L.bt + bs[b];
                const double* f = L.bf + bs[b];
                const int ne = uniform_int(count_lt(t, bm[b], early_end));          // :414 t < t_early_end
                const int l0 = uniform_int(count_le(t, bm[b], late_start));         // :415 t > t_late_start
                if (ne >= 2 && bm[b] - l0 >= 2) {                   // :417
                    double em, ev, lm, lv, mn, mx;
                    wave_moments<W>(f, ne, em, ev, mn, mx);
                    wave_moments<W>(f + l0, bm[b] - l0, lm, lv, mn, mx);
                    if (em > 0) fr = lm / em;                       // :421-424
                    if (ev > 0) vr = lv / ev;                       // :429-432
                }
            }
            if (lane == 0) { o[31 + 2 * b] = fr; o[32 + 2 * b] = vr; }
        }
    }
    W::sync();
    // higher-order statistics: all rows in file order, then g and r of band_data (:571-584)
    advanced_hos<W, CAP>(L.f, n, S, o + 37);
    advanced_hos<W, CAP>(L.bf + bs[0], have[0] ? bm[0] : 0, S, o + 40);
    advanced_hos<W, CAP>(L.bf + bs[1], have[1] ? bm[1] : 0, S, o + 43);
    // peak lags and flux ratios at peak (:587-620)
    if (lane == 0) {
        o[46] = (have[0] && have[1]) ? pt[0] - pt[1] : qnan();
        o[47] = (have[1] && have[2]) ? pt[1] - pt[2] : qnan();
        o[48] = (have[0] && have[1] && pf[1] > 0) ? pf[0] / pf[1] : qnan();
        o[49] = (have[1] && have[2] && pf[2] > 0) ? pf[1] / pf[2] : qnan();
    }
    W::sync();
    return fits ? 0 : -100;
}

template <class W, class G, int CAP>   // RunSet's hook (feature_sets.hpp); G: policy of one per-band pass or fit
LCFE_FN int run_object(const ObjLds<CAP>& L, const ObjIn& in, AdvancedLds<CAP>& S, int32_t* st) {
    const int rc = advanced_object<W, CAP>(L, in.z, S);
    if (st && W::lane() == 0) st[0] = rc;
    return rc;
}

}  // namespace lcfe
