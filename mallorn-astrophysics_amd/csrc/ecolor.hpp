// ecolor.hpp -- enhanced post-peak colours (reference: src/features/enhanced_colors.py,
// extract_enhanced_colors_single) -> 45 columns.
//
// Every lookup of the reference masks a band with a +-5 day window, sorts the window and interpolates it
// (get_flux_at_time, :22-56).  The staged band segments are already sorted by (time, file index), so a window
// is a contiguous range of its segment: two binary searches give it, a third finds the interpolation interval.
// The 5 bands x 8 epochs lookups run one per lane; a long band costs a lane O(log n), never a loop over the band.
#pragma once
#include "stage.hpp"

namespace lcfe {

constexpr int ECOLOR_NCOL = 45;

struct EcolorLds {
    double fx[40];               // flux at (epoch e, band k = u..z): fx[5 * e + k]
    double out[ECOLOR_NCOL + 3];
};

// first index of t[0..n) with t >= x (t ascending)
LCFE_FN int lower_index(const double* t, int n, double x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (t[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// first index of t[0..n) with t > x (t ascending)
LCFE_FN int upper_index(const double* t, int n, double x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (t[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// get_flux_at_time (enhanced_colors.py:22-56) on a time-sorted band (t, f, n) at `target`, window 5 days.
// interp1d(kind='linear', bounds_error=False, fill_value=nan) on 1-D float64 data hands the window to np.interp
// and then fills points outside [x[0], x[-1]] with NaN; the branches below are np.interp's (numpy
// compiled_base.c, arr_interp): exact hit -> fp[j], a NaN from one side is retried from the other.
LCFE_FN double flux_at_time(const double* t, const double* f, int n, double target) {
    const double lo_t = target - 5.0, hi_t = target + 5.0;           // :37
    const int lo = lower_index(t, n, lo_t), hi = upper_index(t, n, hi_t);
    const int m = hi - lo;
    if (m < 2) return qnan();                                          // :39-40
    const double* x = t + lo;
    const double* y = f + lo;
    if (is_nan(target) || target < x[0] || target > x[m - 1]) return qnan();
    const int j = upper_index(x, m, target) - 1;                       // x[j] <= target < x[j + 1]
    if (j == m - 1 || x[j] == target) return y[j];
    const double slope = (y[j + 1] - y[j]) / (x[j + 1] - x[j]);
    double r = slope * (target - x[j]) + y[j];
    if (is_nan(r)) {
        r = slope * (target - x[j + 1]) + y[j + 1];
        if (is_nan(r) && y[j] == y[j + 1]) r = y[j];
    }
    return r;
}

// compute_color (enhanced_colors.py:59-78): NaN unless both fluxes are finite and positive
LCFE_FN double ecolor_color(double f1, double f2) {
    if (!(f1 > 0) || !(f2 > 0) || !__builtin_isfinite(f1) || !__builtin_isfinite(f2)) return qnan();
    return -2.5 * log10(f1 / f2);
}

// numpy's add.reduce of exactly 8 contiguous doubles v(0..7): the 8-way pairwise tree (below 8 it is a plain loop)
template <class F>
LCFE_FN double tree8(F v) {
    return ((v(0) + v(1)) + (v(2) + v(3))) + ((v(4) + v(5)) + (v(6) + v(7)));
}

// position (in band k's sorted segment) of Series.idxmax on the time-sorted band: the first maximum in time order,
// NaN fluxes skipped.  -1 if the band has no non-NaN flux.  Uniform over the wave.
template <class W, int CAP>
LCFE_FN int band_idxmax_skipna(const ObjLds<CAP>& L, int k) {
    const int s = uniform_int(L.boff[k]), n = uniform_int(L.boff[k + 1]) - s;
    const double* f = L.bf + s;
    bool have = false;
    double best = -__builtin_inf();
    for (int i = W::lane(); i < n; i += W::LANES) {
        const double v = f[i];
        if (!is_nan(v)) { have = true; best = (v > best) ? v : best; }
    }
    if (!W::any(have)) return -1;
    best = W::max(best);
    int cand = 0x7fffffff;
    for (int i = W::lane(); i < n; i += W::LANES)
        if (f[i] == best) { cand = i; break; }
    return uniform_int(W::min(cand));
}

template <class W, int CAP>
LCFE_FN void ecolor_object(const ObjLds<CAP>& L, EcolorLds& S) {
    const int lane = W::lane();
    double* o = S.out;
    // peak time: g band if it has rows, else r band (:96-107); neither -> all NaN.  A g band of only NaN fluxes makes the
    // reference raise (idxmax of an all-NaN column); it gets the NaN row here.
    const int kb = uniform_int((L.boff[2] > L.boff[1]) ? 1 : ((L.boff[3] > L.boff[2]) ? 2 : -1));
    const int p = (kb >= 0) ? band_idxmax_skipna<W, CAP>(L, kb) : -1;
    if (p < 0) {
        for (int q = lane; q < ECOLOR_NCOL; q += W::LANES) o[q] = qnan();
        W::sync();
        return;
    }
    const double peak = L.bt[L.boff[kb] + p];
    const int EP[8] = {0, 10, 20, 30, 50, 75, 100, 150};              // :110
    // 40 lookups (8 epochs x bands u..z), one per lane
    for (int q = lane; q < 40; q += W::LANES) {
        const int e = q / 5, k = q % 5;
        const int s = L.boff[k], n = L.boff[k + 1] - s;
        S.fx[q] = (n > 0) ? flux_at_time(L.bt + s, L.bf + s, n, peak + EP[e]) : qnan();
    }
    W::sync();
    // 32 colours: epoch-major, pair-minor; pair p = bands (p, p + 1) = ug, gr, ri, iz (:113-118, :151)
    for (int q = lane; q < 32; q += W::LANES) {
        const int e = q / 4, pp = q % 4;
        o[q] = ecolor_color(S.fx[5 * e + pp], S.fx[5 * e + pp + 1]);
    }
    W::sync();
    if (lane == 0) {
        // The finite colours of a pair in epoch order are read from o[] in place (no per-lane list: a dynamically
        // indexed array would live in scratch).  np.sum's order: a plain loop below 8 values, the pairwise tree at 8.
        for (int pp = 0; pp < 4; ++pp) {                                 // :159-168, np.std with ddof = 0
            double s = 0., mn = __builtin_inf(), mx = -__builtin_inf();
            int n = 0;
            for (int e = 0; e < 8; ++e) {
                const double c = o[4 * e + pp];
                if (__builtin_isfinite(c)) { s += c; ++n; mn = (c < mn) ? c : mn; mx = (c > mx) ? c : mx; }
            }
            double sd = qnan(), rg = qnan(), mean = qnan();
            if (n >= 3) {
                if (n == 8) s = tree8([&](int e) { return o[4 * e + pp]; });
                mean = s / n;
                double q = 0.;
                if (n == 8) {
                    q = tree8([&](int e) { const double d = o[4 * e + pp] - mean; return d * d; });
                } else {
                    for (int e = 0; e < 8; ++e) {
                        const double c = o[4 * e + pp];
                        if (__builtin_isfinite(c)) { const double d = c - mean; q += d * d; }
                    }
                }
                sd = sqrt(q / n);
                rg = mx - mn;
            }
            o[32 + 3 * pp] = sd;
            o[33 + 3 * pp] = rg;
            o[34 + 3 * pp] = mean;
        }
        // gr / ri correlation (:173-187): the two finite-colour lists zipped BY POSITION, truncated to the shorter one;
        // np.corrcoef = (c01 / (n - 1)) / sqrt(c00 / (n - 1)) / sqrt(c11 / (n - 1)), clipped to [-1, 1]
        int na = 0, nb = 0;
        for (int e = 0; e < 8; ++e) {
            na += __builtin_isfinite(o[4 * e + 1]) ? 1 : 0;
            nb += __builtin_isfinite(o[4 * e + 2]) ? 1 : 0;
        }
        const int m = (na < nb) ? na : nb;
        double r = qnan();
        if (na >= 2 && nb >= 2 && m >= 3) {
            double sa = 0., sb = 0.;
            if (m == 8) {
                sa = tree8([&](int e) { return o[4 * e + 1]; });
                sb = tree8([&](int e) { return o[4 * e + 2]; });
            } else {
                for (int i = 0, ea = 0, eb = 0; i < m; ++i, ++ea, ++eb) {
                    while (!__builtin_isfinite(o[4 * ea + 1])) ++ea;
                    while (!__builtin_isfinite(o[4 * eb + 2])) ++eb;
                    sa += o[4 * ea + 1];
                    sb += o[4 * eb + 2];
                }
            }
            const double ma = sa / m, mb = sb / m;
            double caa = 0, cbb = 0, cab = 0;
            for (int i = 0, ea = 0, eb = 0; i < m; ++i, ++ea, ++eb) {
                while (!__builtin_isfinite(o[4 * ea + 1])) ++ea;
                while (!__builtin_isfinite(o[4 * eb + 2])) ++eb;
                const double da = o[4 * ea + 1] - ma, db = o[4 * eb + 2] - mb;
                caa += da * da;
                cbb += db * db;
                cab += da * db;
            }
            const double inv = 1.0 / (m - 1);
            r = cab * inv / sqrt(caa * inv) / sqrt(cbb * inv);
            if (r < -1.0) r = -1.0;
            if (r > 1.0) r = 1.0;
        }
        o[44] = r;
    }
    W::sync();
}

template <class W, class G, int CAP>   // RunSet's hook (feature_sets.hpp); G: policy of one per-band pass or fit
LCFE_FN int run_object(const ObjLds<CAP>& L, const ObjIn&, EcolorLds& S, int32_t*) { ecolor_object<W, CAP>(L, S); return 0; }

}  // namespace lcfe
