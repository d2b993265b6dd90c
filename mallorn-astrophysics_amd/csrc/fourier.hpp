// fourier.hpp -- frequency-domain features (reference: src/features/fourier_features.py,
// extract_fourier_features_single_band) -> 24 columns: per band u..y fourier_dominant_freq, fourier_dominant_power,
// fourier_power_ratio, fourier_spectral_entropy.
//
// Per band: the rows with a finite flux are compacted (in time order), interpolated onto n = min(rows, 128) equidistant
// times (np.interp), centred and weighted by np.hanning(n); the power of the bins 1 .. n/2 - 1 is a direct DFT, one
// frequency bin per lane, with a table of the n twiddle factors indexed by j k mod n (n is any integer from 10 to 128, so
// there is no radix to exploit, and at most 63 x 128 complex products per band do not call for one).
//
// The reference hands np.interp the band's rows in FILE order; here they are in time order (stable by time, file index),
// which is the same thing for a band whose rows arrive in time order, and the reference's result for the sorted light curve
// otherwise.
#pragma once
#include "stage.hpp"
#include "advanced.hpp"      // np_interp_at

namespace lcfe {

constexpr int FOURIER_NCOL = 24;
constexpr int FOURIER_NMAX = 128;     // :57
constexpr int FOURIER_NMIN = 10;      // :34, :46

template <int CAP>
struct FourierLds {
    double x[CAP], y[CAP];            // times and fluxes of a band's finite rows
    double u[FOURIER_NMAX];           // the windowed signal
    double twc[FOURIER_NMAX], tws[FOURIER_NMAX];
    double pw[FOURIER_NMAX / 2];      // pw[k - 1] = power of bin k
    double out[FOURIER_NCOL];
};

template <class W, int CAP>
LCFE_FN void fourier_band(const double* t, const double* f, int m, FourierLds<CAP>& S, double* o) {
    const int lane = W::lane();
    double res[4] = {qnan(), qnan(), qnan(), qnan()};
    // rows with finite time and flux, in order (:42-44)
    int mc = 0;
    if (m < FOURIER_NMIN) m = 0;                                           // :34
    for (int base = 0; base < m; base += W::LANES) {
        const int i = base + lane;
        const bool ok = i < m && __builtin_isfinite(f[i]) && __builtin_isfinite(t[i]);
        const unsigned long long b = W::ballot(ok);
        if (ok) { const int p = mc + W::prefix(b); S.x[p] = t[i]; S.y[p] = f[i]; }
        mc += popcll(b);
    }
    W::sync();
    if (mc >= FOURIER_NMIN) {                                              // :46
        const int n = (mc < FOURIER_NMAX) ? mc : FOURIER_NMAX;
        const double t_min = S.x[0], t_max = S.x[mc - 1];
        // np.linspace(t_min, t_max, n): arange(n) * step + start, the last one set to the stop (:58)
        const double delta = t_max - t_min, div = (double)(n - 1), step = delta / div;
        const double PI = 3.141592653589793;
        double a_u = 0;
        for (int j = lane; j < n; j += W::LANES) {
            double tu = (step == 0) ? ((double)j / div) * delta + t_min : (double)j * step + t_min;
            if (j == n - 1) tu = t_max;
            const double v = np_interp_at(S.x, S.y, mc, tu);               // :61
            S.u[j] = v;
            a_u += v;
            const double ang = 2.0 * PI * (double)j / (double)n;
            S.twc[j] = cos(ang);
            S.tws[j] = sin(ang);
        }
        const double mean = W::sum(a_u) / (double)n;                       // :64
        for (int j = lane; j < n; j += W::LANES) {
            const double win = 0.5 + 0.5 * cos(PI * (double)(1 - n + 2 * j) / div);      // np.hanning (:67)
            S.u[j] = (S.u[j] - mean) * win;
        }
        W::sync();
        // power of the bins 1 .. n / 2 - 1 (:71-85): X_k = sum_j u_j (cos - i sin)(2 pi j k / n)
        const int nb = n / 2 - 1;
        for (int k0 = 0; k0 < nb; k0 += W::LANES) {
            const int k = k0 + lane + 1;
            if (k <= nb) {
                double re = 0, im = 0;
                int q = 0;
                for (int j = 0; j < n; ++j) {
                    const double uj = S.u[j];
                    re += uj * S.twc[q];
                    im -= uj * S.tws[q];
                    q += k;
                    q -= (q >= n) ? n : 0;
                }
                const double a = hypot(re, im);                            // np.abs(fft) ** 2
                S.pw[k - 1] = a * a;
            }
        }
        W::sync();
        // :87-115
        double a_p = 0, pmax = -__builtin_inf();
        bool pnan = false;
        for (int i = lane; i < nb; i += W::LANES) { const double p = S.pw[i]; a_p += p; pmax = (p > pmax) ? p : pmax; pnan = pnan || is_nan(p); }
        const double total = W::sum(a_p);
        pmax = W::max(pmax);
        const bool any_nan = W::any(pnan);
        if (any_nan || pmax != 0) {                                        // np.max(power) == 0 -> four NaN (:87)
            const int d = uniform_int(wave_argmax_first<W>(S.pw, nb));     // :97
            const double dt = (t_max - t_min) / (double)(n - 1);           // :79
            const double dom_f = fabs((double)(d + 1) * (1.0 / ((double)n * dt)));       // np.fft.fftfreq (:80, :98)
            const double dom_p = S.pw[d];
            const double ratio = dom_p / (total / (double)nb + 1e-10);     // :102-103
            double a_e = 0;
            int cnt = 0;
            for (int i = lane; i < nb; i += W::LANES) {
                const double pn = S.pw[i] / (total + 1e-10);               // :107
                if (pn > 1e-10) { a_e += pn * log2(pn + 1e-10); ++cnt; }   // :109-110
            }
            cnt = W::sum(cnt);
            double ent = -W::sum(a_e);
            const double max_ent = log2((double)cnt);                      // :113
            if (max_ent > 0) ent = ent / max_ent;
            res[0] = dom_f; res[1] = dom_p; res[2] = ratio; res[3] = ent;
        }
    }
    if (lane == 0) { o[0] = res[0]; o[1] = res[1]; o[2] = res[2]; o[3] = res[3]; }
    W::sync();
}

template <class W, int CAP>
LCFE_FN void fourier_object(const ObjLds<CAP>& L, FourierLds<CAP>& S) {
    for (int k = 0; k < 6; ++k) {
        const int s = uniform_int(L.boff[k]), n = uniform_int(L.boff[k + 1]) - s;
        fourier_band<W, CAP>(L.bt + s, L.bf + s, n, S, S.out + 4 * k);
    }
}

template <class W, class G, int CAP>   // RunSet's hook (feature_sets.hpp); G: policy of one per-band pass or fit
LCFE_FN int run_object(const ObjLds<CAP>& L, const ObjIn&, FourierLds<CAP>& S, int32_t*) { fourier_object<W, CAP>(L, S); return 0; }

}  // namespace lcfe
