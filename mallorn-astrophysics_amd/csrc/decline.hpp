// decline.hpp -- time to decline (reference: src/features/time_to_decline.py, extract_time_to_decline_single)
// -> 36 columns: per band u..y the time from the peak to 80 / 60 / 40 / 20 / 10 % of the peak flux, and the
// decline velocity.
//
// Per band: the peak is one wave reduction (wave_argmax_first: numpy.argmax, a NaN wins), the post-peak rows are
// a suffix of the time-sorted segment (one binary search), and the first crossing of all five thresholds is one
// ballot per threshold and 64-row chunk, so a long band is scanned by the whole wavefront and the scan stops at the
// chunk where the last threshold is crossed.
#pragma once
#include "stage.hpp"

namespace lcfe {

constexpr int DECLINE_NCOL = 36;

struct DeclineLds {
    double out[DECLINE_NCOL + 4];
};

template <class W, int CAP>
LCFE_FN void decline_object(const ObjLds<CAP>& L, DeclineLds& S) {
    const int lane = W::lane();
    const double THR[5] = {0.8, 0.6, 0.4, 0.2, 0.1};                     // :123
    for (int k = 0; k < 6; ++k) {
        const int s = uniform_int(L.boff[k]), n = uniform_int(L.boff[k + 1]) - s;
        const double* t = L.bt + s;
        const double* f = L.bf + s;
        double res[5] = {qnan(), qnan(), qnan(), qnan(), qnan()};
        bool valid = false;
        if (n >= 3) {                                                     // :131, :35
            const int p = uniform_int(wave_argmax_first<W>(f, n));        // :39 (first maximum, a NaN wins)
            const double pt = t[p], pf = f[p];
            valid = uniform_int(!is_nan(pt) && !is_nan(pf)) != 0;        // :144
            if (valid) {
                // post-peak rows (:63): t > pt, i.e. the rows from the first one after the last row of time pt
                int lo = p + 1, hi = n;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (t[mid] <= pt) lo = mid + 1; else hi = mid;
                }
                const int q0 = uniform_int(lo);
                double target[5];
                int first[5];
#pragma unroll
                for (int m = 0; m < 5; ++m) { target[m] = pf * THR[m]; first[m] = -1; }    // :77
                // first post-peak row with flux < target, per threshold (:80-86); a NaN flux is never below
                for (int base = q0; base < n; base += W::LANES) {
                    const int i = base + lane;
                    const double v = (i < n) ? f[i] : qnan();
                    bool done = true;
#pragma unroll
                    for (int m = 0; m < 5; ++m) {
                        const unsigned long long b = W::ballot(v < target[m]);
                        if (first[m] < 0 && b != 0ull) first[m] = base + __builtin_ctzll(b);
                        done = done && first[m] >= 0;
                    }
                    if (done) break;
                }
#pragma unroll
                for (int m = 0; m < 5; ++m) {
                    const int j = first[m];
                    if (j < 0) continue;
                    double crossing;
                    if (j > q0) {                                         // :89-100
                        const double t1 = t[j - 1], t2 = t[j], f1 = f[j - 1], f2 = f[j];
                        crossing = (f1 != f2) ? t1 + (target[m] - f1) * (t2 - t1) / (f2 - f1) : t2;
                    } else {
                        crossing = t[j];                                  // :102
                    }
                    res[m] = crossing - pt;                               // :105
                }
            }
        }
        double vel = qnan();                                              // :161-173
        if (valid) {
            int nfin = 0;
            for (int m = 0; m < 5; ++m) nfin += __builtin_isfinite(res[m]) ? 1 : 0;
            const double t80 = res[0], t20 = res[3];
            if (nfin >= 2 && __builtin_isfinite(t80) && __builtin_isfinite(t20) && t20 > t80) vel = (0.8 - 0.2) / (t20 - t80);
        }
        if (lane == 0) {
            for (int m = 0; m < 5; ++m) S.out[6 * k + m] = res[m];
            S.out[6 * k + 5] = vel;
        }
    }
    W::sync();
}

template <class W, class G, int CAP>   // RunSet's hook (feature_sets.hpp); G: policy of one per-band pass or fit
LCFE_FN int run_object(const ObjLds<CAP>& L, const ObjIn&, DeclineLds& S, int32_t*) { decline_object<W, CAP>(L, S); return 0; }

}  // namespace lcfe
