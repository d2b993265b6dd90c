// variability.cpp -- TEST INFRASTRUCTURE (tests/test_variability_cpu.py compiles it with g++ into a temporary directory,
// once per capacity): the templates of the registered sets `cesium` and `fourier` (csrc/cesium.hpp, csrc/fourier.hpp)
// through RunSet on the one-lane WaveHost policy, with the object's working set SetLds<SET, VARIABILITY_CAP> in heap
// memory, and the log-normal-CDF of cesium.hpp on its own.  Light curves of more than VARIABILITY_CAP rows get the NaN row,
// as beyond the device's last tier.
#include "run_all.hpp"

using namespace lcfe;

#ifndef VARIABILITY_CAP
#define VARIABILITY_CAP 2048
#endif

extern "C" int variability_cap() { return VARIABILITY_CAP; }

// set: 14 = cesium, 15 = fourier; returns 1 for any other set
extern "C" int variability_extract(int set, int64_t n_obj, const int64_t* offsets, const double* t, const double* flux,
                                   const double* err, const uint8_t* band, double* out) {
    return for_set(set, [&](auto s) {
        if constexpr (s() == SET_CESIUM || s() == SET_FOURIER) {
            run_all<s(), VARIABILITY_CAP>(n_obj, offsets, t, flux, err, band, nullptr, out, nullptr);
            return 0;
        }
        return 1;
    }, 1);
}

// log of the standard normal CDF at x[0..n) and the scaled complementary error function at y[0..n) (y >= 1 / sqrt 2)
extern "C" void variability_log_ndtr(int64_t n, const double* x, double* out) {
    for (int64_t i = 0; i < n; ++i) out[i] = log_ndtr(x[i]);
}
extern "C" void variability_erfcx_tail(int64_t n, const double* y, double* out) {
    for (int64_t i = 0; i < n; ++i) out[i] = erfcx_tail(y[i]);
}
