// postpeak.cpp -- TEST INFRASTRUCTURE (tests/test_postpeak_cpu.py compiles it with g++ into a temporary directory, once
// per capacity): the ecolor / decline templates (csrc/ecolor.hpp, csrc/decline.hpp) through RunSet on the one-lane
// WaveHost policy, with the object's working set SetLds<SET, POSTPEAK_CAP> in heap memory.  Light curves of more than
// POSTPEAK_CAP rows get the NaN row, as beyond the device's last tier.
#include "run_all.hpp"

using namespace lcfe;

#ifndef POSTPEAK_CAP
#define POSTPEAK_CAP 2048
#endif

extern "C" int postpeak_cap() { return POSTPEAK_CAP; }

// set: 10 = ecolor, 11 = decline; returns 1 for any other set
extern "C" int postpeak_extract(int set, int64_t n_obj, const int64_t* offsets, const double* t, const double* flux,
                                const double* err, const uint8_t* band, double* out) {
    return for_set(set, [&](auto s) {
        if constexpr (s() == SET_ECOLOR || s() == SET_DECLINE) {
            run_all<s(), POSTPEAK_CAP>(n_obj, offsets, t, flux, err, band, nullptr, out, nullptr);
            return 0;
        }
        return 1;
    }, 1);
}
