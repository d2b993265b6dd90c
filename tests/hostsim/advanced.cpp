// advanced.cpp -- TEST INFRASTRUCTURE (tests/test_advanced_cpu.py compiles it with g++ into a temporary directory, once
// per capacity): the templates of the extension set `advanced` (csrc/advanced.hpp) through RunSet on the one-lane
// WaveHost policy, with the object's working set SetLds<SET_ADVANCED, ADVANCED_CAP> in heap memory.  Light curves of more
// than ADVANCED_CAP rows get the NaN row and status -100, as beyond the device's last tier.
#include "run_all.hpp"

using namespace lcfe;

#ifndef ADVANCED_CAP
#define ADVANCED_CAP 2048
#endif

extern "C" int advanced_cap() { return ADVANCED_CAP; }

// z may be NULL (every redshift NaN); status: one word per object
extern "C" int advanced_extract(int64_t n_obj, const int64_t* offsets, const double* t, const double* flux, const double* err,
                                const uint8_t* band, const double* z, double* out, int32_t* status) {
    run_all<SET_ADVANCED, ADVANCED_CAP>(n_obj, offsets, t, flux, err, band, z, out, status);
    return 0;
}
