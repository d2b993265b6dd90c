// advanced.cpp -- TEST INFRASTRUCTURE (tests/test_advanced_cpu.py compiles it with g++ into a temporary directory, once
// per capacity): the templates of the extension set `advanced` (csrc/advanced.hpp) through RunSet on the one-lane
// WaveHost policy, with the object's working set SetLds<SET_ADVANCED, ADVANCED_CAP> in heap memory.  Light curves of more
// than ADVANCED_CAP rows get the NaN row and status -100, as beyond the device's last tier.
#include <cstdint>
#include <memory>

#include "../../mallorn-astrophysics_amd/csrc/feature_sets.hpp"

using namespace lcfe;

#ifndef ADVANCED_CAP
#define ADVANCED_CAP 2048
#endif

extern "C" int advanced_cap() { return ADVANCED_CAP; }

// z may be NULL (every redshift NaN); status: one word per object
extern "C" int advanced_extract(int64_t n_obj, const int64_t* offsets, const double* t, const double* flux, const double* err,
                                const uint8_t* band, const double* z, double* out, int32_t* status) {
    using W = WaveHost;
    auto ws = std::make_unique<SetLds<SET_ADVANCED, ADVANCED_CAP>>();
    const int ncol = set_ncols(SET_ADVANCED);
    for (int64_t i = 0; i < n_obj; ++i) {
        const int64_t s = offsets[i];
        const int n = (int)(offsets[i + 1] - s);
        double* row = out + i * ncol;
        if (n > ADVANCED_CAP) {
            fill_row_nan<W>(row, ncol);
            status[i] = -100;
            continue;
        }
        ObjIn in{t + s, flux + s, err + s, band + s, n, z ? z[i] : qnan()};
        RunSet<W, SET_ADVANCED, ADVANCED_CAP>::run(in, *ws, row, status + i);
    }
    return 0;
}
