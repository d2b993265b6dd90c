// postpeak.cpp -- TEST INFRASTRUCTURE (tests/test_postpeak_cpu.py compiles it with g++ into a temporary directory, once
// per capacity): the ecolor / decline templates (csrc/ecolor.hpp, csrc/decline.hpp) through RunSet on the one-lane
// WaveHost policy, with the object's working set SetLds<SET, POSTPEAK_CAP> in heap memory.  Light curves of more than
// POSTPEAK_CAP rows get the NaN row, as beyond the device's last tier.
#include <cstdint>
#include <memory>

#include "../../mallorn-astrophysics_amd/csrc/feature_sets.hpp"

using namespace lcfe;

#ifndef POSTPEAK_CAP
#define POSTPEAK_CAP 2048
#endif

extern "C" int postpeak_cap() { return POSTPEAK_CAP; }

template <int SET>
static void run_all(int64_t n_obj, const int64_t* offsets, const double* t, const double* flux, const double* err,
                    const uint8_t* band, double* out) {
    using W = WaveHost;
    auto ws = std::make_unique<SetLds<SET, POSTPEAK_CAP>>();
    const int ncol = set_ncols(SET);
    for (int64_t i = 0; i < n_obj; ++i) {
        const int64_t s = offsets[i];
        const int n = (int)(offsets[i + 1] - s);
        double* row = out + i * ncol;
        if (n > POSTPEAK_CAP) {
            fill_row_nan<W>(row, ncol);
            continue;
        }
        ObjIn in{t + s, flux + s, err + s, band + s, n, qnan()};
        RunSet<W, SET, POSTPEAK_CAP>::run(in, *ws, row, nullptr);
    }
}

// set: 10 = ecolor, 11 = decline; returns 1 for any other set
extern "C" int postpeak_extract(int set, int64_t n_obj, const int64_t* offsets, const double* t, const double* flux,
                                const double* err, const uint8_t* band, double* out) {
    switch (set) {
        case SET_ECOLOR: run_all<SET_ECOLOR>(n_obj, offsets, t, flux, err, band, out); return 0;
        case SET_DECLINE: run_all<SET_DECLINE>(n_obj, offsets, t, flux, err, band, out); return 0;
    }
    return 1;
}
