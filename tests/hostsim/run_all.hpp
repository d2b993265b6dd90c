// run_all.hpp -- TEST INFRASTRUCTURE: one per-object set over a batch through RunSet on the one-lane WaveHost policy, with the
// object's working set SetLds<SET, CAP> in heap memory.  z may be NULL (every redshift NaN), status too (no status words
// wanted); light curves of more than CAP rows get the NaN row and status -100, as beyond the device's last tier.
#pragma once
#include <cstdint>
#include <memory>

#include "../../mallorn-astrophysics_amd/csrc/feature_sets.hpp"

template <int SET, int CAP>
static void run_all(int64_t n_obj, const int64_t* offsets, const double* t, const double* flux, const double* err,
                    const uint8_t* band, const double* z, double* out, int32_t* status) {
    using namespace lcfe;
    using W = WaveHost;
    auto ws = std::make_unique<SetLds<SET, CAP>>();
    constexpr int ncol = SetTraits<SET>::ncols, nst = SetTraits<SET>::nstatus;
    for (int64_t i = 0; i < n_obj; ++i) {
        const int64_t s = offsets[i];
        const int n = (int)(offsets[i + 1] - s);
        double* row = out + i * ncol;
        int32_t* st = (status && nst) ? status + i * nst : nullptr;
        if (n > CAP) {
            fill_row_nan<W>(row, ncol);
            for (int k = 0; k < nst; ++k) if (st) st[k] = -100;
            continue;
        }
        ObjIn in{t + s, flux + s, err + s, band + s, n, z ? z[i] : qnan()};
        RunSet<W, SET, CAP>::run(in, *ws, row, st);
    }
}
