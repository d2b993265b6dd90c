// gp_grid.cpp -- TEST INFRASTRUCTURE: the 2-D GP's grid stage (csrc/gp.hpp: gp_object with a GpGridTail, gp_grid_stage)
// compiled for the host with the one-lane WaveHost policy, on the row capacities of the small tiers.  Compiled by
// tests/test_gp_grid_cpu.py; never loaded by the product package.
#include <cstdint>
#include <memory>
#include <vector>

#include "../../mallorn-astrophysics_amd/csrc/gp.hpp"

using namespace lcfe;

namespace {

template <int NP>
void run(const ObjIn& in, const GpGridSpec& G, const double* theta_in, double* mean, double* var, double* theta_out, double* row27,
         int32_t* status) {
    using W = WaveHost;
    auto S = std::make_unique<GpLds<NP, 1>>();
    std::vector<double> K((size_t)gp_store_doubles(NP));
    const GpGridTail<double*> tail{theta_in != nullptr, G, K.data(), theta_in, theta_out, mean, var};
    gp_object<W, NP>(in, *S, [&](const double* x, int nn, double& f, double* g, bool need) {
        gp_eval<W, NP, double*>(x, nn, *S, K.data(), f, g, need); }, status, tail);
    if (row27)
        for (int k = 0; k < GP_NCOL; ++k) row27[k] = S->out[k];
}

}  // namespace

// One light curve of n_rows rows (CSR slice) through the tier its row count bins into (capacities up to 240 rows).  Arguments
// as lcfe_gp2d_grid_device's, all on the host; outputs are NaN until the stage writes them.  Returns 1 outside the limits.
extern "C" int gp_grid_host(int n_rows, const double* t, const double* flux, const double* err, const uint8_t* band, int n_times,
                            const double* offsets, int origin, int n_bands, const int* bands, const double* theta_in, double* mean,
                            double* var, double* theta_out, double* row27, int32_t* status) {
    if (n_rows < 0 || n_rows > 239 || n_times < 1 || n_times > GP_GRID_MAX_TIMES || n_bands < 1 || n_bands > GP_GRID_MAX_BANDS) return 1;
    unsigned codes = 0;
    for (int b = 0; b < n_bands; ++b) {
        if (bands[b] < 0 || bands[b] > 5) return 1;
        codes |= (unsigned)bands[b] << (4 * b);
    }
    const GpGridSpec G{offsets, n_times, n_bands, origin, codes};
    for (int g = 0; g < n_times * n_bands; ++g) { mean[g] = qnan(); if (var) var[g] = qnan(); }
    for (int k = 0; k < 4; ++k) theta_out[k] = qnan();
    const ObjIn in{t, flux, err, band, n_rows, qnan()};
    switch (gp_bin_of(n_rows)) {
        case 0: run<64>(in, G, theta_in, mean, var, theta_out, row27, status); break;
        case 1: run<112>(in, G, theta_in, mean, var, theta_out, row27, status); break;
        case 2: run<160>(in, G, theta_in, mean, var, theta_out, row27, status); break;
        case 3: run<240>(in, G, theta_in, mean, var, theta_out, row27, status); break;
        default: return 1;
    }
    return 0;
}
