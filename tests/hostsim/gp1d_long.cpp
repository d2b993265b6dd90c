// gp1d_long.cpp -- TEST INFRASTRUCTURE (tests/test_gp1d_long_cpu.py compiles it with g++ into a temporary directory):
// the per-band GP objective gp1d_eval at the capacity of the long-object tier (NP = 2048) with its working set in heap
// memory, Gp1dLds<..., IN_LDS = false> -- the layout the device keeps in a slab of global scratch -- on the one-lane
// WaveHost policy.  The caller stages normalised data (times in [0, 1], standardised flux, alpha_i) itself.
#include <cstdint>
#include <memory>
#include <vector>

#include "../../mallorn-astrophysics_amd/csrc/gp1d.hpp"

using namespace lcfe;

constexpr int NP = 2048;

extern "C" int gp1d_long_np() { return NP; }

// f = -LML(theta), g = -dLML/dtheta for each of the n_theta parameter vectors; returns 1 if n + 1 > NP
extern "C" int gp1d_long_eval(int n, const double* t, const double* y, const double* alpha, int n_theta, const double* theta,
                              double* f, double* g) {
    if (n + 1 > NP) return 1;
    using W = WaveHost;
    auto S = std::make_unique<Gp1dLds<NP, 1, false>>();
    static_assert(!Gp1dLds<NP, 1, false>::kInLds, "working set outside LDS");
    std::vector<double> K((size_t)gp_store_doubles(NP));
    for (int i = 0; i < n; ++i) { S->t[i] = t[i]; S->y[i] = y[i]; S->e2[i] = alpha[i]; }
    for (int k = 0; k < n_theta; ++k) gp1d_eval<W, NP, double*>(theta + 3 * k, n, *S, K.data(), f[k], g + 3 * k);
    return 0;
}
