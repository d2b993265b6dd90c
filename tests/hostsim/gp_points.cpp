// gp_points.cpp -- TEST INFRASTRUCTURE: the 2-D GP's posterior at scattered points (csrc/gp.hpp: gp_object with a
// GpGridTail over a GpPointSpec, gp_grid_stage) compiled for the host with the one-lane WaveHost policy, on the row
// capacities of the small tiers.  tests/test_gp_points_cpu.py compiles it twice: as a shared library (gp_points_host below)
// and as a stand-alone program -- `main` runs a self-check on a synthetic light curve and is what a sanitizer build
// (-fsanitize=address,undefined) runs.  Never loaded by the product package.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <vector>

#include "../../mallorn-astrophysics_amd/csrc/gp.hpp"

using namespace lcfe;

namespace {

template <int NP>
void run(const ObjIn& in, const GpPointSpec& G, const double* theta_in, double* mean, double* var, double* theta_out, double* row27,
         int32_t* status) {
    using W = WaveHost;
    auto S = std::make_unique<GpLds<NP, 1>>();
    std::vector<double> K((size_t)gp_store_doubles(NP));
    const GpGridTail<double*, GpPointSpec> tail{theta_in != nullptr, G, K.data(), theta_in, theta_out, mean, var};
    gp_object<W, NP>(in, *S, [&](const double* x, int nn, double& f, double* g, bool need) {
        gp_eval<W, NP, double*>(x, nn, *S, K.data(), f, g, need); }, status, tail);
    if (row27)
        for (int k = 0; k < GP_NCOL; ++k) row27[k] = S->out[k];
}

}  // namespace

// One light curve of n_rows rows (CSR slice) through the tier its row count bins into (capacities up to 240 rows), asked at
// nq points.  Arguments as lcfe_gp2d_points_device's for one light curve, all on the host; outputs are NaN until the stage
// writes them.  Returns 1 outside the limits.
extern "C" int gp_points_host(int n_rows, const double* t, const double* flux, const double* err, const uint8_t* band, int nq,
                              const double* q_t, const double* q_lam, int origin, const double* theta_in, double* mean, double* var,
                              double* theta_out, double* row27, int32_t* status) {
    if (n_rows < 0 || n_rows > 239 || nq < 0 || (origin != GP_GRID_FROM_PEAK && origin != GP_GRID_FROM_FIRST)) return 1;
    const GpPointSpec G{q_t, q_lam, nq, origin};
    for (int g = 0; g < nq; ++g) { mean[g] = qnan(); if (var) var[g] = qnan(); }
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

// Self-check: a 70-row light curve (the 112-row tier) in fit mode at 35 points -- three passes, the last partial --, two of
// them bad; then the same points without the bad ones, in given mode at the fitted parameters.  The good points must agree
// bit for bit (a bad point leaves its pass alone, given mode repeats fit mode), the bad ones must be NaN, and a list of no
// points must run.  Exit status 0: all held.
int main() {
    const int n = 70, nq = 35;
    std::vector<double> t(n), f(n), e(n);
    std::vector<uint8_t> b(n);
    for (int i = 0; i < n; ++i) {
        t[i] = 59000.0 + 1.7 * i + 0.3 * ((i * 7) % 5);
        b[i] = (uint8_t)((i * 5) % 6);
        const double x = (t[i] - 59040.0) / 18.0;
        f[i] = 40.0 * std::exp(-0.5 * x * x) * (1.0 + 0.1 * b[i]) + 2.0 * std::sin(1.3 * i);
        e[i] = 1.0 + 0.05 * ((i * 3) % 7);
    }
    std::vector<double> qt(nq), ql(nq);
    for (int g = 0; g < nq; ++g) {
        qt[g] = -30.0 + 4.1 * g;
        ql[g] = 3000.0 + 260.0 * g;
    }
    const int bad_t = 5, bad_l = 20;
    qt[bad_t] = std::nan("");
    ql[bad_l] = -1.0;
    std::vector<double> mean(nq), var(nq), row(GP_NCOL);
    double theta[4], theta2[4];
    int32_t st[8] = {0};
    int fails = 0;
    auto check = [&](bool ok, const char* what) { if (!ok) { std::printf("FAILED: %s\n", what); ++fails; } };
    check(gp_points_host(n, t.data(), f.data(), e.data(), b.data(), nq, qt.data(), ql.data(), GP_GRID_FROM_PEAK, nullptr, mean.data(),
                         var.data(), theta, row.data(), st) == 0, "fit mode runs");
    check(st[3] == n && std::isfinite(theta[0]) && std::isfinite(row[5]), "the fit has a GP");
    for (int g = 0; g < nq; ++g) {
        const bool bad = (g == bad_t || g == bad_l);
        check(bad ? (std::isnan(mean[g]) && std::isnan(var[g])) : (std::isfinite(mean[g]) && std::isfinite(var[g])), "NaN exactly at the bad points");
    }
    std::vector<double> qt2, ql2, m1, v1;
    for (int g = 0; g < nq; ++g)
        if (g != bad_t && g != bad_l) { qt2.push_back(qt[g]); ql2.push_back(ql[g]); m1.push_back(mean[g]); v1.push_back(var[g]); }
    std::vector<double> m2(qt2.size()), v2(qt2.size());
    check(gp_points_host(n, t.data(), f.data(), e.data(), b.data(), (int)qt2.size(), qt2.data(), ql2.data(), GP_GRID_FROM_PEAK, theta,
                         m2.data(), v2.data(), theta2, nullptr, st) == 0, "given mode runs");
    for (size_t g = 0; g < qt2.size(); ++g) check(m1[g] == m2[g] && v1[g] == v2[g], "good points do not depend on the bad ones nor on the mode");
    check(gp_points_host(n, t.data(), f.data(), e.data(), b.data(), 0, nullptr, nullptr, GP_GRID_FROM_FIRST, nullptr, nullptr, nullptr,
                         theta2, row.data(), st) == 0 && theta2[0] == theta[0] && theta2[3] == theta[3], "no points: the fit alone");
    // nine rows: no GP, NaN at every point, the set's status words
    check(gp_points_host(9, t.data(), f.data(), e.data(), b.data(), nq, qt.data(), ql.data(), GP_GRID_FROM_FIRST, nullptr, mean.data(),
                         var.data(), theta2, row.data(), st) == 0 && st[3] == 9, "nine rows run");
    for (int g = 0; g < nq; ++g) check(std::isnan(mean[g]) && std::isnan(var[g]), "no GP: NaN at all points");
    std::printf(fails ? "gp_points self-check: %d failures\n" : "gp_points self-check: ok\n", fails);
    return fails ? 1 : 0;
}
