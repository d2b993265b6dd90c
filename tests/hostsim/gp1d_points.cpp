// gp1d_points.cpp -- TEST INFRASTRUCTURE (tests/test_gp1d_points_cpu.py compiles it with g++ into a temporary directory):
// the per-band GP's posterior at a caller's times (csrc/gp1d_points.hpp: gp1d_band with Gp1dPointsTail, the 2-D GP's grid
// stage with the Gp1dPointSpec column source) on the one-lane WaveHost policy, at a row capacity of the device's tier
// table (csrc/gp1d_tiers.hpp) chosen per call.  One light curve per call, its rows in time order; the queries are grouped
// by band with the stable counting pass the device kernel makes.  Built as a program, its `main` is a self-check.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <vector>

#include "../../mallorn-astrophysics_amd/csrc/gp1d_points.hpp"

using namespace lcfe;

namespace {

template <int NP, bool IN_LDS>
int run(int n, const double* t, const double* f, const double* e, const uint8_t* band, int nq, const double* q_t, const uint8_t* q_band,
        const double* theta_in, double* mean, double* sd, double* theta_out, double* norm, double* cols, int32_t* status) {
    using W = WaveHost;
    auto S = std::make_unique<Gp1dLds<NP, 1, IN_LDS>>();
    std::vector<double> K((size_t)gp_store_doubles(NP));
    for (int q = 0; q < nq; ++q) mean[q] = sd[q] = qnan();
    for (int k = 0; k < GP1D_NBAND * GP1D_NTHETA; ++k) theta_out[k] = qnan();
    for (int k = 0; k < GP1D_NBAND * GP1D_NNORM; ++k) norm[k] = qnan();
    std::vector<int> perm;
    int qoff[GP1D_NBAND + 1] = {0};
    for (int j = 0; j < GP1D_NBAND; ++j) {
        for (int q = 0; q < nq; ++q)
            if (q_band[q] == j + 1) perm.push_back(q);
        qoff[j + 1] = (int)perm.size();
    }
    for (int j = 0; j < GP1D_NBAND; ++j) {
        std::vector<double> vt, vf, ve;
        for (int r = 0; r < n; ++r)
            if (band[r] == j + 1 && !is_nan(f[r]) && !is_nan(e[r]) && e[r] > 0) { vt.push_back(t[r]); vf.push_back(f[r]); ve.push_back(e[r]); }
        const Gp1dPointsTail<double*> tail{theta_in != nullptr, K.data(), theta_in ? theta_in + GP1D_NTHETA * j : nullptr,
                                          theta_out + GP1D_NTHETA * j, norm + GP1D_NNORM * j, q_t, perm.data() + qoff[j], qoff[j + 1] - qoff[j],
                                          mean, sd};
        gp1d_band<W, NP, IN_LDS>([&](int r, double& tt, double& ff, double& ee) { tt = vt[r]; ff = vf[r]; ee = ve[r]; }, (int)vt.size(), *S,
                                 [&](const double* x, int nn, double& fv, double* gv) { gp1d_eval<W, NP, double*, IN_LDS>(x, nn, *S, K.data(), fv, gv); },
                                 cols + 4 * j, status + j, tail);
    }
    return 0;
}

}  // namespace

// np: a row capacity of the tier table (32 and 64: the wave path; 64, 112, 160: the workgroup path; 768: the long band;
// 2048: the long-object tier, working set outside LDS).  theta_in [4][3] or null (fit mode).  mean, sd [nq]; theta_out
// [4][3]; norm [4][4]; cols [16]; status [4].  Returns 1 for an unknown capacity.
extern "C" int gp1d_points_host(int np, int n, const double* t, const double* f, const double* e, const uint8_t* band, int nq,
                                const double* q_t, const uint8_t* q_band, const double* theta_in, double* mean, double* sd,
                                double* theta_out, double* norm, double* cols, int32_t* status) {
#define ARGS n, t, f, e, band, nq, q_t, q_band, theta_in, mean, sd, theta_out, norm, cols, status
    switch (np) {
        case 32: return run<32, true>(ARGS);
        case 64: return run<64, true>(ARGS);
        case 112: return run<112, true>(ARGS);
        case 160: return run<160, true>(ARGS);
        case 768: return run<768, true>(ARGS);
        case 2048: return run<2048, false>(ARGS);
        default: return 1;
    }
#undef ARGS
}

// what the stage stores for a posterior variance v (the clamp at 0 and the square root)
extern "C" double gp1d_points_spread(double v) { return GpStageModel<Gp1dPointSpec>::spread(v, 1.0); }

// self-check: a 21-row band against the textbook formulas in plain loops (Cholesky solve), given mode, 17 queries with a
// bad one; the other bands have no rows
int main() {
    const int n = 21, nq = 17;
    std::vector<double> t(n), f(n), e(n), qt(nq);
    std::vector<uint8_t> b(n, 2), qb(nq, 2);
    for (int i = 0; i < n; ++i) { t[i] = 60000.0 + 3.7 * i + 0.3 * std::sin(1.0 * i); f[i] = 10.0 + 4.0 * std::sin(0.45 * i); e[i] = 0.3 + 0.02 * (i % 5); }
    for (int q = 0; q < nq; ++q) qt[q] = 59990.0 + 6.1 * q;
    qt[5] = std::nan("");
    qb[9] = 7;
    double theta[12];
    for (int k = 0; k < 12; ++k) theta[k] = std::nan("");
    theta[3] = std::log(1.3); theta[4] = std::log(0.15); theta[5] = std::log(0.05);
    std::vector<double> mean(nq), sd(nq);
    double th_out[12], norm[16], cols[16];
    int32_t st[4];
    if (gp1d_points_host(32, n, t.data(), f.data(), e.data(), b.data(), nq, qt.data(), qb.data(), theta, mean.data(), sd.data(), th_out, norm, cols, st))
        return 1;
    const double tmin = norm[4], tr = norm[5], fm = norm[6], fs = norm[7];
    const double c = 1.3, l = 0.15, s2 = 0.05;
    std::vector<double> x(n), y(n), L(n * n, 0.0);
    for (int i = 0; i < n; ++i) { x[i] = (t[i] - tmin) / tr; y[i] = (f[i] - fm) / fs; }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) {
            double k = c * std::exp(-0.5 * (x[i] - x[j]) * (x[i] - x[j]) / (l * l));
            if (i == j) { const double a = (e[i] / fs) * (e[i] / fs); k += s2 + (a < 1e-10 ? 1e-10 : a); }
            for (int p = 0; p < j; ++p) k -= L[i * n + p] * L[j * n + p];
            L[i * n + j] = (i == j) ? std::sqrt(k) : k / L[j * n + j];
        }
    auto solve_l = [&](std::vector<double> v) {
        for (int i = 0; i < n; ++i) { for (int p = 0; p < i; ++p) v[i] -= L[i * n + p] * v[p]; v[i] /= L[i * n + i]; }
        return v;
    };
    const std::vector<double> z = solve_l(y);
    int bad = 0;
    for (int q = 0; q < nq; ++q) {
        if (q == 5 || q == 9) { bad += !(std::isnan(mean[q]) && std::isnan(sd[q])); continue; }
        double xs = (qt[q] - tmin) / tr;
        xs = xs < 0 ? 0 : (xs > 1 ? 1 : xs);
        std::vector<double> ks(n);
        for (int i = 0; i < n; ++i) ks[i] = c * std::exp(-0.5 * (xs - x[i]) * (xs - x[i]) / (l * l));
        const std::vector<double> v = solve_l(ks);
        double m = 0, vv = c + s2;
        for (int i = 0; i < n; ++i) { m += v[i] * z[i]; vv -= v[i] * v[i]; }
        const double s = std::sqrt(vv < 0 ? 0 : vv);
        if (!(std::fabs(mean[q] - m) <= 1e-9 * (1 + std::fabs(m)) && std::fabs(sd[q] - s) <= 1e-8)) {
            std::printf("query %d: mean %.17g want %.17g sd %.17g want %.17g\n", q, mean[q], m, sd[q], s);
            ++bad;
        }
    }
    if (st[1] != 1 || st[0] != 0 || !std::isnan(cols[0]) || std::isnan(cols[4])) ++bad;
    std::printf(bad ? "self-check: FAILED\n" : "self-check: ok\n");
    return bad ? 1 : 0;
}
