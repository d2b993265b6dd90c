// gp_resample.cpp -- TEST INFRASTRUCTURE: the query and write passes of the GP-resampled copies (csrc/gp_resample.hpp) compiled
// for the host with the one-lane WaveHost policy.  tests/test_gp_resample_cpu.py compiles it as a shared library (the two
// functions below) and as a stand-alone program -- `main` runs a hand-computed three-row case and is what a sanitizer build
// (-fsanitize=address,undefined) runs.  Never loaded by the product package.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../mallorn-astrophysics_amd/csrc/gp_resample.hpp"

using namespace lcfe;

extern "C" int gp_resample_query_host(int64_t n_src, int k, int origin, const int64_t* offsets, const double* t, const double* flux,
                                      const double* err, const uint8_t* band, const double* z_old, const int64_t* copy_offsets,
                                      const double* copy_t, const uint8_t* copy_band, const double* z_new, const double* shift, int64_t* q_off,
                                      double* q_t, double* q_lam) {
    if (k < 1 || n_src < 0 || (origin != GP_GRID_FROM_PEAK && origin != GP_GRID_FROM_FIRST)) return 1;
    const GpResSource S{offsets, t, flux, err, band, z_old};
    const GpResCopies C{copy_offsets, copy_t, nullptr, copy_band, k};
    const GpResPlan P{z_new, nullptr, nullptr, shift, nullptr};
    for (int64_t o = 0; o < n_src; ++o) gp_res_query_object<WaveHost>(S, C, P, o, n_src, origin, q_off, q_t, q_lam);
    return 0;
}

extern "C" int gp_resample_write_host(int64_t n_copies, int k, const int64_t* copy_offsets, const double* copy_err, const double* mean,
                                      const double* var, const double* dim, const double* noise, const uint64_t* seed, const double* n1,
                                      const double* n2, const int32_t* src_status, int n_status, double* flux_out, double* err_out,
                                      int32_t* status_out) {
    if (k < 1 || n_copies < 0 || n_copies % k || (n1 == nullptr) != (n2 == nullptr) || (!n1 && !seed)) return 1;
    const GpResCopies C{copy_offsets, nullptr, copy_err, nullptr, k};
    const GpResPlan P{nullptr, dim, noise, nullptr, seed ? seed : reinterpret_cast<const uint64_t*>(dim)};
    for (int64_t oc = 0; oc < n_copies; ++oc)
        gp_res_write_copy<WaveHost>(C, P, oc, mean, var, n1, n2, src_status, n_status, flux_out, err_out, status_out);
    return 0;
}

// Self-check on one source of three rows (bands r, g, unknown; the r row is the peak) with two copies: a neutral one and one
// at s = 2 with shift 1.5, dim 0.5, noise 2.  Every expected number below is worked out by hand from the formulas.
int main() {
    const int64_t off[2] = {0, 3}, coff[3] = {0, 3, 6};
    const double t[3] = {100.0, 104.0, 108.0}, f[3] = {5.0, 9.0, 7.0}, e[3] = {1.0, 2.0, 3.0};
    const uint8_t b[3] = {2, 1, 255};
    const double z_old[1] = {1.0}, z_new[2] = {1.0, 3.0}, shift[2] = {0.0, 1.5};
    const double ct[6] = {100.0, 104.0, 108.0, 101.5, 105.5, 109.5};
    const uint8_t cb[6] = {2, 1, 255, 2, 1, 255};
    int64_t q_off[2];
    double q_t[6], q_lam[6];
    int fails = 0;
    auto check = [&](bool ok, const char* what) { if (!ok) { std::printf("FAILED: %s\n", what); ++fails; } };
    check(gp_resample_query_host(1, 2, GP_GRID_FROM_PEAK, off, t, f, e, b, z_old, coff, ct, cb, z_new, shift, q_off, q_t, q_lam) == 0, "query runs");
    // the peak is the r row (t = 100): the neutral copy asks at its own times from the peak and its bands' wavelengths
    check(q_off[0] == 0 && q_off[1] == 6, "q_off");
    check(q_t[0] == 0.0 && q_t[1] == 4.0 && q_lam[0] == 6222.0 && q_lam[1] == 4825.0, "neutral copy: own time and wavelength");
    check(std::isnan(q_t[2]) && std::isnan(q_lam[2]) && std::isnan(q_t[5]) && std::isnan(q_lam[5]), "unknown filter asks for NaN");
    // s = (1 + 3) / (1 + 1) = 2: (101.5 - 1.5 - 100) / 2 = 0, (105.5 - 1.5 - 100) / 2 = 2; 6222 / 2, 4825 / 2
    check(q_t[3] == 0.0 && q_t[4] == 2.0 && q_lam[3] == 3111.0 && q_lam[4] == 2412.5, "copy at s = 2");
    check(gp_resample_query_host(1, 2, GP_GRID_FROM_FIRST, off, t, f, e, b, z_old, coff, ct, cb, z_new, shift, q_off, q_t, q_lam) == 0 &&
          q_t[1] == 4.0 && q_t[4] == 2.0, "first origin: the first valid row is t = 100 too");
    const double ce[6] = {1.0, 2.0, 3.0, 1.0, 2.0, 3.0};
    const double mean[6] = {10.0, 20.0, std::nan(""), 10.0, 20.0, std::nan("")}, var[6] = {4.0, -1.0, 1.0, 4.0, 9.0, 1.0};
    const double dim[2] = {1.0, 0.5}, noise[2] = {0.0, 2.0}, n1[6] = {0, 0, 0, 1.0, -1.0, 0}, n2[6] = {0, 0, 0, 0.5, 2.0, 0};
    const int32_t st[4] = {2, 17, 21, 3};
    double fo[6], eo[6];
    int32_t so[2];
    check(gp_resample_write_host(2, 2, coff, ce, mean, var, dim, noise, nullptr, n1, n2, st, 4, fo, eo, so) == 0, "write runs");
    // neutral: flux = mu, err_out = sqrt(err^2 + sd^2): sqrt(1 + 4), and sqrt(4 + 0) for the negative variance
    check(fo[0] == 10.0 && fo[1] == 20.0 && eo[0] == std::sqrt(5.0) && eo[1] == 2.0, "neutral copy");
    check(std::isnan(fo[2]) && std::isnan(eo[2]) && std::isnan(fo[5]) && std::isnan(eo[5]), "NaN point: NaN flux and error");
    // 0.5 (10 + 2 * 1) + (1 * 2) * 0.5 = 7;  sqrt(1 * 5 + (0.5 * 2)^2) = sqrt(6)
    // 0.5 (20 + 3 * -1) + (2 * 2) * 2 = 16.5;  sqrt(4 * 5 + (0.5 * 3)^2) = sqrt(22.25)
    check(fo[3] == 7.0 && eo[3] == std::sqrt(6.0) && fo[4] == 16.5 && eo[4] == std::sqrt(22.25), "copy with dim, noise and normals");
    check(so[0] == 2 && so[1] == 2, "status word 0 of the source");
    const uint64_t seed[2] = {0x0123456789ABCDEFull, 42};
    double f2[6], e2[6];
    check(gp_resample_write_host(2, 2, coff, ce, mean, var, dim, noise, seed, nullptr, nullptr, st, 4, fo, eo, so) == 0 &&
          gp_resample_write_host(2, 2, coff, ce, mean, var, dim, noise, seed, nullptr, nullptr, st, 4, f2, e2, so) == 0, "Philox mode runs");
    check(fo[3] == f2[3] && fo[4] == f2[4] && fo[0] == f2[0] && std::isfinite(fo[3]) && fo[0] != 10.0, "Philox mode repeats itself");
    std::printf(fails ? "gp_resample self-check: %d failures\n" : "gp_resample self-check: ok\n", fails);
    return fails ? 1 : 0;
}
