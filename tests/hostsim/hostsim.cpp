// hostsim.cpp -- TEST INFRASTRUCTURE: the kernel templates of mallorn-astrophysics_amd/csrc
// compiled for the host with the one-lane WaveHost policy (reductions are identities), so the
// feature arithmetic can be checked against the oracle in the GPU-less build container and run
// under -fsanitize=address,undefined.  Never loaded by the product package.
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "run_all.hpp"
#include "../../mallorn-astrophysics_amd/csrc/workspace.hpp"

using namespace lcfe;

#ifndef HOSTSIM_CAP
#define HOSTSIM_CAP 2048
#endif

extern "C" int hostsim_max_points() { return HOSTSIM_CAP; }

// the GP kernel has its own working set (Gram matrix) and reads the CSR slice directly; like the
// device it uses the 8-wide sweep for short light curves and the 16-wide one for long ones
static void run_gp(int64_t n_obj, const int64_t* offsets, const double* t, const double* flux, const double* err,
                   const uint8_t* band, double* out, int32_t* status) {
    using W = WaveHost;
    constexpr int NS = 176, NL = 512;      // NL = 512 exercises the 16-wide sweep
    auto ws = std::make_unique<GpLds<NS, 1>>();
    auto wl = std::make_unique<GpLds<NL, 1>>();
    std::vector<double> K((size_t)gp_store_doubles(NL));
    for (int64_t i = 0; i < n_obj; ++i) {
        const int64_t s = offsets[i];
        const int n = (int)(offsets[i + 1] - s);
        ObjIn in{t + s, flux + s, err + s, band + s, n, qnan()};
        int32_t* st = status ? status + set_nstatus(SET_GP2D) * i : nullptr;
        const double* o;
        // like the device: the small working set for short light curves, the large one otherwise
        if (n + 1 <= NS) {
            gp_object<W, NS>(in, *ws, [&](const double* x, int nn, double& f, double* g, bool need) {
                gp_eval<W, NS, double*>(x, nn, *ws, K.data(), f, g, need); }, st);
            o = ws->out;
        } else {
            gp_object<W, NL>(in, *wl, [&](const double* x, int nn, double& f, double* g, bool need) {
                gp_eval<W, NL, double*>(x, nn, *wl, K.data(), f, g, need); }, st);
            o = wl->out;
        }
        for (int k = 0; k < GP_NCOL; ++k) out[i * GP_NCOL + k] = o[k];
    }
}

// the objective alone (tests/test_gp_eval_cpu.py; the device counterpart is tests/devprobe/gp_probe.hip): m prepared
// points -- what gp_object leaves in S.t, S.y, S.e2 and hands to S.sm.set_band -- and ne evaluations, evaluation e on the
// first n_e[e] points at p_e[e][0..4).  f: [ne], g: [ne][4], alpha: [ne][m].  Returns 1 on sizes outside the working set.
extern "C" int hostsim_gp_eval(int m, const double* t, const uint8_t* band, const double* y, const double* e2, int ne,
                               const int* n_e, const double* p_e, const uint8_t* need, double* f, double* g, double* alpha) {
    using W = WaveHost;
    constexpr int NP = 240;
    if (m < 1 || m + 1 > NP || ne < 0) return 1;
    for (int i = 0; i < m; ++i)
        if (band[i] >= 6) return 1;
    for (int e = 0; e < ne; ++e)
        if (n_e[e] < 1 || n_e[e] > m) return 1;
    auto S = std::make_unique<GpLds<NP, 1>>();
    std::vector<double> K((size_t)gp_store_doubles(NP));
    for (int i = 0; i < m; ++i) { S->t[i] = t[i]; S->sm.set_band(i, band[i]); S->y[i] = y[i]; S->e2[i] = e2[i]; }
    for (int e = 0; e < ne; ++e) {
        gp_eval<W, NP, double*>(p_e + 4 * e, n_e[e], *S, K.data(), f[e], g + 4 * e, need[e] != 0);
        for (int i = 0; i < n_e[e]; ++i) alpha[(size_t)e * m + i] = S->alpha[i];
    }
    return 0;
}

// the tier table of the 2-D GP (csrc/gp_tier_table.hpp), for the tests' own restatements of it (tests/test_gp_tier_table_cpu.py)
extern "C" int hostsim_gp_tiers() { return kGpNumTiers; }
// o[8]: row capacity NP, first row count, cap, threads, matrix in global scratch, fused sweep, compacted trip lists, slabs
extern "C" int hostsim_gp_tier_info(int ti, int* o) {
    if (ti < 0 || ti >= kGpNumTiers) return 1;
    const GpTierRow& r = kGpTierTable[ti];
    const int v[8] = {r.np, gp_tier_first(ti), gp_tier_cap(ti), r.threads, r.global_k, r.fuse, r.compact, r.slabs};
    // the binning agrees with the caps: a tier takes its first count and its cap, and nothing beyond
    if (gp_bin_of(v[1]) != ti || gp_bin_of(v[2]) != ti || gp_bin_of(v[2] + 1) != ti + 1 || gp_cap_of(ti) != v[2]) return 2;
    for (int k = 0; k < 8; ++k) o[k] = v[k];
    return 0;
}

// the band-length tiers of the fit-by-fit kernels (csrc/fit_tier_table.hpp) and the object-level cap behind them
// (csrc/workspace.hpp), for the tests' own restatements (tests/test_fit_tier_table_cpu.py)
extern "C" int hostsim_fit_tiers() { return kFitTiers; }
// o[5]: rows of one band, lanes per fit, lane groups per wave, has kernels of its own, the tier whose kernels run its list
extern "C" int hostsim_fit_tier_info(int t, int* o) {
    if (t < 0 || t >= kFitTiers) return 1;
    const FitTierRow& r = kFitTierTable[t];
    const int v[5] = {fit_tier_cap(t), r.lanes, r.groups, r.kernel, fit_tier_host(t)};
    for (int k = 0; k < 5; ++k) o[k] = v[k];
    return 0;
}
extern "C" int hostsim_fit_tier_of(int m, int narrow) { return fit_tier_of(m, narrow); }
extern "C" int hostsim_fit_object_rows() { return kFitObjectRows; }

extern "C" int hostsim_extract(int set, int64_t n_obj, const int64_t* offsets, const double* t,
                               const double* flux, const double* err, const uint8_t* band,
                               const double* z, double* out, int32_t* status) {
    if (set == SET_GP2D) { run_gp(n_obj, offsets, t, flux, err, band, out, status); return 0; }
    // the per-object sets up to `research` (the later ones have libraries of their own)
    return for_set(set, [&](auto s) {
        if constexpr (s() <= SET_RESEARCH && SetTraits<s()>::per_object) {
            run_all<s(), HOSTSIM_CAP>(n_obj, offsets, t, flux, err, band, z, out, status);
            return 0;
        }
        return 1;
    }, 1);
}

// ---- per-band 1-D GP (csrc/gp1d.hpp): the four bands g, r, i, z of every object, one after the other
#include "../../mallorn-astrophysics_amd/csrc/gp1d.hpp"

extern "C" int hostsim_gp1d(int64_t n_obj, const int64_t* offsets, const double* t, const double* flux, const double* err,
                            const uint8_t* band, double* out, int32_t* status) {
    using W = WaveHost;
    constexpr int NP = 256;
    auto obj = std::make_unique<ObjLds<HOSTSIM_CAP>>();
    auto ws = std::make_unique<Gp1dLds<NP, 1>>();
    std::vector<double> K((size_t)gp_store_doubles(NP));
    for (int64_t i = 0; i < n_obj; ++i) {
        const int64_t s = offsets[i];
        const int n = (int)(offsets[i + 1] - s);
        double* o = out + i * GP1D_NCOL;
        for (int k = 0; k < GP1D_NCOL; ++k) o[k] = qnan();
        if (n > HOSTSIM_CAP) continue;
        ObjIn in{t + s, flux + s, err + s, band + s, n, qnan()};
        stage_object<W, HOSTSIM_CAP>(in, *obj);
        bool fitted[4];
        for (int j = 0; j < 4; ++j) {
            const int b = j + 1;                                   // g, r, i, z
            const int bs = obj->boff[b], m = obj->boff[b + 1] - bs;
            fitted[j] = m >= 5;
            // gp1d_band takes the band's valid rows only (on the device: csrc/gp1d_rows.hpp)
            std::vector<double> vt, vf, ve;
            for (int r = bs; r < bs + m; ++r)
                if (!is_nan(obj->bf[r]) && !is_nan(obj->be[r]) && obj->be[r] > 0) { vt.push_back(obj->bt[r]); vf.push_back(obj->bf[r]); ve.push_back(obj->be[r]); }
            gp1d_band<W, NP>([&](int r, double& tt, double& ff, double& ee) { tt = vt[r]; ff = vf[r]; ee = ve[r]; }, (int)vt.size(), *ws,
                             [&](const double* x, int nn, double& f, double* g) { gp1d_eval<W, NP, double*>(x, nn, *ws, K.data(), f, g); },
                             o + 4 * j, status ? status + i * GP1D_NSTATUS + j : nullptr);
        }
        gp1d_cross_band(o, fitted);
    }
    return 0;
}

// the per-band objective alone (tests/test_gp1d_eval_cpu.py; the device counterpart is tests/devprobe/gp1d_probe.hip): m
// prepared points -- what gp1d_band leaves in S.t, S.y, S.e2 -- and ne evaluations, evaluation e on the first n_e[e] points
// at th_e[e][0..3).  f: [ne], g: [ne][3], alpha: [ne][m].  Returns 1 on sizes outside the working set.
extern "C" int hostsim_gp1d_eval(int m, const double* t, const double* y, const double* e2, int ne, const int* n_e,
                                 const double* th_e, double* f, double* g, double* alpha) {
    using W = WaveHost;
    constexpr int NP = 768;
    if (m < 1 || m + 1 > NP || ne < 0) return 1;
    for (int e = 0; e < ne; ++e)
        if (n_e[e] < 1 || n_e[e] > m) return 1;
    auto S = std::make_unique<Gp1dLds<NP, 1>>();
    std::vector<double> K((size_t)gp_store_doubles(NP));
    for (int i = 0; i < m; ++i) { S->t[i] = t[i]; S->y[i] = y[i]; S->e2[i] = e2[i]; }
    for (int e = 0; e < ne; ++e) {
        gp1d_eval<W, NP, double*>(th_e + 3 * e, n_e[e], *S, K.data(), f[e], g + 3 * e);
        for (int i = 0; i < n_e[e]; ++i) alpha[(size_t)e * m + i] = S->alpha[i];
    }
    return 0;
}

// ---- bounded L-BFGS-B (csrc/lbfgsb_box.hpp) with the objective supplied by the caller: the test
// drives it with the same Python function it hands to scipy.optimize.minimize.
#include "../../mallorn-astrophysics_amd/csrc/lbfgsb_box.hpp"

typedef void (*hostsim_fg_t)(const double* x, double* f, double* g);

extern "C" int hostsim_lbfgsb_box3(double* x, const double* lo, const double* hi, hostsim_fg_t fg, int maxiter,
                                   int maxfun, double factr, double pgtol, double* f_out, int* n_iter, int* n_eval,
                                   double* trace, int trace_cap) {
    double Sm[10][3], Ym[10][3];
    double xx[3] = {x[0], x[1], x[2]}, f = 0;
    int nt = 0;
    auto ev = [&](const double* p, double& fv, double* gv) {
        fg(p, &fv, gv);
        if (trace && nt < trace_cap) { trace[4 * nt] = p[0]; trace[4 * nt + 1] = p[1]; trace[4 * nt + 2] = p[2]; trace[4 * nt + 3] = fv; ++nt; }
    };
    const int rc = lcfe::lbfgsb_box_minimize<3, 10>(xx, lo, hi, f, ev, maxiter, maxfun, factr, pgtol, 20, *n_iter, *n_eval, Sm, Ym);
    for (int i = 0; i < 3; ++i) x[i] = xx[i];
    *f_out = f;
    return rc;
}

// ---- unbounded L-BFGS-B (csrc/lbfgsb.hpp), the 2-D GP's driver, by itself (tests/test_lbfgsb_cpu.py): the product's
// constants -- factr 1e7, pgtol 1e-5, maxls 20 (gp_object's lb_start) -- and M = 10 pairs over 4 variables.
// Closed loop: lbfgsb_minimize on the caller's objective, the same Python function the test hands to scipy.
extern "C" int hostsim_lbfgsb4(double* x, hostsim_fg_t fg, int maxiter, double* f_out, int* n_iter, int* n_eval) {
    auto S = std::make_unique<LbState<4, 10>>();
    double xx[4] = {x[0], x[1], x[2], x[3]}, f = 0;
    auto ev = [&](const double* p, double& fv, double* gv) { fg(p, &fv, gv); };
    const int why = lbfgsb_minimize<4, 10>(xx, f, ev, maxiter, 1e7, 1e-5, 20, *n_iter, *n_eval, *S);
    for (int i = 0; i < 4; ++i) x[i] = xx[i];
    *f_out = f;
    return why;
}

// Replay of a recorded run (tests/lb_reference.py): lb_start, then for k < ne the taped f[k], g[k][4] are stored and
// lb_advance<4, 10> is called; stops at the first result other than LB_EVAL or at the end of the tape.  x_out: [ne + 1][4],
// the requested point after every step (row 0 = x0); why, n_iter, n_eval: [ne] per step; x_final[4], f_final.  Returns the
// number of steps taken.  The device counterpart is tests/devprobe/lb_probe.hip.
extern "C" int hostsim_lb_replay(const double* x0, int maxiter, int ne, const double* tape_f, const double* tape_g,
                                 double* x_out, int* why, int* n_iter, int* n_eval, double* x_final, double* f_final) {
    auto S = std::make_unique<LbState<4, 10>>();
    lb_start(*S, x0, maxiter, 1e7, 1e-5, 20);
    for (int i = 0; i < 4; ++i) x_out[i] = S->x[i];
    int k = 0;
    while (k < ne) {
        S->f = tape_f[k];
        for (int i = 0; i < 4; ++i) S->g[i] = tape_g[4 * k + i];
        const int w = lb_advance<4, 10>(*S);
        why[k] = w; n_iter[k] = S->n_iter; n_eval[k] = S->n_eval;
        ++k;
        for (int i = 0; i < 4; ++i) x_out[4 * k + i] = S->x[i];
        if (w != LB_EVAL) break;
    }
    for (int i = 0; i < 4; ++i) x_final[i] = S->x[i];
    *f_final = S->f;
    return k;
}
