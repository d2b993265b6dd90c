// gp_probe.hip -- device probe of the 2-D GP objective, gp_eval of csrc/gp.hpp, tier by tier.
//
// Test infrastructure (tests/test_gpu_gp_eval.py), never loaded by the product path.  The device branches of gp_eval and
// gp_sweep_inverse (Gram fill in D-operand layout, MFMA sweep, pivot look-ahead, masked gradient tile pass) exist only for
// 64-lane wavefronts, so the host simulation never runs them.  Here ONE workgroup stages prepared points and evaluates the
// objective at the parameter vectors the test chooses.  Every instantiation takes its policy, working-set type, matrix
// pointer type and launch bounds from csrc/gp_tiers.hpp exactly as gp_kernel<NP, GLOBAL_K> / gp_long_kernel of lcfe.hip do,
// and hands gp_eval its parameters through S.lb.x, as gp_object does.
//
// The probe's own code has no tickets, no atomics and no loop whose trip count depends on anything but the evaluation list
// (conventions of probe.hip: host pointers in, sizes checked on the host, one launch, guard bytes behind every output).
#include "gp_tiers.hpp"

#include "call.hpp"

#include <cmath>

using namespace lcfe;
using std::isfinite;

namespace {

constexpr int kGpMaxEvals = 16;            // evaluations of one call
constexpr int kScratchOverrun = -3;        // the guard region behind the Gram slab was written
constexpr int kGpTiers = kGpNumTiers + 1;   // + the long-object tier

struct GpProbeArgs {
    const double *t, *y, *e2;              // m prepared points: what gp_object leaves in S.t, S.y, S.e2
    const unsigned char* band;             // ... and hands to S.sm.set_band
    int m, ne;
    const int* n_e;                        // [ne] points of evaluation e (the first n_e of the m)
    const double* p_e;                     // [ne][4]
    const unsigned char* need;             // [ne] need_grad
    double *f, *g, *alpha;                 // [ne], [ne][4], [ne][astride]
    int astride;
};

template <class W, class LDS, class Ev>
__device__ __forceinline__ void gp_probe_run(const GpProbeArgs& a, LDS& S, Ev&& ev) {
    const int lane = W::lane();
    for (int i = lane; i < a.m; i += W::LANES) {
        S.t[i] = a.t[i];
        S.sm.set_band(i, a.band[i]);
        S.y[i] = a.y[i];
        S.e2[i] = a.e2[i];
    }
    W::sync();
    for (int k = 0; k < a.ne; ++k) {
        const int n = a.n_e[k];
        if (lane == 0)
            for (int c = 0; c < 4; ++c) S.lb.x[c] = a.p_e[4 * k + c];
        W::sync();
        double fe, ge[4];
        ev(S.lb.x, n, fe, ge, a.need[k] != 0);
        if (lane == 0) {
            a.f[k] = fe;
            for (int c = 0; c < 4; ++c) a.g[4 * k + c] = ge[c];
        }
        for (int i = lane; i < n; i += W::LANES) a.alpha[(size_t)k * a.astride + i] = S.alpha[i];
        W::sync();
    }
}

// the LDS and global-scratch tiers: a tier of the table, as gp_kernel<NP, GLOBAL_K> declares it
template <int NP, bool GLOBAL_K>
__global__ __launch_bounds__(gp_threads<NP>::T, (gp_waves<NP>::N)) void k_gp_eval(GpProbeArgs a, double* kscratch) {
    using Tier = GpTier<NP, GLOBAL_K>;
    __shared__ typename Tier::Set S;
    __shared__ double Klds[Tier::kLdsDoubles];
    gp_probe_run<typename Tier::W>(a, S, [&](const double* x, int n, double& f, double* g, bool need) {
        Tier::eval(S, Tier::matrix(Klds, kscratch), x, n, f, g, need); });
}

// the long-object tier, as gp_long_kernel declares it (working set in global memory)
__global__ __launch_bounds__(kGpLongThreads, 1) void k_gp_eval_long(GpProbeArgs a, double* kscratch, char* wset) {
    using Tier = GpLongTier;
    Tier::Set& S = *reinterpret_cast<Tier::Set*>(wset);
    gp_probe_run<Tier::W>(a, S, [&](const double* x, int n, double& f, double* g, bool need) { Tier::eval(S, kscratch, x, n, f, g, need); });
}

// tier ids of the ABI: the ids of LCFE_GP_TIERS, then the long-object tier
struct TierInfo { int np, threads, global_k, fuse, long_tier, compact; };
bool tier_info(int tier, TierInfo& o) {
    if (tier == kGpTiers - 1) { o = {kGpLongNP, kGpLongThreads, 1, 0, 1, GpLongTier::Set::kCompactTrips}; return true; }
    if (tier < 0 || tier >= kGpNumTiers) return false;
    // what the tier's kernel is built with, not the row it was built from
    switch (tier) {
#define X(id, NP, GK, ...) case id: { using S = GpTier<NP, GK>::Set; o = {NP, GpTier<NP, GK>::W::LANES, GK, S::kFuse, 0, S::kCompactTrips}; } break;
        LCFE_GP_TIERS(X)
#undef X
    }
    return true;
}

}  // namespace

extern "C" {

int devprobe_gp_tiers() { return kGpTiers; }
int devprobe_gp_max_evals() { return kGpMaxEvals; }

// o[6]: row capacity NP, threads of the workgroup, matrix in global scratch, fused sweep, working set in global memory,
// compacted trip lists
int devprobe_gp_tier_info(int tier, int* o) {
    TierInfo ti;
    if (!tier_info(tier, ti)) return kBadShape;
    o[0] = ti.np; o[1] = ti.threads; o[2] = ti.global_k; o[3] = ti.fuse; o[4] = ti.long_tier; o[5] = ti.compact;
    return 0;
}

// One workgroup of tier `tier` stores the m prepared points and evaluates the objective ne times, evaluation e on the first
// n_e[e] points at p_e[e][0..4) with need_grad = need[e].  f: [ne], g: [ne][4], alpha: [ne][m] (row e: its first n_e[e] slots).
int devprobe_gp_eval(int tier, int m, const double* t, const unsigned char* band, const double* y, const double* e2, int ne,
                     const int* n_e, const double* p_e, const unsigned char* need, double* f, double* g, double* alpha) {
    TierInfo ti;
    if (!tier_info(tier, ti)) return kBadShape;
    // gp_object's window: at least 10 points, and room for the augmented row
    if (m < 10 || m + 1 > ti.np || ne < 1 || ne > kGpMaxEvals) return kBadSize;
    for (int i = 0; i < m; ++i)
        if (band[i] >= 6 || !isfinite(t[i]) || !isfinite(y[i]) || !isfinite(e2[i])) return kBadSize;
    for (int e = 0; e < ne; ++e) {
        if (n_e[e] < 10 || n_e[e] > m || need[e] > 1) return kBadSize;
        for (int c = 0; c < 4; ++c)
            if (!isfinite(p_e[4 * e + c])) return kBadSize;
    }
    Call c;
    GpProbeArgs a;
    a.t = c.in(t, m);
    a.y = c.in(y, m);
    a.e2 = c.in(e2, m);
    a.band = c.in(band, m);
    a.m = m;
    a.ne = ne;
    a.n_e = c.in(n_e, ne);
    a.p_e = c.in(p_e, (size_t)4 * ne);
    a.need = c.in(need, ne);
    a.f = c.out(f, ne);
    a.g = c.out(g, (size_t)4 * ne);
    a.alpha = c.out(alpha, (size_t)ne * m);
    a.astride = m;
    // Gram slab of the global-scratch tiers (one workgroup's share of the product's slab) with a guard region of its own,
    // sentinel-filled like the product's never-initialised scratch may be anything
    const size_t kbytes = ti.global_k ? (size_t)gp_store_doubles(ti.np) * sizeof(double) : 0;
    unsigned char* ks = (unsigned char*)c.alloc(kbytes + kPad);
    if (ks) c.err = hipMemset(ks, kFill, kbytes + kPad);
    char* ws = nullptr;
    if (ti.long_tier) {
        const size_t wbytes = GpLongTier::kSetBytes;
        ws = (char*)c.alloc(wbytes);
        if (ws && c.ok()) c.err = hipMemset(ws, kFill, wbytes);
    }
    if (c.ok()) {
        switch (tier) {
#define X(id, NP, GK, ...) case id: k_gp_eval<NP, GK><<<1, gp_threads<NP>::T>>>(a, (double*)ks); break;
            LCFE_GP_TIERS(X)
#undef X
            default: k_gp_eval_long<<<1, kGpLongThreads>>>(a, (double*)ks, ws); break;
        }
    }
    unsigned char guard[kPad];
    bool guard_read = false;
    if (c.ok()) c.err = hipGetLastError();
    if (c.ok()) c.err = hipDeviceSynchronize();
    if (c.ok()) { c.err = hipMemcpy(guard, ks + kbytes, kPad, hipMemcpyDeviceToHost); guard_read = c.ok(); }
    const int rc = c.finish();
    if (rc != 0) return rc;
    if (guard_read)
        for (int i = 0; i < kPad; ++i)
            if (guard[i] != kFill) return kScratchOverrun;
    return 0;
}

}  // extern "C"
