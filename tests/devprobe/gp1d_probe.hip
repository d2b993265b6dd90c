// gp1d_probe.hip -- device probe of the per-band GP objective, gp1d_eval of csrc/gp1d.hpp, shape by shape.
//
// Test infrastructure (tests/test_gpu_gp1d_eval.py), never loaded by the product path.  gp1d_eval has a Gram fill and a
// gradient pass of its own and instantiates gp_sweep_inverse in forms the 2-D probe never builds (no look-ahead, no fused
// pass; one wavefront of a 256-thread workgroup under wave-level fences; 256 threads on 64 .. 2048 rows); the host
// simulation runs none of them.  Here ONE workgroup stages prepared points and evaluates the objective at the parameter
// vectors the test chooses.  Every shape takes its policy, working-set type, matrix pointer type, thread count and launch
// bounds from csrc/gp1d_tiers.hpp exactly as gp1d_kernel<NP, ROWCAP, T, WNP, MW> / gp1d_long_kernel of lcfe.hip do, and
// hands gp1d_eval its parameters in a private array, as lbfgsb_box_minimize does.
//
//   shapes 0..2  phase 1 of gp1d_kernel tiers 0..2: the four wavefronts side by side, each on WaveOfBlock with its own
//                Gp1dWaveLds<WNP> slice of the raw LDS buffer
//   shapes 3..5  phase 2 of tiers 0..2: the whole workgroup on Gp1dBlockLds<NP, 4> in the same buffer
//   shape 6      phase 3 of the last tier: working set of a kGp1dLongNP-row fit aliased on the raw LDS buffer, matrix in
//                global scratch
//   shape 7      gp1d_long_kernel: matrix AND working set (Gp1dLongTierWs) in global scratch
//
// The probe's own code has no tickets, no atomics and no loop whose trip count depends on anything but the evaluation list
// (conventions of probe.hip: host pointers in, sizes checked on the host, one launch, guard bytes behind every output).
#include "gp1d_tiers.hpp"

#include "call.hpp"

#include <cmath>

using namespace lcfe;
using std::isfinite;

namespace {

constexpr int kGp1dMaxEvals = 16;          // evaluations of one point set in one call
constexpr int kScratchOverrun = -3;        // the guard region behind the Gram slab was written
constexpr int kGp1dShapes = 8;
constexpr int kSets = kGp1dThreads / 64;   // point sets of a wave shape: one per wavefront
enum { kPathWave = 0, kPathBlock = 1, kPathLong = 2 };

struct KernelTier { int np, rowcap, wnp, mw; };
constexpr KernelTier kTier[kGp1dKernelTiers] = {
#define X(id, NP, ROWCAP, WNP, MW) {NP, ROWCAP, WNP, MW},
    LCFE_GP1D_KERNEL_TIERS(X)
#undef X
};
constexpr int kSlabTier = kGp1dKernelTiers - 1;              // the tier with ROWCAP > NP
static_assert(kTier[kSlabTier].rowcap > kTier[kSlabTier].np && kTier[kSlabTier - 1].rowcap == kTier[kSlabTier - 1].np, "one slab tier, last");
static_assert(kSets == 4 && kSlabTier == 3, "shape ids of the ABI");

struct Gp1dProbeSet {
    const double *t, *y, *e2;              // m prepared points: what gp1d_band leaves in S.t, S.y, S.e2
    int m, ne;
    const int* n_e;                        // [ne] points of evaluation e (the first n_e of the m)
    const double* th_e;                    // [ne][3]
    double *f, *g, *alpha;                 // [ne], [ne][3], [ne][astride]
    int astride;
};
struct Gp1dProbeArgs { Gp1dProbeSet s[kSets]; };

template <class W, int NP, class LDS, class KP>
__device__ __forceinline__ void gp1d_probe_run(const Gp1dProbeSet& a, LDS& S, KP K) {
    const int lane = W::lane();
    for (int i = lane; i < a.m; i += W::LANES) {
        S.t[i] = a.t[i];
        S.y[i] = a.y[i];
        S.e2[i] = a.e2[i];
    }
    W::sync();
    for (int k = 0; k < a.ne; ++k) {
        const int n = a.n_e[k];
        const double th[3] = {a.th_e[3 * k], a.th_e[3 * k + 1], a.th_e[3 * k + 2]};
        double fe, ge[3];
        gp1d_eval<W, NP, KP>(th, n, S, K, fe, ge);
        if (lane == 0) {
            a.f[k] = fe;
            for (int c = 0; c < 3; ++c) a.g[3 * k + c] = ge[c];
        }
        for (int i = lane; i < n; i += W::LANES) a.alpha[(size_t)k * a.astride + i] = S.alpha[i];
        W::sync();
    }
}

// phase 1 of gp1d_kernel<NP, ROWCAP, kGp1dThreads, WNP, MW>: wavefront j on point set j (m = 0: it skips, as under the
// product's `if (nvalid(j) + 1 <= WNP)`)
template <int TI>
__global__ __launch_bounds__(kGp1dThreads, kTier[TI].mw) void k_gp1d_wave(Gp1dProbeArgs a) {
    constexpr int NP = kTier[TI].np, WNP = kTier[TI].wnp;
    __shared__ __attribute__((aligned(16))) unsigned char raw[gp1d_lds_bytes<NP, kGp1dThreads, WNP>()];
    const int j = threadIdx.x >> 6;
    const Gp1dProbeSet& s = a.s[j];
    if (s.m > 0) {
        auto& LW = reinterpret_cast<Gp1dWaveLds<WNP>*>(raw)[j];
        gp1d_probe_run<WaveOfBlock, WNP>(s, LW.S, (lds_double*)LW.K);
    }
    __syncthreads();
}

// phase 2: the whole workgroup on the NP-row layout of the same buffer
template <int TI>
__global__ __launch_bounds__(kGp1dThreads, kTier[TI].mw) void k_gp1d_block(Gp1dProbeArgs a) {
    using W = BlockDev<kGp1dThreads>;
    constexpr int NP = kTier[TI].np, WNP = kTier[TI].wnp;
    __shared__ __attribute__((aligned(16))) unsigned char raw[gp1d_lds_bytes<NP, kGp1dThreads, WNP>()];
    auto& LB = *reinterpret_cast<Gp1dBlockLds<NP, W::NWAVES>*>(raw);
    gp1d_probe_run<W, NP>(a.s[0], LB.S, (lds_double*)LB.K);
    __syncthreads();
}

// phase 3 (ROWCAP > NP): the working set of a kGp1dLongNP-row fit aliases the raw buffer, the matrix is this workgroup's slab
template <int TI>
__global__ __launch_bounds__(kGp1dThreads, kTier[TI].mw) void k_gp1d_slab(Gp1dProbeArgs a, double* kslab) {
    using W = BlockDev<kGp1dThreads>;
    constexpr int NP = kTier[TI].np, WNP = kTier[TI].wnp;
    static_assert(kTier[TI].rowcap > NP && kTier[TI].rowcap == kGp1dLongNP, "the tier of the long bands");
    __shared__ __attribute__((aligned(16))) unsigned char raw[gp1d_lds_bytes<NP, kGp1dThreads, WNP>()];
    static_assert(sizeof(Gp1dLds<kGp1dLongNP, W::NWAVES>) <= sizeof(raw), "long-band working set must fit the LDS buffer");
    auto& LG = *reinterpret_cast<Gp1dLds<kGp1dLongNP, W::NWAVES>*>(raw);
    double* Kg = kslab;
    gp1d_probe_run<W, kGp1dLongNP>(a.s[0], LG, (global_double*)Kg);
    __syncthreads();
}

// the long-object tier: the declarations of gp1d_long_kernel
__global__ __launch_bounds__(kGp1dThreads, 1) void k_gp1d_long(Gp1dProbeArgs a, double* kslab, char* wset) {
    constexpr int NP = kGp1dLongTierNP;
    using W = BlockDev<kGp1dThreads>;
    double* Kg = kslab;
    Gp1dLongTierWs& S = *reinterpret_cast<Gp1dLongTierWs*>(wset);
    gp1d_probe_run<W, NP>(a.s[0], S, (global_double*)Kg);
    __syncthreads();
}

struct ShapeInfo { int path, np, threads, global_k, global_ws, mw; };
bool shape_info(int shape, ShapeInfo& o) {
    if (shape < 0 || shape >= kGp1dShapes) return false;
    if (shape < kSlabTier) o = {kPathWave, kTier[shape].wnp, kGp1dThreads, 0, 0, kTier[shape].mw};
    else if (shape < 2 * kSlabTier) o = {kPathBlock, kTier[shape - kSlabTier].np, kGp1dThreads, 0, 0, kTier[shape - kSlabTier].mw};
    else if (shape == 2 * kSlabTier) o = {kPathBlock, kGp1dLongNP, kGp1dThreads, 1, 0, kTier[kSlabTier].mw};
    else o = {kPathLong, kGp1dLongTierNP, kGp1dThreads, 1, 1, 1};
    return true;
}

}  // namespace

extern "C" {

int devprobe_gp1d_shapes() { return kGp1dShapes; }
int devprobe_gp1d_max_evals() { return kGp1dMaxEvals; }

// o[6]: path (0 wave, 1 block, 2 long), row capacity NP of the fit, threads of the workgroup, matrix in global scratch,
// working set in global memory, waves per SIMD of the launch bounds
int devprobe_gp1d_shape_info(int shape, int* o) {
    ShapeInfo si;
    if (!shape_info(shape, si)) return kBadShape;
    o[0] = si.path; o[1] = si.np; o[2] = si.threads; o[3] = si.global_k; o[4] = si.global_ws; o[5] = si.mw;
    return 0;
}

// One workgroup of shape `shape`.  Point set w (w < 4; the wave shapes give wavefront w set w, the others take set 0 only
// and want m4[1..3] = 0) has m4[w] prepared points and ne4[w] evaluations, evaluation e on the set's first n_e points at
// th_e[0..3); m4[w] = 0: the wavefront skips.  The sets follow one another in every array: t, y, e2: [sum m4]; n_e:
// [sum ne4]; th_e: [sum ne4][3]; f: [sum ne4]; g: [sum ne4][3]; alpha: [sum ne4][astride] with astride = max m4 (row e:
// its first n_e slots).
int devprobe_gp1d_eval(int shape, const int* m4, const double* t, const double* y, const double* e2, const int* ne4,
                       const int* n_e, const double* th_e, double* f, double* g, double* alpha) {
    ShapeInfo si;
    if (!shape_info(shape, si)) return kBadShape;
    int mt = 0, et = 0, astride = 0;
    for (int w = 0; w < kSets; ++w) {
        const int m = m4[w], ne = ne4[w];
        if (m == 0) {
            if (ne != 0) return kBadSize;
            continue;
        }
        if (w > 0 && si.path != kPathWave) return kBadSize;
        // gp1d_band's window: at least 5 points, and room for the augmented row
        if (m < 5 || m + 1 > si.np || ne < 1 || ne > kGp1dMaxEvals) return kBadSize;
        for (int i = mt; i < mt + m; ++i)
            if (!isfinite(t[i]) || !isfinite(y[i]) || !isfinite(e2[i])) return kBadSize;
        for (int e = et; e < et + ne; ++e) {
            if (n_e[e] < 5 || n_e[e] > m) return kBadSize;
            for (int c = 0; c < 3; ++c)
                if (!isfinite(th_e[3 * e + c])) return kBadSize;
        }
        mt += m;
        et += ne;
        astride = (m > astride) ? m : astride;
    }
    if (et == 0 || (si.path != kPathWave && m4[0] == 0)) return kBadSize;
    Call c;
    const double *dt = c.in(t, mt), *dy = c.in(y, mt), *de2 = c.in(e2, mt);
    const int* dn = c.in(n_e, et);
    const double* dth = c.in(th_e, (size_t)3 * et);
    double *df = c.out(f, et), *dg = c.out(g, (size_t)3 * et), *da = c.out(alpha, (size_t)et * astride);
    Gp1dProbeArgs a;
    for (int w = 0, mo = 0, eo = 0; w < kSets; ++w) {
        a.s[w] = {dt + mo, dy + mo, de2 + mo, m4[w], ne4[w], dn + eo, dth + (size_t)3 * eo,
                  df + eo, dg + (size_t)3 * eo, da + (size_t)eo * astride, astride};
        mo += m4[w];
        eo += ne4[w];
    }
    // Gram slab of the global-scratch shapes (one workgroup's share of the product's slab) with a guard region of its own,
    // sentinel-filled like the product's never-initialised scratch may be anything
    const size_t kbytes = si.global_k ? (size_t)gp_store_doubles(si.np) * sizeof(double) : 0;
    unsigned char* ks = (unsigned char*)c.alloc(kbytes + kPad);
    if (ks) c.err = hipMemset(ks, kFill, kbytes + kPad);
    char* ws = nullptr;
    if (si.global_ws) {
        ws = (char*)c.alloc(kGp1dLongTierSBytes);
        if (ws && c.ok()) c.err = hipMemset(ws, kFill, kGp1dLongTierSBytes);
    }
    if (c.ok()) {
        switch (shape) {
            case 0: k_gp1d_wave<0><<<1, kGp1dThreads>>>(a); break;
            case 1: k_gp1d_wave<1><<<1, kGp1dThreads>>>(a); break;
            case 2: k_gp1d_wave<2><<<1, kGp1dThreads>>>(a); break;
            case 3: k_gp1d_block<0><<<1, kGp1dThreads>>>(a); break;
            case 4: k_gp1d_block<1><<<1, kGp1dThreads>>>(a); break;
            case 5: k_gp1d_block<2><<<1, kGp1dThreads>>>(a); break;
            case 6: k_gp1d_slab<kSlabTier><<<1, kGp1dThreads>>>(a, (double*)ks); break;
            default: k_gp1d_long<<<1, kGp1dThreads>>>(a, (double*)ks, ws); break;
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
