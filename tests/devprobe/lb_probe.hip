// lb_probe.hip -- device probe of the 2-D GP's L-BFGS-B driver, lb_start / lb_advance<4, 10> of csrc/lbfgsb.hpp, by itself.
//
// Test infrastructure (tests/test_gpu_lbfgsb.py), never loaded by the product path.  The host simulation cannot reach what
// the device runs: lb_advance<4, 10, IN_LDS = true> on an address_space(3) cast of the state, called by thread 0 between
// two workgroup barriers while every other thread reads S.lb.x / S.lb_why afterwards (gp_object of csrc/gp.hpp), and the
// IN_LDS = false instantiation on a state in global memory (the long-object tier).  Here one 256-thread workgroup per
// tape replays a recorded run (tests/lb_reference.py): thread 0 stores the taped f and g and advances the state, and after
// the barrier lane 0 of every wavefront writes out the x and lb_why it reads.  The host counterpart is hostsim_lb_replay.
//
// Conventions of probe.hip / gp_probe.hip: host pointers in, sizes checked on the host, one launch, guard bytes behind every
// output; no tickets, no atomics, no loop whose trip count depends on anything but ne; workgroups never wait for one another.
#include "lbfgsb.hpp"

#include "call.hpp"

#include <cmath>

using namespace lcfe;

namespace {

constexpr int kLbThreads = 256, kLbWaves = kLbThreads / 64;
constexpr int kLbMaxGrid = 32;             // workgroups of the launch; a workgroup takes tapes b, b + grid, ...
constexpr int kLbMaxTapes = 64, kLbMaxEvals = 4096;

struct LbProbeArgs {
    int ntape, maxne;
    const int *ne, *maxiter, *off;         // [ntape] steps of a tape, its iteration limit, its first row in f / g
    const double *x0, *f, *g;              // [ntape][4], [sum ne], [sum ne][4]
    double* x_out;                         // [ntape][kLbWaves][maxne + 1][4]: row 0 = x0, row k + 1 = the point asked for after step k
    int* why_out;                          // [ntape][kLbWaves][maxne]
    int *n_iter, *n_eval, *steps;          // [ntape][maxne] x 2, [ntape]
    double *x_final, *f_final;             // [ntape][4], [ntape]
};

// the optimiser's part of gp_object's working set
struct LbShared {
    LbState<4, 10> lb;
    int lb_why;
};

template <bool IN_LDS>
__device__ __forceinline__ void lb_replay_tape(const LbProbeArgs& a, LbShared& S, int tape) {
    const int tid = threadIdx.x, wave = tid / 64, lane = tid % 64;
    const int ne = a.ne[tape], off = a.off[tape];
    double* xo = a.x_out + (size_t)(tape * kLbWaves + wave) * (a.maxne + 1) * 4;
    int* wo = a.why_out + (size_t)(tape * kLbWaves + wave) * a.maxne;
    if (tid == 0) lb_start(S.lb, a.x0 + 4 * tape, a.maxiter[tape], 1e7, 1e-5, 20);   // gp_object's constants
    __syncthreads();
    if (lane == 0)
        for (int c = 0; c < 4; ++c) xo[c] = S.lb.x[c];
    int k = 0;
    while (k < ne) {
        if (tid == 0) {
            S.lb.f = a.f[off + k];
            for (int c = 0; c < 4; ++c) S.lb.g[c] = a.g[4 * (size_t)(off + k) + c];
            S.lb_why = lb_advance<4, 10, IN_LDS>(S.lb);
        }
        __syncthreads();
        const int why = S.lb_why;
        if (lane == 0) {
            for (int c = 0; c < 4; ++c) xo[4 * (k + 1) + c] = S.lb.x[c];
            wo[k] = why;
        }
        if (tid == 0) {
            a.n_iter[(size_t)tape * a.maxne + k] = S.lb.n_iter;
            a.n_eval[(size_t)tape * a.maxne + k] = S.lb.n_eval;
        }
        ++k;
        __syncthreads();                   // (in gp_object: the barriers of the next evaluation) all have read x and lb_why
        if (why != LB_EVAL) break;
    }
    if (tid == 0) {
        a.steps[tape] = k;
        for (int c = 0; c < 4; ++c) a.x_final[4 * tape + c] = S.lb.x[c];
        a.f_final[tape] = S.lb.f;
    }
    __syncthreads();
}

// variant 0: the state in LDS, as GpLds holds it
__global__ __launch_bounds__(kLbThreads) void k_lb_replay_lds(LbProbeArgs a) {
    __shared__ LbShared S;
    for (int tape = blockIdx.x; tape < a.ntape; tape += gridDim.x) lb_replay_tape<true>(a, S, tape);
}

// variant 1: the state in global memory, as the long-object tier's working set holds it (one slot per workgroup)
__global__ __launch_bounds__(kLbThreads) void k_lb_replay_global(LbProbeArgs a, LbShared* slots) {
    LbShared& S = slots[blockIdx.x];
    for (int tape = blockIdx.x; tape < a.ntape; tape += gridDim.x) lb_replay_tape<false>(a, S, tape);
}

}  // namespace

extern "C" {

int devprobe_lb_waves() { return kLbWaves; }

// Replays ntape recorded runs in one launch, one workgroup per tape (grid capped at 32).  variant 0: state in LDS and
// lb_advance<4, 10, true>; variant 1: state in global memory and lb_advance<4, 10, false>.  tape_f: [sum ne], tape_g:
// [sum ne][4], tape after tape.  With maxne = max(ne): x_out [ntape][waves][maxne + 1][4], why_out [ntape][waves][maxne],
// n_iter and n_eval [ntape][maxne], steps [ntape], x_final [ntape][4], f_final [ntape].
int devprobe_lb_replay(int variant, int ntape, const int* ne, const int* maxiter, const double* x0, const double* tape_f,
                       const double* tape_g, double* x_out, int* why_out, int* n_iter, int* n_eval, int* steps,
                       double* x_final, double* f_final) {
    if (variant < 0 || variant > 1) return kBadShape;
    if (ntape < 1 || ntape > kLbMaxTapes) return kBadSize;
    std::vector<int> off(ntape);
    int total = 0, maxne = 0;
    for (int i = 0; i < ntape; ++i) {
        if (ne[i] < 1 || ne[i] > kLbMaxEvals || maxiter[i] < 1) return kBadSize;
        for (int c = 0; c < 4; ++c)
            if (!std::isfinite(x0[4 * i + c])) return kBadSize;
        off[i] = total;
        total += ne[i];
        if (ne[i] > maxne) maxne = ne[i];
    }
    const int grid = ntape < kLbMaxGrid ? ntape : kLbMaxGrid;
    Call c;
    LbProbeArgs a;
    a.ntape = ntape;
    a.maxne = maxne;
    a.ne = c.in(ne, ntape);
    a.maxiter = c.in(maxiter, ntape);
    a.off = c.in(off.data(), ntape);
    a.x0 = c.in(x0, (size_t)4 * ntape);
    a.f = c.in(tape_f, total);
    a.g = c.in(tape_g, (size_t)4 * total);
    a.x_out = c.out(x_out, (size_t)ntape * kLbWaves * (maxne + 1) * 4);
    a.why_out = c.out(why_out, (size_t)ntape * kLbWaves * maxne);
    a.n_iter = c.out(n_iter, (size_t)ntape * maxne);
    a.n_eval = c.out(n_eval, (size_t)ntape * maxne);
    a.steps = c.out(steps, ntape);
    a.x_final = c.out(x_final, (size_t)4 * ntape);
    a.f_final = c.out(f_final, ntape);
    // the global states, sentinel-filled like the product's never-initialised scratch, with a guard region of their own
    const size_t sbytes = (size_t)grid * sizeof(LbShared);
    unsigned char* slots = (unsigned char*)c.alloc(sbytes + kPad);
    if (slots) c.err = hipMemset(slots, kFill, sbytes + kPad);
    if (c.ok()) {
        if (variant == 0) k_lb_replay_lds<<<grid, kLbThreads>>>(a);
        else k_lb_replay_global<<<grid, kLbThreads>>>(a, (LbShared*)slots);
    }
    unsigned char guard[kPad];
    bool guard_read = false;
    if (c.ok()) c.err = hipGetLastError();
    if (c.ok()) c.err = hipDeviceSynchronize();
    if (c.ok()) { c.err = hipMemcpy(guard, slots + sbytes, kPad, hipMemcpyDeviceToHost); guard_read = c.ok(); }
    const int rc = c.finish();
    if (rc != 0) return rc;
    if (guard_read)
        for (int i = 0; i < kPad; ++i)
            if (guard[i] != kFill) return -3;
    return 0;
}

}  // extern "C"
